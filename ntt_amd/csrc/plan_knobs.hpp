// Every environment variable that changes what a plan does, one named function each (ntt_plan.cpp reads
// the environment nowhere else; DESIGN.md §1.1 has the table).  Standard C++ only.  They are A/B switches
// and diagnostics: no product path depends on one being set.  When a knob is read is part of its
// behaviour (tests set some between plans): once per process (a function-local static, at the first
// use), per schedule computation, or when a plan first builds its single-launch / in-place state.
#pragma once
#include <cstddef>
#include <cstdlib>

namespace {
namespace knob {

// the one parser: a variable's text (nullptr when unset) and the readings the knobs take of it
struct Env {
  const char* v;
  explicit Env(const char* name) : v(getenv(name)) {}
  bool is(char c) const { return v && v[0] == c; }                  // first character
  long num(long unset) const { return v && *v ? atol(v) : unset; }  // unset or empty: the default
  const char* text() const { return v && *v ? v : nullptr; }
};
#define NTT_KNOB_ONCE(type, name, expr) \
  inline type name() {                  \
    static const auto v = (expr);       \
    return v;                           \
  }

// ---- once per process
// NTT_FUSED_ORDER=0: no per-device ordering of the single launches (FusedSerial; A/B only)
NTT_KNOB_ONCE(bool, fused_order, !Env("NTT_FUSED_ORDER").is('0'))
// Diagnostics (NTT_FUSED_TRACE=<file>): the two-pass single launch writes per-workgroup wall-clock
// stamps (start, after pass 1, after the barrier, end; 100 MHz), appended to <file> after each call,
// which then synchronises its stream.  Never on in measured runs.
NTT_KNOB_ONCE(const char*, fused_trace_path, Env("NTT_FUSED_TRACE").text())
// NTT_SHOUP_OUTER=0 keeps the Montgomery outer-twiddle tables (A/B switch); =1 keeps pass 1 on its
// Montgomery table (round-4 behaviour); default 2: Shoup pairs wherever the table fits
NTT_KNOB_ONCE(int, shoup_outer, (int)Env("NTT_SHOUP_OUTER").num(2))
// NTT_ROWS=0: single-tile transforms run one per workgroup (KIND_SINGLE), never KIND_ROWS
NTT_KNOB_ONCE(bool, rows, !Env("NTT_ROWS").is('0'))
// NTT_PASS1_FULL=1: pass 1 streams its full outer-twiddle table on every engine (A/B)
NTT_KNOB_ONCE(bool, pass1_full, Env("NTT_PASS1_FULL").num(0) > 0)
// NTT_XCD_ORDER: the XCD-grouped tile order (PlanImpl::pass_args).  =0 off, =1 on every column pass,
// =3 not on the one-column passes (A/B); default 2
NTT_KNOB_ONCE(int, xcd_order, (int)Env("NTT_XCD_ORDER").num(2))
// NTT_DREV_DIAG=0 (or empty): the in-place digit reversal (k_digitrev_swap) takes its tile pairs in
// row-major order instead of the diagonal one (A/B)
NTT_KNOB_ONCE(bool, drev_diag, !Env("NTT_DREV_DIAG").v || Env("NTT_DREV_DIAG").num(0) != 0)
// NTT_SINGLE_LAUNCH=1 / =0 forces the single-launch schedule on / off for every plan (A/B); unset (-1):
// the plan's NTT_PLAN_SINGLE_LAUNCH flag decides
NTT_KNOB_ONCE(int, single_launch, (int)Env("NTT_SINGLE_LAUNCH").num(-1))
// NTT_WIDE_TILES=0: no second plan of 4096-element tiles (make_wide_plan)
NTT_KNOB_ONCE(bool, wide_tiles, !Env("NTT_WIDE_TILES").is('0'))
// NTT_TWO_PASS_24=1 routes a default 2^24 4-limb plan's single-vector transforms to the 4096-element
// tiles (12 + 12)
NTT_KNOB_ONCE(bool, two_pass_24, Env("NTT_TWO_PASS_24").is('1'))
// At most NTT_SHIM_CACHE_PLANS (default 8, at least 1; empty counts as 0) plans in the shims' cache
NTT_KNOB_ONCE(long, shim_cache_env, Env("NTT_SHIM_CACHE_PLANS").v ? Env("NTT_SHIM_CACHE_PLANS").num(0) : 8)
inline size_t shim_cache_plans() { return (size_t)(shim_cache_env() > 0 ? shim_cache_env() : 1); }
#undef NTT_KNOB_ONCE

// ---- at every schedule computation
// NTT_SCHEDULE="r1,r2,..." (experiments only): that radix sequence for the sizes it sums to, when the
// pass kernels accept it (plan_schedule.hpp)
inline const char* schedule() { return Env("NTT_SCHEDULE").text(); }

// ---- at every ntt_fri_fold call (tools/bench_fold.py times both forms interleaved in one process)
// NTT_FOLD_STAGED=1 / =0: the fibres of k_fri_fold reach their threads through LDS / each thread loads its
// own fibre (A/B); unset or empty (-1): the plan's default form
inline int fold_staged() { return (int)Env("NTT_FOLD_STAGED").num(-1); }

// ---- at every ntt_batch_inverse call (tools/bench_scan.py times the forms interleaved in one process)
// NTT_INV_FORM=0 / 1 / 2: how k_batch_inv shares an inversion (scan_shape.hpp InvShape: a run of 16 words, of 32,
// or one inversion per wave; A/B); unset or empty (-1): the default form
inline int inv_form() { return (int)Env("NTT_INV_FORM").num(-1); }

// ---- when a plan first builds its single-launch or in-place state
// NTT_FUSED_MODE=0: the dataflow form of k_fused3 (per-tile hand-offs), else the grid-barrier form (1)
inline unsigned fused_mode() { return Env("NTT_FUSED_MODE").is('0') ? 0u : 1u; }
// NTT_FUSED_VERBOSE (any value): a single-launch build prints its geometry to stderr
inline bool fused_verbose() { return Env("NTT_FUSED_VERBOSE").v != nullptr; }
// NTT_FUSED_DBG=<bits>: FusedArgs::dbg of k_fused3 (diagnostics)
inline unsigned fused_dbg() { return (unsigned)Env("NTT_FUSED_DBG").num(0); }
// NTT_IPN=0 keeps the separate tile-swap pass after an in-place final pass (A/B)
inline bool ipn() { return !Env("NTT_IPN").is('0'); }

// ---- at wide-plan creation, checked build (NTT_DEBUG_CHECKS, libntt_debug.so) only
// NTT_TEST_WIDE_FAIL=1 makes the second plan's attempt fail through a refused allocation
// (tests/test_gpu_wide_tiles.py); the product build has no such hook
inline bool test_wide_fail() {
#if defined(NTT_DEBUG_CHECKS) && NTT_DEBUG_CHECKS
  return Env("NTT_TEST_WIDE_FAIL").is('1');
#else
  return false;
#endif
}

}  // namespace knob
}  // namespace
