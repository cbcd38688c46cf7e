// Host side of libntt.so: plans (twiddle tables + scratch cached per device), pass scheduling, the
// C ABI of include/ntt.h and the reference-shaped shims (SSIP, NTT_GZKP_256, NTT_GZKP_64).
//
// Reference behaviour mirrored (file:line in tie-pilot-qxw/NTT):
//   * w_n = g^((p-1)/n) from the generator argument        GZKP-NTT.cu:1462, big-num.cu:292-296
//   * forward = natural -> natural, in place               SSIP GZKP-NTT.cu:1452-1558
//   * inverse = forward with g^-1, then * n^-1             GZKP-NTT.cu:1725-1732
//   * modulus-generic 256-bit path (prime argument)        big-num.cu:68,173,260
// Differences: tables are built once per plan (the reference rebuilt pq/omegas on every call and
// freed them with a new[]/free mismatch, GZKP-NTT.cu:1554-1555); errors are returned as status
// codes instead of asserts; nothing is printed.
#include <algorithm>
#include <hip/hip_runtime.h>

#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <tuple>
#include <type_traits>
#include <vector>

#include "../../include/ntt.h"
#include "eng29_args.hpp"
#include "ntt_internal.hpp"
#include "ntt_kernels.hpp"
#include "plan_devmem.hpp"    // the plan's own parts, included here alone: DevBuf, Lazy, the watchdog-word pool
#include "plan_hostmath.hpp"  // HostField, EngHost<E>
#include "plan_knobs.hpp"     // every environment variable, as knob::name()
#include "plan_schedule.hpp"  // schedule_for, schedule_palindrome, mid_digits, overlaps

using namespace ntt;

namespace {

thread_local int g_last_error = NTT_OK;

// What the first pass of a transform reads and multiplies by (run_io).  Every route that exists has a
// named constructor; a call site names its route.
struct FirstPass {
  const uint32_t* src2 = nullptr;   // second operand: the pass starts from the product in * src2
  const uint32_t* outer = nullptr;  // outer-twiddle table (w R_e, element format) that replaces the plan's own
  // factors applied at load: one table (u^d, the fused coset; hi null) or a two-level pair (lo scaled by R_e, hi)
  const uint32_t* at_load = nullptr;
  const uint32_t* at_load_hi = nullptr;
  // nonzero: the pass is the low-degree extension's (PRO_LDE), which reads n_in <= n inputs per transform
  // and takes the padding from registers.  Without a table of its own it computes its outer twiddles
  // from the plan's two-level tables.
  size_t n_in = 0;
  // staging: the inputs are first scaled by the two-level pair into `stage` (one launch, recorded
  // unlabelled), which the pass then reads
  const uint32_t* scale_lo = nullptr;
  const uint32_t* scale_hi = nullptr;
  uint32_t* stage = nullptr;

  static FirstPass plain() { return {}; }
  static FirstPass make(const uint32_t* src2, const uint32_t* outer, const uint32_t* lo, const uint32_t* hi, size_t n_in) {
    FirstPass f;
    f.src2 = src2, f.outer = outer, f.at_load = lo, f.at_load_hi = hi, f.n_in = n_in;
    return f;
  }
  // fused polymul inverse: the product at load, the inverse's pass-1 table scaled by n^-1 R_e
  static FirstPass product(const uint32_t* b, const uint32_t* outer_ninv) { return make(b, outer_ninv, nullptr, nullptr, 0); }
  // fused coset forward: u^d at load, c^col folded into the outer table
  static FirstPass coset(const uint32_t* outer_c, const uint32_t* u_pow) { return make(nullptr, outer_c, u_pow, nullptr, 0); }
  // low-degree extension without a shift on the plan's own pass-1 table
  static FirstPass lde_plan_table(size_t n_in, const uint32_t* plan_outer) { return make(nullptr, plan_outer, nullptr, nullptr, n_in); }
  static FirstPass lde_coset(size_t n_in, const uint32_t* outer_c, const uint32_t* u_pow) {
    return make(nullptr, outer_c, u_pow, nullptr, n_in);
  }
  // the shift's two-level factors at load (none: no shift), two-level outer twiddles
  static FirstPass lde_at_load(size_t n_in, const uint32_t* lo = nullptr, const uint32_t* hi = nullptr) {
    return make(nullptr, nullptr, lo, hi, n_in);
  }
  // the engines without the product at load: the shift's factors through the staging buffer
  static FirstPass lde_staged(size_t n_in, const uint32_t* lo, const uint32_t* hi, uint32_t* stage) {
    FirstPass f = lde_at_load(n_in);
    f.scale_lo = lo, f.scale_hi = hi, f.stage = stage;
    return f;
  }
};

}  // namespace

// the plan's features, each a struct the plan owns and hands a reference to itself; they name FirstPass
#include "plan_prover.hpp"  // Prover<E, Plan>: the prover-stage calls (matrix, fold, DEEP, Merkle, scans), HasMat engines only
#include "plan_rivals.hpp"  // Rivals<E, Plan>: the rival schedules
#include "plan_shift.hpp"   // Shift<E, Plan>: the shift cache, coset transforms, low-degree extension
#include "plan_single.hpp"  // Single<E, Plan>: the single-launch schedules, the in-place final pass

namespace {

// ------------------------------------------------------------------------------ plan
// the address of kEngineTag<E> names engine E (PlanBase::engine)
template <class E>
constexpr char kEngineTag = 0;

struct PlanBase {
  // Destruction: ~PlanImpl makes the plan's device current, its DevBuf members free themselves there,
  // and this, which runs last, returns the watchdog slot and the events and restores the caller's device
  virtual ~PlanBase() {
    watch_slot_release(h_watch);
    for (auto& row : ev)
      for (auto& e : row)
        if (e) (void)hipEventDestroy(e);
    if (caller_device >= 0) (void)hipSetDevice(caller_device);
  }
  int caller_device = -1;  // set by ~PlanImpl
  const void* engine = nullptr;  // &kEngineTag<E> of the PlanImpl<E> this is
  virtual int run(void* d, unsigned batch, bool inverse, hipStream_t st) = 0;
  virtual int pointwise(const void* a, const void* b, void* c, hipStream_t st) = 0;
  virtual int polymul(void* a, void* b, void* c, hipStream_t st) = 0;
  virtual int fill(void* d, uint64_t count, int kind, uint64_t seed, uint64_t row0, unsigned log_inner,
                   unsigned log_stride, hipStream_t st) = 0;
  virtual int twiddle_pack(const void* src, void* dst, unsigned log_rows, unsigned log_len, unsigned log_bw,
                           uint64_t row0, bool inverse, uint64_t peer_stride, hipStream_t st) = 0;
  virtual int transpose(const void* src, void* dst, unsigned log_rows, unsigned log_cols, unsigned log_blk_rows,
                        uint64_t blk_stride, hipStream_t st) = 0;
  virtual int inverse_pointwise(const void* a, const void* b, void* c, unsigned batch, hipStream_t st) = 0;
  virtual int run_fs(const void* in, const void* in2, void* out, unsigned batch, bool inverse, const ntt::FsIO& io,
                     hipStream_t st) = 0;
  virtual int build_fs_table(void* table, unsigned log_rows, unsigned log_cols, uint64_t row0, uint64_t col0,
                             bool inverse, unsigned scale_log, hipStream_t st) = 0;
  virtual size_t table_entry_bytes() const = 0;
  // pass kernels a transform of 2^log_x points takes with this plan's engine (its schedule()), and
  // the largest radix (log2) among them
  virtual unsigned passes_for(unsigned log_x) const = 0;
  virtual unsigned max_radix_for(unsigned log_x) const = 0;
  virtual int coset(void* d, const uint64_t* shift, unsigned limbs64, bool inverse, hipStream_t st) = 0;
  // low-degree extension (ntt_lde_batch): batch inputs of n >> log_blowup coefficients to batch outputs of n
  virtual int lde(const void* in, void* out, unsigned log_blowup, const uint64_t* shift, unsigned limbs64,
                  unsigned batch, hipStream_t st) = 0;
  virtual int count_noncanonical(const void* d, uint64_t count, uint64_t* bad, hipStream_t st) = 0;
  virtual int device_status(unsigned* bad) = 0;
  // the plan's batch-1 forward / inverse run as ONE launch (NTT_PLAN_SINGLE_LAUNCH): its single-launch
  // state is built now (a second plan of 4096-element tiles is kept only when this holds)
  virtual bool single_launch_ready() { return false; }
  uint64_t n = 0;
  unsigned flags = 0;
  unsigned log_n = 0, elem_bytes = 0, npass = 0;
  unsigned r[8] = {0};
  int device = 0;
  // optional per-launch timing: events recorded on the caller's stream between launches, one
  // slot per transform in a ring of kSlots transforms (no host synchronisation per transform).
  // Each interval between two events carries a label naming the launch it timed (kind letter +
  // log2 radix, "s" for a Shoup-pair outer table: c8, c8s, f8, r8, s12, i8, d, b; tools/pmc_to_traffic.py
  // derives the same labels from the rocprofv3 kernel names), "" when unlabelled.
  // Grouping (ntt_plan_profile_group, the rank plan's four-step transforms): once a plan has been put
  // in group mode, a transform continues the current slot until the next group call, so the slot holds
  // every launch of one caller-level operation (e.g. a row transform run as two launches of 2^15 rows);
  // the time between two transforms of a group is an interval labelled "-" and is not a launch.
  static constexpr unsigned kSlots = 64, kEv = 17;
  bool profiling = false;
  hipEvent_t ev[kSlots][kEv] = {};
  char lab[kSlots][kEv][6] = {};  // label of the interval that ends at event k
  unsigned ev_used = 0, slot = 0, nrec = 0;
  bool grouped = false, group_new = false;
  // Watchdog report (ntt_kernels.hpp): a host-mapped word that a kernel sets when one of its bounded
  // inter-workgroup waits gives up.  Every later call on the plan returns NTT_ERR_DEVICE (a plain host
  // read, no device query) until ntt_plan_device_status reads and clears it.
  // The word is a slot of a process-wide pinned page (watch_slot_acquire below), taken when the plan
  // first builds a schedule with such waits; plans that never do hold none.
  uint32_t* h_watch = nullptr;  // host pointer (a slot of the mapped, coherent page)
  uint32_t* d_watch = nullptr;  // its device alias (the kernels' Watchdog::report)
  uint32_t wd_spins = 1u << 21; // poll limit of a wait (~2 s); ntt_plan_set_watchdog
  bool tripped() const { return h_watch && __atomic_load_n(h_watch, __ATOMIC_ACQUIRE) != 0u; }
  void clear_trip() {
    if (h_watch) __atomic_store_n(h_watch, 0u, __ATOMIC_RELEASE);
  }
  ntt::Watchdog watchdog(uint32_t* abort_w) const { return ntt::Watchdog{d_watch, abort_w, wd_spins}; }
  bool alloc_watch();  // true once the plan holds a report word (defined after the slot pool)
  void begin(hipStream_t st) {
    if (!profiling) return;
    if (grouped && !group_new && nrec > 0 && ev_used > 0 && ev_used + 1 < kEv) {
      mark(st, "-");  // the same group: the time since its previous transform is a gap
      return;
    }
    group_new = false;
    slot = nrec % kSlots;
    ev_used = 0;
    ++nrec;
    mark(st);
  }
  void mark(hipStream_t st, const char* kind = "", unsigned log_radix = 0, bool shoup = false) {
    if (!profiling || ev_used >= kEv) return;
    char* l = lab[slot][ev_used];
    if (log_radix)
      snprintf(l, sizeof lab[0][0], "%s%u%s", kind, log_radix, shoup ? "s" : "");
    else
      snprintf(l, sizeof lab[0][0], "%s", kind);
    (void)hipEventRecord(ev[slot][ev_used++], st);
  }
};

bool PlanBase::alloc_watch() {
  if (h_watch) return true;
  h_watch = watch_slot_acquire();
  if (!h_watch) return false;
  void* d = nullptr;
  if (hipHostGetDevicePointer(&d, h_watch, 0) != hipSuccess) {
    watch_slot_release(h_watch);
    h_watch = nullptr;
    return false;
  }
  d_watch = static_cast<uint32_t*>(d);
  return true;
}

// The schedule of an engine: plan_schedule.hpp's schedule_for at the engine's parameters.  An engine
// may name a wider column group than MIN_COLS_LOG that it prefers (Eng31::PREF_COLS_LOG).
template <class E>
static bool schedule_for(unsigned log_n, unsigned* r, unsigned& p) {
  unsigned pref = E::MIN_COLS_LOG;
  if constexpr (std::is_same_v<E, Eng31>) pref = Eng31::PREF_COLS_LOG;
  return schedule_for(log_n, E::TILE_LOG, E::MIN_COLS_LOG, pref, E::NARROW_FIRST, r, p);
}

template <class E>
struct PlanImpl;

// The engines whose plans hold a Prover (plan_prover.hpp), named here and nowhere else: the prover-stage entry
// points of the C ABI find the plan's engine by its tag and call the final class, with no virtual per call.
template <class... Es>
struct EngineList {
  template <class E>
  static constexpr bool has = (std::is_same_v<E, Es> || ...);
  static_assert((HasMat<Es>::value && ...), "a Prover needs the engine's prover-stage kernels");
  // f(the plan's Prover); NTT_ERR_ARG, with f not called, for a plan of any other engine
  template <class F>
  static int visit(PlanBase& P, F& f) {
    int rc = NTT_ERR_ARG;
    (void)((P.engine == &kEngineTag<Es> && ((rc = f(static_cast<PlanImpl<Es>&>(P).prover)), true)) || ...);
    return rc;
  }
};
using ProverEngines = EngineList<Eng64G, Eng31>;
struct NoProver {  // what the other engines' plans hold instead
  template <class Plan>
  explicit NoProver(Plan&) {}
};

template <class E>
struct PlanImpl final : PlanBase {
  static constexpr int NH = EngHost<E>::NH;
  static constexpr int TW = E::TW;
  static constexpr int MEMW = E::MEMW;
  static constexpr int SCRW = E::SCRW;  // scratch (engines.hpp)
  static constexpr int TABW = E::TABW;  // element-format twiddle tables (engines.hpp)
  HostField<NH> H;
  EngHost<E> EH;
  typename E::Args Ff{}, Fi{};
  DevBuf d_tab;
  DevBuf d_scratch;  // (size_t)n * batch elements of SCRW words, grown on demand (ensure_scratch)
  // per-pass outer twiddle tables (w R_e, HBM element format), one allocation per direction: the
  // forward's at plan creation, the inverse's at the first inverse call (a forward-only user pays for
  // one direction: 2^24 BN254 plan 1.55 -> 1.03 GB)
  DevBuf d_fulls[2];
  Lazy full_state[2];       // ready: d_fulls[dir] is built; unavailable: the two-level tables serve
  size_t full_off[8] = {};  // element offsets of pass i's table in d_fulls[dir]
  size_t full_elems = 0;    // entries per direction
  bool use_full = false;
  DevBuf d_full_sh;               // passes >= 2: the same tables as Shoup pairs (E::TW words per entry)
  size_t full_sh_off[2][8] = {};  // entry offsets into d_full_sh, [dir][pass]
  bool full_sh_ok[8] = {};         // pass i takes its outer twiddles from d_full_sh
  size_t off_pinvB = 0;           // p^-1 mod B (E::W limbs) in d_tab (Shoup-pair table build)
  // table word offsets, [dir]: 0 forward, 1 inverse
  size_t off_int[2][8] = {};
  size_t off_los[2] = {}, off_hi[2] = {};  // los: the lo table scaled by R_e (left factor of on-the-fly twiddles)
  size_t off_hi_is = 0, off_r2 = 0;                        // off_hi_is: the inverse's hi table scaled by n^-1
  size_t off_rm = 0;                    // R_e R^-1 (Montgomery-form pointwise product)
  size_t off_pow2inv = 0;               // 2^-k, k = 0..log_n, E::TW words each (build_fs_table's scale)
  size_t off_hi_ipm = 0;                // inverse hi table scaled by n^-1 R_e (fused polymul, pass 1)
  DevBuf d_full_pm;                     // inverse pass-1 outer twiddles x n^-1 R_e (fused polymul)
  // the plan's features, each in a header of its own with a reference to the plan
  Rivals<E, PlanImpl> rivals{*this};  // the rival schedules (plan_rivals.hpp)
  Shift<E, PlanImpl> shift{*this};    // the shift cache, coset transforms, low-degree extension (plan_shift.hpp)
  // the prover-stage calls, on the engines that have their kernels (plan_prover.hpp)
  static_assert(ProverEngines::has<E> == HasMat<E>::value, "ProverEngines lists the HasMat engines");
  std::conditional_t<ProverEngines::has<E>, Prover<E, PlanImpl>, NoProver> prover{*this};
  Single<E, PlanImpl> single{*this};  // single-launch schedules, the in-place final pass (plan_single.hpp)
  unsigned lo_bits = 0;
  uint32_t nrand = 1, top_bits = 28;

  // The two-level tables (lo scaled by R_e, hi) that the outer twiddles w_n^e of a direction are computed
  // from.  The inverse's hi table for pass 1 (index 0) carries n^-1; every other reader takes the plain one.
  const uint32_t* outer_lo(int dir) const { return d_tab.get() + off_los[dir]; }
  const uint32_t* outer_hi(int dir, unsigned pass) const {
    return d_tab.get() + (dir && pass == 0 ? off_hi_is : off_hi[dir]);
  }

  PlanImpl() { engine = &kEngineTag<E>; }
  // the members' buffers are freed after this body, with the plan's device current (~PlanBase)
  ~PlanImpl() override {
    (void)hipGetDevice(&caller_device);
    (void)hipSetDevice(device);
  }

  // modulus / generator as NH 32-bit words
  int init(const uint32_t* p, const uint32_t* g, unsigned log_n_, int dev, unsigned flags_) {
    device = dev;
    flags = flags_;
    log_n = log_n_;
    n = 1ull << log_n;
    elem_bytes = 4 * MEMW;
    // ---- modulus checks: odd, top word < 2^31 - 1 (no-carry host Montgomery)
    for (int i = 0; i < NH; ++i) H.M.p[i] = p[i];
    if (!(p[0] & 1)) return NTT_ERR_FIELD;
    if (p[NH - 1] >= 0x7fffffffu) return NTT_ERR_FIELD;
    EH.init(H);
    if (!EH.check_modulus(p)) return NTT_ERR_FIELD;
    uint32_t inv = 1;
    for (int i = 0; i < 5; ++i) inv *= 2 - p[0] * inv;
    H.M.pinv = 0u - inv;
    // R mod p, R^2 mod p by doubling (R = 2^(32 NH))
    {
      Vec<NH> x{};
      x[0] = 1;
      for (int k = 0; k < 32 * NH; ++k) x = H.add(x, x);
      H.r1 = x;
      for (int k = 0; k < 32 * NH; ++k) x = H.add(x, x);
      H.r2 = x;
    }
    EH.init(H);  // needs r2 for to_mont
    Vec<NH> gv;
    for (int i = 0; i < NH; ++i) gv[i] = g[i];
    if (!H.below_p(gv)) return NTT_ERR_FIELD;
    // (p - 1) >> log_n, and n | p - 1
    std::vector<uint32_t> pm1(p, p + NH);
    pm1[0] -= 1;  // p odd: no borrow
    for (unsigned b = 0; b < log_n; ++b)
      if ((pm1[b / 32] >> (b % 32)) & 1) return NTT_ERR_FIELD;
    std::vector<uint32_t> e(NH, 0);
    for (int i = 0; i < NH; ++i) {
      const unsigned wsh = log_n / 32, bsh = log_n % 32;
      uint64_t lo = (i + wsh < (unsigned)NH) ? pm1[i + wsh] : 0;
      uint64_t hi = (i + wsh + 1 < (unsigned)NH) ? pm1[i + wsh + 1] : 0;
      e[i] = (uint32_t)(((hi << 32) | lo) >> bsh);
    }
    const Vec<NH> gm = H.to_mont(gv);
    const Vec<NH> w = H.pow(gm, e);  // w_n (32-bit Montgomery form)
    if (log_n >= 1) {                // primitive: w^(n/2) == -1
      Vec<NH> pm1v;
      for (int i = 0; i < NH; ++i) pm1v[i] = pm1[i];
      if (H.from_mont(H.pow_u64(w, n / 2)) != pm1v) return NTT_ERR_FIELD;
    }
    std::vector<uint32_t> pm2(p, p + NH);  // p - 2 with borrow (BLS12-381 Fr has p[0] = 1)
    {
      uint64_t br = 2;
      for (int i = 0; i < NH && br; ++i) {
        const uint64_t d = (uint64_t)pm2[i] - br;
        pm2[i] = (uint32_t)d;
        br = (d >> 63) & 1;
      }
    }
    const Vec<NH> winv = H.pow(w, pm2);
    Vec<NH> nv{};
    nv[0] = (uint32_t)n;
    if (NH > 1) nv[1] = (uint32_t)(n >> 32);
    const Vec<NH> ninv_c = H.from_mont(H.pow(H.to_mont(nv), pm2));
    // field args per direction: w_8^k canonical
    auto fill_args = [&](typename E::Args& F, const Vec<NH>& wn) {
      const Vec<NH> w8m = (log_n >= 3) ? H.pow_u64(wn, n / 8) : H.r1;
      Vec<NH> acc = w8m, w8c[3];
      for (int k = 0; k < 3; ++k) {
        w8c[k] = H.from_mont(acc);
        acc = H.mul(acc, w8m);
      }
      EH.fill_args(F, p, w8c, ninv_c);
    };
    fill_args(Ff, w);
    fill_args(Fi, winv);
    wn_m[0] = w;
    wn_m[1] = winv;

    // random-fill parameters: top nonzero 64-bit limb of p, masked to bitlen-1 bits
    {
      const int L64 = (NH + 1) / 2;
      int top = 0;
      for (int i = L64 - 1; i >= 0; --i) {
        const uint64_t limb = (uint64_t)p[2 * i] | ((2 * i + 1 < NH) ? (uint64_t)p[2 * i + 1] << 32 : 0);
        if (limb) { top = i; break; }
      }
      const uint64_t tl = (uint64_t)p[2 * top] | ((2 * top + 1 < NH) ? (uint64_t)p[2 * top + 1] << 32 : 0);
      nrand = top + 1;
      top_bits = 63 - __builtin_clzll(tl);  // bitlen - 1
    }

    // ---- schedule + tables (engine-encoded)
    if (!schedule_for<E>(log_n, r, npass)) return NTT_ERR_ARG;
    if (flags & NTT_PLAN_IN_PLACE) {
      // passes store their lazily reduced values where they read them: the scratch element must be
      // the caller's element
      if (E::SCRW != E::MEMW) return NTT_ERR_ARG;
      if (npass >= 2 &&
          !schedule_palindrome(log_n, tile_log_of<E>(), tile_log_of<E>() - E::MIN_COLS_LOG, npass, r, npass))
        return NTT_ERR_ARG;
    }
    const bool twiddle_only = (flags & NTT_PLAN_TWIDDLE_ONLY) != 0;
    std::vector<uint32_t> host;
    auto push_powers = [&](const Vec<NH>& base_m, uint64_t count, const Vec<NH>* scale_m,
                           bool scaled = false) -> size_t {
      return push_powers_to(host, base_m, count, scale_m, scaled);
    };
    const Vec<NH> ninv_m = H.to_mont(ninv_c);
    for (int dir = 0; dir < 2; ++dir) {
      const Vec<NH>& wn = dir ? winv : w;
      if (twiddle_only) {
        // no transform tables
      } else if (npass == 0) {
        off_int[dir][0] = push_powers(wn, n, nullptr);
      } else {
        for (unsigned i = 0; i < npass; ++i)
          off_int[dir][i] = push_powers(H.pow_u64(wn, n >> r[i]), 1ull << r[i], nullptr);
      }
      {  // two-level tables of w_n^e (outer twiddles, four-step twiddle_pack)
        lo_bits = (log_n + 1) / 2;
        (void)push_powers(wn, 1ull << lo_bits, nullptr);  // the plain lo table: no reader, kept for the table's layout
        off_los[dir] = push_powers(wn, 1ull << lo_bits, nullptr, true);
        const Vec<NH> step = H.pow_u64(wn, 1ull << lo_bits);
        off_hi[dir] = push_powers(step, 1ull << (log_n - lo_bits), nullptr);
        if (dir == 1) {
          off_hi_is = push_powers(step, 1ull << (log_n - lo_bits), &ninv_m);
          // fused polymul: the pointwise Montgomery product leaves a b / R_e; fold R_e in here
          const Vec<NH> ninv_re_m = H.mul(ninv_m, H.to_mont(engine_radix_mod_p()));
          off_hi_ipm = push_powers(step, 1ull << (log_n - lo_bits), &ninv_re_m);
        }
      }
    }
    if (!twiddle_only)
      if (int rc = rivals.host_tables([&](unsigned shift, uint64_t count) {
            return push_powers(H.pow_u64(w, n >> shift), count, nullptr);
          }))
        return rc;
    {  // pointwise product constants: mulv leaves a b / R_e (R_e the engine's Montgomery radix);
       // multiplying by R_e gives a b, by R_e R^-1 the Montgomery product a b R^-1 (R = 2^(64 limbs64);
       // 2^32 on the 4-byte elements of Eng31)
      off_r2 = host.size();
      uint32_t enc[TW];
      EH.encode(engine_radix_mod_p(), enc);
      host.insert(host.end(), enc, enc + TW);
      while (host.size() % 4) host.push_back(0);
      Vec<NH> rio{};  // R = 2^(64 limbs64) mod p by doubling
      rio[0] = 1;
      constexpr int kIoBits = std::is_same_v<E, Eng31> ? 32 : 64 * ((NH + 1) / 2);
      for (int k = 0; k < kIoBits; ++k) rio = H.add(rio, rio);
      const Vec<NH> rio_inv = H.from_mont(H.pow(H.to_mont(rio), pm2));
      off_rm = host.size();
      EH.encode(H.from_mont(H.mul(H.to_mont(engine_radix_mod_p()), H.to_mont(rio_inv))), enc);
      host.insert(host.end(), enc, enc + TW);
      while (host.size() % 4) host.push_back(0);
    }
    {  // 2^-k mod p for k = 0..log_n as twiddles (Tw encoding): the four-step folds a row transform's
       // n2^-1 into its inverse epilogue table (build_fs_table's scale_log, ntt_rplan.cpp)
      off_pow2inv = host.size();
      uint32_t enc[TW];
      std::vector<std::vector<uint32_t>> ent(log_n + 1);
      Vec<NH> x = ninv_m;  // 2^-log_n (Montgomery form); doubling walks k down to 0
      for (int k = (int)log_n; k >= 0; --k) {
        EH.encode(H.from_mont(x), enc);
        ent[k].assign(enc, enc + TW);
        x = H.add(x, x);
      }
      for (unsigned k = 0; k <= log_n; ++k) host.insert(host.end(), ent[k].begin(), ent[k].end());
      while (host.size() % 4) host.push_back(0);
    }
    if constexpr (E::SHOUP_OUTER) {
      off_pinvB = host.size();
      host.insert(host.end(), EH.pinvB, EH.pinvB + E::W);
      while (host.size() % 4) host.push_back(0);
    }
    pm2_ = pm2;
    int cur = 0;
    (void)hipGetDevice(&cur);
    if (hipSetDevice(device) != hipSuccess) return NTT_ERR_HIP;
    int rc = NTT_OK;
    if (!d_tab.alloc(host.size() * 4) ||
        hipMemcpy(d_tab.get(), host.data(), host.size() * 4, hipMemcpyHostToDevice) != hipSuccess)
      rc = NTT_ERR_HIP;
#if NTT_DEBUG_CHECKS
    // debug builds: the status word every kernel of this plan records check failures in
    if (rc == NTT_OK && (!d_dbg.alloc(4) || hipMemset(d_dbg.get(), 0, 4) != hipSuccess)) rc = NTT_ERR_HIP;
    Ff.dbg = Fi.dbg = d_dbg.get();
#endif
    if (rc == NTT_OK && npass >= 2 && !twiddle_only && !(flags & NTT_PLAN_IN_PLACE)) rc = ensure_scratch(1);
    if (rc == NTT_OK && npass >= 2 && !twiddle_only) rc = build_full_tables();
    if (rc == NTT_OK) rc = rivals.build();
    (void)hipSetDevice(cur);
    return rc;
  }

  // Full per-pass outer-twiddle tables: pass i needs N_i entries (N_1 = n, N_2 = n / R_1, ...),
  // streamed from HBM like the data in pass 1 and L2-resident afterwards.  They replace the
  // two-level lookup's extra Montgomery product per element.  Skipped when a direction's tables
  // would not fit (the two-level tables are then used).
  // Cap: both directions together within a quarter of the free HBM at plan creation.
  int build_full_tables() {
    size_t elems = 0;
    unsigned blk = log_n;
    for (unsigned i = 0; i + 1 < npass; ++i) {
      full_off[i] = elems;
      elems += 1ull << blk;
      blk -= r[i];
    }
    full_elems = elems;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return NTT_OK;
    if (2 * elems * TABW * 4 > free_b / 4) return NTT_OK;  // both directions within a quarter of free HBM
    if (int rc = ensure_full(0, nullptr)) return rc;
    if (hipDeviceSynchronize() != hipSuccess) return NTT_ERR_HIP;  // plan creation is synchronous
    use_full = true;
    return build_shoup_tables();
  }
  // The per-pass tables of one direction (the inverse's pass-1 table carries n^-1), built on `st`.
  // The forward's are built at plan creation, the inverse's at the first inverse call (a forward-only
  // plan never holds them): that build is enqueued on the call's stream ahead of its passes, with no
  // device-wide synchronisation.  If the allocation fails then, the direction keeps its two-level
  // tables (one more product per element in pass 1) instead of failing the call; at
  // creation (direction 0) the plan reports it.
  int ensure_full(int dir, hipStream_t st) {
    const bool ok = full_state[dir].ready([&] { return build_full(dir, st); });
    return (ok || dir != 0) ? NTT_OK : NTT_ERR_HIP;
  }
  bool build_full(int dir, hipStream_t st) {
    DevBuf& tab = d_fulls[dir];
    if (!tab.alloc(full_elems * TABW * 4)) return false;
    unsigned blk = log_n;
    for (unsigned i = 0; i + 1 < npass; ++i) {
      // column-group-major layout of the pass kernel's tiles (T = TILE / R columns per workgroup)
      if (launch_build_tw<E>(tab.get() + full_off[i] * TABW, 1ull << blk, r[i], tile_log_of<E>() - r[i], log_n - blk,
                             outer_lo(dir), outer_hi(dir, i), lo_bits, dir ? Fi : Ff, st) != hipSuccess) {
        // a partly built table must never be read as a built one: drop it; the
        // direction falls back to the two-level tables (the inverse) or the plan fails (creation)
        tab.reset();
        (void)hipGetLastError();
        return false;
      }
      blk -= r[i];
    }
    return true;
  }

  // Column passes whose table is small enough to stay in L2 (N_i entries of E::TW words <= 8 MiB):
  // Shoup pairs instead of w R_e, so their outer-twiddle product is a Shoup product (143 MADs)
  // instead of a Montgomery one (162).  Measured (profiles/r02_sh/): 2^24 pass 2 (5 MiB table)
  // -0.5 %, 2^28 pass 3 (1.3 MiB) -1.2 %, 2^28 pass 2 (168 MiB, not L2-resident) +6 % -- hence the cap.
  // Round 5: pass 1 too when its table fits (plans of <= 2^16 points: the four-step's 2^16-point
  // column transforms of 2^24, C4's 2^14-point rows and columns), on engines whose scratch and caller
  // layouts agree (one kernel instance reads both); the inverse's pass-1 table carries n^-1 as its
  // Montgomery twin does (knob::shoup_outer: 0 none, 1 not pass 1).
  int build_shoup_tables() {
    if constexpr (!E::SHOUP_OUTER) {
      return NTT_OK;
    } else {
      if (knob::shoup_outer() == 0) return NTT_OK;
      if (npass < 2 || !Ff.red_ok) return NTT_OK;  // the Shoup-pair column kernels are FAST instances
      constexpr size_t kMaxTableBytes = 8ull << 20;
      constexpr bool pass1_ok = E::SCRW == E::MEMW;  // pass 1 reads the caller's layout
      const unsigned i0 = (pass1_ok && knob::shoup_outer() >= 2) ? 0u : 1u;
      size_t elems = 0;
      unsigned blk = log_n;
      for (unsigned i = 0; i + 1 < npass; ++i) {
        full_sh_off[0][i] = elems;
        full_sh_ok[i] = i >= i0 && ((1ull << blk) * TW * 4) <= kMaxTableBytes;
        if (full_sh_ok[i]) elems += 1ull << blk;
        blk -= r[i];
      }
      if (elems == 0) return NTT_OK;
      size_t free_b = 0, total_b = 0;
      if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return NTT_OK;
      if (2 * elems * TW * 4 > free_b / 8) {
        for (auto& ok : full_sh_ok) ok = false;
        return NTT_OK;
      }
      if (!d_full_sh.alloc(2 * elems * TW * 4)) return NTT_ERR_HIP;
      for (int dir = 0; dir < 2; ++dir) {
        blk = log_n;
        for (unsigned i = 0; i + 1 < npass; ++i) {
          full_sh_off[dir][i] = dir * elems + full_sh_off[0][i];
          if (!full_sh_ok[i]) {
            blk -= r[i];
            continue;
          }
          if (launch_build_tw_sh<E>(d_full_sh.get() + full_sh_off[dir][i] * TW, 1ull << blk, r[i], tile_log_of<E>() - r[i],
                                    log_n - blk, outer_lo(dir), outer_hi(dir, i), lo_bits, dir ? Fi : Ff,
                                    d_tab.get() + off_pinvB, nullptr) != hipSuccess)
            return NTT_ERR_HIP;
          blk -= r[i];
        }
      }
      return hipDeviceSynchronize() == hipSuccess ? NTT_OK : NTT_ERR_HIP;
    }
  }

  // Append count entries base^k * scale (engine table format) to host; returns their word offset.
  // scaled: entries hold value * R_e (the left factor of two-level products, see encode_scaled).
  size_t push_powers_to(std::vector<uint32_t>& host, const Vec<NH>& base_m, uint64_t count, const Vec<NH>* scale_m,
                        bool scaled) const {
    const size_t off = host.size();
    Vec<NH> cur = scale_m ? *scale_m : H.r1;
    uint32_t enc[TW];
    for (uint64_t k = 0; k < count; ++k) {
      if (scaled)
        EH.encode_scaled(H.from_mont(cur), enc);
      else
        EH.encode(H.from_mont(cur), enc);
      host.insert(host.end(), enc, enc + TW);
      cur = H.mul(cur, base_m);
    }
    while (host.size() % 4) host.push_back(0);
    return off;
  }

  Vec<NH> wn_m[2];              // w_n, w_n^-1 (Montgomery form), for tables built after init
  std::vector<uint32_t> pm2_;  // p - 2 (inversion exponent)

  DevBuf d_bad;  // canonical-range check counter
  int count_noncanonical(const void* d, uint64_t count, uint64_t* bad, hipStream_t st) override {
    if (!d || !bad) return NTT_ERR_ARG;
    if (!d_bad && !d_bad.alloc(sizeof(unsigned long long))) return NTT_ERR_HIP;
    auto* cnt = d_bad.get<unsigned long long>();
    ModWords<MEMW> pw{};
    for (int i = 0; i < NH && i < MEMW; ++i) pw.w[i] = H.M.p[i];
    unsigned long long h = 0;
    if (hipMemsetAsync(cnt, 0, sizeof(h), st) != hipSuccess ||
        launch_count_noncanonical<E>(static_cast<const uint32_t*>(d), count, pw, cnt, st) != hipSuccess ||
        hipMemcpyAsync(&h, cnt, sizeof(h), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
      return NTT_ERR_HIP;
    *bad = h;
    return NTT_OK;
  }

  // ---- the features' entry points (PlanBase), each in its part
  int coset(void* d, const uint64_t* c, unsigned limbs64, bool inverse, hipStream_t st) override {
    return shift.coset(d, c, limbs64, inverse, st);
  }
  int lde(const void* in, void* out, unsigned log_blowup, const uint64_t* c, unsigned limbs64, unsigned batch,
          hipStream_t st) override {
    return shift.lde(in, out, log_blowup, c, limbs64, batch, st);
  }
  bool single_launch_ready() override { return single.ready(); }

  // the engine's fast (quotient-estimate) reduction holds for this modulus in direction F
  static bool fast(const typename E::Args& F) {
    if constexpr (E::FASTRED) return F.red_ok != 0;
    else return false;
  }

  // canonical value of the engine's Montgomery radix R_e mod p
  Vec<NH> engine_radix_mod_p() const {
    if constexpr (IsEng32<E>::value || std::is_same_v<E, Eng31>) {
      return H.r1;  // 2^(32N) mod p
    } else if constexpr (std::is_same_v<E, Eng64G>) {
      Vec<NH> one{};  // plain canonical values: no radix
      one[0] = 1;
      return one;
    } else {
      return EH.kR;  // 2^(29L) mod p
    }
  }

  int ensure_scratch(unsigned batch) { return d_scratch.grow((size_t)n * batch * SCRW * 4) ? NTT_OK : NTT_ERR_HIP; }

  // debug builds: element extents of a pass's src / dst from the transform's first element (n per
  // transform, n 2^il in Mode I); the four-step maps into the caller's exchange blocks stay unchecked
  void set_extents(PassArgs<E>& A, const FsIO* io, uint32_t il) const {
    const size_t ext = (size_t)n << il;
    A.dbg_src_n = (io && (A.fs & FS_MAP_IN)) ? ~(size_t)0 : ext;
    A.dbg_dst_n = (io && (A.fs & FS_MAP_OUT)) ? ~(size_t)0 : ext;
  }
  // a four-step piece's position maps (`bits`: which of FS_MAP_IN / FS_MAP_OUT this pass takes)
  void set_fs(PassArgs<E>& A, const FsIO* io, uint32_t il, uint32_t bits) const {
    if (!io) return;
    A.fs = io->fs & (bits | FS_IL | FS_MAP_EPI);
    A.il = il;
    A.min = io->min;
    A.mout = io->mout;
    A.mepi = io->mepi;
  }
  static int rc_of(hipError_t e) { return e == hipSuccess ? NTT_OK : NTT_ERR_HIP; }
  PassArgs<E> base_args(bool inverse) const {
    PassArgs<E> A;
    memset(&A, 0, sizeof(A));
    A.F = inverse ? Fi : Ff;
    A.log_n = log_n;
    A.lo_bits = lo_bits;
    A.batch_stride = (size_t)n * MEMW;
    A.dbg_src_n = A.dbg_dst_n = ~(size_t)0;  // debug builds: unchecked unless run_io knows the extents
    return A;
  }

  unsigned passes_for(unsigned log_x) const override {
    unsigned rr[8] = {0}, p = 0;
    if (!schedule_for<E>(log_x, rr, p)) return 99;
    return p == 0 ? 1 : p;
  }
  unsigned max_radix_for(unsigned log_x) const override {
    unsigned rr[8] = {0}, p = 0;
    if (!schedule_for<E>(log_x, rr, p)) return 99;
    unsigned m = p == 0 ? log_x : 0;
    for (unsigned i = 0; i < p; ++i) m = rr[i] > m ? rr[i] : m;
    return m;
  }

  int run(void* d, unsigned batch, bool inverse, hipStream_t st) override {
    if (!d || batch == 0 || (flags & NTT_PLAN_TWIDDLE_ONLY)) return NTT_ERR_ARG;
    if (int rc = NTT_OK; !inverse && batch == 1 && rivals.run(static_cast<uint32_t*>(d), st, rc)) return rc;
    return run_io(static_cast<uint32_t*>(d), static_cast<uint32_t*>(d), batch, inverse, st, FirstPass::plain());
  }

  // The first pass's arguments from its descriptor, for a column pass (PA[0] of pass_args) and for the
  // one pass of a single-tile transform alike (which has no outer twiddles: tw_full is unused there).
  // A table of the descriptor's own replaces the plan's; the low-degree extension's pass without one
  // falls back to the two-level tables, never to the plan's table or its Shoup pairs.
  void apply_first_pass(PassArgs<E>& A, const FirstPass& fp) const {
    A.src2 = fp.src2;
    A.tw_in = fp.at_load;
    A.tw_in_hi = fp.at_load_hi;
    if (fp.outer || fp.n_in) {
      A.tw_full = fp.outer;
      A.tw_sh = 0;
    }
    if (fp.n_in) {
      A.src_stride = fp.n_in * MEMW;
      A.dbg_src_n = fp.n_in;
    }
  }

  // The arguments of a multi-pass transform's launches: column passes 0..npass-2, then the final pass
  // (PA[npass - 1]).  The parameters are run_io's.
  void pass_args(PassArgs<E>* PA, bool inverse, bool inplace, uint32_t il, const FirstPass& fp, const FsIO* io) const {
    const int dir = inverse ? 1 : 0;
    const bool full_dir = use_full && d_fulls[dir];  // else: the two-level tables
    unsigned blk = log_n;
    for (unsigned i = 0; i + 1 < npass; ++i) {
      PassArgs<E>& A = PA[i];
      A = base_args(inverse);
      A.tw_int = d_tab.get() + off_int[dir][i];
      A.tw_lo = outer_lo(dir);
      A.tw_hi = outer_hi(dir, i);
      // pass 1 of a memory-bound engine (8-B P path) computes its outer twiddles from the
      // L2-resident two-level tables: two 32-bit products are cheaper than streaming an n-entry table (A/B: knob)
      A.tw_full = (full_dir && (i > 0 || E::PASS1_FULL_TABLE || knob::pass1_full()))
                      ? d_fulls[dir].get() + full_off[i] * TABW
                      : nullptr;
      if (d_full_sh && full_sh_ok[i] && (i > 0 || full_dir)) {
        A.tw_full = d_full_sh.get() + full_sh_off[dir][i] * TW;
        A.tw_sh = 1;
      }
      A.log_blk = blk + il;
      A.log_m = log_n - blk;
      A.src_user = (i == 0) ? 1u : 0u;
      set_fs(A, io, il, i == 0 ? FS_MAP_IN : 0u);
      blk -= r[i];
    }
    PassArgs<E>& A = PA[npass - 1];
    A = base_args(inverse);
    A.tw_int = d_tab.get() + off_int[dir][npass - 1];
    A.r1 = r[0];
    A.nmid = npass - 2;
    mid_digits(r, npass, A.mid_bits, A.mid_off);
    set_fs(A, io, il, FS_MAP_OUT);
    if (io) A.tw_epi = static_cast<const uint32_t*>(io->tw_epi);
    if (inplace) A.flags |= 2u;
    for (unsigned i = 0; i < npass; ++i) set_extents(PA[i], io, il);
    apply_first_pass(PA[0], fp);
    // XCD-grouped tile order (k_pass flag bit 2) for the column passes after the first whose runs are
    // shorter than a 128-B line (the 8-B path's 4-B scratch at radix 512: 64-B runs), so that the
    // two tiles sharing each line meet on one XCD's L2.  Passes of one column per tile (radix 4096 on
    // the 4096-element tiles) read and write 32-B runs, their final pass's stores too: every such
    // pass takes the order, so the four tiles of each 128-B line run together.  knob::xcd_order: 0 off,
    // 1 on every column pass, 3 not on the one-column passes (A/B).
    const int xcd_order = knob::xcd_order();
    if (!io && xcd_order > 0)
      for (unsigned i = 0; i < npass; ++i) {
        const unsigned cols = 1u << (tile_log_of<E>() - r[i]);
        const unsigned run_bytes = cols * SCRW * 4;
        const bool column = i + 1 < npass;
        if ((column && (xcd_order == 1 || (i > 0 && run_bytes < 128))) || (cols == 1 && xcd_order != 3))
          PA[i].flags |= 4u;
      }
  }

  // One transform (or a batch): reads `in`, writes `out` (may equal `in`); `fp` says what the first pass
  // reads besides and multiplies by (FirstPass), `io` is a four-step piece's interface (the rank plan's).
  int run_io(const uint32_t* in, uint32_t* out, unsigned batch, bool inverse, hipStream_t st, const FirstPass& fp,
             const FsIO* io = nullptr) {
    const uint32_t il = (io && (io->fs & FS_IL)) ? io->il : 0u;
    if (io && (log_n == 0 || npass == 0)) return NTT_ERR_ARG;  // four-step pieces are >= 8 points
    if (log_n == 0) {
      if (out != in && hipMemcpyAsync(out, in, (size_t)batch * MEMW * 4, hipMemcpyDeviceToDevice, st) != hipSuccess)
        return NTT_ERR_HIP;
      return NTT_OK;
    }
    const int dir = inverse ? 1 : 0;
    const bool lde = fp.n_in != 0;
    hipError_t e = hipSuccess;
    begin(st);
    if (fp.stage) {  // an interval of the call's record, unlabelled (no pass kind of its own)
      if constexpr (HasLde<E>::value) {
        if (launch_lde_scale<E>(in, fp.stage, fp.n_in, batch, fp.scale_lo, fp.scale_hi, lo_bits, Ff, st) != hipSuccess)
          return NTT_ERR_HIP;
      }
      mark(st);
      in = fp.stage;
    }
    if (npass == 0) {
      PassArgs<E> A = base_args(inverse);
      A.tw_int = d_tab.get() + off_int[dir][0];
      A.flags = inverse ? 1u : 0u;
      e = launch_naive<E>(in, out, A, batch, st);
      mark(st, "n");
    } else if (npass == 1) {
      PassArgs<E> A = base_args(inverse);
      A.tw_int = d_tab.get() + off_int[dir][0];
      A.flags = (inverse && !(io && io->no_scale)) ? 1u : 0u;  // no_scale: n^-1 folded in by the caller
      set_fs(A, io, il, FS_MAP_IN | FS_MAP_OUT);
      if (io) A.tw_epi = static_cast<const uint32_t*>(io->tw_epi);
      set_extents(A, io, il);
      if (lde) {  // low-degree extension of at most one tile: one transform per workgroup
        apply_first_pass(A, fp);
        if constexpr (HasLde<E>::value) e = launch_lde_pass<E>(KIND_SINGLE, (int)r[0], in, out, A, 1, batch, st);
        else e = hipErrorInvalidValue;
        mark(st, "s", r[0]);
        return rc_of(e);
      }
      const uint32_t nt = il ? (1u << il) : batch;  // transforms of this launch
      // KIND_ROWS: TILE / n transforms per workgroup (the final pass's block layout: wave-uniform trivial
      // twiddles, 4-wave workgroups) when the engine has it and the count divides; knob::rows off: one per
      // workgroup (KIND_SINGLE)
      const unsigned rows_log = (unsigned)tile_log_of<E>() - r[0];
      bool rows = false;
      if constexpr (HasRows<E>::value) {
        // the quotient-estimate engines run KIND_ROWS in their FAST form only
        rows = knob::rows() && (!E::FASTRED || fast(Ff)) && r[0] >= (unsigned)kRowsMinLog &&
               r[0] <= (unsigned)rows_max_log<E>() && rows_log >= 1 && nt >= (1u << rows_log) &&
               (nt & ((1u << rows_log) - 1)) == 0;
      }
      if (rows) {
        if (!il) {  // the transform index is part of every position: extents over the whole batch
          if (A.dbg_src_n != ~(size_t)0) A.dbg_src_n = (size_t)n * batch;
          if (A.dbg_dst_n != ~(size_t)0) A.dbg_dst_n = (size_t)n * batch;
        }
        e = launch_pass<E>(KIND_ROWS, (int)r[0], in, out, A, nt >> rows_log, 1, st);
      } else {
        e = launch_pass<E>(KIND_SINGLE, (int)r[0], in, out, A, 1, nt, st);
      }
      mark(st, rows ? "r" : "s", r[0]);
    } else {
      if (il) batch = 1;  // Mode I: the 2^il interleaved transforms are one long column sweep
      // NTT_PLAN_IN_PLACE (not for four-step pieces, whose passes map positions): every pass reads and
      // writes `out`'s positions, the final pass included; the digit reversal follows as tile swaps
      const bool inplace = (flags & NTT_PLAN_IN_PLACE) && !io;
      if (!inplace)
        if (int rc = ensure_scratch(il ? (1u << il) : batch)) return rc;
      uint32_t* work = inplace ? out : d_scratch.get();
      const uint32_t grid = (uint32_t)((n << il) >> tile_log_of<E>());
      if (use_full)
        if (int rc = ensure_full(dir, st)) return rc;
      // build the arguments, try the single launch, else launch the passes
      PassArgs<E> PA[8];
      pass_args(PA, inverse, inplace, il, fp, io);
      const PassArgs<E>& A = PA[npass - 1];
      if (!io && !lde && batch == 1 && single.enabled())
        if (int rc = NTT_OK; single.launch(PA, in, work, out, inplace, st, rc)) return rc;
      for (unsigned i = 0; i + 1 < npass && e == hipSuccess; ++i) {
        const uint32_t* src = (i == 0) ? in : work;
        if (i == 0 && lde) {
          if constexpr (HasLde<E>::value) e = launch_lde_pass<E>(KIND_COLUMN, (int)r[0], src, work, PA[0], grid, batch, st);
          else e = hipErrorInvalidValue;
        } else {
          e = launch_pass<E>(KIND_COLUMN, (int)r[i], src, work, PA[i], grid, batch, st);
        }
        mark(st, "c", r[i], PA[i].tw_sh != 0);
      }
      if (e == hipSuccess && inplace && batch == 1 && single.ipn_ready(A)) {
        // the final pass writes natural positions in place, the digit reversal fused (k_final_ipn)
        e = launch_final_ipn<E>((int)r[npass - 1], out, single.ipn_args(A), grid, st);
        mark(st, "i", r[npass - 1]);
      } else if (e == hipSuccess) {
        e = launch_pass<E>(KIND_FINAL, (int)r[npass - 1], work, out, A, grid, batch, st);
        mark(st, "f", r[npass - 1]);
        if (inplace && e == hipSuccess) {
          DrevArgs D{};
          D.log_n = log_n;
          D.R = r[0];
          D.tb_log = r[0] < 4 ? r[0] : 4;
          D.nmid = A.nmid;
          for (unsigned m = 0; m < A.nmid; ++m) D.mid_bits[m] = A.mid_bits[m], D.mid_off[m] = A.mid_off[m];
          D.batch_stride = (size_t)n * MEMW;
          D.diag = knob::drev_diag() ? 1u : 0u;
          e = launch_digitrev_swap<E>(out, D, batch, st);
          mark(st, "d");
        }
      }
    }
    return rc_of(e);
  }

  // bit 0: a bounded wait gave up (the watchdog report, PlanBase::h_watch); then cleared.  Blocking:
  // the device is synchronised first, so the report covers every call enqueued before.
  int device_status(unsigned* bad) override {
    *bad = 0;
    if (hipDeviceSynchronize() != hipSuccess) return NTT_ERR_HIP;
    if (tripped()) *bad |= 1u;
    clear_trip();
    if (d_dbg) {  // debug builds: NTT_DBG_* bits (engines.hpp)
      uint32_t w = 0;
      if (hipMemcpy(&w, d_dbg.get(), 4, hipMemcpyDeviceToHost) != hipSuccess) return NTT_ERR_HIP;
      if (w && hipMemset(d_dbg.get(), 0, 4) != hipSuccess) return NTT_ERR_HIP;
      *bad |= w;
    }
    return NTT_OK;
  }
  DevBuf d_dbg;  // debug builds (NTT_DEBUG_CHECKS): the kernels' check-failure bits

  // ---- distributed four-step pieces (ntt_rplan, ntt_amd/csrc/ntt_rplan.cpp)
  int run_fs(const void* in, const void* in2, void* out, unsigned batch, bool inverse, const FsIO& io,
             hipStream_t st) override {
    if (!in || !out || batch == 0 || (flags & NTT_PLAN_TWIDDLE_ONLY)) return NTT_ERR_ARG;
    auto pin = static_cast<const uint32_t*>(in), pin2 = static_cast<const uint32_t*>(in2);
    auto pout = static_cast<uint32_t*>(out);
    if (!in2) return run_io(pin, pout, batch, inverse, st, FirstPass::plain(), &io);
    if (!inverse) return NTT_ERR_ARG;  // the product is taken at the inverse's load
    const size_t count = (size_t)n * ((io.fs & FS_IL) ? (1ull << io.il) : batch);
    if (polymul_fusable() && npass >= 2) {  // in2 read through the input map like in
      if (int rc = ensure_polymul_table(st)) return rc;
      return run_io(pin, pout, batch, true, st, FirstPass::product(pin2, d_full_pm.get()), &io);
    }
    if (!(io.fs & (FS_MAP_IN | FS_MAP_OUT))) {  // same layout in and out: the product in place in out
      if (int rc = pointwise_n(pin, pin2, pout, count, st)) return rc;
      return run_io(pout, pout, batch, true, st, FirstPass::plain(), &io);
    }
    // a mapped piece (the column pieces of ntt_rplan_inverse_cols_piece): the product gathered into a
    // plan-owned buffer first (out's other pieces may still be in flight)
    if (!d_pw.grow(count * MEMW * 4)) return NTT_ERR_HIP;
    const size_t off = (flags & NTT_PLAN_MONTGOMERY_IO) ? off_rm : off_r2;
    if (launch_pointwise<E>(pin, pin2, d_pw.get(), count, Ff, d_tab.get() + off, st,
                            (io.fs & FS_MAP_IN) ? &io.min : nullptr) != hipSuccess)
      return NTT_ERR_HIP;
    FsIO io2 = io;
    io2.fs &= ~FS_MAP_IN;
    return run_io(d_pw.get(), pout, batch, true, st, FirstPass::plain(), &io2);
  }
  DevBuf d_pw;  // gathered pointwise products of mapped pieces (run_fs), on first use

  // scale_log k > 0: every entry also carries 2^-k (the four-step's row n2^-1, folded into the inverse
  // columns' epilogue so that the single-pass inverse rows need no scaling product)
  int build_fs_table(void* table, unsigned log_rows, unsigned log_cols, uint64_t row0, uint64_t col0, bool inverse,
                     unsigned scale_log, hipStream_t st) override {
    if (!table || log_rows + log_cols > 40 || scale_log > log_n) return NTT_ERR_ARG;
    const uint32_t *lo = outer_lo(inverse), *hi = outer_hi(inverse, 1);
    const uint32_t* scale = scale_log ? d_tab.get() + off_pow2inv + (size_t)scale_log * TW : nullptr;
    return rc_of(launch_build_fs_tw<E>(static_cast<uint32_t*>(table), log_rows, log_cols, row0, col0, log_n, lo, hi,
                                       lo_bits, inverse ? Fi : Ff, st, scale));
  }

  size_t table_entry_bytes() const override { return (size_t)TABW * 4; }

  // Fused polymul is available for multi-pass FAST plans with full outer-twiddle tables.
  bool polymul_fusable() const { return use_full && npass >= 2 && fast(Fi) && !(flags & NTT_PLAN_MONTGOMERY_IO); }
  // Inverse pass-1 outer-twiddle table scaled by n^-1 R_e (built on first use, same layout as d_full).
  // Built on the call's stream ahead of the passes that read it (no device-wide synchronisation).
  int ensure_polymul_table(hipStream_t st) {
    if (d_full_pm) return NTT_OK;
    const size_t elems = 1ull << log_n;
    if (!d_full_pm.alloc(elems * TABW * 4)) return NTT_ERR_HIP;
    if (launch_build_tw<E>(d_full_pm.get(), elems, r[0], tile_log_of<E>() - r[0], 0, outer_lo(1),
                           d_tab.get() + off_hi_ipm, lo_bits, Fi, st) != hipSuccess) {
      d_full_pm.reset();  // never leave a partly built table behind as if it were built
      return NTT_ERR_HIP;
    }
    return NTT_OK;
  }

  // c = a * b (cyclic convolution of length n): forward(a), forward(b) in place, then the inverse of
  // their pointwise product into c.  Fused: the inverse's first pass reads both transforms and
  // multiplies at load (one HBM pass and one kernel fewer than forward / pointwise / inverse).
  int polymul(void* a, void* b, void* c, hipStream_t st) override {
    if (!a || !b || !c || (flags & NTT_PLAN_TWIDDLE_ONLY)) return NTT_ERR_ARG;
    uint32_t *pa = static_cast<uint32_t*>(a), *pb = static_cast<uint32_t*>(b);
    if (int rc = run_io(pa, pa, 1, false, st, FirstPass::plain())) return rc;
    if (pb != pa)  // squaring (a == b): one forward transform, then the product of it with itself
      if (int rc = run_io(pb, pb, 1, false, st, FirstPass::plain())) return rc;
    return inverse_pointwise(pa, pb, c, 1, st);
  }

  // c = INTT(a * b) over `batch` transforms (the polymul's second half; a, b forward transforms).
  // Fused: the inverse's first pass reads both transforms and multiplies at load (one HBM pass and
  // one kernel fewer than pointwise + inverse).  c may alias a or b.
  int inverse_pointwise(const void* a, const void* b, void* c, unsigned batch, hipStream_t st) override {
    if (!a || !b || !c || batch == 0 || (flags & NTT_PLAN_TWIDDLE_ONLY)) return NTT_ERR_ARG;
    auto pa = static_cast<const uint32_t*>(a), pb = static_cast<const uint32_t*>(b);
    auto pc = static_cast<uint32_t*>(c);
    if (polymul_fusable()) {
      if (int rc = ensure_polymul_table(st)) return rc;
      return run_io(pa, pc, batch, true, st, FirstPass::product(pb, d_full_pm.get()));
    }
    if (int rc = pointwise_n(pa, pb, pc, (size_t)n * batch, st)) return rc;
    return run_io(pc, pc, batch, true, st, FirstPass::plain());
  }

  int pointwise_n(const uint32_t* a, const uint32_t* b, uint32_t* c, size_t count, hipStream_t st) {
    const size_t off = (flags & NTT_PLAN_MONTGOMERY_IO) ? off_rm : off_r2;
    return launch_pointwise<E>(a, b, c, count, Ff, d_tab.get() + off, st) == hipSuccess ? NTT_OK : NTT_ERR_HIP;
  }

  int pointwise(const void* a, const void* b, void* c, hipStream_t st) override {
    if (!a || !b || !c) return NTT_ERR_ARG;
    return pointwise_n(static_cast<const uint32_t*>(a), static_cast<const uint32_t*>(b), static_cast<uint32_t*>(c), n,
                       st);
  }

  int fill(void* d, uint64_t count, int kind, uint64_t seed, uint64_t row0, unsigned log_inner, unsigned log_stride,
           hipStream_t st) override {
    if (!d || (kind != 0 && kind != 1)) return NTT_ERR_ARG;
    return rc_of(launch_fill<E>(kind, static_cast<uint32_t*>(d), count, seed, nrand, top_bits, row0, log_inner,
                                  log_stride, st));
  }

  int twiddle_pack(const void* src, void* dst, unsigned log_rows, unsigned log_len, unsigned log_bw, uint64_t row0,
                   bool inverse, uint64_t peer_stride, hipStream_t st) override {
    if (!src || !dst || src == dst || log_bw > log_len || log_rows + log_len > 40) return NTT_ERR_ARG;
    if (peer_stride < (1ull << (log_rows + log_bw))) return NTT_ERR_ARG;  // peer chunks must not overlap
    const uint32_t *lo = outer_lo(inverse), *hi = outer_hi(inverse, 1);
    return rc_of(launch_twiddle_pack<E>(static_cast<const uint32_t*>(src), static_cast<uint32_t*>(dst), log_rows,
                                          log_len, log_bw, row0, log_n, lo, hi, lo_bits, inverse ? Fi : Ff,
                                          peer_stride, st));
  }

  int transpose(const void* src, void* dst, unsigned log_rows, unsigned log_cols, unsigned log_blk_rows,
                uint64_t blk_stride, hipStream_t st) override {
    if (!src || !dst || src == dst || log_rows + log_cols > 40 || log_blk_rows > log_rows) return NTT_ERR_ARG;
    if (blk_stride < (1ull << (log_blk_rows + log_cols))) return NTT_ERR_ARG;
    return rc_of(launch_transpose<E>(static_cast<const uint32_t*>(src), static_cast<uint32_t*>(dst), log_rows,
                                       log_cols, log_blk_rows, blk_stride, st));
  }
};

// ------------------------------------------------------------------------------ built-in fields
struct FieldDef {
  uint64_t p[4];
  uint64_t g;
};
static const FieldDef kFields[6] = {
    {{469762049ull, 0, 0, 0}, 3},
    {{0x43e1f593f0000001ull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull}, 5},
    {{0xffffffff00000001ull, 0x53bda402fffe5bfeull, 0x3339d80809a1d805ull, 0x73eda753299d7d48ull}, 7},
    {{kGoldilocksP, 0, 0, 0}, 7},
    {{0x78000001ull, 0, 0, 0}, 31},  // BabyBear, 2^31 - 2^27 + 1
    {{0x7f000001ull, 0, 0, 0}, 3},   // KoalaBear, 2^31 - 2^24 + 1
};

// modulus and generator as 32-bit words, the form PlanImpl::init takes
static void split_limbs(uint32_t* p32, uint32_t* g32, const uint64_t* p64, const uint64_t* g64, unsigned limbs64) {
  for (unsigned i = 0; i < limbs64; ++i) {
    p32[2 * i] = (uint32_t)p64[i];
    p32[2 * i + 1] = (uint32_t)(p64[i] >> 32);
    g32[2 * i] = (uint32_t)g64[i];
    g32[2 * i + 1] = (uint32_t)(g64[i] >> 32);
  }
}
// a plan of engine E into `out`; nothing is kept of one whose creation failed
template <class E>
static int make_impl(std::unique_ptr<PlanBase>& out, const uint32_t* p32, const uint32_t* g32, unsigned log_n,
                     int device, unsigned flags) {
  auto impl = std::make_unique<PlanImpl<E>>();
  const int rc = impl->init(p32, g32, log_n, device, flags);
  if (rc == NTT_OK) out = std::move(impl);
  return rc;
}

static int make_plan(std::unique_ptr<PlanBase>& out, const uint64_t* p64, const uint64_t* g64, unsigned limbs64,
                     unsigned log_n, int device, unsigned flags) {
  if (log_n > 40) return NTT_ERR_ARG;
  if (limbs64 != 1 && limbs64 != 4 && limbs64 != 6) return NTT_ERR_ARG;  // before packing into p32[12] / g32[12]
  const unsigned rivals = flags & kRivalFlags;
  if (rivals & (rivals - 1)) return NTT_ERR_ARG;  // one rival schedule per plan
  if ((flags & NTT_PLAN_IN_PLACE) && (rivals || (flags & NTT_PLAN_TWIDDLE_ONLY)))
    return NTT_ERR_ARG;
  // NTT_PLAN_ELEM32 (4-B elements, Eng31): one limb, a modulus below 2^31, the default schedule only
  const bool elem32 = (flags & NTT_PLAN_ELEM32) != 0;
  if (elem32) {
    if (limbs64 != 1 || rivals || (flags & NTT_PLAN_IN_PLACE)) return NTT_ERR_ARG;
    if (!f31::modulus_ok(p64[0])) return NTT_ERR_FIELD;
  }
  // Goldilocks (8-B elements, Eng64G): the default schedule only
  const bool goldilocks = limbs64 == 1 && p64[0] == kGoldilocksP;
  if (goldilocks && (rivals || (flags & (NTT_PLAN_IN_PLACE | NTT_PLAN_MONTGOMERY_IO)))) return NTT_ERR_ARG;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return NTT_ERR_NODEV;
  if (device < 0 || device >= ndev) return NTT_ERR_ARG;
  uint32_t p32[12] = {0}, g32[12] = {0};
  split_limbs(p32, g32, p64, g64, limbs64);
  if (elem32) return make_impl<Eng31>(out, p32, g32, log_n, device, flags);
  if (goldilocks) return make_impl<Eng64G>(out, p32, g32, log_n, device, flags);
  const bool inplace = (flags & NTT_PLAN_IN_PLACE) != 0;
  if (limbs64 == 1) {
    if (p64[0] >= (1ull << 31)) return NTT_ERR_FIELD;  // `long long` path: 31-bit primes
    // in place needs 8-B scratch elements (the caller's layout)
    return inplace ? make_impl<EngPI>(out, p32, g32, log_n, device, flags)
                   : make_impl<EngP>(out, p32, g32, log_n, device, flags);
  }
  if (limbs64 == 4) return make_impl<Eng256>(out, p32, g32, log_n, device, flags);
  // the 384-bit element layout: 256-bit arithmetic when the modulus allows it (BN254 Fr, BLS12-381 Fr:
  // the upper two 64-bit limbs of every element are zero), 14 limbs otherwise.  In place: the
  // intermediates live in the caller's 48-B elements (no 32-B plan scratch)
  if (p64[4] != 0 || p64[5] != 0 || (p64[3] >> 63) != 0) return make_impl<Eng384>(out, p32, g32, log_n, device, flags);
  return inplace ? make_impl<Eng256wI>(out, p32, g32, log_n, device, flags)
                 : make_impl<Eng256w>(out, p32, g32, log_n, device, flags);
}

// BASELINE config 2 (2^20, 4 x 64-bit limbs): a single transform runs fastest on 4096-element tiles,
// one 1024-thread workgroup per CU, in two passes (10 + 10) instead of three (7 + 7 + 6): 0.105
// against 0.114 ms (BN254), 0.102 against 0.108 (BLS12-381), DESIGN §4.  Batched calls keep the
// 1024-element tiles, which overlap the batch's transforms better (batch 4: 0.082 against 0.091 ms
// per transform).  So a default 4-limb plan of 2^20 holds a second plan of 4096-element tiles for
// one vector's transforms (forward, inverse, coset, polymul); knob::wide_tiles off: none.
// The second plan is an optimisation: when it cannot be built the plan runs alone, and nothing of the
// failure may leak into the plan's calls.  A failed hipMalloc inside its init leaves the error as the
// thread's last HIP error, which the next launch check (hipGetLastError) would return as NTT_ERR_HIP
// from a healthy plan, so it is cleared here.  It is not attempted at all when the
// device is short of memory (its scratch and tables take ~100 MiB at 2^20).  In the checked build
// (NTT_DEBUG_CHECKS, libntt_debug.so) only, NTT_TEST_WIDE_FAIL=1 makes the attempt fail through a
// refused allocation (tests/test_gpu_wide_tiles.py); the product build has no such hook.
static constexpr size_t kWideMinFreeBytes = 512ull << 20;
// NTT_PLAN_SINGLE_LAUNCH plans (BASELINE config 2's "single-kernel" form) get the second plan too:
// their batch-1 transforms are then ONE launch of the two passes (k_fused2b; in place k_fused2bi),
// and the second plan is kept only if that single launch is available (single_launch_ready).  An
// in-place single-launch plan sends only its plain forward / inverse there (wide_transforms_only).
static bool wide_flags_ok(unsigned flags) {
  const unsigned f = flags & ~NTT_PLAN_MONTGOMERY_IO;
  return f == 0 || f == NTT_PLAN_SINGLE_LAUNCH || f == (NTT_PLAN_SINGLE_LAUNCH | NTT_PLAN_IN_PLACE);
}
// 2^24 (the headline) on the same tiles in two passes, 12 + 12 with one column per column-pass tile:
// one HBM round trip of the vector fewer than 8 + 8 + 8 on the 1024-element tiles.
// knob::two_pass_24 routes a default 2^24 4-limb plan's single-vector transforms there.
static void make_wide_plan(std::unique_ptr<PlanBase>& out, const uint64_t* p64, const uint64_t* g64,
                           unsigned limbs64, unsigned log_n, int device, unsigned flags) {
  if (limbs64 != 4 || !wide_flags_ok(flags) || !knob::wide_tiles()) return;
  if (log_n == 24) {
    if (!knob::two_pass_24() || (flags & ~NTT_PLAN_MONTGOMERY_IO)) return;
  } else if (log_n != 20) {
    return;
  }
  if ((flags & NTT_PLAN_IN_PLACE) && (flags & NTT_PLAN_MONTGOMERY_IO)) return;
  uint32_t p32[12] = {0}, g32[12] = {0};
  split_limbs(p32, g32, p64, g64, 4);
  int cur = 0;
  (void)hipGetDevice(&cur);
  if (cur != device) (void)hipSetDevice(device);
  size_t free_b = 0, total_b = 0;
  const bool room = hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b >= kWideMinFreeBytes;
  if (room) {
    if (knob::test_wide_fail()) {  // checked build only
      void* p = nullptr;
      if (hipMalloc(&p, ~(size_t)0 >> 4) == hipSuccess) (void)hipFree(p);  // refused: the sticky error
    } else {
      std::unique_ptr<PlanBase> impl;
      if (make_impl<Eng256T>(impl, p32, g32, log_n, device, flags) == NTT_OK &&
          (!(flags & NTT_PLAN_SINGLE_LAUNCH) || impl->single_launch_ready()))
        out = std::move(impl);
    }
  }
  if (!out) (void)hipGetLastError();  // the plan runs alone, with a clean error state
  if (cur != device) (void)hipSetDevice(cur);
}

static int set_err(int rc) {
  g_last_error = rc;
  return rc;
}

}  // namespace

struct ntt_plan {
  std::unique_ptr<PlanBase> impl;
  std::unique_ptr<PlanBase> wide;  // one vector's transforms of a 2^20 4-limb plan (make_wide_plan)
  PlanBase* last = nullptr;        // the plan that ran the latest transform (ntt_plan_last_launch_ms)
  // In-place single-launch plans: the second plan runs the plain forward / inverse only (its
  // k_fused2bi); polymul, cosets and the fused pointwise inverse stay on the 1024-element tiles.
  bool wide_transforms_only() const {
    return wide && (wide->flags & NTT_PLAN_IN_PLACE) && (wide->flags & NTT_PLAN_SINGLE_LAUNCH);
  }
  // The plan that transforms `batch` vectors (plain forward / inverse: transform = true), remembered
  // for the profiling readers.
  PlanBase& exec(unsigned batch, bool transform = false) {
    last = (wide && batch == 1 && (transform || !wide_transforms_only())) ? wide.get() : impl.get();
    return *last;
  }
};

extern "C" {

static int create_plan(ntt_plan** out, const uint64_t* modulus, const uint64_t* generator, unsigned limbs64,
                       unsigned log_n, int device, unsigned flags, bool allow_wide) {
  if (!out || !modulus || !generator) return set_err(NTT_ERR_ARG);
  *out = nullptr;
  std::unique_ptr<PlanBase> impl;
  int rc = make_plan(impl, modulus, generator, limbs64, log_n, device, flags);
  if (rc != NTT_OK) return set_err(rc);
  std::unique_ptr<PlanBase> wide;
  if (allow_wide) make_wide_plan(wide, modulus, generator, limbs64, log_n, device, flags);
  *out = new ntt_plan{std::move(impl), std::move(wide)};
  return set_err(NTT_OK);
}

int ntt_plan_create_custom_ex(ntt_plan** out, const uint64_t* modulus, const uint64_t* generator, unsigned limbs64,
                              unsigned log_n, int device, unsigned flags) {
  return create_plan(out, modulus, generator, limbs64, log_n, device, flags, true);
}

int ntt_plan_create_custom(ntt_plan** out, const uint64_t* modulus, const uint64_t* generator, unsigned limbs64,
                           unsigned log_n, int device) {
  return ntt_plan_create_custom_ex(out, modulus, generator, limbs64, log_n, device, 0);
}

int ntt_plan_create(ntt_plan** out, int field_id, unsigned log_n, unsigned limbs64, int device) {
  return ntt_plan_create_ex(out, field_id, log_n, limbs64, device, 0);
}

static int create_field_plan(ntt_plan** out, int field_id, unsigned log_n, unsigned limbs64, int device,
                             unsigned flags, bool allow_wide) {
  if (field_id < 0 || field_id > 5) return set_err(NTT_ERR_ARG);
  if (limbs64 != 1 && limbs64 != 4 && limbs64 != 6) return set_err(NTT_ERR_ARG);
  const bool field31 = field_id == NTT_FIELD_BABYBEAR || field_id == NTT_FIELD_KOALABEAR;
  if (limbs64 == 1 && field_id != NTT_FIELD_P469762049 && field_id != NTT_FIELD_GOLDILOCKS && !field31)
    return set_err(NTT_ERR_ARG);
  if (field_id == NTT_FIELD_GOLDILOCKS && limbs64 != 1) return set_err(NTT_ERR_ARG);  // 8-byte elements only
  if (field31 && limbs64 != 1) return set_err(NTT_ERR_ARG);                            // 4-byte elements only
  if (field31) flags |= NTT_PLAN_ELEM32;  // implied
  else if (flags & NTT_PLAN_ELEM32) return set_err(NTT_ERR_ARG);  // fields 0-3 keep their element layouts
  const FieldDef& F = kFields[field_id];
  uint64_t p[6] = {0}, g[6] = {0};
  for (unsigned i = 0; i < limbs64 && i < 4; ++i) p[i] = F.p[i];
  g[0] = F.g;
  return create_plan(out, p, g, limbs64, log_n, device, flags, allow_wide);
}

int ntt_plan_create_ex(ntt_plan** out, int field_id, unsigned log_n, unsigned limbs64, int device, unsigned flags) {
  return create_field_plan(out, field_id, log_n, limbs64, device, flags, true);
}

// Every entry point that launches work runs it on the plan's device (saved and restored around
// the call), so a caller whose current device differs still gets the right one.  A plan whose
// watchdog has tripped (PlanBase::h_watch) refuses work with NTT_ERR_DEVICE until
// ntt_plan_device_status clears the report.
extern "C++" template <class F>
static int on_device(ntt_plan* plan, F&& f, bool check_watchdog = true) {
  if (!plan || !plan->impl) return set_err(NTT_ERR_ARG);
  if (check_watchdog && (plan->impl->tripped() || (plan->wide && plan->wide->tripped())))
    return set_err(NTT_ERR_DEVICE);
  int cur = 0;
  (void)hipGetDevice(&cur);
  if (cur != plan->impl->device) (void)hipSetDevice(plan->impl->device);
  const int rc = f(*plan->impl);
  if (cur != plan->impl->device) (void)hipSetDevice(cur);
  return set_err(rc);
}

extern "C++" inline hipStream_t S(void* s) { return static_cast<hipStream_t>(s); }

int ntt_forward(ntt_plan* plan, void* d, void* s) {
  return on_device(plan, [&](PlanBase&) { return plan->exec(1, true).run(d, 1, false, S(s)); });
}
int ntt_inverse(ntt_plan* plan, void* d, void* s) {
  return on_device(plan, [&](PlanBase&) { return plan->exec(1, true).run(d, 1, true, S(s)); });
}
int ntt_forward_batch(ntt_plan* plan, void* d, unsigned b, void* s) {
  return on_device(plan, [&](PlanBase&) { return plan->exec(b, true).run(d, b, false, S(s)); });
}
int ntt_inverse_batch(ntt_plan* plan, void* d, unsigned b, void* s) {
  return on_device(plan, [&](PlanBase&) { return plan->exec(b, true).run(d, b, true, S(s)); });
}

static int run_coset(ntt_plan* plan, void* d, const uint64_t* shift, bool inv, void* s) {
  return on_device(plan, [&](PlanBase&) {
    PlanBase& P = plan->exec(1);
    const unsigned limbs64 = P.elem_bytes >= 32 ? P.elem_bytes / 8 : 1;
    return P.coset(d, shift, limbs64, inv, S(s));
  });
}
int ntt_forward_coset(ntt_plan* plan, void* d, const uint64_t* shift, void* s) { return run_coset(plan, d, shift, false, s); }
int ntt_inverse_coset(ntt_plan* plan, void* d, const uint64_t* shift, void* s) { return run_coset(plan, d, shift, true, s); }

// The plan's own engine on its default schedule (never the second plan of 4096-element tiles)
int ntt_lde_batch(ntt_plan* plan, const void* d_in, void* d_out, unsigned log_blowup, const uint64_t* shift,
                  unsigned batch, void* s) {
  return on_device(plan, [&](PlanBase& P) {
    plan->last = &P;
    const unsigned limbs64 = P.elem_bytes >= 32 ? P.elem_bytes / 8 : 1;
    return P.lde(d_in, d_out, log_blowup, shift, limbs64, batch, S(s));
  });
}

// The prover-stage calls run on the plan's own engine (never the second plan of 4096-element tiles), through its
// Prover: f(X) with X the plan's Prover<E, PlanImpl<E>>; NTT_ERR_ARG from a plan whose engine has none.
// A launching call, on the plan's device like every other and remembered for the profiling readers ...
extern "C++" template <class F>
static int on_prover(ntt_plan* plan, F&& f, bool launches = true) {
  return on_device(plan, [&](PlanBase& P) {
    if (launches) plan->last = &P;
    return ProverEngines::visit(P, f);
  });
}
// ... and a question about a shape: no device is touched, ntt_last_error stays as it is
extern "C++" template <class F>
static int prover_info(const ntt_plan* plan, F&& f) {
  if (!plan || !plan->impl) return NTT_ERR_ARG;
  return ProverEngines::visit(*plan->impl, f);
}

// Row-major matrix transforms, on the matrix schedule
static int run_matrix(ntt_plan* plan, const void* in, void* out, unsigned width, bool inverse, bool is_lde,
                      unsigned log_blowup, const uint64_t* shift, unsigned order, void* s) {
  return on_prover(plan, [&](auto& X) { return X.mat.run(in, out, width, inverse, is_lde, log_blowup, shift, 1, order, S(s)); });
}
int ntt_forward_matrix(ntt_plan* plan, void* d, unsigned width, void* s) {
  return run_matrix(plan, d, d, width, false, false, 0, nullptr, 0, s);
}
int ntt_inverse_matrix(ntt_plan* plan, void* d, unsigned width, void* s) {
  return run_matrix(plan, d, d, width, true, false, 0, nullptr, 0, s);
}
int ntt_lde_matrix(ntt_plan* plan, const void* d_in, void* d_out, unsigned log_blowup, const uint64_t* shift,
                   unsigned width, void* s) {
  return run_matrix(plan, d_in, d_out, width, false, true, log_blowup, shift, 0, s);
}
// ... on a coset and / or with the rows of the evaluations in bit-reversed order
int ntt_forward_matrix_ex(ntt_plan* plan, void* d, unsigned width, const uint64_t* shift, unsigned order, void* s) {
  return run_matrix(plan, d, d, width, false, false, 0, shift, order, s);
}
int ntt_inverse_matrix_ex(ntt_plan* plan, void* d, unsigned width, const uint64_t* shift, unsigned order, void* s) {
  return run_matrix(plan, d, d, width, true, false, 0, shift, order, s);
}
int ntt_lde_matrix_ex(ntt_plan* plan, const void* d_in, void* d_out, unsigned log_blowup, const uint64_t* shift,
                      unsigned width, unsigned order, void* s) {
  return run_matrix(plan, d_in, d_out, width, false, true, log_blowup, shift, order, s);
}
int ntt_plan_matrix_info(const ntt_plan* plan, unsigned width, unsigned* npasses, unsigned radix_log[8]) {
  return prover_info(plan, [&](auto& X) { return X.mat.info(width, npasses, radix_log); });
}
// FRI fold: one launch
int ntt_fri_fold(ntt_plan* plan, const void* d_in, void* d_out, unsigned log_rows, unsigned log_arity,
                 unsigned ext_degree, uint64_t ext_w, const uint64_t* beta, const uint64_t* shift, void* s) {
  return on_prover(plan, [&](auto& X) {
    return X.fold.run(d_in, d_out, log_rows, log_arity, ext_degree, ext_w, beta, shift, S(s));
  });
}
// DEEP openings and quotients
int ntt_deep_points(ntt_plan* plan, void* d_inv, unsigned log_rows, unsigned ext_degree, uint64_t ext_w,
                    const uint64_t* z, const uint64_t* shift, unsigned order, void* s) {
  return on_prover(plan, [&](auto& X) { return X.deep.points(d_inv, log_rows, ext_degree, ext_w, z, shift, order, S(s)); });
}
int ntt_matrix_open(ntt_plan* plan, const void* d_mat, unsigned width, unsigned log_rows, const void* d_inv,
                    unsigned ext_degree, uint64_t ext_w, const uint64_t* z, const uint64_t* shift, unsigned order,
                    void* d_values, void* s) {
  return on_prover(plan, [&](auto& X) {
    return X.deep.open(d_mat, width, log_rows, d_inv, ext_degree, ext_w, z, shift, order, d_values, S(s));
  });
}
int ntt_deep_quotient(ntt_plan* plan, const void* d_mat, unsigned width, unsigned log_rows, const void* d_inv,
                      const void* d_values, unsigned ext_degree, uint64_t ext_w, const uint64_t* alpha,
                      const uint64_t* scale, unsigned flags, void* d_out, void* s) {
  return on_prover(plan, [&](auto& X) {
    return X.deep.quotient(d_mat, width, log_rows, d_inv, d_values, ext_degree, ext_w, alpha, scale, flags, d_out, S(s));
  });
}
int ntt_deep_info(const ntt_plan* plan, unsigned width, unsigned log_rows, unsigned ext_degree, unsigned* open_row_chunks,
                  unsigned* quotient_lanes_per_row) {
  return prover_info(plan, [&](auto& X) {
    return X.deep.info(width, log_rows, ext_degree, open_row_chunks, quotient_lanes_per_row);
  });
}
// Poseidon2 Merkle commitments and openings; setting the parameters launches nothing
int ntt_plan_set_poseidon2(ntt_plan* plan, unsigned width, unsigned sbox_degree, unsigned rounds_f, unsigned rounds_p,
                           const uint64_t* ext_rc, const uint64_t* int_rc, const uint64_t* int_diag) {
  return on_prover(plan, [&](auto& X) {
    return X.hash.set(width, sbox_degree, rounds_f, rounds_p, ext_rc, int_rc, int_diag);
  }, false);
}
int ntt_poseidon2_permute(ntt_plan* plan, void* d_states, uint64_t count, void* s) {
  return on_prover(plan, [&](auto& X) { return X.hash.permute(d_states, count, S(s)); });
}
int ntt_merkle_commit(ntt_plan* plan, const void* d_mat, unsigned width, unsigned log_rows, void* d_tree, void* s) {
  return on_prover(plan, [&](auto& X) { return X.hash.commit(d_mat, width, log_rows, d_tree, S(s)); });
}
int ntt_merkle_open(ntt_plan* plan, const void* d_mat, unsigned width, unsigned log_rows, const void* d_tree,
                    const uint32_t* d_index, unsigned nq, void* d_rows, void* d_paths, void* s) {
  return on_prover(plan, [&](auto& X) {
    return X.hash.open(d_mat, width, log_rows, d_tree, d_index, nq, d_rows, d_paths, S(s));
  });
}
int ntt_merkle_info(const ntt_plan* plan, unsigned width, unsigned log_rows, unsigned* digest_elems, uint64_t* tree_elems,
                    unsigned* launches, unsigned* tail_log) {
  return prover_info(plan, [&](auto& X) { return X.hash.info(width, log_rows, digest_elems, tree_elems, launches, tail_log); });
}
// Batch inversion and running sums / products
int ntt_batch_inverse(ntt_plan* plan, const void* d_in, void* d_out, uint64_t count, unsigned ext_degree, uint64_t ext_w,
                      void* s) {
  return on_prover(plan, [&](auto& X) { return X.scan.inverse(d_in, d_out, count, ext_degree, ext_w, S(s)); });
}
int ntt_matrix_scan(ntt_plan* plan, const void* d_in, void* d_out, uint64_t rows, unsigned width, unsigned ext_degree,
                    uint64_t ext_w, unsigned op, unsigned flags, void* d_totals, void* s) {
  return on_prover(plan, [&](auto& X) {
    return X.scan.scan(d_in, d_out, rows, width, ext_degree, ext_w, op, flags, d_totals, S(s));
  });
}
int ntt_scan_info(const ntt_plan* plan, uint64_t rows, unsigned width, unsigned ext_degree, unsigned op,
                  unsigned* strip_cols, unsigned* run_rows, unsigned* chunk_rows, unsigned* chunks, unsigned* launches) {
  return prover_info(plan, [&](auto& X) {
    return X.scan.info(rows, width, ext_degree, op, strip_cols, run_rows, chunk_rows, chunks, launches);
  });
}

int ntt_pointwise_mul(ntt_plan* plan, const void* a, const void* b, void* c, void* s) {
  return on_device(plan, [&](PlanBase& P) { return P.pointwise(a, b, c, S(s)); });
}

int ntt_count_noncanonical(ntt_plan* plan, const void* d, uint64_t count, uint64_t* bad, void* s) {
  return on_device(plan, [&](PlanBase& P) { return P.count_noncanonical(d, count, bad, S(s)); });
}

int ntt_plan_device_status(ntt_plan* plan, unsigned* bad) {
  if (!bad) return set_err(NTT_ERR_ARG);
  return on_device(plan, [&](PlanBase& P) {
    int rc = P.device_status(bad);
    unsigned b2 = 0;
    if (rc == NTT_OK && plan->wide && (rc = plan->wide->device_status(&b2)) == NTT_OK) *bad |= b2;
    return rc;
  }, false);
}

int ntt_plan_set_watchdog(ntt_plan* plan, unsigned spins) {
  if (!plan || !plan->impl) return set_err(NTT_ERR_ARG);
  plan->impl->wd_spins = spins;
  if (plan->wide) plan->wide->wd_spins = spins;
  return set_err(NTT_OK);
}

int ntt_polymul(ntt_plan* plan, void* a, void* b, void* c, void* s) {
  return on_device(plan, [&](PlanBase&) { return plan->exec(1).polymul(a, b, c, S(s)); });
}

int ntt_inverse_pointwise_batch(ntt_plan* plan, const void* a, const void* b, void* c, unsigned batch, void* s) {
  return on_device(plan, [&](PlanBase&) { return plan->exec(batch).inverse_pointwise(a, b, c, batch, S(s)); });
}

int ntt_fill(ntt_plan* plan, void* d, int kind, uint64_t seed, void* s) {
  return on_device(plan, [&](PlanBase& P) { return P.fill(d, P.n, kind, seed, 0, 64, 0, S(s)); });
}

int ntt_fill_map(ntt_plan* plan, void* d, uint64_t count, int kind, uint64_t seed, uint64_t row0, unsigned log_inner,
                 unsigned log_stride, void* s) {
  return on_device(plan, [&](PlanBase& P) { return P.fill(d, count, kind, seed, row0, log_inner, log_stride, S(s)); });
}

int ntt_twiddle_pack(ntt_plan* plan, const void* src, void* dst, unsigned log_rows, unsigned log_row_len,
                     unsigned log_block, uint64_t row0, int inverse, void* s) {
  return ntt_twiddle_pack_ex(plan, src, dst, log_rows, log_row_len, log_block, row0, inverse,
                             1ull << (log_rows + log_block), s);
}

int ntt_twiddle_pack_ex(ntt_plan* plan, const void* src, void* dst, unsigned log_rows, unsigned log_row_len,
                        unsigned log_block, uint64_t row0, int inverse, uint64_t peer_stride, void* s) {
  if (log_rows + log_block >= 64) return set_err(NTT_ERR_ARG);
  return on_device(plan, [&](PlanBase& P) {
    return P.twiddle_pack(src, dst, log_rows, log_row_len, log_block, row0, inverse != 0, peer_stride, S(s));
  });
}

int ntt_transpose(ntt_plan* plan, const void* src, void* dst, unsigned log_rows, unsigned log_cols, void* s) {
  return ntt_transpose_ex(plan, src, dst, log_rows, log_cols, log_rows, 1ull << (log_rows + log_cols), s);
}

int ntt_transpose_ex(ntt_plan* plan, const void* src, void* dst, unsigned log_rows, unsigned log_cols,
                     unsigned log_block_rows, uint64_t block_stride, void* s) {
  if (log_rows + log_cols >= 64) return set_err(NTT_ERR_ARG);
  return on_device(plan, [&](PlanBase& P) {
    return P.transpose(src, dst, log_rows, log_cols, log_block_rows, block_stride, S(s));
  });
}

int ntt_plan_info(const ntt_plan* plan, uint64_t* n, unsigned* elem_bytes, unsigned* npasses, unsigned radix_log[8]) {
  if (!plan || !plan->impl) return NTT_ERR_ARG;
  const PlanBase& P = plan->wide ? *plan->wide : *plan->impl;  // one vector's schedule
  if (n) *n = P.n;
  if (elem_bytes) *elem_bytes = P.elem_bytes;
  if (npasses) *npasses = P.npass;
  if (radix_log)
    for (int i = 0; i < 8; ++i) radix_log[i] = P.r[i];
  return NTT_OK;
}

static int set_profiling(PlanBase& P, int enable) {
  if (enable && !P.ev[0][0]) {
    int cur = 0;
    (void)hipGetDevice(&cur);
    (void)hipSetDevice(P.device);
    for (auto& row : P.ev)
      for (auto& e : row)
        if (hipEventCreate(&e) != hipSuccess) { (void)hipSetDevice(cur); return NTT_ERR_HIP; }
    (void)hipSetDevice(cur);
  }
  P.profiling = enable != 0;
  P.nrec = 0;
  P.ev_used = 0;
  return NTT_OK;
}

// Group mode (PlanBase::begin): the next transform on the plan starts a new slot, the later ones
// continue it until the next call.
int ntt_plan_profile_group(ntt_plan* plan) {
  if (!plan || !plan->impl) return set_err(NTT_ERR_ARG);
  for (PlanBase* P : {plan->impl.get(), plan->wide.get()})
    if (P) P->grouped = P->group_new = true;
  return set_err(NTT_OK);
}

// Labels of the launches of the latest recorded transform (or group), comma-separated, in launch
// order: the same intervals as ntt_plan_last_launch_ms.
int ntt_plan_last_launch_labels(ntt_plan* plan, char* buf, unsigned cap) {
  if (!plan || !plan->impl || !buf || cap == 0) return set_err(NTT_ERR_ARG);
  PlanBase& P = plan->last ? *plan->last : *plan->impl;
  std::string out;
  for (unsigned i = 1; i < P.ev_used && P.nrec; ++i) {
    const char* l = P.lab[P.slot][i];
    if (l[0] == '-' && l[1] == 0) continue;
    if (!out.empty()) out += ',';
    out += l;
  }
  if (out.size() + 1 > cap) return set_err(NTT_ERR_ARG);
  memcpy(buf, out.c_str(), out.size() + 1);
  return set_err(NTT_OK);
}

int ntt_plan_set_profiling(ntt_plan* plan, int enable) {
  if (!plan || !plan->impl) return set_err(NTT_ERR_ARG);
  int rc = set_profiling(*plan->impl, enable);
  if (rc == NTT_OK && plan->wide) rc = set_profiling(*plan->wide, enable);
  return set_err(rc);
}

// Average per-launch durations over the transforms recorded since profiling was enabled (at most
// the last 64); waits for the most recent one.
int ntt_plan_last_launch_ms(ntt_plan* plan, float* ms, unsigned max_launches, unsigned* nlaunches) {
  if (!plan || !plan->impl || !ms) return set_err(NTT_ERR_ARG);
  PlanBase& P = plan->last ? *plan->last : *plan->impl;  // the plan that ran the latest transform
  const unsigned k = P.ev_used ? P.ev_used - 1 : 0;  // intervals of the latest slot (gaps included)
  auto gap = [&](unsigned i) {
    const char* l = P.lab[P.slot][i + 1];
    return l[0] == '-' && l[1] == 0;
  };
  unsigned nl = 0;
  for (unsigned i = 0; i < k; ++i) nl += gap(i) ? 0u : 1u;
  if (nlaunches) *nlaunches = P.nrec ? nl : 0u;
  if (nl == 0 || P.nrec == 0) return set_err(NTT_OK);
  if (hipEventSynchronize(P.ev[P.slot][k]) != hipSuccess) return set_err(NTT_ERR_HIP);
  const unsigned nslots = P.nrec < PlanBase::kSlots ? P.nrec : PlanBase::kSlots;
  unsigned j = 0;
  for (unsigned i = 0; i < k && j < max_launches; ++i) {
    if (gap(i)) continue;
    double acc = 0;
    for (unsigned sl = 0; sl < nslots; ++sl) {
      float t = 0;
      if (hipEventElapsedTime(&t, P.ev[sl][i], P.ev[sl][i + 1]) != hipSuccess) return set_err(NTT_ERR_HIP);
      acc += t;
    }
    ms[j++] = (float)(acc / nslots);
  }
  return set_err(NTT_OK);
}

int ntt_plan_destroy(ntt_plan* plan) {
  delete plan;
  return NTT_OK;
}

const char* ntt_strerror(int status) {
  switch (status) {
    case NTT_OK: return "ok";
    case NTT_ERR_ARG: return "invalid argument";
    case NTT_ERR_HIP: return "HIP runtime error";
    case NTT_ERR_RCCL: return "RCCL error";
    case NTT_ERR_FIELD: return "unsupported modulus or no root of unity of this order";
    case NTT_ERR_NODEV: return "no HIP device";
    case NTT_ERR_DEVICE:
      return "an inter-workgroup wait of an earlier call gave up (watchdog): that call's output is wrong; "
             "ntt_plan_device_status clears the report";
    default: return "unknown status";
  }
}

int ntt_last_error(void) { return g_last_error; }

// ---------------------------------------------------------------- reference-shaped shims
// Plans are cached per (modulus, generator, limbs, log_n, device) like a persistent version of the
// reference drivers' per-call table setup.  Threads calling a shim with the same key share the plan
// and its scratch, so each cached plan has its own lock, held for the whole blocking call
// (tests/test_gpu_threads.py: without it, concurrent calls overwrote each other's scratch).
namespace {
struct CachedPlan {
  std::unique_ptr<ntt_plan> plan;
  std::mutex run_mu;
  uint64_t last_use = 0;
  hipEvent_t done = nullptr;  // the blocking shims wait on this, like the reference's cudaEventSynchronize
  ~CachedPlan() {
    if (done) (void)hipEventDestroy(done);
  }
};
}  // namespace
static std::mutex g_cache_mu;
// Heap-held and never destroyed: cached plans outliving main() are not torn down after the HIP runtime
// (static destructors run in an unspecified order relative to it); ntt_shim_cache_clear frees them.
static auto& g_cache = *new std::map<std::tuple<std::vector<uint64_t>, std::vector<uint64_t>, unsigned, unsigned, int>,
                                     std::shared_ptr<CachedPlan>>();
static uint64_t g_cache_tick = 0;
// At most knob::shim_cache_plans() (default 8) cached plans; the least recently used one is dropped
// when a new key arrives (a call still running on it keeps it alive through its shared_ptr).

static std::shared_ptr<CachedPlan> cached_plan(const uint64_t* p, const uint64_t* g, unsigned limbs64, unsigned log_n,
                                               int* rc) {
  int dev = 0;
  (void)hipGetDevice(&dev);
  auto key = std::make_tuple(std::vector<uint64_t>(p, p + limbs64), std::vector<uint64_t>(g, g + limbs64), limbs64,
                             log_n, dev);
  std::lock_guard<std::mutex> lk(g_cache_mu);
  auto it = g_cache.find(key);
  if (it != g_cache.end()) {
    it->second->last_use = ++g_cache_tick;
    *rc = NTT_OK;
    return it->second;
  }
  ntt_plan* pl = nullptr;
  *rc = ntt_plan_create_custom(&pl, p, g, limbs64, log_n, dev);
  if (*rc != NTT_OK) return nullptr;
  while (g_cache.size() >= knob::shim_cache_plans()) {
    auto lru = g_cache.begin();
    for (auto jt = g_cache.begin(); jt != g_cache.end(); ++jt)
      if (jt->second->last_use < lru->second->last_use) lru = jt;
    g_cache.erase(lru);
  }
  auto e = std::make_shared<CachedPlan>();
  e->plan.reset(pl);
  e->last_use = ++g_cache_tick;
  g_cache[key] = e;
  return e;
}

extern "C" void ntt_shim_cache_clear(void) {
  std::lock_guard<std::mutex> lk(g_cache_mu);
  g_cache.clear();
}

// Forward on the default stream, then wait for an event recorded after it (GZKP-NTT.cu:1547 waits on
// its own event the same way), under the plan's lock: work the caller runs on other non-blocking
// streams is not waited on.  A tripped watchdog (the plan's report, read after the wait) is this
// call's error, and is cleared so that the cached plan serves the next call.
static int blocking_forward(const std::shared_ptr<CachedPlan>& cp, void* d) {
  std::lock_guard<std::mutex> lk(cp->run_mu);
  int rc = ntt_forward(cp->plan.get(), d, nullptr);
  if (rc == NTT_OK && !cp->done && hipEventCreateWithFlags(&cp->done, hipEventDisableTiming) != hipSuccess) {
    cp->done = nullptr;
    rc = NTT_ERR_HIP;
  }
  if (rc == NTT_OK && (hipEventRecord(cp->done, nullptr) != hipSuccess || hipEventSynchronize(cp->done) != hipSuccess))
    rc = NTT_ERR_HIP;
  for (PlanBase* P : {cp->plan->impl.get(), cp->plan->wide.get()}) {
    if (P && P->tripped()) {
      P->clear_trip();
      if (rc == NTT_OK) rc = NTT_ERR_DEVICE;
    }
  }
  return set_err(rc);
}

void SSIP(long long* x, long long omega, unsigned log_n) {
  const uint64_t p = 469762049ull, g = (uint64_t)omega;
  int rc = NTT_OK;
  std::shared_ptr<CachedPlan> pl = cached_plan(&p, &g, 1, log_n, &rc);
  if (!pl) { set_err(rc); return; }
  blocking_forward(pl, x);
}

int NTT_GZKP_64(long long* data, const void* /*reverse*/, long long len, long long omega, int /*B*/, int /*G*/,
                long long /*reverse_num*/) {
  if (len <= 0 || (len & (len - 1))) return set_err(NTT_ERR_ARG);
  const unsigned log_n = (unsigned)__builtin_ctzll((unsigned long long)len);
  const uint64_t p = 469762049ull, g = (uint64_t)omega;
  int rc = NTT_OK;
  std::shared_ptr<CachedPlan> pl = cached_plan(&p, &g, 1, log_n, &rc);
  if (!pl) return set_err(rc);
  return blocking_forward(pl, data);
}

int NTT_GZKP_256(uint32_t* data, uint32_t len, const void* /*reverse*/, uint32_t /*reverse_len*/,
                 const uint32_t prime[8], const uint32_t omega[8], uint32_t /*B*/, uint32_t /*G*/) {
  if (!data || !prime || !omega || len == 0 || (len & (len - 1))) return set_err(NTT_ERR_ARG);
  const unsigned log_n = (unsigned)__builtin_ctz(len);
  uint64_t p[4], g[4];
  for (int i = 0; i < 4; ++i) {
    p[i] = (uint64_t)prime[2 * i] | ((uint64_t)prime[2 * i + 1] << 32);
    g[i] = (uint64_t)omega[2 * i] | ((uint64_t)omega[2 * i + 1] << 32);
  }
  int rc = NTT_OK;
  std::shared_ptr<CachedPlan> pl = cached_plan(p, g, 4, log_n, &rc);
  if (!pl) return set_err(rc);
  return blocking_forward(pl, data);
}

}  // extern "C"

// ---------------------------------------------------------------- library-internal (ntt_internal.hpp)
namespace ntt {
int plan_run_fs(ntt_plan* plan, const void* in, const void* in2, void* out, unsigned batch, bool inverse,
                const FsIO& io, hipStream_t st) {
  if (!plan || !plan->impl) return NTT_ERR_ARG;
  return plan->impl->run_fs(in, in2, out, batch, inverse, io, st);
}
int plan_build_fs_table(ntt_plan* plan, void* table, unsigned log_rows, unsigned log_cols, uint64_t row0,
                        uint64_t col0, bool inverse, hipStream_t st, unsigned scale_log) {
  if (!plan || !plan->impl) return NTT_ERR_ARG;
  return plan->impl->build_fs_table(table, log_rows, log_cols, row0, col0, inverse, scale_log, st);
}
size_t plan_table_entry_bytes(const ntt_plan* plan) { return plan && plan->impl ? plan->impl->table_entry_bytes() : 0; }
int plan_device(const ntt_plan* plan) { return plan && plan->impl ? plan->impl->device : -1; }
int plan_create_internal(ntt_plan** out, int field_id, unsigned log_n, unsigned limbs64, int device) {
  return create_field_plan(out, field_id, log_n, limbs64, device, 0, false);
}
unsigned plan_max_radix_for(const ntt_plan* plan, unsigned log_x) {
  return plan && plan->impl ? plan->impl->max_radix_for(log_x) : 99u;
}
unsigned plan_passes_for(const ntt_plan* plan, unsigned log_x) {
  return plan && plan->impl ? plan->impl->passes_for(log_x) : 99u;
}
}  // namespace ntt
