// The single-launch schedules (NTT_PLAN_SINGLE_LAUNCH) and the in-place final pass: state built on the
// plan's first use of it (Lazy), each with its own geometry of sync words (plan_fused.hpp has the
// arithmetic).  A plan owns one Single and hands it a reference to itself.  Included by ntt_plan.cpp alone.
#pragma once
#include <cstdio>
#include <vector>

#include "ntt_kernels.hpp"
#include "plan_devmem.hpp"
#include "plan_knobs.hpp"

namespace {

template <class E, class Plan>
struct Single {
  Plan& P;
  explicit Single(Plan& plan) : P(plan) {}

  // knob::single_launch forces the schedule on / off for every plan (A/B); unset: the plan's flag
  bool enabled() const {
    const int env = knob::single_launch();
    return env >= 0 ? env > 0 : (P.flags & NTT_PLAN_SINGLE_LAUNCH) != 0;
  }
  // The sync words of a schedule with inter-workgroup waits (its builder has taken the plan's watchdog
  // slot, alloc_watch, before its capacity query): `words` zeroed words in `buf`, followed by `tail` when
  // given (each launch leaves the words zeroed).  Synchronous.
  static bool alloc_sync(DevBuf& buf, size_t words, const std::vector<uint32_t>* tail = nullptr) {
    const size_t extra = tail ? tail->size() : 0;
    if (!buf.alloc((words + extra) * 4) || hipMemset(buf.get(), 0, words * 4) != hipSuccess) return false;
    if (extra && hipMemcpy(buf.get() + words, tail->data(), extra * 4, hipMemcpyHostToDevice) != hipSuccess)
      return false;
    return hipDeviceSynchronize() == hipSuccess;
  }
  // where a launch finds its sync words: the layout S over `words`
  static void set_sync(FusedArgs& F, uint32_t* words, const FusedSync& S) {
    F.sync = words;
    F.rbase = S.rbase;
    F.wd.abort = words + S.abort_word();
    F.shards = words + S.shards();
  }
  static void fused_verbose(const char* form, uint32_t tiles, uint32_t nwg, uint32_t cap, uint32_t mode = 0) {
    if (knob::fused_verbose())
      fprintf(stderr, form, mode), fprintf(stderr, ", %u tiles per pass, %u workgroups (capacity %u)\n", tiles, nwg, cap);
  }
  // what both 3-pass single launches need of the passes: full tables for passes 1 and 2 (pass 2: Shoup
  // pairs), no fused prologue
  static bool fused3_passes_ok(const PassArgs<E>* PA) {
    return PA[0].tw_full && PA[1].tw_full && PA[1].tw_sh && !PA[0].src2 && !PA[0].tw_in;
  }
  // 3-pass FAST 256-bit plans whose passes 1 and 2 take full tables
  bool fused3_plan_ok() const {
    return P.npass == 3 && P.use_full && P.d_full_sh && P.full_sh_ok[1] && P.Ff.red_ok;
  }

  // The whole batch-1 transform as ONE launch, where the plan has such a schedule (built on first use)
  // and these passes fit it: true when it was launched, rc its status.  Two passes on the 4096-element
  // tiles (k_fused2b, in place k_fused2bi), else three on Eng256 (k_fused3 / k_fused3b, in place k_fused3bi).
  bool launch(const PassArgs<E>* PA, const uint32_t* in, uint32_t* work, uint32_t* out, bool inplace, hipStream_t st,
              int& rc) {
    constexpr bool two = fused2_engine<E>();
    if constexpr (!two && !fused3_engine<E>()) {
      return false;
    } else {
      const unsigned npass = P.npass;
      const unsigned* r = P.r;
      if (!(two ? npass == 2 && fused2_ready(PA, inplace) : inplace ? fused_ip_ready(PA) : fused_ready(PA)))
        return false;
      FusedArgs F = two ? (inplace ? fargs2_ip : fargs2) : (inplace ? fargs_ip : fargs);
      F.wd = P.watchdog(F.wd.abort);
      if (two) F.trace = fused_trace_buffer(F.nwg);
      PassArgs<E> A1 = PA[0], B = PA[npass - 1];
      if (inplace) {  // every pass in the caller's buffer, no scratch
        constexpr FusedSync S = fused_sync_barriers(two ? FUSED2BI_BARRIERS : FUSED3BI_BARRIERS);
        A1.ipn_go = F.sync + S.go(1);  // pass 1's stores wait for the residency decision (barrier 1)
        A1.wd = F.wd;
        B.flags &= ~2u;
        B.ipn_sync = F.sync;
        B.ipn_go = F.sync + S.go(S.lines);  // the final pass's barrier (the form's last): its go word
        B.ipn_shards = F.shards;            // its arrival shards (cumulative, like the top counter)
        B.wd = F.wd;
        in = out;
        work = nullptr;
      }
      hipError_t e;
      {
        FusedSerial order(P.device, st);
        if constexpr (two) e = launch_fused2<E>((int)r[0], (int)r[1], in, work, out, A1, B, F, st);
        else e = launch_fused3<E>((int)r[0], (int)r[1], (int)r[2], in, work, out, A1, PA[1], B, F, st);
        order.done(e);
      }
      P.mark(st, "b");
      if (F.trace && e == hipSuccess) dump_fused_trace(F, inplace, st);
      rc = Plan::rc_of(e);
      return true;
    }
  }

  // ---- k_fused3 (ntt_fused_impl.hpp): plans whose radices the fused kernel is instantiated for
  DevBuf d_sync;  // FusedArgs::sync words
  FusedArgs fargs{};
  Lazy fused_state;
  bool fused_ready(const PassArgs<E>* PA) {
    return fused_state.ready([&] { return build_fused(); }) && fused3_passes_ok(PA);
  }
  bool build_fused() {
    if constexpr (!fused3_engine<E>()) {
      return false;
    } else {
      const unsigned* r = P.r;
      if (!fused3_plan_ok() || !P.alloc_watch()) return false;
      const uint32_t mode = knob::fused_mode();  // 0: the dataflow form (per-tile hand-offs), 1: grid barriers
      uint32_t cap = 0;
      if (fused3_capacity<E>((int)r[0], (int)r[1], (int)r[2], P.device, &cap, mode) != hipSuccess || cap == 0) return false;
      const FusedGeom g = fused_geometry(tile_log_of<E>(), P.n, r[0], r[1], r[2], cap, mode);
      if (!g.ok) return false;  // schedule_ok guarantees it; kept as the kernel's contract
      fused_verbose("libntt: fused schedule mode %u", g.tiles, g.nwg, cap, mode);
      if (!alloc_sync(d_sync, g.sync().total())) return false;
      FusedArgs F{};
      F.tiles = g.tiles, F.nwg = g.nwg;
      F.k1_mask = g.k1_mask, F.k1_shift = g.k1_shift;
      F.cg_log = g.cg_log, F.k2_shift = g.k2_shift, F.t3_log = g.t3_log, F.r2 = g.r2;
      F.n12 = g.n12, F.n23 = g.n23, F.need12 = g.need12, F.need23 = g.need23;
      F.dbg = knob::fused_dbg();
      F.mode = g.mode;
      set_sync(F, d_sync.get(), g.sync());
      fargs = F;
      return true;
    }
  }

  // ---- the two-pass single launch on 4096-element tiles (2^20 4-limb plans: k_fused2b, and k_fused2bi
  // in place; ntt_fused_impl.hpp).  Plain launches of at most the occupancy query's workgroups; the
  // in-place form needs every one of the 256 final tiles resident.
  // Sync words: both forms share the in-place form's (FUSED2BI_BARRIERS go words: residency, pass barrier,
  // final barrier; k_fused2b uses the first), FusedSync in plan_fused.hpp.
  DevBuf d_sync2;
  FusedArgs fargs2{}, fargs2_ip{};
  Lazy fused2_state[2];  // [in place]
  bool fused2_built(bool inplace) {
    return fused2_state[inplace ? 1 : 0].ready([&] { return build_fused2(inplace); });
  }
  bool fused2_ready(const PassArgs<E>* PA, bool inplace) {
    return fused2_built(inplace) && PA[0].tw_full && !PA[0].tw_sh && !PA[0].src2 && !PA[0].tw_in;
  }
  bool build_fused2(bool inplace) {
    if constexpr (!fused2_engine<E>()) {
      return false;
    } else {
      const unsigned* r = P.r;
      if (P.npass != 2 || r[0] != 10 || r[1] != 10 || !P.use_full || !P.Ff.red_ok || !P.alloc_watch()) return false;
      const uint32_t tiles = (uint32_t)(P.n >> tile_log_of<E>()), mode = inplace ? 4u : 3u;
      uint32_t cap = 0;
      if (fused2_capacity<E>((int)r[0], (int)r[1], P.device, &cap, mode) != hipSuccess || cap == 0) return false;
      if (inplace && cap < tiles) return false;
      constexpr FusedSync S = fused_sync_barriers(FUSED2BI_BARRIERS);
      if (!d_sync2 && !alloc_sync(d_sync2, S.total())) return false;
      FusedArgs F{};
      F.tiles = tiles;
      F.nwg = inplace ? tiles : (tiles < cap ? tiles : cap);
      F.mode = mode;
      set_sync(F, d_sync2.get(), S);
      fused_verbose("libntt: two-pass single launch (mode %u)", tiles, F.nwg, cap, mode);
      (inplace ? fargs2_ip : fargs2) = F;
      return true;
    }
  }
  // knob::fused_trace_path (diagnostics): the stamps buffer, and its dump after the call
  DevBuf d_trace;
  unsigned long long* fused_trace_buffer(uint32_t nwg) {
    if (!knob::fused_trace_path()) return nullptr;
    if (!d_trace) (void)d_trace.alloc((size_t)4 * 8 * 1024);
    return (d_trace && nwg <= 1024) ? d_trace.get<unsigned long long>() : nullptr;
  }
  void dump_fused_trace(const FusedArgs& F, bool inplace, hipStream_t st) {
    std::vector<unsigned long long> h((size_t)4 * F.nwg);
    if (hipStreamSynchronize(st) != hipSuccess ||
        hipMemcpy(h.data(), F.trace, h.size() * 8, hipMemcpyDeviceToHost) != hipSuccess)
      return;
    if (FILE* f = fopen(knob::fused_trace_path(), "a")) {
      fprintf(f, "{\"kernel\": \"%s\", \"log_n\": %u, \"nwg\": %u, \"stamps\": [", inplace ? "k_fused2bi" : "k_fused2b",
              P.log_n, F.nwg);
      for (size_t i = 0; i < h.size(); ++i) fprintf(f, "%s%llu", i ? ", " : "", h[i]);
      fprintf(f, "]}\n");
      fclose(f);
    }
  }
  // the plan's batch-1 forward / inverse run as ONE launch: its single-launch state is built now
  bool ready() {
    if constexpr (fused2_engine<E>())
      return P.ensure_full(0, nullptr) == NTT_OK && P.d_fulls[0] && fused2_built((P.flags & NTT_PLAN_IN_PLACE) != 0);
    return false;
  }

  // ---- the in-place single launch (NTT_PLAN_SINGLE_LAUNCH on an NTT_PLAN_IN_PLACE plan, k_fused3bi):
  // 3-pass palindromic FAST 256-bit schedules whose tiles all fit the device at once (2^18 .. 2^20)
  DevBuf d_sync_ip;  // FusedSync of FUSED3BI_BARRIERS barriers: go words for residency and the three grid barriers
  FusedArgs fargs_ip{};
  Lazy fused_ip_state;
  bool fused_ip_ready(const PassArgs<E>* PA) {
    return fused_ip_state.ready([&] { return build_fused_ip(); }) && fused3_passes_ok(PA);
  }
  bool build_fused_ip() {
    if constexpr (!fused3_engine<E>()) {
      return false;
    } else {
      const unsigned* r = P.r;
      if (!fused3_plan_ok() || r[0] != r[2] || !P.alloc_watch()) return false;
      const uint32_t tiles = (uint32_t)(P.n >> tile_log_of<E>());
      uint32_t cap = 0;
      if (fused3_capacity<E>((int)r[0], (int)r[1], (int)r[2], P.device, &cap, 2) != hipSuccess || cap < tiles) return false;
      FusedArgs F{};
      F.tiles = F.nwg = tiles;
      F.mode = 2;
      constexpr FusedSync S = fused_sync_barriers(FUSED3BI_BARRIERS);
      fused_verbose("libntt: in-place single launch", tiles, tiles, cap);
      if (!alloc_sync(d_sync_ip, S.total())) return false;
      set_sync(F, d_sync_ip.get(), S);
      fargs_ip = F;
      return true;
    }
  }

  // ---- in-place final pass with the fused digit reversal (NTT_PLAN_IN_PLACE, k_final_ipn)
  DevBuf d_ipn;  // 32 (2 + slabs) sync words (line 0, one line per slab, the abort line), then the slab order table
  uint32_t ipn_slabs = 0, ipn_strips = 0;
  Lazy ipn_state;
  // knob::ipn off keeps the separate tile-swap pass (A/B)
  bool ipn_ready(const PassArgs<E>& A) {
    return ipn_state.ready([&] { return knob::ipn() && build_ipn(A); });
  }
  // k_final_ipn's arguments from the plain final pass's
  PassArgs<E> ipn_args(const PassArgs<E>& A) const {
    PassArgs<E> B = A;
    B.flags &= ~2u;
    B.ipn_sync = d_ipn.get();
    B.ipn_order = d_ipn.get() + 32 * (2 + ipn_slabs);
    B.ipn_strips = ipn_strips;
    B.wd = P.watchdog(d_ipn.get() + 32 * (1 + ipn_slabs));
    return B;
  }
  bool build_ipn(const PassArgs<E>& A) {
    const unsigned npass = P.npass;
    const unsigned* r = P.r;
    const unsigned tl = tile_log_of<E>(), rp = r[npass - 1];
    if (npass < 2 || r[0] != rp || rp > 9 || tl < rp || !P.alloc_watch()) return false;
    const unsigned mid_log = P.log_n - r[0] - rp;
    ipn_slabs = 1u << mid_log;
    ipn_strips = 1u << (r[0] - (tl - rp));  // R_1 / T, T = TILE / R_p
    // the deadlock-freedom argument of k_final_ipn needs a slab pair's tiles resident together: at
    // most 128 per pair, and no more than the device keeps resident
    if (r[0] < tl - rp || 2 * ipn_strips > 128) return false;
    if (launch_final_ipn_capacity<E>((int)rp, P.device) < 2 * ipn_strips) return false;
    // slab order: m, then its mirror (the final pass's middle-digit reversal, as k_pass computes it)
    std::vector<uint32_t> order, seen(ipn_slabs, 0);
    auto rev = [&](uint32_t m) {
      uint32_t out = 0;
      for (unsigned i = 0; i < A.nmid; ++i) {
        out |= (m & ((1u << A.mid_bits[i]) - 1)) << A.mid_off[i];
        m >>= A.mid_bits[i];
      }
      return out;
    };
    for (uint32_t m = 0; m < ipn_slabs; ++m) {
      if (seen[m]) continue;
      const uint32_t q = rev(m);
      if (q >= ipn_slabs || rev(q) != m) return false;  // the schedule is not palindromic
      order.push_back(m);
      seen[m] = 1;
      if (q != m) {
        order.push_back(q);
        seen[q] = 1;
      }
    }
    return alloc_sync(d_ipn, 32 * (2 + (size_t)ipn_slabs), &order);
  }
};

}  // namespace
