// The rival schedules (ntt.h: NTT_PLAN_STOCKHAM, _GZKP, _NAIVE, _NO_SWAP, _BELLPERSON, _IMPROVED_V1..V4):
// measurement baselines that run a plan's batch-1 forward the way the reference's kernels do, kept out
// of the product path's way.  A plan owns one Rivals and hands it a reference to itself; Rivals uses
// the plan's tables, field arguments, schedule and profiling marks.  Included by ntt_plan.cpp alone.
#pragma once
#include <algorithm>

#include "../../include/ntt.h"
#include "ntt_kernels.hpp"
#include "plan_devmem.hpp"

namespace {
using namespace ntt;

// the bealto-family rival schedules (ntt.h): one k_bealto variant each
constexpr unsigned kBealtoFlags = NTT_PLAN_BELLPERSON | NTT_PLAN_IMPROVED_V1 | NTT_PLAN_IMPROVED_V2 |
                                  NTT_PLAN_IMPROVED_V3 | NTT_PLAN_IMPROVED_V4;
constexpr unsigned kRivalFlags = NTT_PLAN_STOCKHAM | NTT_PLAN_GZKP | NTT_PLAN_NAIVE | NTT_PLAN_NO_SWAP | kBealtoFlags;

template <class E, class Plan>
struct Rivals {
  static constexpr int MEMW = E::MEMW, TABW = E::TABW;
  Plan& P;
  explicit Rivals(Plan& plan) : P(plan) {}

  DevBuf d_stk_tab;     // NTT_PLAN_STOCKHAM: per-pass input-twiddle tables
  DevBuf d_stk_buf[2];  // NTT_PLAN_STOCKHAM ping-pong buffers (E::MEMW words)
  DevBuf d_naive_pw;    // NTT_PLAN_NAIVE: w_n^i R_e, i < n/2 (the reference's `roots`)
  DevBuf d_naive_buf;   // NTT_PLAN_NAIVE: the bit-reversed copy the rounds work on
                        // (NO_SWAP, bealto family: the ping-pong partner of the caller's buffer)
  size_t stk_off[8] = {};    // element offsets into d_stk_tab (pass >= 1)
  unsigned stk_ord[8] = {};  // Stockham pass i runs radix r[stk_ord[i]] (widest first)
  size_t off_bealto_pq = 0;  // bealto family: w_{2^max_deg}^j, j < 2^(max_deg - 1), Shoup pairs (plan table)
  unsigned bealto_max_deg = 0, bealto_log_g = 0;

  // At plan creation, while the plan's host table is assembled: the reference's pq table
  // (GZKP-NTT.cu:489-499, 740-750): max_deg = min(8 - log_g, log_n), one group per workgroup for
  // bellperson, 2^5 for the improved kernels (GZKP-NTT.cu:1674-1704).  push(exponent shift, count)
  // appends the powers of w_n^(n >> shift) and returns their word offset.
  template <class Push>
  int host_tables(Push&& push) {
    if (!(P.flags & kBealtoFlags)) return NTT_OK;
    if (P.log_n < 1 || !HasStockham<E>::value) return NTT_ERR_ARG;
    bealto_log_g = (P.flags & NTT_PLAN_BELLPERSON) ? 0u : 5u;
    bealto_max_deg = std::min(8u - bealto_log_g, P.log_n);
    off_bealto_pq = push(bealto_max_deg, 1ull << (bealto_max_deg - 1));
    return NTT_OK;
  }
  // At plan creation, after the plan's own tables: the device state of the plan's rival schedule.
  // NTT_PLAN_GZKP runs on the Stockham tables: Stockham pass i's w_n^((k pi) << (log_n - lgp_i - r_i))
  // for k < 2^lgp_i is the GZKP DIT pass's w_N^(c d), N = 2^(lgp_i + r_i)
  int build() {
    if constexpr (HasStockham<E>::value) {  // the rival kernels exist for P and 4 x 64-bit plans only
      if (P.flags & (NTT_PLAN_STOCKHAM | NTT_PLAN_GZKP)) return build_stockham();
      if (P.flags & (NTT_PLAN_NAIVE | NTT_PLAN_NO_SWAP)) return build_naive();
      if (P.flags & kBealtoFlags) return build_bealto();
    }
    return (P.flags & kRivalFlags) ? NTT_ERR_ARG : NTT_OK;
  }
  // A batch-1 forward in place in `d` on the plan's rival schedule: false when the plan has none (the
  // default schedule runs), else rc is the call's status.
  bool run(uint32_t* d, hipStream_t st, int& rc) {
    if constexpr (HasStockham<E>::value) {
      if ((P.flags & NTT_PLAN_STOCKHAM) && d_stk_tab) rc = run_stockham(d, d, st);
      else if ((P.flags & NTT_PLAN_GZKP) && d_stk_tab) rc = run_gzkp(d, d, st);
      else if ((P.flags & NTT_PLAN_NAIVE) && d_naive_pw) rc = run_naive(d, d, st);
      else if ((P.flags & NTT_PLAN_NO_SWAP) && d_naive_pw) rc = run_noswap(d, st);
      else if ((P.flags & kBealtoFlags) && d_naive_buf) rc = run_bealto(d, st);
      else return false;
      return true;
    }
    return false;
  }

  // NTT_PLAN_STOCKHAM (rival schedule, bellperson family): pass i (i >= 1) multiplies element pi of
  // group k < p_i = 2^(r_0 + ... + r_{i-1}) by w_n^((k pi) << (log_n - lgp_i - r_i)) from a table in
  // the column-group-major layout of the pass kernels (k_build_tw with c := k); two ping-pong buffers.
  int build_stockham() {
    const unsigned npass = P.npass, log_n = P.log_n;
    const unsigned* r = P.r;
    if (npass < 2) return NTT_ERR_ARG;
    // widest radix first: pass i >= 1 needs p_i = 2^(r_0 + ... + r_{i-1}) >= T_i = TILE / R_i
    for (unsigned i = 0; i < npass; ++i) stk_ord[i] = i;
    std::stable_sort(stk_ord, stk_ord + npass, [&](unsigned a, unsigned b) { return r[a] > r[b]; });
    size_t elems = 0;
    unsigned lgp = 0;
    const unsigned tl = tile_log_of<E>();
    for (unsigned i = 0; i < npass; ++i) {
      const unsigned ri = r[stk_ord[i]];
      if (i > 0) {
        if (lgp + ri < tl) return NTT_ERR_ARG;
        stk_off[i] = elems;
        elems += 1ull << (lgp + ri);
      }
      lgp += ri;
    }
    if (!d_stk_tab.alloc(elems * TABW * 4)) return NTT_ERR_HIP;
    for (auto& b : d_stk_buf)
      if (!b.alloc((size_t)P.n * MEMW * 4)) return NTT_ERR_HIP;
    lgp = r[stk_ord[0]];
    for (unsigned i = 1; i < npass; ++i) {
      const unsigned ri = r[stk_ord[i]];
      if (launch_build_tw<E>(d_stk_tab.get() + stk_off[i] * TABW, 1ull << (lgp + ri), ri, tl - ri, log_n - lgp - ri,
                             P.outer_lo(0), P.outer_hi(0, 0), P.lo_bits, P.Ff, nullptr) != hipSuccess)
        return NTT_ERR_HIP;
      lgp += ri;
    }
    return hipDeviceSynchronize() == hipSuccess ? NTT_OK : NTT_ERR_HIP;
  }

  int run_stockham(const uint32_t* in, uint32_t* out, hipStream_t st) {
    const uint32_t grid = (uint32_t)(P.n >> tile_log_of<E>());
    hipError_t e = hipSuccess;
    unsigned lgp = 0;
    P.begin(st);
    for (unsigned i = 0; i < P.npass && e == hipSuccess; ++i) {
      const unsigned ri = P.r[stk_ord[i]];
      PassArgs<E> A = P.base_args(false);
      A.tw_int = P.d_tab.get() + P.off_int[0][stk_ord[i]];  // w_R^e for this pass's radix
      A.tw_full = i ? d_stk_tab.get() + stk_off[i] * TABW : nullptr;
      A.log_blk = P.log_n;
      A.lgp = lgp;
      A.src_user = 1;
      const uint32_t* src = i == 0 ? in : d_stk_buf[(i - 1) & 1].get();
      uint32_t* dst = i + 1 == P.npass ? out : d_stk_buf[i & 1].get();
      e = launch_pass<E>(KIND_STOCKHAM, (int)ri, src, dst, A, grid, 1, st);
      P.mark(st);
      lgp += ri;
    }
    return e == hipSuccess ? NTT_OK : NTT_ERR_HIP;
  }

  // NTT_PLAN_GZKP (rival schedule, GZKP(B, G), GZKP-NTT.cu:115-233): digit reversal into a plan buffer
  // (`rearrange`; the bit reversal of the reference's radix-2 rounds), contiguous radix-2^r_0 DFTs (the reference's first rounds, `naive` / a GZKP launch
  // at stride 1), then in-place DIT passes over stride-2^lgp columns with input twiddles; the last
  // pass writes the caller's buffer.  Widest radix first, as for Stockham (lgp_i >= T_i).
  int run_gzkp(const uint32_t* in, uint32_t* out, hipStream_t st) {
    const unsigned tl = tile_log_of<E>(), npass = P.npass;
    const size_t n = P.n;
    uint32_t* buf = d_stk_buf[0].get();
    uint32_t digits[8];
    for (unsigned i = 0; i < npass; ++i) digits[i] = P.r[stk_ord[i]];
    P.begin(st);
    hipError_t e = launch_bitrev<E>(in, buf, P.log_n, digits, npass, st);
    P.mark(st);
    unsigned lgp = 0;
    for (unsigned i = 0; i < npass && e == hipSuccess; ++i) {
      const unsigned ri = P.r[stk_ord[i]];
      PassArgs<E> A = P.base_args(false);
      A.tw_int = P.d_tab.get() + P.off_int[0][stk_ord[i]];  // w_R^e for this pass's radix
      uint32_t* dst = i + 1 == npass ? out : buf;
      if (i == 0) {  // s = 1: contiguous 2^r_0-point DFTs, batched (grid.y chunks of <= 2^15 blocks)
        A.batch_stride = ((size_t)1 << ri) * MEMW;
        const size_t blocks = n >> ri, chunk = size_t(1) << 15;
        for (size_t b0 = 0; b0 < blocks && e == hipSuccess; b0 += chunk) {
          const size_t off = (b0 << ri) * MEMW;
          e = launch_pass<E>(KIND_SINGLE, (int)ri, buf + off, buf + off, A, 1,
                             (uint32_t)(blocks - b0 < chunk ? blocks - b0 : chunk), st);
        }
      } else {
        A.tw_full = d_stk_tab.get() + stk_off[i] * TABW;  // w_N^(c d), N = 2^(lgp + r_i)
        A.log_blk = lgp + ri;
        A.lgp = lgp;
        A.src_user = 1;
        e = launch_pass<E>(KIND_DIT, (int)ri, buf, dst, A, (uint32_t)(n >> tl), 1, st);
      }
      P.mark(st);
      lgp += ri;
    }
    return e == hipSuccess ? NTT_OK : NTT_ERR_HIP;
  }

  // NTT_PLAN_NAIVE (rival schedule, the reference's `naive`, GZKP-NTT.cu:59-95 / big-num.cu:67-170):
  // the bit reversal (`rearrange`), then log2 n radix-2 DIT rounds of one launch each, every round
  // a full read and write of the vector (HBM-bound; the measure of what the pass kernels' fusion
  // buys).  The reference's n-entry `roots` table is the n/2 entries its rounds read.
  int build_naive() {
    if (P.log_n < 1 || P.log_n > 32) return NTT_ERR_ARG;
    const size_t half = P.n / 2;
    if (!d_naive_pw.alloc(half * TABW * 4)) return NTT_ERR_HIP;
    if (!d_naive_buf.alloc((size_t)P.n * MEMW * 4)) return NTT_ERR_HIP;
    if (launch_build_pow<E>(d_naive_pw.get(), half, P.outer_lo(0), P.outer_hi(0, 0), P.lo_bits, P.Ff, nullptr) !=
        hipSuccess)
      return NTT_ERR_HIP;
    return hipDeviceSynchronize() == hipSuccess ? NTT_OK : NTT_ERR_HIP;
  }

  int run_naive(const uint32_t* in, uint32_t* out, hipStream_t st) {
    const unsigned log_n = P.log_n;
    uint32_t* buf = d_naive_buf.get();
    P.begin(st);
    hipError_t e = launch_bitrev<E>(in, buf, log_n, nullptr, 0, st);  // radix-2 rounds: the bit reversal
    P.mark(st);
    for (unsigned s = 0; s < log_n && e == hipSuccess; ++s)
      e = launch_naive_round<E>(buf, s + 1 == log_n ? out : buf, log_n, s, d_naive_pw.get(), P.Ff, st);
    P.mark(st);  // last_launch_ms: [bit reversal, all rounds]
    return e == hipSuccess ? NTT_OK : NTT_ERR_HIP;
  }

  // NTT_PLAN_NO_SWAP (rival schedule, the reference's `naive_no_swap`, GZKP-NTT.cu:237-296): a radix-2
  // Stockham autosort, one launch per round, ping-pong between the caller's buffer and the plan
  // buffer (natural order in and out, no bit reversal); an odd round count ends in the plan buffer
  // and one device copy brings it back.  The same n/2-entry power table as NTT_PLAN_NAIVE.
  int run_noswap(uint32_t* data, hipStream_t st) {
    const unsigned log_n = P.log_n;
    P.begin(st);
    hipError_t e = hipSuccess;
    uint32_t* buf[2] = {data, d_naive_buf.get()};
    for (unsigned s = 0; s < log_n && e == hipSuccess; ++s)
      e = launch_noswap_round<E>(buf[s & 1], buf[(s + 1) & 1], log_n, s, d_naive_pw.get(), P.Ff, st);
    if (e == hipSuccess && (log_n & 1))
      e = hipMemcpyAsync(data, buf[1], (size_t)P.n * MEMW * 4, hipMemcpyDeviceToDevice, st);
    P.mark(st);  // last_launch_ms: [all rounds (and the copy)]
    return e == hipSuccess ? NTT_OK : NTT_ERR_HIP;
  }

  // NTT_PLAN_BELLPERSON / NTT_PLAN_IMPROVED_V1..V4 (rival schedules, the reference's bealto.com group
  // FFT and its four refinements, GZKP-NTT.cu:391-464, 556-1296): rounds of 2^deg-point groups,
  // deg = min(max_deg, log_n - lgp), one launch each (k_bealto), ping-pong between the caller's buffer
  // and the plan buffer; an odd round count ends in the plan buffer and one device copy brings it back.
  int build_bealto() {
    if (P.log_n < 1 || P.log_n > 32 || bealto_max_deg < 1) return NTT_ERR_ARG;
    if (!d_naive_buf.alloc((size_t)P.n * MEMW * 4)) return NTT_ERR_HIP;
    return NTT_OK;
  }
  int bealto_variant() const {
    if (P.flags & NTT_PLAN_BELLPERSON) return BEALTO_BELLPERSON;
    if (P.flags & NTT_PLAN_IMPROVED_V1) return BEALTO_V1;
    if (P.flags & NTT_PLAN_IMPROVED_V2) return BEALTO_V2;
    if (P.flags & NTT_PLAN_IMPROVED_V3) return BEALTO_V3;
    return BEALTO_V4;
  }
  int run_bealto(uint32_t* data, hipStream_t st) {
    const int variant = bealto_variant();
    const unsigned log_n = P.log_n;
    PassArgs<E> A = P.base_args(false);
    A.tw_int = P.d_tab.get() + off_bealto_pq;
    A.tw_lo = P.outer_lo(0);  // lo R_e: (lo R_e) hi, then the Montgomery product leaves x w
    A.tw_hi = P.outer_hi(0, 0);
    BealtoArgs B{log_n, 0u, 0u, 0u, bealto_max_deg};
    uint32_t* buf[2] = {data, d_naive_buf.get()};
    const unsigned nr = (log_n + bealto_max_deg - 1) / bealto_max_deg;
    const bool per_round = nr + 2 < P.kEv;  // one profiling interval per round while they fit
    const char* lab = variant == BEALTO_BELLPERSON ? "g" : "v";
    P.begin(st);
    hipError_t e = hipSuccess;
    unsigned rounds = 0;
    while (B.lgp < log_n && e == hipSuccess) {
      B.deg = std::min(bealto_max_deg, log_n - B.lgp);
      B.log_g = std::min(bealto_log_g, log_n - B.deg);
      e = launch_bealto<E>(variant, buf[rounds & 1], buf[(rounds + 1) & 1], A, B, st);
      if (per_round) P.mark(st, lab, B.deg);
      B.lgp += B.deg;
      ++rounds;
    }
    if (e == hipSuccess && (rounds & 1))
      e = hipMemcpyAsync(data, buf[1], (size_t)P.n * MEMW * 4, hipMemcpyDeviceToDevice, st);
    if (!per_round || (rounds & 1)) P.mark(st, per_round ? "cp" : lab);
    return e == hipSuccess ? NTT_OK : NTT_ERR_HIP;
  }
};

}  // namespace
