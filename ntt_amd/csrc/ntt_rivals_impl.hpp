// The rival schedules kept for comparison: the reference's radix-2 `naive` and `naive_no_swap` rounds,
// the bealto / bellperson radix-2^deg Stockham family (k_bealto) and the out-of-place digit reversal of
// the GZKP rival (k_digitrev).  (The Stockham and DIT passes of the pass tile are pass kinds of
// ntt_kernels_impl.hpp.)  Instantiated by the ntt_*_misc.hip units.
#pragma once
#include "ntt_elementwise_impl.hpp"

namespace ntt {

// One radix-2 DIT round of the `naive` rival over a bit-reversed vector: butterfly id < n/2 pairs
// pos = 2 (id - off) + off and pos + s (s = 2^log_s, off = id mod s) as (a + w b, a - w b) with
// w = w_n^(off n / 2s) -- the reference kernel's indexing (GZKP-NTT.cu:59-71), one thread per
// butterfly, canonical in and out (the product through the element-format power table: mulv).
// HBM-bound by construction: every round reads and writes the whole vector.  src and dst alias (every
// round but the last runs in place), so neither is __restrict__: each thread reads its two
// elements before it writes them, and no other thread touches them in the round.
template <class E>
__global__ void k_naive_round(const uint32_t* src, uint32_t* dst, uint32_t log_n,
                              uint32_t log_s, const uint32_t* __restrict__ pw, const typename E::Args F) {
  const size_t half = size_t(1) << (log_n - 1), s = size_t(1) << log_s;
  NTT_GRID_STRIDE(id, half) {
    const size_t off = id & (s - 1), pos = ((id - off) << 1) + off;
    uint32_t a[E::W], b[E::W], w[E::W];
    E::load(a, src, pos);
    E::load(b, src, pos + s);
    E::template load<E::TABW>(w, pw, off << (log_n - 1 - log_s));
    E::mulv(b, w, F);  // w R_e: the Montgomery product leaves w b, < 3p (Eng29) / < 2p (Eng32)
    E::template bfly_l<E::IN>(a, b, F);
    E::template store<2 * E::IN>(dst, pos, a, F);
    E::template store<2 * E::IN>(dst, pos + s, b, F);
  }
}

// One radix-2 round of the `naive_no_swap` rival (GZKP-NTT.cu:237-258): butterfly i < n/2 reads
// x[i] and x[i + n/2], multiplies the second by w = w_n^(k n / 2s) (k = i mod s, s = 2^log_s: the
// reference's roots[k * (len / (stride << 1))]) and writes a + w b to y[2i - k], a - w b to
// y[2i - k + s] -- a radix-2 Stockham autosort: natural order in and out after log2 n rounds.
// src != dst (ping-pong).  HBM-bound by construction, like k_naive_round.
template <class E>
__global__ void k_noswap_round(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, uint32_t log_n,
                               uint32_t log_s, const uint32_t* __restrict__ pw, const typename E::Args F) {
  const size_t half = size_t(1) << (log_n - 1), s = size_t(1) << log_s;
  NTT_GRID_STRIDE(i, half) {
    const size_t k = i & (s - 1), j = (i << 1) - k;
    uint32_t a[E::W], b[E::W], w[E::W];
    E::load(a, src, i);
    E::load(b, src, i + half);
    E::template load<E::TABW>(w, pw, k << (log_n - 1 - log_s));
    E::mulv(b, w, F);  // w R_e: the Montgomery product leaves w b
    E::template bfly_l<E::IN>(a, b, F);
    E::template store<2 * E::IN>(dst, j, a, F);
    E::template store<2 * E::IN>(dst, j + s, b, F);
  }
}

template <class E>
hipError_t launch_noswap_round(const uint32_t* src, uint32_t* dst, uint32_t log_n, uint32_t log_s, const uint32_t* pw,
                               const typename E::Args& F, hipStream_t st) {
  if (log_n == 0 || log_s >= log_n || src == dst) return hipErrorInvalidValue;
  hipLaunchKernelGGL((k_noswap_round<E>), dim3(grid_1d(size_t(1) << (log_n - 1))), dim3(256), 0, st, src, dst, log_n,
                     log_s, pw, F);
  return hipGetLastError();
}

template <class E>
hipError_t launch_naive_round(const uint32_t* src, uint32_t* dst, uint32_t log_n, uint32_t log_s, const uint32_t* pw,
                              const typename E::Args& F, hipStream_t st) {
  if (log_n == 0 || log_s >= log_n) return hipErrorInvalidValue;
  hipLaunchKernelGGL((k_naive_round<E>), dim3(grid_1d(size_t(1) << (log_n - 1))), dim3(256), 0, st, src, dst, log_n,
                     log_s, pw, F);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------- bealto / bellperson rivals
// The reference's radix-2^deg Stockham family (bealto.com's group FFT as bellperson ships it,
// FIELD_radix_fft_revised, GZKP-NTT.cu:391-464, and the four "improved" kernels, GZKP-NTT.cu:556-630,
// 632-719, 892-989, 1077-1210; ntt.h NTT_PLAN_BELLPERSON / NTT_PLAN_IMPROVED_V1..V4) as ONE kernel
// with the variant as a template argument: they compute the same round and differ only in how
// threads, groups and LDS rows are mapped, which is what they are kept for (comparison).  A round
// takes groups `index` of 2^deg elements x[index + i t] (t = n >> deg), multiplies element i by
// w_n^(e i), e = (n >> lgp >> deg) (index mod 2^lgp) (from the two-level tables: the reference raises
// FIELD_pow_lookup's twiddle per thread), runs deg radix-2 rounds in LDS with the pq table and writes
// y[((index - k) << deg) + k + i 2^lgp].  lsize = 2^(deg-1) threads per group, two elements each.
//   bellperson: inputs land bit-reversed in LDS, DIT rounds (twiddle, then butterfly), natural out;
//   v1:         DIF rounds (butterfly, then twiddle), bit-reversed out; 2^log_g groups per workgroup;
//   v2:         loads on the transposed map (thread -> group tid mod G: coalesced x[index + i t]);
//   v3:         and stores on it too when lgp > 0 (consecutive k: coalesced y);
//   v4:         and LDS rows of 2 lsize + 1 elements (the reference's bank-conflict padding).
// Lazy bounds (Eng29): loads < p, input products < 3p, every butterfly's outputs brought back < 4p.
__device__ __forceinline__ uint32_t brev_rt(uint32_t v, uint32_t bits) {
  return bits ? __builtin_bitreverse32(v) >> (32u - bits) : 0u;
}
template <class E>
__device__ __forceinline__ void lds_put_el(uint32_t* u, uint32_t slot, const uint32_t (&v)[E::W]) {
#pragma unroll
  for (int w = 0; w < E::W; ++w) u[(size_t)slot * E::W + w] = v[w];
}
template <class E>
__device__ __forceinline__ void lds_get_el(uint32_t (&v)[E::W], const uint32_t* u, uint32_t slot) {
#pragma unroll
  for (int w = 0; w < E::W; ++w) v[w] = u[(size_t)slot * E::W + w];
}
template <class E, int V>
__global__ __launch_bounds__(1024) void k_bealto(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst,
                                                 const PassArgs<E> A, const BealtoArgs B) {
  extern __shared__ __attribute__((aligned(16))) uint32_t u_g[];
  const uint32_t deg = B.deg, lsz = 1u << (deg - 1), G = 1u << B.log_g, tid = threadIdx.x;
  const size_t t = (size_t)1 << (B.log_n - deg), p = (size_t)1 << B.lgp;
  const uint32_t rl = 2 * lsz + (V == BEALTO_V4 ? 1u : 0u);  // one group's LDS row, elements
  // compute map: group gid, lane lid; load map: transposed from v2 on
  const uint32_t lid = tid & (lsz - 1), gid = tid >> (deg - 1);
  const uint32_t gid_r = V >= BEALTO_V2 ? (tid & (G - 1)) : gid, lid_r = V >= BEALTO_V2 ? (tid >> B.log_g) : lid;
  const size_t index = (size_t)blockIdx.x * G + gid, index_r = (size_t)blockIdx.x * G + gid_r;
  const size_t k = index & (p - 1), k_r = index_r & (p - 1);
  {
    const size_t e = (t >> B.lgp) * k_r;  // w_n^(e i): < n for i < 2^deg
    uint32_t* u = u_g + (size_t)gid_r * rl * E::W;
#pragma unroll
    for (uint32_t j = 0; j < 2; ++j) {
      const uint32_t i = 2 * lid_r + j;
      uint32_t v[E::W];
      E::load(v, src, index_r + i * t);
      const size_t ei = e * i;
      typename E::Tw tl, th;
      E::tload(tl, A.tw_lo, (uint32_t)(ei & ((1u << A.lo_bits) - 1)));
      E::tload(th, A.tw_hi, (uint32_t)(ei >> A.lo_bits));
      E::mul(tl.w, th, A.F);  // (lo R_e) hi
      E::mulv(v, tl.w, A.F);  // v w_n^(e i), < 3p
      lds_put_el<E>(u, V == BEALTO_BELLPERSON ? brev_rt(i, deg) : i, v);
    }
  }
  __syncthreads();
  {
    uint32_t* u = u_g + (size_t)gid * rl * E::W;
    const uint32_t pqshift = B.max_deg - deg;
    for (uint32_t s = 0; s < deg; ++s) {
      const uint32_t rnd = V == BEALTO_BELLPERSON ? deg - 1 - s : s;
      const uint32_t bit = lsz >> rnd, di = lid & (bit - 1), i0 = (lid << 1) - di, i1 = i0 + bit;
      uint32_t a[E::W], b[E::W];
      lds_get_el<E>(a, u, i0);
      lds_get_el<E>(b, u, i1);
      typename E::Tw w;
      if (di) E::tload(w, A.tw_int, di << rnd << pqshift);  // w_{2^(deg - rnd)}^di
      if constexpr (V == BEALTO_BELLPERSON) {  // DIT: twiddle, then butterfly
        if (di) E::mul(b, w, A.F);
        E::template bfly_l<E::IN>(a, b, A.F);
        E::template reduce<2 * E::IN, E::IN>(b, A.F);
      } else {  // DIF: butterfly, then twiddle
        E::template bfly_l<E::IN>(a, b, A.F);
        if (di) E::mul(b, w, A.F);
        else E::template reduce<2 * E::IN, E::IN>(b, A.F);
      }
      E::template reduce<2 * E::IN, E::IN>(a, A.F);
      lds_put_el<E>(u, i0, a);
      lds_put_el<E>(u, i1, b);
      __syncthreads();
    }
  }
  // stores: the load map for v3 / v4 after the first round (consecutive k: coalesced), else the compute map
  const bool rmap = V >= BEALTO_V3 && B.lgp != 0;
  const size_t gi = rmap ? index_r : index, kk = rmap ? k_r : k;
  const uint32_t li = rmap ? lid_r : lid;
  const uint32_t* u = u_g + (size_t)(rmap ? gid_r : gid) * rl * E::W;
  const size_t base = ((gi - kk) << deg) + kk;
#pragma unroll
  for (uint32_t j = 0; j < 2; ++j) {
    const uint32_t i = li + j * lsz;
    uint32_t v[E::W];
    lds_get_el<E>(v, u, V == BEALTO_BELLPERSON ? i : brev_rt(i, deg));
    E::template store<E::IN>(dst, base + i * p, v, A.F);
  }
}

template <class E>
hipError_t launch_bealto(int variant, const uint32_t* src, uint32_t* dst, const PassArgs<E>& A, const BealtoArgs& B,
                         hipStream_t st) {
  if constexpr (!HasStockham<E>::value) {
    return hipErrorInvalidValue;
  } else {
    if (B.deg < 1 || B.deg > B.max_deg || B.deg > B.log_n || B.log_n - B.deg < B.log_g || src == dst)
      return hipErrorInvalidValue;
    const uint32_t threads = (1u << (B.deg - 1)) << B.log_g;
    const size_t grid = ((size_t)1 << (B.log_n - B.deg)) >> B.log_g;
    const size_t lds = ((size_t)((2u << (B.deg - 1)) + (variant == BEALTO_V4 ? 1u : 0u)) << B.log_g) * E::W * 4;
    if (threads > 1024 || grid > 0x7fffffffull || lds > 64 * 1024) return hipErrorInvalidValue;
    const dim3 g((uint32_t)grid), b(threads);
    switch (variant) {
      case BEALTO_BELLPERSON: hipLaunchKernelGGL((k_bealto<E, BEALTO_BELLPERSON>), g, b, lds, st, src, dst, A, B); break;
      case BEALTO_V1: hipLaunchKernelGGL((k_bealto<E, BEALTO_V1>), g, b, lds, st, src, dst, A, B); break;
      case BEALTO_V2: hipLaunchKernelGGL((k_bealto<E, BEALTO_V2>), g, b, lds, st, src, dst, A, B); break;
      case BEALTO_V3: hipLaunchKernelGGL((k_bealto<E, BEALTO_V3>), g, b, lds, st, src, dst, A, B); break;
      case BEALTO_V4: hipLaunchKernelGGL((k_bealto<E, BEALTO_V4>), g, b, lds, st, src, dst, A, B); break;
      default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
  }
}

// GZKP rival's `rearrange` (GZKP-NTT.cu:167-233 via reverse pairs), out of place: dst[i] = src[drev(i)].
// The reference's rounds are radix 2, so its permutation is the bit reversal; here every pass is a
// natural-order radix-2^r_q DFT, so the permutation that gives natural-order output is the mixed-radix
// digit reversal: digit q of i (r_q bits, from the low end, in pass order) becomes digit q of the
// source index counted from the HIGH end.  (All r_q = 1 gives the bit reversal.)
struct DigitRev {
  uint32_t nd;
  uint32_t r[8];
};
template <int MEMW>
__global__ void k_digitrev(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, uint32_t log_n,
                           DigitRev D) {
  NTT_GRID_STRIDE(i, (size_t(1) << log_n)) {
    size_t j = 0, rem = i;
    uint32_t top = log_n;
    for (uint32_t q = 0; q < D.nd; ++q) {
      top -= D.r[q];
      j |= (rem & ((1ull << D.r[q]) - 1)) << top;
      rem >>= D.r[q];
    }
    if (D.nd == 0) j = (size_t)(__brevll((unsigned long long)i) >> (64 - log_n));  // log_n 1-bit digits
    if constexpr (MEMW % 4 == 0) {
#pragma unroll
      for (int q = 0; q < MEMW / 4; ++q)
        reinterpret_cast<uint4*>(dst + i * MEMW)[q] = reinterpret_cast<const uint4*>(src + j * MEMW)[q];
    } else {
#pragma unroll
      for (int q = 0; q < MEMW; ++q) dst[i * MEMW + q] = src[j * MEMW + q];
    }
  }
}

template <class E>
hipError_t launch_bitrev(const uint32_t* src, uint32_t* dst, uint32_t log_n, const uint32_t* digits, uint32_t nd,
                         hipStream_t st) {
  DigitRev D{};
  uint32_t sum = 0;
  if (nd > 8 || log_n == 0 || log_n > 40) return hipErrorInvalidValue;
  D.nd = nd;
  for (uint32_t q = 0; q < nd; ++q) sum += (D.r[q] = digits[q]);
  if (nd > 0 && sum != log_n) return hipErrorInvalidValue;  // nd = 0: the bit reversal (digits unused)
  const size_t n = 1ull << log_n;
  hipLaunchKernelGGL((k_digitrev<E::MEMW>), dim3(grid_1d(n)), dim3(256), 0, st, src, dst, log_n,
                     D);
  return hipGetLastError();
}

// The rival schedules of one engine (ntt_*_misc.hip)
#define NTT_INSTANTIATE_RIVALS(E)                                                                                  \
  template hipError_t launch_naive_round<E>(const uint32_t*, uint32_t*, uint32_t, uint32_t, const uint32_t*,       \
                                            const typename E::Args&, hipStream_t);                                 \
  template hipError_t launch_noswap_round<E>(const uint32_t*, uint32_t*, uint32_t, uint32_t, const uint32_t*,      \
                                             const typename E::Args&, hipStream_t);                                 \
  template hipError_t launch_bealto<E>(int, const uint32_t*, uint32_t*, const PassArgs<E>&, const BealtoArgs&,     \
                                       hipStream_t);                                                               \
  template hipError_t launch_bitrev<E>(const uint32_t*, uint32_t*, uint32_t, const uint32_t*, uint32_t,           \
                                       hipStream_t);

}  // namespace ntt
