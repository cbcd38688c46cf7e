// k_fri_fold: one FRI fold of arity 2^K over bit-reversed coset evaluations of degree-D extension elements
// (ntt_fri_fold).  Included by ntt_eg_fold.hip and ntt_e31_fold.hip alone.
//
// Input [N][D], output [M = N >> K][D].  The 2^K rows i' 2^K + j of the input are the fibre over output row
// i': one thread folds one fibre, in registers, as K arity-2 stages.  Stage s halves the fibre with the
// uniform challenge beta^(2^s):
//     x[m] <- (x[2m] + x[2m+1]) + beta^(2^s) ((x[2m] - x[2m+1]) t),   t = y^(2^s) zeta^-(2^s rev(m)),
// where y = c^-1 w_N^-rev(i') is the thread's own (two table loads and two products, squared between
// stages), zeta = w_N^M has order 2^K, and rev reverses the K - 1 - s bits of m.  The halves of all stages
// are paid at the end by one product with 2^-K.  t is a base-field scalar in the form mulv wants (t R_e), so
// the difference keeps the data's form; beta^(2^s) and W beta^(2^s) are Shoup pairs in scalar registers, so
// the extension product is fieldext.hpp's mul_pre: D^2 twiddle-style products and no product by W.
//
// Global access.  A fibre is FW = 2^K D E::MEMW words, 8 B to 512 B.  Direct form: a thread loads its own
// fibre, 16 B at a time; from 32 B up each load instruction of a wave then touches 64 separate runs of 16 B.
// Staged form (STAGED, fibres of 32 B and more): lane l of the workgroup loads 16 B at base + 16 l, so a
// wave's load covers 1 KiB of consecutive addresses, and the fibres reach their threads through LDS, each
// fibre's row padded by 4 words (stride FW + 4 = 4 mod 8 words: the 16 lanes of a ds_read_b128 phase fall
// on 16 different groups of 4 banks).  Fibres up to 16 B are one load per lane at consecutive addresses in
// either form.  An output row is D E::MEMW words at consecutive addresses in consecutive lanes.
#pragma once
#include <type_traits>

#include "fieldext.hpp"
#include "ntt_kernels.hpp"

namespace ntt {

template <class E>
using fold_val_t = std::conditional_t<std::is_same_v<E, Eng31>, uint32_t, uint64_t>;

template <int D, int K, int MEMW>
struct FoldShape {
  static constexpr int ROWW = D * MEMW;           // words per row
  static constexpr int FW = ROWW << K;            // words per fibre
  static constexpr bool can_stage = FW >= 8;      // 32 B and more
  static constexpr int STRIDE = FW + 4;           // LDS words per fibre
  static constexpr int threads(bool staged) { return (staged && can_stage) ? (FW >= 128 ? 64 : 128) : 256; }
};

// x t for the thread's own scalar t (held as t R_e)
template <class E, int D>
__device__ __forceinline__ void fold_scalev(fold_val_t<E> (&x)[D], const uint32_t (&t)[E::W], const typename E::Args& F) {
  if constexpr (std::is_same_v<E, Eng31>)
    f31x::scalev<D>(x, x, t[0], F.p, F.pinv);
  else
    gl64x::scale<D>(x, x, Eng64G::u64(t));
}
// x b for the uniform extension element b (b and W b as twiddles)
template <class E, int D>
__device__ __forceinline__ void fold_mul_pre(fold_val_t<E> (&x)[D], const typename E::Tw (&b)[4], const typename E::Tw (&wb)[4],
                                             const typename E::Args& F) {
  if constexpr (std::is_same_v<E, Eng31>) {
    uint32_t v[D], vs[D], w[D], ws[D];
#pragma unroll
    for (int j = 0; j < D; ++j) {
      v[j] = b[j].w[0];
      vs[j] = b[j].ws;
      w[j] = wb[j].w[0];
      ws[j] = wb[j].ws;
    }
    f31x::mul_pre<D>(x, x, v, vs, w, ws, F.p);
  } else {
    uint64_t v[D], w[D];
#pragma unroll
    for (int j = 0; j < D; ++j) {
      v[j] = Eng64G::u64(b[j].w);
      w[j] = Eng64G::u64(wb[j].w);
    }
    gl64x::mul_pre<D>(x, x, v, w);
  }
}

// Stage S of K (and the ones after it) on the fibre x; y holds (c^-1 w_N^-rev(row))^(2^S) R_e
template <class E, int D, int K, int S>
struct FoldStage {
  using V = fold_val_t<E>;
  static __device__ __forceinline__ void run(V (&x)[1 << K][D], uint32_t (&y)[E::W], const FoldArgs<E>& A) {
    constexpr int BITS = K - 1 - S, HALF = 1 << BITS;
#pragma unroll
    for (int m = 0; m < HALF; ++m) {
      int rv = 0;  // rev(m) over BITS bits; times 2^S it stays below 2^(K - 1)
#pragma unroll
      for (int b = 0; b < BITS; ++b) rv |= ((m >> b) & 1) << (BITS - 1 - b);
      uint32_t t[E::W];
#pragma unroll
      for (int i = 0; i < E::W; ++i) t[i] = y[i];
      if (rv) E::mul(t, A.zeta[rv << S], A.F);
      V sum[D], dif[D];
      if constexpr (E::MEMW == 1) {
        f31x::add<D>(sum, x[2 * m], x[2 * m + 1], A.F.p);
        f31x::sub<D>(dif, x[2 * m], x[2 * m + 1], A.F.p);
      } else {
        gl64x::add<D>(sum, x[2 * m], x[2 * m + 1]);
        gl64x::sub<D>(dif, x[2 * m], x[2 * m + 1]);
      }
      fold_scalev<E, D>(dif, t, A.F);
      fold_mul_pre<E, D>(dif, A.beta[S], A.wbeta[S], A.F);
      if constexpr (E::MEMW == 1)
        f31x::add<D>(x[m], sum, dif, A.F.p);
      else
        gl64x::add<D>(x[m], sum, dif);
    }
    if constexpr (S + 1 < K) {
      E::mulv(y, y, A.F);  // (y R_e)^2 / R_e = y^2 R_e
      FoldStage<E, D, K, S + 1>::run(x, y, A);
    }
  }
};

template <class E, int D, int K, bool STAGED>
__global__ __launch_bounds__((FoldShape<D, K, E::MEMW>::threads(STAGED))) void k_fri_fold(
    const uint32_t* __restrict__ in, uint32_t* __restrict__ out, const FoldArgs<E> A) {
  using S = FoldShape<D, K, E::MEMW>;
  using V = fold_val_t<E>;
  constexpr int W = E::MEMW, ROWW = S::ROWW, FW = S::FW, ROWS = 1 << K;
  constexpr bool LDS = STAGED && S::can_stage;
  constexpr int BT = S::threads(STAGED);
  const uint32_t tid = threadIdx.x;
  const size_t row = (size_t)blockIdx.x * BT + tid;  // output row
  const size_t m_rows = (size_t)1 << A.log_m;
  const bool live = row < m_rows;
  uint32_t raw[FW];

  if constexpr (LDS) {
    // the workgroup's BT fibres are BT FW consecutive words: BT FW / 4 runs of 16 B, FW / 4 per thread
    constexpr int Q = FW / 4;
    __shared__ uint4 lds[BT * S::STRIDE / 4];
    const uint4* __restrict__ in4 = reinterpret_cast<const uint4*>(in);
    const size_t base4 = (size_t)blockIdx.x * BT * Q, end4 = A.src_words / 4;
#pragma unroll
    for (int it = 0; it < Q; ++it) {
      const uint32_t g = it * BT + tid;
      if (base4 + g < end4) lds[(g / Q) * (S::STRIDE / 4) + g % Q] = in4[base4 + g];
    }
    __syncthreads();
    if (!live) return;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const uint4 v = lds[tid * (S::STRIDE / 4) + q];
      raw[4 * q] = v.x;
      raw[4 * q + 1] = v.y;
      raw[4 * q + 2] = v.z;
      raw[4 * q + 3] = v.w;
    }
  } else {
    if (!live) return;
    size_t base = row * FW;
#if NTT_DEBUG_CHECKS
    if (base + FW > A.src_words) {
      ntt_dbg_flag(A.F.dbg, NTT_DBG_BOUNDS);
      base = 0;
    }
#endif
    if (A.vec && FW >= 4) {
      const uint4* __restrict__ p4 = reinterpret_cast<const uint4*>(in + base);
#pragma unroll
      for (int q = 0; q < FW / 4; ++q) {
        const uint4 v = p4[q];
        raw[4 * q] = v.x;
        raw[4 * q + 1] = v.y;
        raw[4 * q + 2] = v.z;
        raw[4 * q + 3] = v.w;
      }
    } else if (W == 2 || (A.vec && FW == 2)) {  // 8-byte elements are 8-byte aligned
      const uint2* __restrict__ p2 = reinterpret_cast<const uint2*>(in + base);
#pragma unroll
      for (int q = 0; q < FW / 2; ++q) {
        const uint2 v = p2[q];
        raw[2 * q] = v.x;
        raw[2 * q + 1] = v.y;
      }
    } else {
#pragma unroll
      for (int q = 0; q < FW; ++q) raw[q] = in[base + q];
    }
  }

  V x[ROWS][D];
#pragma unroll
  for (int j = 0; j < ROWS; ++j)
#pragma unroll
    for (int b = 0; b < D; ++b) {
      if constexpr (W == 1)
        x[j][b] = raw[j * D + b];
      else
        x[j][b] = ((uint64_t)raw[2 * (j * D + b) + 1] << 32) | raw[2 * (j * D + b)];
#if NTT_DEBUG_CHECKS
      bool ok;
      if constexpr (W == 1)
        ok = f31::is_canonical(x[j][b], A.F.p);
      else
        ok = gl64::is_canonical(x[j][b]);
      if (!ok) ntt_dbg_flag(A.F.dbg, NTT_DBG_INPUT);
#endif
    }

  // y R_e = c^-1 w_N^-rev(row) R_e: lo_s holds w_n^-e R_e, hi and cinv are twiddles
  uint32_t y[E::W];
  {
    const uint32_t r = A.log_m ? (__brev((uint32_t)row) >> (32 - A.log_m)) : 0u;
    const uint64_t e = (uint64_t)r << A.tab_shift;
    typename E::Tw lo, hi;
    E::tload(lo, A.lo_s, (size_t)(e & ((1ull << A.lo_bits) - 1)));
    E::tload(hi, A.hi, (size_t)(e >> A.lo_bits));
    E::mul(lo.w, hi, A.F);
    E::mul(lo.w, A.cinv, A.F);
#pragma unroll
    for (int i = 0; i < E::W; ++i) y[i] = lo.w[i];
  }

  FoldStage<E, D, K, 0>::run(x, y, A);

  uint32_t res[ROWW];
#pragma unroll
  for (int b = 0; b < D; ++b) {
    if constexpr (W == 1) {
      const uint32_t v = f31::mulc(x[0][b], A.scale.w[0], A.scale.ws, A.F.p);
      res[b] = v;
#if NTT_DEBUG_CHECKS
      if (!f31::is_canonical(v, A.F.p)) ntt_dbg_flag(A.F.dbg, NTT_DBG_OUTPUT);
#endif
    } else {
      const uint64_t v = gl64::mul(x[0][b], Eng64G::u64(A.scale.w));
      res[2 * b] = (uint32_t)v;
      res[2 * b + 1] = (uint32_t)(v >> 32);
#if NTT_DEBUG_CHECKS
      if (!gl64::is_canonical(v)) ntt_dbg_flag(A.F.dbg, NTT_DBG_OUTPUT);
#endif
    }
  }
  size_t ob = row * ROWW;
#if NTT_DEBUG_CHECKS
  if (ob + ROWW > A.dst_words) {
    ntt_dbg_flag(A.F.dbg, NTT_DBG_BOUNDS);
    ob = 0;
  }
#endif
  if (A.vec && ROWW >= 4) {
    uint4* __restrict__ o4 = reinterpret_cast<uint4*>(out + ob);
#pragma unroll
    for (int q = 0; q < ROWW / 4; ++q) o4[q] = make_uint4(res[4 * q], res[4 * q + 1], res[4 * q + 2], res[4 * q + 3]);
  } else if (ROWW >= 2 && (W == 2 || A.vec)) {
    uint2* __restrict__ o2 = reinterpret_cast<uint2*>(out + ob);
#pragma unroll
    for (int q = 0; q < ROWW / 2; ++q) o2[q] = make_uint2(res[2 * q], res[2 * q + 1]);
  } else {
#pragma unroll
    for (int q = 0; q < ROWW; ++q) out[ob + q] = res[q];
  }
}

template <class E, int D, int K>
static hipError_t launch_fold_dk(bool staged, const uint32_t* in, uint32_t* out, const FoldArgs<E>& A, hipStream_t st) {
  using S = FoldShape<D, K, E::MEMW>;
  const size_t m_rows = (size_t)1 << A.log_m;
  if (staged && S::can_stage && A.vec) {
    constexpr int BT = S::threads(true);
    hipLaunchKernelGGL((k_fri_fold<E, D, K, true>), dim3((unsigned)((m_rows + BT - 1) / BT)), dim3(BT), 0, st, in, out, A);
  } else {
    constexpr int BT = S::threads(false);
    hipLaunchKernelGGL((k_fri_fold<E, D, K, false>), dim3((unsigned)((m_rows + BT - 1) / BT)), dim3(BT), 0, st, in, out, A);
  }
  return hipGetLastError();
}

template <class E, int D>
static hipError_t launch_fold_d(unsigned k, bool staged, const uint32_t* in, uint32_t* out, const FoldArgs<E>& A,
                                hipStream_t st) {
  switch (k) {
    case 1: return launch_fold_dk<E, D, 1>(staged, in, out, A, st);
    case 2: return launch_fold_dk<E, D, 2>(staged, in, out, A, st);
    case 3: return launch_fold_dk<E, D, 3>(staged, in, out, A, st);
    case 4: return launch_fold_dk<E, D, 4>(staged, in, out, A, st);
  }
  return hipErrorInvalidValue;
}

template <class E>
hipError_t launch_fri_fold(unsigned log_arity, unsigned ext_degree, bool staged, const uint32_t* in, uint32_t* out,
                           const FoldArgs<E>& A, hipStream_t st) {
  switch (ext_degree) {
    case 1: return launch_fold_d<E, 1>(log_arity, staged, in, out, A, st);
    case 2: return launch_fold_d<E, 2>(log_arity, staged, in, out, A, st);
    case 4: return launch_fold_d<E, 4>(log_arity, staged, in, out, A, st);
  }
  return hipErrorInvalidValue;
}

#define NTT_INSTANTIATE_FOLD(E)                                                                                  \
  template hipError_t launch_fri_fold<E>(unsigned, unsigned, bool, const uint32_t*, uint32_t*, const FoldArgs<E>&, \
                                         hipStream_t);

}  // namespace ntt
