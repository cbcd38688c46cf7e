// Row-major matrix transforms (ntt_forward_matrix / ntt_inverse_matrix / ntt_lde_matrix): k_pass_mat, the
// strip form of the pass tile (pass_tile's MAT option, ntt_kernels_impl.hpp), and k_mat_naive for 2 and 4
// rows.  Included by ntt_eg_mat.hip and ntt_e31_mat.hip alone.
#pragma once
#include "ntt_elementwise_impl.hpp"  // grid_1d, NTT_GRID_STRIDE (k_mat_naive)
#include "ntt_kernels_impl.hpp"

namespace ntt {

// One pass over the columns of a row-major matrix (pass_tile's strip form, MAT): workgroup g runs strip
// g mod A.mat_ns of tile g / A.mat_ns, so the strips of one tile -- which share the lines that a row
// boundary or a strip boundary cuts -- are dispatched together.  One scalar division per workgroup.
template <class E, int LOGR, int KIND, int PRO>
__global__ __launch_bounds__((1 << E::TILE_LOG) / E::EPT) __attribute__((amdgpu_waves_per_eu(E::WAVES_PER_EU)))
void k_pass_mat(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, const PassArgs<E> A) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[pass_lds_words<E, LOGR, KIND>()];
  __shared__ __attribute__((aligned(16))) uint32_t lds_tw[pass_ltw<E, KIND, false>() ? (1 << LOGR) * E::TW : 1];
  const uint32_t w = blockIdx.x / A.mat_ns, strip = blockIdx.x - w * A.mat_ns;
  pass_tile<E, LOGR, KIND, TW_TWO_LEVEL, RED_GENERIC, PRO, SRC_CALLER, FSM_MAPS, OUTER_MONT, STORE_PLAIN, TILE_ONCE, IPN_NONE,
            STRIP_FORM>(src, dst, A, w, strip, lds, lds_tw);
}

template <class E, int LOGR>
static hipError_t launch_mat_r(int kind, bool lde, const uint32_t* src, uint32_t* dst, const PassArgs<E>& A,
                               uint32_t grid, hipStream_t st) {
  if constexpr (!HasMat<E>::value || LOGR > mat_max_radix_log<E>()) {
    return hipErrorInvalidValue;
  } else {
    static_assert(!E::FASTRED && lde_mul_at_load<E, KIND_COLUMN>(), "matrix engines");
    const dim3 g(grid), b((1 << E::TILE_LOG) / E::EPT);
    // the strip is no wider than the tile's columns (column pass) or blocks (final pass), and no narrower
    // than the 64-byte rule allows
    if (A.mat_w == 0 || A.mat_ns == 0 || A.il + LOGR > (uint32_t)E::TILE_LOG || A.fs || A.tw_epi || A.src2 ||
        A.tw_full || A.tw_sh)
      return hipErrorInvalidValue;
    // the row maps reverse log_n bits of a 32-bit row; the epilogue needs both of its tables, and is the
    // only use of tw_in outside the PRO_LDE pass
    if (A.log_n < (uint32_t)LOGR || A.log_n > 31 || (A.mat_ops & ~(MAT_REV_IN | MAT_REV_OUT | MAT_MUL_OUT)))
      return hipErrorInvalidValue;
    const bool mul_out = (A.mat_ops & MAT_MUL_OUT) != 0;
    if (mul_out && (lde || !A.tw_in || !A.tw_in_hi)) return hipErrorInvalidValue;
    if (kind == KIND_COLUMN && lde) {
      if (A.src_stride == 0 || (A.mat_ops & MAT_REV_IN)) return hipErrorInvalidValue;
      hipLaunchKernelGGL((k_pass_mat<E, LOGR, KIND_COLUMN, PRO_LDE>), g, b, 0, st, src, dst, A);
    } else if (lde || (A.tw_in && !mul_out)) {
      return hipErrorInvalidValue;
    } else if (kind == KIND_COLUMN) {
      hipLaunchKernelGGL((k_pass_mat<E, LOGR, KIND_COLUMN, PRO_NONE>), g, b, 0, st, src, dst, A);
    } else if (kind == KIND_FINAL) {
      hipLaunchKernelGGL((k_pass_mat<E, LOGR, KIND_FINAL, PRO_NONE>), g, b, 0, st, src, dst, A);
    } else {
      return hipErrorInvalidValue;
    }
    return hipGetLastError();
  }
}

template <class E>
hipError_t launch_mat_pass(int kind, int logr, bool lde, const uint32_t* src, uint32_t* dst, const PassArgs<E>& A,
                           uint32_t grid, hipStream_t st) {
  return with_radix<3, 9>(logr, [&](auto R) { return launch_mat_r<E, R>(kind, lde, src, dst, A, grid, st); });
}

// Matrix transforms of 2 and 4 rows: a thread per column holds the column's inputs in registers (so
// src may be dst) and forms the n outputs as k_dft_naive does.
template <class E>
__global__ void k_mat_naive(const uint32_t* src, uint32_t* dst, const PassArgs<E> A, uint32_t n_in) {
  const uint32_t n = 1u << A.log_n;
  const bool mul_out = (A.mat_ops & MAT_MUL_OUT) != 0;
  // the row maps (MAT_REV_IN / MAT_REV_OUT): log_n is 1 or 2 here
  auto row_of = [&](uint32_t r, uint32_t bit) -> uint32_t {
    return (A.mat_ops & bit) ? __builtin_bitreverse32(r) >> (32 - A.log_n) : r;
  };
  // debug builds: an index outside its buffer is recorded and redirected to element 0
  auto ck = [&](size_t i, [[maybe_unused]] size_t lim) -> size_t {
#if NTT_DEBUG_CHECKS
    if (i >= lim) {
      ntt_dbg_flag(A.F.dbg, NTT_DBG_BOUNDS);
      return 0;
    }
#endif
    return i;
  };
  NTT_GRID_STRIDE(b, A.mat_w) {
    uint32_t x[4][E::W];
    static_for<4>([&](auto J) {
      constexpr int j = J;
      if (j < n_in) {
        E::load(x[j], src, ck((size_t)row_of(j, MAT_REV_IN) * A.mat_w + b, A.dbg_src_n));
#if NTT_DEBUG_CHECKS
        if (!E::dbg_canonical(x[j], A.F)) ntt_dbg_flag(A.F.dbg, NTT_DBG_INPUT);
#endif
        if (A.tw_in && !mul_out) {  // c^j from the shift's two-level tables
          typename E::Tw tl, th;
          E::tload(tl, A.tw_in, (uint32_t)(j & ((1u << A.lo_bits) - 1)));
          E::tload(th, A.tw_in_hi, (uint32_t)(j >> A.lo_bits));
          E::mul(tl.w, th, A.F);
          E::mulv(x[j], tl.w, A.F);
        }
      }
    });
    static_for<4>([&](auto K) {
      constexpr int k = K;
      if (k < n) {
        uint32_t acc[E::W], v[E::W];
        typename E::Tw w;
#pragma unroll
        for (int l = 0; l < E::W; ++l) acc[l] = x[0][l];
        E::tload(w, A.tw_int, 0);
        E::mul(acc, w, A.F);
        static_for<3>([&](auto J1) {
          constexpr int j = J1 + 1;
          if (j < n_in) {
#pragma unroll
            for (int l = 0; l < E::W; ++l) v[l] = x[j][l];
            E::tload(w, A.tw_int, (j * k) & (n - 1));
            E::mul(v, w, A.F);
            E::template bfly_l<E::IN>(acc, v, A.F);  // acc <- acc + v (the difference is discarded)
            E::template reduce<2 * E::IN, E::IN>(acc, A.F);
          }
        });
        if (A.flags & 1u) E::mul(acc, A.F.ninv, A.F);
        if (mul_out) {  // c^-k, the shift's inverse tables
          typename E::Tw tl, th;
          E::tload(tl, A.tw_in, (uint32_t)(k & ((1u << A.lo_bits) - 1)));
          E::tload(th, A.tw_in_hi, (uint32_t)(k >> A.lo_bits));
          E::mul(tl.w, th, A.F);
          E::mulv(acc, tl.w, A.F);
        }
        E::template store<E::IN>(dst, ck((size_t)row_of(k, MAT_REV_OUT) * A.mat_w + b, A.dbg_dst_n), acc, A.F);
      }
    });
  }
}

template <class E>
hipError_t launch_mat_naive(const uint32_t* src, uint32_t* dst, const PassArgs<E>& A, uint32_t n_in, hipStream_t st) {
  if constexpr (!HasMat<E>::value) {
    return hipErrorInvalidValue;
  } else {
    if (A.log_n < 1 || A.log_n > 2 || n_in == 0 || n_in > (1u << A.log_n) || A.mat_w == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL((k_mat_naive<E>), dim3(grid_1d(A.mat_w)), dim3(256), 0, st, src, dst, A, n_in);
    return hipGetLastError();
  }
}

// The row-major matrix passes of one engine (a translation unit of their own: ntt_*_mat.hip)
#define NTT_INSTANTIATE_MAT(E)                                                                                 \
  template hipError_t launch_mat_pass<E>(int, int, bool, const uint32_t*, uint32_t*, const PassArgs<E>&, uint32_t, \
                                         hipStream_t);                                                         \
  template hipError_t launch_mat_naive<E>(const uint32_t*, uint32_t*, const PassArgs<E>&, uint32_t, hipStream_t);

}  // namespace ntt
