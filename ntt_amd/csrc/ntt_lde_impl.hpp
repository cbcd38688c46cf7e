// Low-degree extension (ntt_lde_batch): the launchers of the PRO_LDE first passes (k_pass with the
// pass tile's PRO_LDE prologue, ntt_kernels_impl.hpp) and k_lde_scale, which scales the inputs where
// the pass cannot.  Included by the ntt_*_lde.hip units alone.
#pragma once
#include "ntt_elementwise_impl.hpp"
#include "ntt_kernels_impl.hpp"

namespace ntt {

// The PRO_LDE pass (low-degree extension, ntt_lde_batch): one outer-table form per engine.  Fast-
// reduction engines on a modulus that takes them (A.F.red_ok) run the column pass with the shift's
// full table (A.tw_full and A.tw_in, as PRO_COSET) and KIND_SINGLE in the FAST form; every other case
// the generic reductions with two-level outer twiddles.
template <class E, int KIND, int LOGR>
static hipError_t launch_lde_r(const uint32_t* src, uint32_t* dst, const PassArgs<E>& A, uint32_t grid, uint32_t batch,
                               hipStream_t st) {
  constexpr int TL = tile_log_of<E>();
  constexpr int MAXR = (KIND == KIND_SINGLE) ? TL : TL - E::MIN_COLS_LOG;
  if constexpr (LOGR > MAXR || !HasLde<E>::value) {
    return hipErrorInvalidValue;
  } else {
    constexpr int TE = (KIND == KIND_SINGLE) ? (1 << LOGR) : (1 << TL);
    constexpr int NT = TE / E::EPT;
    const dim3 g(grid, batch), b(NT < 64 ? 64 : NT);
    if (A.fs || A.tw_epi || A.src2 || A.tw_sh || A.src_stride == 0) return hipErrorInvalidValue;
    if constexpr (E::FASTRED) {
      if (A.F.red_ok) {
        // a plan's passes are all FAST or all generic: no generic column pass beside FAST later ones
        // (a FAST plan without full tables takes the staging route instead)
        if constexpr (KIND == KIND_COLUMN) {
          if (!A.tw_full) return hipErrorInvalidValue;
          hipLaunchKernelGGL((k_pass<E, LOGR, KIND_COLUMN, true, true, PRO_LDE>), g, b, 0, st, src, dst, A);
        } else {
          hipLaunchKernelGGL((k_pass<E, LOGR, KIND_SINGLE, false, true, PRO_LDE>), g, b, 0, st, src, dst, A);
        }
        return hipGetLastError();
      }
    }
    if (A.tw_full || (A.tw_in && !lde_mul_at_load<E, KIND>())) return hipErrorInvalidValue;
    if constexpr (!lde_pass_available<E>(KIND, LOGR, false)) {
      return hipErrorInvalidValue;
    } else {
      hipLaunchKernelGGL((k_pass<E, LOGR, KIND, false, false, PRO_LDE>), g, b, 0, st, src, dst, A);
      return hipGetLastError();
    }
  }
}

template <class E, int KIND>
static hipError_t launch_lde_kind(int logr, const uint32_t* src, uint32_t* dst, const PassArgs<E>& A, uint32_t grid,
                                  uint32_t batch, hipStream_t st) {
  return with_radix<3, 13>(logr, [&](auto R) { return launch_lde_r<E, KIND, R>(src, dst, A, grid, batch, st); });
}

// The inputs of a low-degree extension times c^j, into a staging buffer of the same layout
// (launch_lde_scale, ntt_kernels.hpp); input v is blockIdx.y
template <class E>
__global__ void k_lde_scale(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, size_t n_in,
                            const uint32_t* __restrict__ lo_s, const uint32_t* __restrict__ hi, uint32_t lo_bits,
                            const typename E::Args F) {
  NTT_GRID_STRIDE(j, n_in) {
    const size_t i = (size_t)blockIdx.y * n_in + j;
    uint32_t x[E::W];
    typename E::Tw w, h;
    E::load(x, src, i);
#if NTT_DEBUG_CHECKS
    if (!E::dbg_canonical(x, F)) ntt_dbg_flag(F.dbg, NTT_DBG_INPUT);
#endif
    E::tload(w, lo_s, (uint32_t)(j & ((1ull << lo_bits) - 1)));
    E::tload(h, hi, (uint32_t)(j >> lo_bits));
    E::mul(w.w, h, F);
    E::mulv(x, w.w, F);
    E::template store<E::MUL_OUT>(dst, i, x, F);
  }
}

template <class E>
hipError_t launch_lde_scale(const uint32_t* src, uint32_t* dst, size_t n_in, uint32_t batch, const uint32_t* lo_s,
                            const uint32_t* hi, uint32_t lo_bits, const typename E::Args& F, hipStream_t st) {
  hipLaunchKernelGGL((k_lde_scale<E>), dim3(grid_1d(n_in), batch), dim3(256), 0, st, src, dst, n_in, lo_s, hi, lo_bits, F);
  return hipGetLastError();
}

template <class E>
hipError_t launch_lde_pass(int kind, int logr, const uint32_t* src, uint32_t* dst, const PassArgs<E>& A, uint32_t grid,
                           uint32_t batch, hipStream_t st) {
  if (kind == KIND_COLUMN) return launch_lde_kind<E, KIND_COLUMN>(logr, src, dst, A, grid, batch, st);
  if (kind == KIND_SINGLE) return launch_lde_kind<E, KIND_SINGLE>(logr, src, dst, A, grid, batch, st);
  return hipErrorInvalidValue;
}

// The PRO_LDE passes of one engine (a translation unit of their own: ntt_*_lde.hip)
#define NTT_INSTANTIATE_LDE(E)                                                                                  \
  template hipError_t launch_lde_pass<E>(int, int, const uint32_t*, uint32_t*, const PassArgs<E>&, uint32_t, \
                                         uint32_t, hipStream_t);                                             \
  template hipError_t launch_lde_scale<E>(const uint32_t*, uint32_t*, size_t, uint32_t, const uint32_t*,       \
                                          const uint32_t*, uint32_t, const typename E::Args&, hipStream_t);

}  // namespace ntt
