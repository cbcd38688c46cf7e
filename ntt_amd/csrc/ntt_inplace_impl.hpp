// NTT_PLAN_IN_PLACE: the in-place final pass with the digit reversal fused (k_final_ipn, the pass tile's
// IPN_SLAB form, ntt_kernels_impl.hpp) and the tile-swap digit reversal that follows a plain in-place
// final pass (k_digitrev_swap).  Instantiated by the ntt_*_misc.hip units.
#pragma once
#include "ntt_kernels_impl.hpp"

namespace ntt {

// In-place final pass with the fused digit reversal: one tile per workgroup, tiles taken from a
// ticket counter in slab-pair order (slab m's tiles, then slab rev(m)'s), so that a tile waits only
// for tiles of its own pair.  Deadlock-free at any residency: every ticket below the newest pair's
// was taken by a running workgroup, those pairs complete, and a pair has 2 R_1 / T <= 128 tiles.
// The last workgroup out re-zeroes the counters for the next launch.
template <class E, int LOGR>
__global__ __launch_bounds__((1 << E::TILE_LOG) / E::EPT) __attribute__((amdgpu_waves_per_eu(E::WAVES_PER_EU)))
void k_final_ipn(uint32_t* data, const PassArgs<E> A) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[pass_lds_words<E, LOGR, KIND_FINAL>()];
  __shared__ __attribute__((aligned(16))) uint32_t lds_tw[pass_ltw<E, KIND_FINAL, false>() ? (1 << LOGR) * E::TW : 1];
  __shared__ uint32_t s_w, s_last;
  const uint32_t t = threadIdx.x;
  if (t == 0) {
    const uint32_t tk = __hip_atomic_fetch_add(A.ipn_sync, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint32_t slab = A.ipn_order[tk / A.ipn_strips], strip = tk % A.ipn_strips;
    s_w = (strip << (A.log_n - A.r1 - LOGR)) | slab;  // the final pass's tile index: (k1 group, mid)
  }
  __syncthreads();
  const uint32_t w = s_w;
  if constexpr (E::FASTRED) {
    if (A.F.red_ok)
      pass_tile<E, LOGR, KIND_FINAL, TW_TWO_LEVEL, RED_FAST, PRO_NONE, SRC_CALLER, FSM_NONE, OUTER_MONT, STORE_PLAIN, TILE_ONCE, IPN_SLAB>(
          data, data, A, w, 0, lds, lds_tw);
    else
      pass_tile<E, LOGR, KIND_FINAL, TW_TWO_LEVEL, RED_GENERIC, PRO_NONE, SRC_CALLER, FSM_NONE, OUTER_MONT, STORE_PLAIN, TILE_ONCE, IPN_SLAB>(
          data, data, A, w, 0, lds, lds_tw);
  } else {
    pass_tile<E, LOGR, KIND_FINAL, TW_TWO_LEVEL, RED_GENERIC, PRO_NONE, SRC_CALLER, FSM_NONE, OUTER_MONT, STORE_PLAIN, TILE_ONCE, IPN_SLAB>(
        data, data, A, w, 0, lds, lds_tw);
  }
  if (t == 0)
    s_last = __hip_atomic_fetch_add(A.ipn_sync + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1;
  __syncthreads();
  if (s_last) {  // nobody touches the counters again in this launch
    const uint32_t slabs = (uint32_t)(gridDim.x / A.ipn_strips);
    for (uint32_t m = t; m < slabs; m += blockDim.x) {
      A.ipn_sync[32 * (1 + m)] = 0u;
      A.ipn_sync[32 * (1 + m) + 1] = 0u;
    }
    if (t == 0) {
      A.ipn_sync[0] = A.ipn_sync[1] = 0u;
      if (A.wd.abort) *A.wd.abort = 0u;
    }
  }
}

// The host function of k_final_ipn<E, logr>, or null where the radix has no instance: the launcher and
// the capacity query take their kernel from here
template <class E>
auto final_ipn_kernel(int logr) -> void (*)(uint32_t*, const PassArgs<E>) {
  void (*k)(uint32_t*, const PassArgs<E>) = nullptr;
  (void)with_radix<3, 9>(logr, [&](auto R) {
    if constexpr (R <= tile_log_of<E>() - E::MIN_COLS_LOG) k = &k_final_ipn<E, R>;
    return hipSuccess;
  });
  return k;
}

template <class E>
hipError_t launch_final_ipn(int logr, uint32_t* data, const PassArgs<E>& A, uint32_t grid, hipStream_t st) {
  const auto k = final_ipn_kernel<E>(logr);
  if (!k) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k, dim3(grid), dim3((1 << tile_log_of<E>()) / E::EPT), 0, st, data, A);
  return hipGetLastError();
}

// Workgroups of k_final_ipn<E, logr> the device keeps resident at once (occupancy x CUs; 0 if the
// query fails or the radix has no instance)
template <class E>
uint32_t launch_final_ipn_capacity(int logr, int device) {
  int cus = 0, per = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) return 0;
  const auto k = final_ipn_kernel<E>(logr);
  if (!k || hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, reinterpret_cast<const void*>(k),
                                                         (1 << tile_log_of<E>()) / E::EPT, 0) != hipSuccess)
    return 0;
  return (per > 0 && cus > 0) ? (uint32_t)per * (uint32_t)cus : 0u;
}

// In-place digit reversal after an in-place final pass (NTT_PLAN_IN_PLACE; the replacement for the
// reference's SSIP stage-2 mirror pairs, GZKP-NTT.cu:1359-1449).  With a palindromic radix sequence
// (R_1 = R_p = 2^R, middle widths symmetric) the element at position (k1, mid, kn) =
// k1 2^(L-R) + mid 2^R + kn belongs at (kn, midrev, k1): an involution, so the permutation is a set of
// disjoint swaps.  A workgroup owns the tile pair {(I tb + a, mid, J tb + b)} and its image
// {(J tb + a, midrev, I tb + b)} (a, b < tb): both tiles are read as tb-element contiguous rows, swapped
// through LDS and written back transposed.  Of the two workgroups of a pair the one with the larger
// index exits; a tile that is its own image (mid = midrev, I = J) is transposed in place.
template <int MW>
__global__ __launch_bounds__(256) void k_digitrev_swap(uint32_t* data, DrevArgs A) {
  constexpr int SL = MW + 1;  // LDS slot stride (words): odd, so transposed reads spread over banks
  __shared__ uint32_t tile[2][256 * SL];
  const uint32_t tl = A.tb_log, ntl = A.R - tl;
  const uint64_t u = A.unit0 + blockIdx.x;
  const uint32_t nm = (1u << ntl) - 1;
  const uint32_t lo = (uint32_t)(u & nm), hi = (uint32_t)((u >> ntl) & nm);
  // diagonal order (A.diag): I = lo, J = lo + hi, so that neighbouring workgroups differ in both tile
  // coordinates and neither tile of a pair walks down one column of 2^(log_n - R)-element rows
  // (power-of-two strides that land on the same HBM channels); else row-major (I = hi, J = lo)
  const uint32_t I = A.diag ? lo : hi, J = A.diag ? ((lo + hi) & nm) : lo;
  const uint64_t mid = u >> (2 * ntl);
  uint64_t m = mid, midrev = 0;
  for (uint32_t i = 0; i < A.nmid; ++i) {
    midrev |= (m & ((1ull << A.mid_bits[i]) - 1)) << A.mid_off[i];
    m >>= A.mid_bits[i];
  }
  // the image tile (midrev, J, I) in the same order
  const uint64_t partner = (midrev << (2 * ntl)) |
                           (A.diag ? (((uint64_t)((I - J) & nm) << ntl) | J) : (((uint64_t)J << ntl) | I));
  if (partner < u) return;  // the pair is handled by the partner's workgroup (uniform exit)
  uint32_t* d = data + (size_t)blockIdx.y * A.batch_stride;
  const uint32_t t = threadIdx.x, tb = 1u << tl;
  const bool act = t < (tb << tl);
  const uint32_t a = t >> tl, b = t & (tb - 1);
  const uint32_t sh = A.log_n - A.R;
  const size_t posA = ((size_t)(I * tb + a) << sh) + (mid << A.R) + J * tb + b;
  const size_t posB = ((size_t)(J * tb + a) << sh) + (midrev << A.R) + I * tb + b;
  uint32_t va[MW], vb[MW];
  if (act) {
    if constexpr (MW % 4 == 0) {
#pragma unroll
      for (int w = 0; w < MW / 4; ++w) {
        const uint4 x = reinterpret_cast<const uint4*>(d + posA * MW)[w];
        const uint4 y = reinterpret_cast<const uint4*>(d + posB * MW)[w];
        va[4 * w] = x.x, va[4 * w + 1] = x.y, va[4 * w + 2] = x.z, va[4 * w + 3] = x.w;
        vb[4 * w] = y.x, vb[4 * w + 1] = y.y, vb[4 * w + 2] = y.z, vb[4 * w + 3] = y.w;
      }
    } else {
#pragma unroll
      for (int w = 0; w < MW; ++w) va[w] = d[posA * MW + w], vb[w] = d[posB * MW + w];
    }
#pragma unroll
    for (int w = 0; w < MW; ++w) tile[0][t * SL + w] = va[w], tile[1][t * SL + w] = vb[w];
  }
  __syncthreads();
  if (!act) return;
  const uint32_t tt = (b << tl) + a;  // the transposed slot
#pragma unroll
  for (int w = 0; w < MW; ++w) va[w] = tile[1][tt * SL + w], vb[w] = tile[0][tt * SL + w];
  const bool self = partner == u;
  if constexpr (MW % 4 == 0) {
#pragma unroll
    for (int w = 0; w < MW / 4; ++w) {
      reinterpret_cast<uint4*>(d + posA * MW)[w] = make_uint4(va[4 * w], va[4 * w + 1], va[4 * w + 2], va[4 * w + 3]);
      if (!self)
        reinterpret_cast<uint4*>(d + posB * MW)[w] = make_uint4(vb[4 * w], vb[4 * w + 1], vb[4 * w + 2], vb[4 * w + 3]);
    }
  } else {
#pragma unroll
    for (int w = 0; w < MW; ++w) {
      d[posA * MW + w] = va[w];
      if (!self) d[posB * MW + w] = vb[w];
    }
  }
}

template <class E>
hipError_t launch_digitrev_swap(uint32_t* data, const DrevArgs& A, uint32_t batch, hipStream_t st) {
  if (A.R < A.tb_log || 2 * A.R > A.log_n || A.tb_log > 4) return hipErrorInvalidValue;
  // grid.x * blockDim.x must stay below 2^32 threads: 2^(log_n - 2 tb_log) tile pairs go as launches
  // of at most 2^23 workgroups (A.unit0 = the first pair of the launch)
  const uint64_t units = 1ull << (A.log_n - 2 * A.tb_log), chunk = 1ull << 23;
  for (uint64_t u0 = 0; u0 < units; u0 += chunk) {
    DrevArgs B = A;
    B.unit0 = u0;
    const uint64_t cnt = units - u0 < chunk ? units - u0 : chunk;
    hipLaunchKernelGGL((k_digitrev_swap<E::MEMW>), dim3((uint32_t)cnt, batch), dim3(256), 0, st, data, B);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  }
  return hipSuccess;
}

// The in-place kernels of one engine (ntt_*_misc.hip)
#define NTT_INSTANTIATE_INPLACE(E)                                                                                 \
  template hipError_t launch_digitrev_swap<E>(uint32_t*, const DrevArgs&, uint32_t, hipStream_t);                  \
  template hipError_t launch_final_ipn<E>(int, uint32_t*, const PassArgs<E>&, uint32_t, hipStream_t);              \
  template uint32_t launch_final_ipn_capacity<E>(int, int);

}  // namespace ntt
