// Element-wise kernels, one thread per element: the O(n^2) transform of tiny n, the four-step helpers
// (twiddle-pack, coset scale, transpose), the fills, the pointwise product and the canonical-range
// count.  grid_1d and NTT_GRID_STRIDE, which every grid-stride kernel of the other families uses, live
// here.  Instantiated by the ntt_*_misc.hip units.
#pragma once
#include "ntt_kernels.hpp"

namespace ntt {

// Element-wise kernels run as grid-stride loops over at most 2^20 workgroups of 256 threads:
// grid.x * blockDim.x stays far below HIP's 2^32-thread launch limit at every supported size
// (2^32-element BLS12-381 vectors included).
__host__ __device__ constexpr uint32_t grid_1d(size_t count) {
  return (uint32_t)((count + 255) / 256 < (size_t(1) << 20) ? (count + 255) / 256 : (size_t(1) << 20));
}
#define NTT_GRID_STRIDE(idx, count) \
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < (count); idx += (size_t)gridDim.x * blockDim.x)

// O(n^2) transform for tiny n (n <= 4): X_k = sum_j x_j w^(jk); tw_int holds w^e, e < n.
template <class E>
__global__ void k_dft_naive(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, const PassArgs<E> A) {
  const uint32_t n = 1u << A.log_n;
  const uint32_t k = threadIdx.x;
  const size_t boff = (size_t)blockIdx.y * A.batch_stride;
  uint32_t acc[E::W];
  if (k < n) {
    // acc = x_0 * w^0 (Montgomery by w^0 = R brings it to the engine's residue form)
    uint32_t v[E::W];
    typename E::Tw w;
    E::load(acc, src + boff, 0);
    E::tload(w, A.tw_int, 0);
    E::mul(acc, w, A.F);
#pragma unroll 1
    for (uint32_t j = 1; j < n; ++j) {
      E::load(v, src + boff, j);
      E::tload(w, A.tw_int, (j * k) & (n - 1));
      E::mul(v, w, A.F);
      E::template bfly_l<E::IN>(acc, v, A.F);  // acc <- acc + v (the difference is discarded)
      E::template reduce<2 * E::IN, E::IN>(acc, A.F);
    }
    if (A.flags & 1u) E::mul(acc, A.F.ninv, A.F);
  }
  __syncthreads();  // every thread has read src before anyone writes dst (in-place use)
  if (k < n) E::template store<E::IN>(dst + boff, k, acc, A.F);
}

template <class E>
hipError_t launch_naive(const uint32_t* src, uint32_t* dst, const PassArgs<E>& A, uint32_t batch, hipStream_t st) {
  hipLaunchKernelGGL((k_dft_naive<E>), dim3(1, batch), dim3(64), 0, st, src, dst, A);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------- four-step helpers
// Multi-GPU four-step, local steps.  twiddle_pack: src is [rows][row_len] (row-major);
// element (a, b) is multiplied by w_n^((row0 + a) * b) and written to dst block b / bw (bw =
// row_len / G) at blk * peer_stride + a * bw + b % bw, i.e. dst = [G][rows][bw] (peer_stride =
// rows * bw): one contiguous chunk per peer for the all-to-all.  A larger peer_stride interleaves
// several vectors' chunks per peer (the distributed polymul exchanges a and b in one all-to-all).  Twiddles from the plan's two-level tables: lo_s holds lo * R_e (R_e the engine's
// Montgomery radix), so t = lo_s[e & mask] * hi[e >> lo_bits] = w_n^e R_e and mulv(x, t) = x w_n^e.
template <class E>
__global__ void k_twiddle_pack(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, uint32_t log_rows,
                               uint32_t log_len, uint32_t log_bw, uint64_t row0, uint32_t log_n,
                               const uint32_t* __restrict__ lo, const uint32_t* __restrict__ hi, uint32_t lo_bits,
                               const typename E::Args F, uint64_t peer_stride) {
  NTT_GRID_STRIDE(i, (1ull << (log_rows + log_len))) {
    const uint64_t a = i >> log_len, b = i & ((1ull << log_len) - 1);
    const uint64_t e = ((row0 + a) * b) & ((1ull << log_n) - 1);
    uint32_t x[E::W];
    typename E::Tw w, h;
    E::load(x, src, i);
    E::tload(w, lo, (uint32_t)(e & ((1ull << lo_bits) - 1)));
    E::tload(h, hi, (uint32_t)(e >> lo_bits));
    E::mul(w.w, h, F);
    E::mulv(x, w.w, F);
    const size_t blk = b >> log_bw, off = b & ((1ull << log_bw) - 1);
    E::template store<E::MUL_OUT>(dst, blk * peer_stride + (a << log_bw) + off, x, F);
  }
}

// Coset scale (low-degree-extension step): data[j] *= c^j over `batch` vectors of 2^log_n elements,
// c^j from two-level tables (lo_s[j & mask] = c^lo R_e, hi[j >> lo_bits] = Shoup entries), so
// t = lo_s * hi = c^j R_e and mulv(x, t) = x c^j.  One HBM read + write, two products per element.
template <class E>
__global__ void k_scale_pow(uint32_t* __restrict__ data, uint32_t log_n, const uint32_t* __restrict__ lo_s,
                            const uint32_t* __restrict__ hi, uint32_t lo_bits, const typename E::Args F,
                            size_t batch_stride) {
  NTT_GRID_STRIDE(j, (size_t(1) << log_n)) {
    uint32_t* d = data + (size_t)blockIdx.y * batch_stride;
    uint32_t x[E::W];
    typename E::Tw w, h;
    E::load(x, d, j);
    E::tload(w, lo_s, (uint32_t)(j & ((1ull << lo_bits) - 1)));
    E::tload(h, hi, (uint32_t)(j >> lo_bits));
    E::mul(w.w, h, F);
    E::mulv(x, w.w, F);
    E::template store<E::MUL_OUT>(d, j, x, F);
  }
}

template <class E>
hipError_t launch_scale_pow(uint32_t* data, uint32_t log_n, uint32_t batch, const uint32_t* lo_s, const uint32_t* hi,
                            uint32_t lo_bits, const typename E::Args& F, hipStream_t st) {
  const size_t n = 1ull << log_n;
  const dim3 grid(grid_1d(n), batch);
  hipLaunchKernelGGL((k_scale_pow<E>), grid, dim3(256), 0, st, data, log_n, lo_s, hi, lo_bits, F,
                     n * (size_t)E::MEMW);
  return hipGetLastError();
}

// dst[c][r] = src[r][c] for a rows x cols matrix of MEMW-word elements (32x32 tiles through LDS,
// 16-B vector accesses).  Source rows come in blocks of 2^log_blk_rows rows, block b starting at
// element b * blk_stride (blk_stride = 2^(log_blk_rows + log_cols): one dense matrix; larger: the
// per-peer chunks of an all-to-all that carried several vectors).
template <int MEMW>
__global__ void k_transpose(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, uint32_t log_rows,
                            uint32_t log_cols, uint32_t log_blk_rows, uint64_t blk_stride) {
  constexpr int TILE = 32;
  constexpr bool VEC = (MEMW % 4) == 0;
  __shared__ uint32_t tile[TILE][TILE + 1][MEMW];
  const uint64_t rows = 1ull << log_rows, cols = 1ull << log_cols;
  const uint64_t bx = (uint64_t)blockIdx.x * TILE, by = (uint64_t)blockIdx.y * TILE;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 256 threads: 32 x 8
  for (int k = ty; k < TILE; k += 8) {
    const uint64_t r = by + k, c = bx + tx;
    if (r < rows && c < cols) {
      const uint64_t rin = r & ((1ull << log_blk_rows) - 1);
      const uint32_t* s = src + ((r >> log_blk_rows) * blk_stride + (rin << log_cols) + c) * MEMW;
      if constexpr (VEC) {
#pragma unroll
        for (int w = 0; w < MEMW / 4; ++w) {
          const uint4 v = reinterpret_cast<const uint4*>(s)[w];
          tile[k][tx][4 * w] = v.x;
          tile[k][tx][4 * w + 1] = v.y;
          tile[k][tx][4 * w + 2] = v.z;
          tile[k][tx][4 * w + 3] = v.w;
        }
      } else {
#pragma unroll
        for (int w = 0; w < MEMW; ++w) tile[k][tx][w] = s[w];
      }
    }
  }
  __syncthreads();
  for (int k = ty; k < TILE; k += 8) {
    const uint64_t c = bx + k, r = by + tx;
    if (r < rows && c < cols) {
      uint32_t* d = dst + (c * rows + r) * MEMW;
      if constexpr (VEC) {
#pragma unroll
        for (int w = 0; w < MEMW / 4; ++w)
          reinterpret_cast<uint4*>(d)[w] =
              make_uint4(tile[tx][k][4 * w], tile[tx][k][4 * w + 1], tile[tx][k][4 * w + 2], tile[tx][k][4 * w + 3]);
      } else {
#pragma unroll
        for (int w = 0; w < MEMW; ++w) d[w] = tile[tx][k][w];
      }
    }
  }
}

template <class E>
hipError_t launch_twiddle_pack(const uint32_t* src, uint32_t* dst, uint32_t log_rows, uint32_t log_len,
                               uint32_t log_bw, uint64_t row0, uint32_t log_n, const uint32_t* lo, const uint32_t* hi,
                               uint32_t lo_bits, const typename E::Args& F, uint64_t peer_stride, hipStream_t st) {
  const size_t total = 1ull << (log_rows + log_len);
  hipLaunchKernelGGL((k_twiddle_pack<E>), dim3(grid_1d(total)), dim3(256), 0, st, src, dst, log_rows,
                     log_len, log_bw, row0, log_n, lo, hi, lo_bits, F, peer_stride);
  return hipGetLastError();
}

template <class E>
hipError_t launch_transpose(const uint32_t* src, uint32_t* dst, uint32_t log_rows, uint32_t log_cols,
                            uint32_t log_blk_rows, uint64_t blk_stride, hipStream_t st) {
  const uint64_t rows = 1ull << log_rows, cols = 1ull << log_cols;
  const dim3 grid((uint32_t)((cols + 31) / 32), (uint32_t)((rows + 31) / 32));
  hipLaunchKernelGGL((k_transpose<E::MEMW>), grid, dim3(256), 0, st, src, dst, log_rows, log_cols, log_blk_rows,
                     blk_stride);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------- utility kernels
__device__ __forceinline__ uint64_t splitmix64(uint64_t c) {
  uint64_t z = c + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// SURVEY §8d vector B: limb_i = SplitMix64(seed*2^32 + 4j + i) (64-bit limbs), limbs at and above
// `nrand` zero, the top random limb masked to `top_bits` so that every value is < p.
struct FillMap {
  uint64_t row0;       // global index of local row 0
  uint32_t log_inner;  // local row length (log2); 64 = identity map
  uint32_t log_stride; // global stride of the inner index (log2)
};
__device__ __forceinline__ uint64_t fill_index(size_t i, const FillMap& m) {
  if (m.log_inner >= 64) return i;
  return m.row0 + (i >> m.log_inner) + ((uint64_t)(i & ((1ull << m.log_inner) - 1)) << m.log_stride);
}

template <int MEMW>
__global__ void k_fill_random(uint32_t* __restrict__ dst, size_t n, uint64_t seed, uint32_t nrand, uint32_t top_bits,
                              FillMap fm) {
  NTT_GRID_STRIDE(i, n) {
    const uint64_t j = fill_index(i, fm);
    if constexpr (MEMW == 1) {  // 4-B elements: the low limb's draw masked below 2^31 (top_bits <= 30)
      dst[i] = (uint32_t)(splitmix64((seed << 32) + 4 * j) & ((1ull << top_bits) - 1));
    } else if constexpr (MEMW == 2) {
      const uint64_t v = splitmix64((seed << 32) + 4 * j) & ((1ull << top_bits) - 1);
      reinterpret_cast<uint2*>(dst)[i] = make_uint2((uint32_t)v, (uint32_t)(v >> 32));  // P: top_bits < 32
    } else {
      uint32_t v[MEMW];
#pragma unroll
      for (int l = 0; l < MEMW / 2; ++l) {
        uint64_t limb = 0;
        if ((uint32_t)l < nrand) {
          limb = splitmix64((seed << 32) + 4 * j + l);
          if ((uint32_t)l + 1 == nrand && top_bits < 64) limb &= (1ull << top_bits) - 1;
        }
        v[2 * l] = (uint32_t)limb;
        v[2 * l + 1] = (uint32_t)(limb >> 32);
      }
      uint4* p = reinterpret_cast<uint4*>(dst + i * MEMW);
#pragma unroll
      for (int q = 0; q < MEMW / 4; ++q) p[q] = make_uint4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
    }
  }
}

template <int MEMW>
__global__ void k_fill_iota(uint32_t* __restrict__ dst, size_t n, FillMap fm) {
  NTT_GRID_STRIDE(i, n) {
    const uint64_t j = fill_index(i, fm);
    if constexpr (MEMW == 1) {  // 4-B elements: the index's low word (plans of at most 2^27 points)
      dst[i] = (uint32_t)j;
    } else if constexpr (MEMW == 2) {
      reinterpret_cast<uint2*>(dst)[i] = make_uint2((uint32_t)j, (uint32_t)((uint64_t)j >> 32));
    } else {
      uint4* p = reinterpret_cast<uint4*>(dst + i * MEMW);
      p[0] = make_uint4((uint32_t)j, (uint32_t)((uint64_t)j >> 32), 0u, 0u);
#pragma unroll
      for (int q = 1; q < MEMW / 4; ++q) p[q] = make_uint4(0u, 0u, 0u, 0u);
    }
  }
}

template <class E>
__global__ void k_pointwise_mul(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, uint32_t* __restrict__ c,
                                size_t n, const typename E::Args F, const uint32_t* __restrict__ r2, const FsMap m,
                                const uint32_t mapped) {
  NTT_GRID_STRIDE(j, n) {
    uint32_t x[E::W], y[E::W];
    typename E::Tw z;  // R_e mod p as a twiddle: mulv leaves x y / R_e
    const size_t src = mapped ? m(j, 0) : j;  // a four-step piece gathered from the column layout
    E::load(x, a, src);
    E::load(y, b, src);
    E::tload(z, r2, 0);
    E::mulv(x, y, F);
    E::mul(x, z, F);
    E::template store<E::MUL_OUT>(c, j, x, F);
  }
}

// Canonical-range check (the reference's padded-store `BAD LIMB` trap, impl_cuda.cu:1402-1408, as a
// query): counts elements that are not < p in a caller buffer of E::MEMW-word elements.  p holds
// the modulus in MEMW little-endian 32-bit words (zero above its top word).
template <int MEMW>
__global__ void k_count_noncanonical(const uint32_t* __restrict__ d, size_t n, ModWords<MEMW> p,
                                     unsigned long long* __restrict__ bad) {
  NTT_GRID_STRIDE(i, n) {
    const uint32_t* e = d + i * MEMW;
    int cmp = 0;  // sign of e - p, decided by the most significant differing word
#pragma unroll
    for (int k = MEMW - 1; k >= 0; --k)
      if (cmp == 0 && e[k] != p.w[k]) cmp = e[k] < p.w[k] ? -1 : 1;
    if (cmp >= 0) atomicAdd(bad, 1ull);
  }
}

template <class E>
hipError_t launch_count_noncanonical(const uint32_t* d, size_t n, const ModWords<E::MEMW>& p,
                                     unsigned long long* bad, hipStream_t st) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL((k_count_noncanonical<E::MEMW>), dim3(grid_1d(n)), dim3(256), 0, st, d, n, p,
                     bad);
  return hipGetLastError();
}

template <class E>
hipError_t launch_fill(int kind, uint32_t* dst, size_t n, uint64_t seed, uint32_t nrand, uint32_t top_bits,
                       uint64_t row0, uint32_t log_inner, uint32_t log_stride, hipStream_t st) {
  const uint32_t blocks = grid_1d(n);
  const FillMap fm{row0, log_inner, log_stride};
  if (kind == 0)
    hipLaunchKernelGGL((k_fill_iota<E::MEMW>), dim3(blocks), dim3(256), 0, st, dst, n, fm);
  else
    hipLaunchKernelGGL((k_fill_random<E::MEMW>), dim3(blocks), dim3(256), 0, st, dst, n, seed, nrand, top_bits, fm);
  return hipGetLastError();
}

template <class E>
hipError_t launch_pointwise(const uint32_t* a, const uint32_t* b, uint32_t* c, size_t n, const typename E::Args& F,
                            const uint32_t* d_r2, hipStream_t st, const FsMap* in_map) {
  const uint32_t blocks = grid_1d(n);
  const FsMap m = in_map ? *in_map : FsMap{};
  hipLaunchKernelGGL((k_pointwise_mul<E>), dim3(blocks), dim3(256), 0, st, a, b, c, n, F, d_r2, m, in_map ? 1u : 0u);
  return hipGetLastError();
}

// The element-wise kernels of one engine (ntt_*_misc.hip)
#define NTT_INSTANTIATE_ELEMENTWISE(E)                                                                             \
  template hipError_t launch_naive<E>(const uint32_t*, uint32_t*, const PassArgs<E>&, uint32_t, hipStream_t);       \
  template hipError_t launch_fill<E>(int, uint32_t*, size_t, uint64_t, uint32_t, uint32_t, uint64_t, uint32_t,     \
                                     uint32_t, hipStream_t);                                                       \
  template hipError_t launch_twiddle_pack<E>(const uint32_t*, uint32_t*, uint32_t, uint32_t, uint32_t, uint64_t,   \
                                             uint32_t, const uint32_t*, const uint32_t*, uint32_t,                 \
                                             const typename E::Args&, uint64_t, hipStream_t);                      \
  template hipError_t launch_transpose<E>(const uint32_t*, uint32_t*, uint32_t, uint32_t, uint32_t, uint64_t,     \
                                          hipStream_t);                                                            \
  template hipError_t launch_pointwise<E>(const uint32_t*, const uint32_t*, uint32_t*, size_t,                     \
                                          const typename E::Args&, const uint32_t*, hipStream_t, const FsMap*);    \
  template hipError_t launch_scale_pow<E>(uint32_t*, uint32_t, uint32_t, const uint32_t*, const uint32_t*, uint32_t, \
                                          const typename E::Args&, hipStream_t);                                   \
  template hipError_t launch_count_noncanonical<E>(const uint32_t*, size_t, const ModWords<E::MEMW>&,              \
                                                   unsigned long long*, hipStream_t);

}  // namespace ntt
