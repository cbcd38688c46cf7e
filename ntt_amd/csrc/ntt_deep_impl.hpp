// The DEEP kernels (ntt_deep_points, ntt_matrix_open, ntt_deep_quotient) over a row-major
// matrix M = [N][width] of base-field coset evaluations and degree-D extension values.  Included by
// ntt_eg_deep.hip and ntt_e31_deep.hip alone.
//
// Forms.  M, values and out are in the plan's I/O form; inv = (z - x_i)^-1, the table scale alpha^j and the
// host scalars are in the field's working form (fieldext.hpp xf: v 2^32 mod p on Eng31, the value on
// Eng64G), so xf::mul / xf::scale of one of them with a datum is the plain product in the datum's form.
//
//   k_deep_points    A thread owns R = 16 / (D E::MEMW) consecutive rows (64 B of output): x_i from the plan's
//                    two-level tables, the R values z - x_i inverted with ONE extension inverse (Montgomery's
//                    batch trick: prefix products, one inverse, the walk back), the rows through LDS so that
//                    lane l of the workgroup stores 16 B at base + 16 l.
//   k_deep_open      A workgroup owns a strip of 2^strip_log adjacent columns (64 B of a row at least, a wave's
//                    width at most, the last strip masked) x a chunk of rows: thread (r, c) walks rows
//                    r, r + BT / strip, .. of column c with UNROLL rows in flight, so every wave load covers
//                    runs of the strip's bytes; it sums M[i][j] inv_i (D products) and M[i][j] in registers,
//                    the workgroup's threads of one column meet in an LDS tree, and the strip's D + 1 sums go
//                    to the plan's scratch at [chunk][component][column].
//   k_deep_open_fin  A workgroup owns 16 columns x 16 chunk lanes: lane l adds chunks l, l + 16, .. in order, the
//                    lanes meet in a fixed LDS tree (no atomics: the same bits every run), and the column's
//                    thread stores K (z S1 - S0), K = (z^N - c^N) / (N c^N).
//   k_deep_qpro      Workgroup 0: V = scale sum_j alpha^j v_j, each thread a run of columns (one power, then
//                    one product per column), an LDS tree; workgroups 1..: the table scale alpha^j, one
//                    square-and-multiply power per thread.  Both into the plan's scratch.
//   k_deep_quotient  2^lanes_log lanes share a row and stride its columns (DeepShape::lanes_log: runs of 64 B and
//                    more per wave load, four columns a lane where the width allows; rows shorter than 64 B:
//                    one lane per row, the wave reads 64 consecutive rows); a wave
//                    owns 64 consecutive rows and takes 64 >> lanes_log of them per step; the row sums meet by
//                    xor shuffles and lane l fetches row l's sum, so that the output row is one store per
//                    lane at consecutive addresses.  The table's first TAB_COLS columns are in LDS, D values
//                    side by side (one ds_read_b128 / b64 per element, consecutive lanes consecutive slots);
//                    the columns beyond come from the scratch itself.
// Checked build: an index outside its buffer sets 0x100 and goes to element 0, a non-canonical input element
// 0x200, a non-canonical output 0x800.
#pragma once
#include <type_traits>

#include "fieldext.hpp"
#include "ntt_kernels.hpp"

namespace ntt {

template <class E>
__device__ __forceinline__ deep_val_t<E> deep_ld(const uint32_t* __restrict__ base, size_t idx) {
  if constexpr (E::MEMW == 1) {
    return base[idx];
  } else {
    const uint2 v = reinterpret_cast<const uint2*>(base)[idx];
    return ((uint64_t)v.y << 32) | v.x;
  }
}
template <class E>
__device__ __forceinline__ void deep_st(uint32_t* __restrict__ base, size_t idx, deep_val_t<E> v) {
  if constexpr (E::MEMW == 1)
    base[idx] = v;
  else
    reinterpret_cast<uint2*>(base)[idx] = make_uint2((uint32_t)v, (uint32_t)(v >> 32));
}
// checked build: element index idx (count elements from it) against a buffer of n elements
template <class E>
__device__ __forceinline__ size_t deep_idx(size_t idx, [[maybe_unused]] size_t count, [[maybe_unused]] size_t n,
                                           [[maybe_unused]] const DeepArgs<E>& A) {
#if NTT_DEBUG_CHECKS
  if (idx + count > n) {
    ntt_dbg_flag(A.F.dbg, NTT_DBG_BOUNDS);
    return 0;
  }
#endif
  return idx;
}
template <class E>
__device__ __forceinline__ void deep_check([[maybe_unused]] deep_val_t<E> v, [[maybe_unused]] uint32_t bit,
                                           [[maybe_unused]] const DeepArgs<E>& A) {
#if NTT_DEBUG_CHECKS
  if (!xf::canonical(v, A.K)) ntt_dbg_flag(A.F.dbg, bit);
#endif
}
// one row of D elements at element index row D: 16-byte accesses when vec
template <class E, int D>
__device__ __forceinline__ void deep_ld_row(deep_val_t<E> (&x)[D], const uint32_t* __restrict__ base, size_t row, bool vec) {
  constexpr int RW = D * E::MEMW;
  uint32_t w[RW];
  if (vec && RW >= 4) {
    const uint4* p4 = reinterpret_cast<const uint4*>(base + row * RW);
#pragma unroll
    for (int q = 0; q < RW / 4; ++q) {
      const uint4 v = p4[q];
      w[4 * q] = v.x, w[4 * q + 1] = v.y, w[4 * q + 2] = v.z, w[4 * q + 3] = v.w;
    }
  } else if (RW >= 2 && (E::MEMW == 2 || vec)) {
    const uint2* p2 = reinterpret_cast<const uint2*>(base + row * RW);
#pragma unroll
    for (int q = 0; q < RW / 2; ++q) {
      const uint2 v = p2[q];
      w[2 * q] = v.x, w[2 * q + 1] = v.y;
    }
  } else {
#pragma unroll
    for (int q = 0; q < RW; ++q) w[q] = base[row * RW + q];
  }
#pragma unroll
  for (int j = 0; j < D; ++j) {
    if constexpr (E::MEMW == 1)
      x[j] = w[j];
    else
      x[j] = ((uint64_t)w[2 * j + 1] << 32) | w[2 * j];
  }
}
template <class E, int D>
__device__ __forceinline__ void deep_st_row(uint32_t* __restrict__ base, size_t row, const deep_val_t<E> (&x)[D], bool vec) {
  constexpr int RW = D * E::MEMW;
  uint32_t w[RW];
#pragma unroll
  for (int j = 0; j < D; ++j) {
    if constexpr (E::MEMW == 1) {
      w[j] = x[j];
    } else {
      w[2 * j] = (uint32_t)x[j];
      w[2 * j + 1] = (uint32_t)(x[j] >> 32);
    }
  }
  if (vec && RW >= 4) {
    uint4* p4 = reinterpret_cast<uint4*>(base + row * RW);
#pragma unroll
    for (int q = 0; q < RW / 4; ++q) p4[q] = make_uint4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
  } else if (RW >= 2 && (E::MEMW == 2 || vec)) {
    uint2* p2 = reinterpret_cast<uint2*>(base + row * RW);
#pragma unroll
    for (int q = 0; q < RW / 2; ++q) p2[q] = make_uint2(w[2 * q], w[2 * q + 1]);
  } else {
#pragma unroll
    for (int q = 0; q < RW; ++q) base[row * RW + q] = w[q];
  }
}

// ------------------------------------------------------------------------------ points
template <class E, int D>
__global__ __launch_bounds__(DeepShape::BT) void k_deep_points(uint32_t* __restrict__ out, const DeepArgs<E> A) {
  using V = deep_val_t<E>;
  constexpr int BT = DeepShape::BT, RW = D * E::MEMW, RUN = DeepShape::RUN_WORDS, R = RUN / RW;
  constexpr int STRIDE = RUN + 4;  // LDS words per thread: 4 mod 8, as the fold's staging rows
  __shared__ uint4 lds4[BT * STRIDE / 4];
  uint32_t* lds = reinterpret_cast<uint32_t*>(lds4);
  const uint32_t tid = threadIdx.x;
  const size_t n = (size_t)1 << A.log_rows;
  const size_t row0 = ((size_t)blockIdx.x * BT + tid) * R;

  V a[R][D], pre[R][D];
#pragma unroll
  for (int k = 0; k < R; ++k) {
    const size_t row = row0 + k;
#pragma unroll
    for (int j = 0; j < D; ++j) a[k][j] = j ? V(0) : A.K.one;  // rows past the end: 1
    if (row < n) {
      const uint32_t s = (A.bitrev && A.log_rows) ? (__brev((uint32_t)row) >> (32 - A.log_rows)) : (uint32_t)row;
      const uint64_t e = (uint64_t)s << A.tab_shift;
      typename E::Tw lo, hi;
      E::tload(lo, A.lo_s, (size_t)(e & ((1ull << A.lo_bits) - 1)));
      E::tload(hi, A.hi, (size_t)(e >> A.lo_bits));
      E::mul(lo.w, hi, A.F);
      E::mul(lo.w, A.c, A.F);  // x_i in the working form
      V x;
      if constexpr (E::MEMW == 1)
        x = lo.w[0];
      else
        x = Eng64G::u64(lo.w);
      a[k][0] = xf::sub(A.z[0], x, A.K);
#pragma unroll
      for (int j = 1; j < D; ++j) a[k][j] = A.z[j];
    }
  }
#pragma unroll
  for (int j = 0; j < D; ++j) pre[0][j] = a[0][j];
#pragma unroll
  for (int k = 1; k < R; ++k) xf::mul<D>(pre[k], pre[k - 1], a[k], A.K);
  V t[D];
  xf::inv<D>(t, pre[R - 1], A.K);
#pragma unroll
  for (int k = R - 1; k >= 1; --k) {
    V r[D];
    xf::mul<D>(r, t, pre[k - 1], A.K);
    xf::mul<D>(t, t, a[k], A.K);
#pragma unroll
    for (int j = 0; j < D; ++j) pre[k][j] = r[j];
  }
#pragma unroll
  for (int j = 0; j < D; ++j) pre[0][j] = t[j];

  {
    uint32_t w[RUN];
#pragma unroll
    for (int k = 0; k < R; ++k)
#pragma unroll
      for (int j = 0; j < D; ++j) {
        deep_check<E>(pre[k][j], NTT_DBG_OUTPUT, A);
        if constexpr (E::MEMW == 1) {
          w[k * RW + j] = pre[k][j];
        } else {
          w[k * RW + 2 * j] = (uint32_t)pre[k][j];
          w[k * RW + 2 * j + 1] = (uint32_t)(pre[k][j] >> 32);
        }
      }
#pragma unroll
    for (int q = 0; q < RUN / 4; ++q)
      lds4[tid * (STRIDE / 4) + q] = make_uint4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
  }
  __syncthreads();
  const size_t total = n * RW, gb = (size_t)blockIdx.x * BT * RUN;  // words
  if (A.vec) {
    uint4* __restrict__ o4 = reinterpret_cast<uint4*>(out);
#pragma unroll
    for (int it = 0; it < RUN / 4; ++it) {
      const uint32_t f = 4 * (it * BT + tid);
      if (gb + f < total) {
        const size_t at = deep_idx<E>(gb + f, 4, A.inv_elems * E::MEMW, A);
        o4[at / 4] = lds4[(f / RUN) * (STRIDE / 4) + (f % RUN) / 4];
      }
    }
  } else {
#pragma unroll
    for (int it = 0; it < RUN; ++it) {
      const uint32_t f = it * BT + tid;
      if (gb + f < total) out[deep_idx<E>(gb + f, 1, A.inv_elems * E::MEMW, A)] = lds[(f / RUN) * STRIDE + f % RUN];
    }
  }
}

// ------------------------------------------------------------------------------ open
template <class E, int D>
__global__ __launch_bounds__(DeepShape::BT) void k_deep_open(const uint32_t* __restrict__ mat, const uint32_t* __restrict__ inv,
                                                            uint32_t* __restrict__ part, const DeepArgs<E> A) {
  using V = deep_val_t<E>;
  constexpr int BT = DeepShape::BT, U = DeepShape::UNROLL;
  __shared__ V red[D + 1][BT];
  const uint32_t tid = threadIdx.x, csl = A.strip_log, cs = 1u << csl, rps = BT >> csl;
  const uint32_t ns = (A.width + cs - 1) >> csl;
  const uint32_t strip = blockIdx.x % ns, chunk = blockIdx.x / ns;
  const uint32_t col = (strip << csl) + (tid & (cs - 1));
  const bool live = col < A.width;
  const size_t n = (size_t)1 << A.log_rows;
  const size_t r0 = (size_t)chunk * A.chunk_rows, r1 = r0 + A.chunk_rows < n ? r0 + A.chunk_rows : n;
  const bool vec = A.vec != 0;

  V s1[D], s0 = 0;
#pragma unroll
  for (int j = 0; j < D; ++j) s1[j] = 0;
  for (size_t r = r0 + (tid >> csl); r < r1; r += (size_t)rps * U) {
    V m[U], iv[U][D];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const size_t row = r + (size_t)u * rps;
      const bool ok = live && row < r1;
      m[u] = 0;
#pragma unroll
      for (int j = 0; j < D; ++j) iv[u][j] = 0;
      if (ok) {
        m[u] = deep_ld<E>(mat, deep_idx<E>(row * A.width + col, 1, A.mat_elems, A));
        deep_ld_row<E, D>(iv[u], inv, deep_idx<E>(row * D, D, A.inv_elems, A) / D, vec);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      deep_check<E>(m[u], NTT_DBG_INPUT, A);
      V t[D];
#pragma unroll
      for (int j = 0; j < D; ++j) deep_check<E>(iv[u][j], NTT_DBG_INPUT, A);
      xf::scale<D>(t, iv[u], m[u], A.K);
      xf::add<D>(s1, s1, t, A.K);
      s0 = xf::add(s0, m[u], A.K);
    }
  }
#pragma unroll
  for (int j = 0; j < D; ++j) red[j][tid] = s1[j];
  red[D][tid] = s0;
  for (uint32_t s = BT / 2; s >= cs; s >>= 1) {
    __syncthreads();
    if (tid < s) {
#pragma unroll
      for (int j = 0; j <= D; ++j) red[j][tid] = xf::add(red[j][tid], red[j][tid + s], A.K);
    }
  }
  __syncthreads();
  if (tid < cs && live) {
#pragma unroll
    for (int j = 0; j <= D; ++j) {
      const size_t at = ((size_t)chunk * (D + 1) + j) * A.width + col;
      deep_st<E>(part, deep_idx<E>(at, 1, A.scr_elems, A), red[j][tid]);
    }
  }
}

template <class E, int D>
__global__ __launch_bounds__(DeepShape::BT) void k_deep_open_fin(const uint32_t* __restrict__ part, uint32_t* __restrict__ values,
                                                                const DeepArgs<E> A) {
  using V = deep_val_t<E>;
  constexpr uint32_t BT = DeepShape::BT, FC = DeepShape::FIN_COLS, CL = BT / FC;  // FC columns x CL chunk lanes
  __shared__ V red[D + 1][BT];
  const uint32_t tid = threadIdx.x;
  const size_t col = (size_t)blockIdx.x * FC + (tid & (FC - 1));
  const bool live = col < A.width;
  V s[D + 1];
#pragma unroll
  for (int j = 0; j <= D; ++j) s[j] = 0;
  if (live) {
#pragma unroll 4
    for (uint32_t c = tid / FC; c < A.chunks; c += CL) {
#pragma unroll
      for (int j = 0; j <= D; ++j) {
        const size_t at = ((size_t)c * (D + 1) + j) * A.width + col;
        s[j] = xf::add(s[j], deep_ld<E>(part, deep_idx<E>(at, 1, A.scr_elems, A)), A.K);
      }
    }
  }
#pragma unroll
  for (int j = 0; j <= D; ++j) red[j][tid] = s[j];
  for (uint32_t h = BT / 2; h >= FC; h >>= 1) {  // a fixed tree: the same bits every run
    __syncthreads();
    if (tid < h) {
#pragma unroll
      for (int j = 0; j <= D; ++j) red[j][tid] = xf::add(red[j][tid], red[j][tid + h], A.K);
    }
  }
  __syncthreads();
  if (tid >= FC || !live) return;
  V s1[D], z[D], k[D], t[D];
#pragma unroll
  for (int j = 0; j < D; ++j) s1[j] = red[j][tid], z[j] = A.z[j], k[j] = A.k[j];
  xf::mul<D>(t, s1, z, A.K);  // sum_i M x_i / (z - x_i) = z S1 - S0
  t[0] = xf::sub(t[0], red[D][tid], A.K);
  xf::mul<D>(t, t, k, A.K);
#pragma unroll
  for (int j = 0; j < D; ++j) deep_check<E>(t[j], NTT_DBG_OUTPUT, A);
  deep_st_row<E, D>(values, deep_idx<E>(col * D, D, A.val_elems, A) / D, t, A.vec != 0);
}

// ------------------------------------------------------------------------------ quotient
template <class E, int D>
__global__ __launch_bounds__(DeepShape::BT) void k_deep_qpro(const uint32_t* __restrict__ values, uint32_t* __restrict__ scr,
                                                            const DeepArgs<E> A) {
  using V = deep_val_t<E>;
  constexpr int BT = DeepShape::BT;
  __shared__ V red[D][BT];
  const uint32_t tid = threadIdx.x;
  V al[D], sc[D], t[D];
#pragma unroll
  for (int j = 0; j < D; ++j) al[j] = A.alpha[j], sc[j] = A.scale[j];
  if (blockIdx.x != 0) {  // the table: scale alpha^j
    const size_t col = (size_t)(blockIdx.x - 1) * BT + tid;
    if (col >= A.width) return;
    xf::pow<D>(t, al, (uint64_t)col, A.K);
    xf::mul<D>(t, t, sc, A.K);
    const size_t at = deep_idx<E>(DeepShape::SCR_TAB + col * D, D, A.scr_elems, A);
#pragma unroll
    for (int j = 0; j < D; ++j) deep_st<E>(scr, at + j, t[j]);
    return;
  }
  // V = sum_j (scale alpha^j) v_j: thread t takes columns [t len, (t + 1) len)
  const size_t len = ((size_t)A.width + BT - 1) / BT, j0 = tid * len;
  const size_t j1 = j0 + len < A.width ? j0 + len : A.width;
  V acc[D];
#pragma unroll
  for (int j = 0; j < D; ++j) acc[j] = 0;
  if (j0 < j1) {
    xf::pow<D>(t, al, (uint64_t)j0, A.K);
    xf::mul<D>(t, t, sc, A.K);
    for (size_t c = j0; c < j1; ++c) {
      V v[D], pr[D];
      deep_ld_row<E, D>(v, values, deep_idx<E>(c * D, D, A.val_elems, A) / D, A.vec != 0);
#pragma unroll
      for (int j = 0; j < D; ++j) deep_check<E>(v[j], NTT_DBG_INPUT, A);
      xf::mul<D>(pr, v, t, A.K);
      xf::add<D>(acc, acc, pr, A.K);
      xf::mul<D>(t, t, al, A.K);
    }
  }
#pragma unroll
  for (int j = 0; j < D; ++j) red[j][tid] = acc[j];
  for (uint32_t s = BT / 2; s >= 1; s >>= 1) {
    __syncthreads();
    if (tid < s) {
#pragma unroll
      for (int j = 0; j < D; ++j) red[j][tid] = xf::add(red[j][tid], red[j][tid + s], A.K);
    }
  }
  if (tid == 0) {
#pragma unroll
    for (int j = 0; j < D; ++j) deep_st<E>(scr, deep_idx<E>(j, 1, A.scr_elems, A), red[j][0]);
  }
}

template <class E, int D>
__global__ __launch_bounds__(DeepShape::BT) void k_deep_quotient(const uint32_t* __restrict__ mat, const uint32_t* __restrict__ inv,
                                                                const uint32_t* __restrict__ scr, uint32_t* __restrict__ out,
                                                                const DeepArgs<E> A) {
  using V = deep_val_t<E>;
  constexpr int BT = DeepShape::BT;
  constexpr uint32_t TC = DeepShape::TAB_COLS;
  __shared__ __attribute__((aligned(16))) V tab[TC * D];
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t wl = A.width < TC ? A.width : TC;  // columns whose table entries are in LDS
  for (uint32_t i = tid; i < wl * D; i += BT) tab[i] = deep_ld<E>(scr, deep_idx<E>(DeepShape::SCR_TAB + i, 1, A.scr_elems, A));
  __syncthreads();

  const uint32_t gl = A.lanes_log, g = 1u << gl, rpw_log = 6 - gl;
  const uint32_t grp = lane >> gl, li = lane & (g - 1);
  const size_t n = (size_t)1 << A.log_rows;
  const size_t rb = ((size_t)blockIdx.x * (BT / 64) + wave) * 64;  // the wave's 64 rows
  const bool vec = A.vec != 0;
  V res[D];
#pragma unroll
  for (int j = 0; j < D; ++j) res[j] = 0;
  for (uint32_t k = 0; k < g; ++k) {
    const size_t row = rb + ((size_t)k << rpw_log) + grp;
    const bool ok = row < n;
    V acc[D];
#pragma unroll
    for (int j = 0; j < D; ++j) acc[j] = 0;
    if (ok) {
      const size_t mb = row * A.width;
#pragma unroll 4
      for (uint32_t c = li; c < wl; c += g) {
        const V m = deep_ld<E>(mat, deep_idx<E>(mb + c, 1, A.mat_elems, A));
        deep_check<E>(m, NTT_DBG_INPUT, A);
        V t[D], pr[D];
#pragma unroll
        for (int j = 0; j < D; ++j) t[j] = tab[c * D + j];
        xf::scale<D>(pr, t, m, A.K);
        xf::add<D>(acc, acc, pr, A.K);
      }
#pragma unroll 2
      for (uint32_t c = wl + li; c < A.width; c += g) {
        const V m = deep_ld<E>(mat, deep_idx<E>(mb + c, 1, A.mat_elems, A));
        deep_check<E>(m, NTT_DBG_INPUT, A);
        V t[D], pr[D];
        const size_t at = deep_idx<E>(DeepShape::SCR_TAB + (size_t)c * D, D, A.scr_elems, A);
#pragma unroll
        for (int j = 0; j < D; ++j) t[j] = deep_ld<E>(scr, at + j);
        xf::scale<D>(pr, t, m, A.K);
        xf::add<D>(acc, acc, pr, A.K);
      }
    }
    for (uint32_t s = g >> 1; s >= 1; s >>= 1) {
#pragma unroll
      for (int j = 0; j < D; ++j) acc[j] = xf::add(acc[j], (V)__shfl_xor(acc[j], (int)s), A.K);
    }
    // lane l keeps the sum of row rb + l: step l >> rpw_log, group l mod 2^rpw_log
    const int src = (int)((lane & ((1u << rpw_log) - 1)) << gl);
#pragma unroll
    for (int j = 0; j < D; ++j) {
      const V v = (V)__shfl(acc[j], src);
      if ((lane >> rpw_log) == k) res[j] = v;
    }
  }
  const size_t row = rb + lane;
  if (row >= n) return;
  V big[D], iv[D], o[D];
#pragma unroll
  for (int j = 0; j < D; ++j) big[j] = deep_ld<E>(scr, deep_idx<E>(j, 1, A.scr_elems, A));
  deep_ld_row<E, D>(iv, inv, deep_idx<E>(row * D, D, A.inv_elems, A) / D, vec);
#pragma unroll
  for (int j = 0; j < D; ++j) deep_check<E>(iv[j], NTT_DBG_INPUT, A);
  xf::sub<D>(o, big, res, A.K);
  xf::mul<D>(o, o, iv, A.K);
  const size_t orow = deep_idx<E>(row * D, D, A.out_elems, A) / D;
  if (A.flags & 1u) {
    V old[D];
    deep_ld_row<E, D>(old, out, orow, vec);
#pragma unroll
    for (int j = 0; j < D; ++j) deep_check<E>(old[j], NTT_DBG_INPUT, A);
    xf::add<D>(o, o, old, A.K);
  }
#pragma unroll
  for (int j = 0; j < D; ++j) deep_check<E>(o[j], NTT_DBG_OUTPUT, A);
  deep_st_row<E, D>(out, orow, o, vec);
}

// ------------------------------------------------------------------------------ launchers
#define NTT_DEEP_SWITCH_D(d, CALL) \
  switch (d) {                     \
    case 1: CALL(1); break;        \
    case 2: CALL(2); break;        \
    case 4: CALL(4); break;        \
    default: return hipErrorInvalidValue; \
  }

template <class E>
hipError_t launch_deep_points(unsigned d, uint32_t* inv, const DeepArgs<E>& A, hipStream_t st) {
  const size_t n = (size_t)1 << A.log_rows;
#define NTT_DEEP_CALL(DD)                                                                                   \
  {                                                                                                         \
    constexpr size_t per = (size_t)DeepShape::BT * (DeepShape::RUN_WORDS / (DD * E::MEMW));                 \
    hipLaunchKernelGGL((k_deep_points<E, DD>), dim3((unsigned)((n + per - 1) / per)), dim3(DeepShape::BT), 0, st, inv, A); \
  }
  NTT_DEEP_SWITCH_D(d, NTT_DEEP_CALL)
#undef NTT_DEEP_CALL
  return hipGetLastError();
}
template <class E>
hipError_t launch_deep_open(unsigned d, const uint32_t* mat, const uint32_t* inv, uint32_t* part, const DeepArgs<E>& A,
                            hipStream_t st) {
  const unsigned grid = DeepShape::strips(A.width, E::MEMW) * A.chunks;
#define NTT_DEEP_CALL(DD) hipLaunchKernelGGL((k_deep_open<E, DD>), dim3(grid), dim3(DeepShape::BT), 0, st, mat, inv, part, A)
  NTT_DEEP_SWITCH_D(d, NTT_DEEP_CALL)
#undef NTT_DEEP_CALL
  return hipGetLastError();
}
template <class E>
hipError_t launch_deep_open_fin(unsigned d, const uint32_t* part, uint32_t* values, const DeepArgs<E>& A, hipStream_t st) {
  const unsigned grid = (A.width + DeepShape::FIN_COLS - 1) / DeepShape::FIN_COLS;
#define NTT_DEEP_CALL(DD) hipLaunchKernelGGL((k_deep_open_fin<E, DD>), dim3(grid), dim3(DeepShape::BT), 0, st, part, values, A)
  NTT_DEEP_SWITCH_D(d, NTT_DEEP_CALL)
#undef NTT_DEEP_CALL
  return hipGetLastError();
}
template <class E>
hipError_t launch_deep_qpro(unsigned d, const uint32_t* values, uint32_t* scr, const DeepArgs<E>& A, hipStream_t st) {
  const unsigned grid = 1 + (A.width + DeepShape::BT - 1) / DeepShape::BT;
#define NTT_DEEP_CALL(DD) hipLaunchKernelGGL((k_deep_qpro<E, DD>), dim3(grid), dim3(DeepShape::BT), 0, st, values, scr, A)
  NTT_DEEP_SWITCH_D(d, NTT_DEEP_CALL)
#undef NTT_DEEP_CALL
  return hipGetLastError();
}
template <class E>
hipError_t launch_deep_quotient(unsigned d, const uint32_t* mat, const uint32_t* inv, const uint32_t* scr, uint32_t* out,
                                const DeepArgs<E>& A, hipStream_t st) {
  const size_t n = (size_t)1 << A.log_rows;
  const unsigned grid = (unsigned)((n + DeepShape::BT - 1) / DeepShape::BT);
#define NTT_DEEP_CALL(DD) \
  hipLaunchKernelGGL((k_deep_quotient<E, DD>), dim3(grid), dim3(DeepShape::BT), 0, st, mat, inv, scr, out, A)
  NTT_DEEP_SWITCH_D(d, NTT_DEEP_CALL)
#undef NTT_DEEP_CALL
  return hipGetLastError();
}

#define NTT_INSTANTIATE_DEEP(E)                                                                                        \
  template hipError_t launch_deep_points<E>(unsigned, uint32_t*, const DeepArgs<E>&, hipStream_t);                      \
  template hipError_t launch_deep_open<E>(unsigned, const uint32_t*, const uint32_t*, uint32_t*, const DeepArgs<E>&,    \
                                          hipStream_t);                                                                \
  template hipError_t launch_deep_open_fin<E>(unsigned, const uint32_t*, uint32_t*, const DeepArgs<E>&, hipStream_t);   \
  template hipError_t launch_deep_qpro<E>(unsigned, const uint32_t*, uint32_t*, const DeepArgs<E>&, hipStream_t);       \
  template hipError_t launch_deep_quotient<E>(unsigned, const uint32_t*, const uint32_t*, const uint32_t*, uint32_t*,   \
                                              const DeepArgs<E>&, hipStream_t);

}  // namespace ntt
