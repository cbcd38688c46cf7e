// Table builders: the per-pass outer-twiddle table (k_build_tw; as Shoup pairs k_build_tw_sh), the
// power table of the radix-2 rivals (k_build_pow) and the four-step twiddle table of one rank
// (k_build_fs_tw), each built on the device from the plan's two-level tables.  Instantiated by the
// ntt_*_misc.hip units.
#pragma once
#include "ntt_elementwise_impl.hpp"

namespace ntt {

// Per-pass outer-twiddle table of a column pass with radix 2^log_r and T = 2^log_t columns per
// workgroup: entry (c, k) = w_n^((c*k) << log_m) R_e mod p (R_e the engine's Montgomery radix) at
// [c >> log_t][k][c mod T], canonical in the HBM element format, built on the device from the
// two-level tables (lo_s = lo R_e, so lo_s * hi = w R_e).  With clo/chi (two-level tables of a coset
// shift c in the same format) the entry is also multiplied by c^col.
template <class E>
__global__ void k_build_tw(uint32_t* __restrict__ out, size_t count, uint32_t log_r, uint32_t log_t, uint32_t log_m,
                           const uint32_t* __restrict__ lo, const uint32_t* __restrict__ hi, uint32_t lo_bits,
                           const typename E::Args F, const uint32_t* __restrict__ clo,
                           const uint32_t* __restrict__ chi) {
  NTT_GRID_STRIDE(idx, count) {
    const size_t k = (idx >> log_t) & ((1ull << log_r) - 1);
    const size_t c = ((idx >> (log_t + log_r)) << log_t) + (idx & ((1ull << log_t) - 1));
    const size_t e = (c * k) << log_m;
    typename E::Tw a, b;
    E::tload(a, lo, (uint32_t)(e & ((1ull << lo_bits) - 1)));
    E::tload(b, hi, (uint32_t)(e >> lo_bits));
    E::mul(a.w, b, F);
    if (clo) {  // c^col R_e = clo[col & mask] * chi[col >> lo_bits]; mulv removes one R_e
      typename E::Tw u, v;
      E::tload(u, clo, (uint32_t)(c & ((1ull << lo_bits) - 1)));
      E::tload(v, chi, (uint32_t)(c >> lo_bits));
      E::mul(u.w, v, F);
      E::mulv(a.w, u.w, F);
    }
    E::template store<E::MUL_OUT, false, E::TABW>(out, idx, a.w, F);  // outer-twiddle tables: E::TABW words
  }
}

template <class E>
hipError_t launch_build_tw(uint32_t* out, size_t count, uint32_t log_r, uint32_t log_t, uint32_t log_m,
                           const uint32_t* lo, const uint32_t* hi, uint32_t lo_bits, const typename E::Args& F,
                           hipStream_t st, const uint32_t* clo, const uint32_t* chi) {
  hipLaunchKernelGGL((k_build_tw<E>), dim3(grid_1d(count)), dim3(256), 0, st, out, count, log_r,
                     log_t, log_m, lo, hi, lo_bits, F, clo, chi);
  return hipGetLastError();
}

// NTT_PLAN_NAIVE (the reference's `naive` rival, GZKP-NTT.cu:59-71 / big-num.cu:67-104): the power
// table entry i = w_n^i R_e mod p, i < count, canonical in the element format (E::TABW words) -- the
// reference's `roots` table (GZKP-NTT.cu:81-83), built on the device from the two-level tables.
template <class E>
__global__ void k_build_pow(uint32_t* __restrict__ out, size_t count, const uint32_t* __restrict__ lo,
                            const uint32_t* __restrict__ hi, uint32_t lo_bits, const typename E::Args F) {
  NTT_GRID_STRIDE(i, count) {
    typename E::Tw a, b;
    E::tload(a, lo, i & ((size_t(1) << lo_bits) - 1));
    E::tload(b, hi, i >> lo_bits);
    E::mul(a.w, b, F);
    E::template store<E::MUL_OUT, false, E::TABW>(out, i, a.w, F);
  }
}

template <class E>
hipError_t launch_build_pow(uint32_t* out, size_t count, const uint32_t* lo, const uint32_t* hi, uint32_t lo_bits,
                            const typename E::Args& F, hipStream_t st) {
  hipLaunchKernelGGL((k_build_pow<E>), dim3(grid_1d(count)), dim3(256), 0, st, out, count, lo, hi, lo_bits, F);
  return hipGetLastError();
}

// k_build_tw's table as Shoup pairs: entry (c, k) = (w, floor(w B / p)) with w = w_n^((c*k) << log_m)
// canonical, in the engine's twiddle format (E::TW words).  t = lo_s * hi = w B mod p; w = t / B
// (Montgomery product by 1); floor(w B / p) = (-(w B mod p)) p^-1 mod B (shoup_ws29).
template <class E>
__global__ void k_build_tw_sh(uint32_t* __restrict__ out, size_t count, uint32_t log_r, uint32_t log_t,
                              uint32_t log_m, const uint32_t* __restrict__ lo, const uint32_t* __restrict__ hi,
                              uint32_t lo_bits, const typename E::Args F, const uint32_t* __restrict__ pinvB) {
  constexpr int L = E::W;
  NTT_GRID_STRIDE(idx, count) {
    const size_t k = (idx >> log_t) & ((1ull << log_r) - 1);
    const size_t c = ((idx >> (log_t + log_r)) << log_t) + (idx & ((1ull << log_t) - 1));
    const size_t e = (c * k) << log_m;
    typename E::Tw a, b;
    E::tload(a, lo, (uint32_t)(e & ((1ull << lo_bits) - 1)));
    E::tload(b, hi, (uint32_t)(e >> lo_bits));
    E::mul(a.w, b, F);  // w B mod p, < 3p
    uint32_t wr[L], w[L], one[L], t[L], ws[L], pib[L];
#pragma unroll
    for (int i = 0; i < L; ++i) {
      wr[i] = a.w[i];
      one[i] = i == 0 ? 1u : 0u;
      pib[i] = pinvB[i];
    }
    E::template reduce<4, 1, false>(wr, F);  // canonical w B mod p
#pragma unroll
    for (int i = 0; i < L; ++i) w[i] = wr[i];
    E::mulv(w, one, F);  // w, < 3p
    E::template reduce<4, 1, false>(w, F);
    neg29<L>(t, wr);
    mullo29<L>(ws, t, pib);
    uint32_t o[E::TW];
#pragma unroll
    for (int i = 0; i < E::TW; ++i) o[i] = i < L ? w[i] : (i < 2 * L ? ws[i - L] : 0u);
    uint4* p = reinterpret_cast<uint4*>(out + idx * E::TW);
#pragma unroll
    for (int q = 0; q < E::TW / 4; ++q) p[q] = make_uint4(o[4 * q], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3]);
  }
}

template <class E>
hipError_t launch_build_tw_sh(uint32_t* out, size_t count, uint32_t log_r, uint32_t log_t, uint32_t log_m,
                              const uint32_t* lo, const uint32_t* hi, uint32_t lo_bits, const typename E::Args& F,
                              const uint32_t* pinvB, hipStream_t st) {
  if constexpr (!E::SHOUP_OUTER) {
    return hipErrorInvalidValue;
  } else {
    hipLaunchKernelGGL((k_build_tw_sh<E>), dim3(grid_1d(count)), dim3(256), 0, st, out, count,
                       log_r, log_t, log_m, lo, hi, lo_bits, F, pinvB);
    return hipGetLastError();
  }
}

// Four-step twiddle table of one rank (ntt_rplan): entry (a, b) at a 2^log_cols + b holds
// w_n^((row0 + a)(col0 + b) mod n) R_e (the epilogue of the final pass multiplies by it with mulv),
// from the two-level tables (lo_s = lo R_e, so lo_s * hi = w R_e).
template <class E>
__global__ void k_build_fs_tw(uint32_t* __restrict__ out, uint32_t log_rows, uint32_t log_cols, uint64_t row0,
                              uint64_t col0, uint32_t log_n, const uint32_t* __restrict__ lo,
                              const uint32_t* __restrict__ hi, uint32_t lo_bits, const typename E::Args F,
                              const uint32_t* __restrict__ scale) {
  NTT_GRID_STRIDE(idx, (size_t(1) << (log_rows + log_cols))) {
    const uint64_t a = idx >> log_cols, b = idx & ((1ull << log_cols) - 1);
    const uint64_t e = ((row0 + a) * (col0 + b)) & ((1ull << log_n) - 1);
    typename E::Tw x, y;
    E::tload(x, lo, (uint32_t)(e & ((1ull << lo_bits) - 1)));
    E::tload(y, hi, (uint32_t)(e >> lo_bits));
    E::mul(x.w, y, F);
    if (scale) {  // a constant folded into every entry (the four-step's row n2^-1); mul takes any x < B
      E::tload(y, scale, 0);
      E::mul(x.w, y, F);
    }
    E::template store<E::MUL_OUT, false, E::TABW>(out, idx, x.w, F);
  }
}

template <class E>
hipError_t launch_build_fs_tw(uint32_t* out, uint32_t log_rows, uint32_t log_cols, uint64_t row0, uint64_t col0,
                              uint32_t log_n, const uint32_t* lo, const uint32_t* hi, uint32_t lo_bits,
                              const typename E::Args& F, hipStream_t st, const uint32_t* scale) {
  const size_t count = 1ull << (log_rows + log_cols);
  hipLaunchKernelGGL((k_build_fs_tw<E>), dim3(grid_1d(count)), dim3(256), 0, st, out, log_rows,
                     log_cols, row0, col0, log_n, lo, hi, lo_bits, F, scale);
  return hipGetLastError();
}

// The table builders of one engine (ntt_*_misc.hip)
#define NTT_INSTANTIATE_TABLES(E)                                                                                  \
  template hipError_t launch_build_tw<E>(uint32_t*, size_t, uint32_t, uint32_t, uint32_t, const uint32_t*,        \
                                         const uint32_t*, uint32_t, const typename E::Args&, hipStream_t,          \
                                         const uint32_t*, const uint32_t*);                                        \
  template hipError_t launch_build_tw_sh<E>(uint32_t*, size_t, uint32_t, uint32_t, uint32_t, const uint32_t*,     \
                                            const uint32_t*, uint32_t, const typename E::Args&, const uint32_t*,  \
                                            hipStream_t);                                                         \
  template hipError_t launch_build_pow<E>(uint32_t*, size_t, const uint32_t*, const uint32_t*, uint32_t,           \
                                          const typename E::Args&, hipStream_t);                                   \
  template hipError_t launch_build_fs_tw<E>(uint32_t*, uint32_t, uint32_t, uint64_t, uint64_t, uint32_t,           \
                                            const uint32_t*, const uint32_t*, uint32_t, const typename E::Args&,    \
                                            hipStream_t, const uint32_t*);

}  // namespace ntt
