// The Poseidon2 permutation over the one-word engines' fields (host + device), written once over both
// arithmetics through fieldext.hpp's xf interface: width T = 16 on the 4-byte fields (Eng31), T = 8 on
// Goldilocks (Eng64G); the rate and the digest are D = T / 2 elements.  The kernels (ntt_hash_impl.hpp), the
// plan's host side (plan_hash.hpp) and the stand-alone check (tests/c/poseidon2_check.cpp) run this text.
//
// The permutation:  M_E;  rounds_f / 2 external rounds;  rounds_p internal rounds;  rounds_f / 2 external rounds.
//   external round r   s_i += ext_rc[r][i];  s_i = s_i^a;  s = M_E s
//   internal round r   s_0 += int_rc[r];  s_0 = s_0^a;  sigma = sum_i s_i;  s_i = int_diag[i] s_i + sigma
//   M_E                M4 = [[2,3,1,1],[1,2,3,1],[1,1,2,3],[3,1,1,2]] on each group of four adjacent elements,
//                      then to every element the sum of the elements at its position mod 4 over all groups:
//                      circ(2 M4, M4, .., M4)
// The parameters (a in {3, 5, 7}, the round counts, the constants) are the caller's: no constant is built in.
//
// Forms.  The state is in the field's WORKING FORM (xf: v 2^32 mod p on the 4-byte fields, the value on
// Goldilocks), so a product of two state elements is the plain Montgomery product.  The round constants are
// in the working form; the diagonal is a table of Shoup pairs on the 4-byte fields (d_i, floor(d_i 2^32 / p):
// mulc of a working-form value by the canonical d_i stays in the working form at 4 + 2 operations instead of
// 6 + 2) and of plain values on Goldilocks.  load_form / store_form move a datum between the plan's I/O form
// and the working form: one product by R^2 and one by 1 on canonical 4-byte plans, nothing on
// NTT_PLAN_MONTGOMERY_IO plans and on Goldilocks.
//
// Bounds.  Every value between two operations is canonical (field31.hpp and field64.hpp keep them so at
// p > 2^30 and p > 2^63): each addition and each product reduces, no unreduced sum is formed.
//
// The constant table (one array of V, at most Layout<T>::MAX_ELEMS): ext_rc [rounds_f][T], int_rc [rounds_p],
// diag [T], and on the 4-byte fields the diag's Shoup companions [T].  In a kernel the table's address and every
// index are wave-uniform, so the constants arrive through scalar loads.
#pragma once
#include "fieldext.hpp"

#if defined(__HIPCC__) || defined(__HIP__)
#define NTT_P2_HD __host__ __device__ __forceinline__
#define NTT_P2_HDS static __host__ __device__ __forceinline__
#else
#define NTT_P2_HD static inline
#define NTT_P2_HDS static inline
#endif

namespace ntt {
namespace p2 {

// the field's constants: xf's, the I/O form, and on the 4-byte fields R^2 for load_form
struct P31 : xf::K31 {
  uint32_t r2;    // 2^64 mod p
  uint32_t mont;  // the data are in Montgomery form already (NTT_PLAN_MONTGOMERY_IO)
};
struct P64 : xf::K64 {};

NTT_P2_HD uint32_t load_form(uint32_t x, const P31& k) { return k.mont ? x : f31::mulv(x, k.r2, k.p, k.pinv); }
NTT_P2_HD uint64_t load_form(uint64_t x, const P64&) { return x; }
NTT_P2_HD uint32_t store_form(uint32_t s, const P31& k) { return k.mont ? s : f31::mulv(s, 1u, k.p, k.pinv); }
NTT_P2_HD uint64_t store_form(uint64_t s, const P64&) { return s; }

template <int T>
struct Layout {
  static constexpr unsigned MAX_F = 16, MAX_P = 64;
  static constexpr unsigned MAX_ELEMS = MAX_F * T + MAX_P + 2 * T;
  NTT_P2_HDS unsigned internal(unsigned rounds_f) { return rounds_f * T; }
  NTT_P2_HDS unsigned diag(unsigned rounds_f, unsigned rounds_p) { return rounds_f * T + rounds_p; }
  NTT_P2_HDS unsigned elems(unsigned rounds_f, unsigned rounds_p) { return rounds_f * T + rounds_p + 2 * T; }
};

// s d_i for the diagonal table dg (T entries, then their Shoup companions on the 4-byte fields)
template <int T>
NTT_P2_HD uint32_t diag_mul(uint32_t s, const uint32_t* __restrict__ dg, int i, const P31& k) {
  return f31::mulc(s, dg[i], dg[T + i], k.p);
}
template <int T>
NTT_P2_HD uint64_t diag_mul(uint64_t s, const uint64_t* __restrict__ dg, int i, const P64&) {
  return gl64::mul(s, dg[i]);
}

// x^A, A in {3, 5, 7}: 2, 3 and 4 products
template <int A, class V, class K>
NTT_P2_HD V sbox(V x, const K& k) {
  static_assert(A == 3 || A == 5 || A == 7, "S-box degree");
  const V x2 = xf::mul(x, x, k);
  if constexpr (A == 3) {
    return xf::mul(x2, x, k);
  } else if constexpr (A == 5) {
    return xf::mul(xf::mul(x2, x2, k), x, k);
  } else {
    const V x3 = xf::mul(x2, x, k), x4 = xf::mul(x2, x2, k);
    return xf::mul(x3, x4, k);
  }
}

// x = M4 x: seven additions and two doublings
template <class V, class K>
NTT_P2_HD void mat4(V& x0, V& x1, V& x2, V& x3, const K& k) {
  const V t01 = xf::add(x0, x1, k), t23 = xf::add(x2, x3, k);
  const V t = xf::add(t01, t23, k);
  const V ta = xf::add(t, x1, k), tb = xf::add(t, x3, k);  // x0 + 2 x1 + x2 + x3, x0 + x1 + x2 + 2 x3
  const V y3 = xf::add(tb, xf::add(x0, x0, k), k);         // 3 x0 + x1 + x2 + 2 x3
  const V y1 = xf::add(ta, xf::add(x2, x2, k), k);         // x0 + 2 x1 + 3 x2 + x3
  x0 = xf::add(ta, t01, k);                                // 2 x0 + 3 x1 + x2 + x3
  x2 = xf::add(tb, t23, k);                                // x0 + x1 + 2 x2 + 3 x3
  x1 = y1;
  x3 = y3;
}

// s = M_E s
template <int T, class V, class K>
NTT_P2_HD void m_ext(V (&s)[T], const K& k) {
  static_assert(T % 4 == 0 && T >= 8, "width");
#pragma unroll
  for (int g = 0; g < T; g += 4) mat4(s[g], s[g + 1], s[g + 2], s[g + 3], k);
  V sum[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    sum[j] = s[j];
#pragma unroll
    for (int g = 4; g < T; g += 4) sum[j] = xf::add(sum[j], s[g + j], k);
  }
#pragma unroll
  for (int i = 0; i < T; ++i) s[i] = xf::add(s[i], sum[i & 3], k);
}

template <int T, int A, class V, class K>
NTT_P2_HD void ext_round(V (&s)[T], const V* __restrict__ rc, const K& k) {
#pragma unroll
  for (int i = 0; i < T; ++i) s[i] = sbox<A>(xf::add(s[i], rc[i], k), k);
  m_ext<T>(s, k);
}

template <int T, int A, class V, class K>
NTT_P2_HD void int_round(V (&s)[T], V rc, const V* __restrict__ dg, const K& k) {
  s[0] = sbox<A>(xf::add(s[0], rc, k), k);
  V sigma = s[0];
#pragma unroll
  for (int i = 1; i < T; ++i) sigma = xf::add(sigma, s[i], k);
#pragma unroll
  for (int i = 0; i < T; ++i) s[i] = xf::add(diag_mul<T>(s[i], dg, i, k), sigma, k);
}

// the permutation of a working-form state; tab: the constant table of (rounds_f, rounds_p)
template <int T, int A, class V, class K>
NTT_P2_HD void permute(V (&s)[T], const V* __restrict__ tab, unsigned rounds_f, unsigned rounds_p, const K& k) {
  const V* __restrict__ irc = tab + Layout<T>::internal(rounds_f);
  const V* __restrict__ dg = tab + Layout<T>::diag(rounds_f, rounds_p);
  const unsigned half = rounds_f / 2;
  m_ext<T>(s, k);
#pragma unroll 1
  for (unsigned r = 0; r < half; ++r) ext_round<T, A>(s, tab + r * T, k);
#pragma unroll 1
  for (unsigned r = 0; r < rounds_p; ++r) int_round<T, A>(s, irc[r], dg, k);
#pragma unroll 1
  for (unsigned r = half; r < rounds_f; ++r) ext_round<T, A>(s, tab + r * T, k);
}

// ---- the host's side of the table and the sponge (the plan and the stand-alone check)

// a supported parameter set for a field of modulus p: degree 3, 5 or 7 coprime to p - 1, rounds_f even in
// [2, 16], rounds_p in [0, 64]
static inline bool shape_ok(uint64_t p, unsigned alpha, unsigned rounds_f, unsigned rounds_p) {
  if (alpha != 3 && alpha != 5 && alpha != 7) return false;
  if ((p - 1) % alpha == 0) return false;  // alpha is prime: gcd(alpha, p - 1) = 1 iff it does not divide
  if (rounds_f < 2 || rounds_f > 16 || (rounds_f & 1)) return false;
  return rounds_p <= 64;
}

static inline void pack_diag(uint32_t* dg, const uint64_t* d, int t, const P31& k) {
  for (int i = 0; i < t; ++i) {
    dg[i] = (uint32_t)d[i];
    dg[t + i] = f31::shoup_companion((uint32_t)d[i], k.p);
  }
}
static inline void pack_diag(uint64_t* dg, const uint64_t* d, int t, const P64&) {
  for (int i = 0; i < t; ++i) dg[i] = d[i], dg[t + i] = 0;
}
// canonical words -> the table (Layout<T>::elems(rounds_f, rounds_p) entries); false: a word is not canonical
template <int T, class V, class K>
static inline bool pack(V* tab, uint64_t p, unsigned rounds_f, unsigned rounds_p, const uint64_t* ext_rc,
                        const uint64_t* int_rc, const uint64_t* int_diag, const K& k) {
  for (unsigned i = 0; i < rounds_f * T; ++i) {
    if (ext_rc[i] >= p) return false;
    tab[i] = xf::to_work(ext_rc[i], k);
  }
  for (unsigned i = 0; i < rounds_p; ++i) {
    if (int_rc[i] >= p) return false;
    tab[Layout<T>::internal(rounds_f) + i] = xf::to_work(int_rc[i], k);
  }
  for (int i = 0; i < T; ++i)
    if (int_diag[i] >= p) return false;
  pack_diag(tab + Layout<T>::diag(rounds_f, rounds_p), int_diag, T, k);
  return true;
}

// the padding-free sponge over a row of w elements in the I/O form: the digest, T / 2 elements in that form
template <int T, int A, class V, class K>
static inline void hash_row(V* digest, const V* row, size_t w, const V* tab, unsigned rounds_f, unsigned rounds_p,
                            const K& k) {
  constexpr int D = T / 2;
  V s[T];
  for (int i = 0; i < T; ++i) s[i] = 0;
  for (size_t c = 0; c < w; c += D) {
    for (int j = 0; j < D && c + j < w; ++j) s[j] = load_form(row[c + j], k);
    permute<T, A>(s, tab, rounds_f, rounds_p, k);
  }
  for (int j = 0; j < D; ++j) digest[j] = store_form(s[j], k);
}
// the 2-to-1 compression of two digests in the I/O form
template <int T, int A, class V, class K>
static inline void compress(V* digest, const V* left, const V* right, const V* tab, unsigned rounds_f,
                            unsigned rounds_p, const K& k) {
  constexpr int D = T / 2;
  V s[T];
  for (int j = 0; j < D; ++j) s[j] = load_form(left[j], k), s[D + j] = load_form(right[j], k);
  permute<T, A>(s, tab, rounds_f, rounds_p, k);
  for (int j = 0; j < D; ++j) digest[j] = store_form(s[j], k);
}

}  // namespace p2
}  // namespace ntt
