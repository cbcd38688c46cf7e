// Binomial-extension arithmetic over the one-word engines' fields (host + device): an element of
// F_p[X]/(X^D - W), D = 2 or 4 (D = 1: the base field), is D adjacent base-field coefficients
// a_0 + a_1 X + .. + a_{D-1} X^(D-1).  The ring arithmetic is all there is: nothing here needs X^D - W to
// be irreducible.  Built on field31.hpp (f31x) and field64.hpp (gl64x) alone.
//
// The product, with X^D = W:
//   c_k = sum_{i <= k} a_i b_{k-i} + W sum_{i > k} a_i b_{k+D-i}
//       = sum_{i <= k} a_i b_{k-i} +   sum_{i > k} a_i (W b)_{k+D-i},
// so the factor W is paid once per coefficient of ONE operand (D - 1 products by the constant W: b_0 never
// meets it) instead of once per high partial product, and an operand that is a constant (FRI's fold
// challenge) brings (W b)_j precomputed: then no product by W runs at all.  D^2 base-field products and
// D (D - 1) additions per extension product, D products per product by a base-field scalar.
//
// Bounds.  f31x: every value between two operations is canonical (in [0, p)), as field31.hpp keeps them at
// p > 2^30, so each partial product is reduced before it is accumulated:
//   mulc(x, w, ws)   any 32-bit x, w < p: the result is canonical (field31.hpp shoup_lazy + canon2);
//   mulv(x, y)       x, y < p, so x y < p^2 < 2^32 p: the result x y 2^-32 mod p is canonical;
//   add(acc, t)      acc, t < p: acc + t < 2p < 2^32, canonical after canon2.
// An accumulator is therefore below p after each of its D - 1 additions, and every output is canonical.
// No sum of unreduced products is ever formed (two of them may already reach 4p > 2^32).
// gl64x: gl64::mul and gl64::add take and return canonical 64-bit values; the same statement holds.
//
// Forms of the operands (f31x):
//   mul_pre   a: any form; b and wb = W b given as Shoup pairs (w, ws): c = a b exactly, in a's form
//             (a = v R in Montgomery form gives (v b) R);
//   mul       both variable: Montgomery, c = a b 2^-32 coefficient-wise (b = v R gives a v: the form of
//             the NTT_PLAN_MONTGOMERY_IO data and of the element-format tables); W as a Shoup pair;
//   scale     by a constant base-field scalar (Shoup pair): c = a s;
//   scalev    by a variable one: c = a s 2^-32.
// gl64x has one form: plain canonical values (R = 1).
#pragma once
#include "field31.hpp"
#include "field64.hpp"

namespace ntt {

namespace f31x {

// c = a b for constant b: b[j] = (b_j, floor(b_j 2^32 / p)), wb[j] the same for W b_j (wb[0] is not read)
template <int D>
NTT_F31_HD void mul_pre(uint32_t (&c)[D], const uint32_t (&a)[D], const uint32_t (&b)[D], const uint32_t (&bs)[D],
                        const uint32_t (&wb)[D], const uint32_t (&wbs)[D], uint32_t p) {
  uint32_t r[D];
#pragma unroll
  for (int k = 0; k < D; ++k) {
    uint32_t acc = f31::mulc(a[0], b[k], bs[k], p);
#pragma unroll
    for (int i = 1; i < D; ++i) {
      const uint32_t t = i <= k ? f31::mulc(a[i], b[k - i], bs[k - i], p) : f31::mulc(a[i], wb[k + D - i], wbs[k + D - i], p);
      acc = f31::add(acc, t, p);
    }
    r[k] = acc;
  }
#pragma unroll
  for (int k = 0; k < D; ++k) c[k] = r[k];
}

// c = a b 2^-32 (Montgomery product, coefficient-wise factor 2^-32); W = (w, ws) a Shoup pair
template <int D>
NTT_F31_HD void mul(uint32_t (&c)[D], const uint32_t (&a)[D], const uint32_t (&b)[D], uint32_t w, uint32_t ws,
                    uint32_t p, uint32_t pinv) {
  uint32_t wb[D], r[D];
  wb[0] = 0;
#pragma unroll
  for (int j = 1; j < D; ++j) wb[j] = f31::mulc(b[j], w, ws, p);
#pragma unroll
  for (int k = 0; k < D; ++k) {
    uint32_t acc = f31::mulv(a[0], b[k], p, pinv);
#pragma unroll
    for (int i = 1; i < D; ++i) acc = f31::add(acc, f31::mulv(a[i], i <= k ? b[k - i] : wb[k + D - i], p, pinv), p);
    r[k] = acc;
  }
#pragma unroll
  for (int k = 0; k < D; ++k) c[k] = r[k];
}

// c = a s, s = (s, ss) a constant base-field scalar
template <int D>
NTT_F31_HD void scale(uint32_t (&c)[D], const uint32_t (&a)[D], uint32_t s, uint32_t ss, uint32_t p) {
#pragma unroll
  for (int k = 0; k < D; ++k) c[k] = f31::mulc(a[k], s, ss, p);
}
// c = a s 2^-32, s < p variable
template <int D>
NTT_F31_HD void scalev(uint32_t (&c)[D], const uint32_t (&a)[D], uint32_t s, uint32_t p, uint32_t pinv) {
#pragma unroll
  for (int k = 0; k < D; ++k) c[k] = f31::mulv(a[k], s, p, pinv);
}

template <int D>
NTT_F31_HD void add(uint32_t (&c)[D], const uint32_t (&a)[D], const uint32_t (&b)[D], uint32_t p) {
#pragma unroll
  for (int k = 0; k < D; ++k) c[k] = f31::add(a[k], b[k], p);
}
template <int D>
NTT_F31_HD void sub(uint32_t (&c)[D], const uint32_t (&a)[D], const uint32_t (&b)[D], uint32_t p) {
#pragma unroll
  for (int k = 0; k < D; ++k) c[k] = f31::sub(a[k], b[k], p);
}

}  // namespace f31x

namespace gl64x {

// c = a b with wb[j] = W b_j given (wb[0] is not read)
template <int D>
NTT_F64_HD void mul_pre(uint64_t (&c)[D], const uint64_t (&a)[D], const uint64_t (&b)[D], const uint64_t (&wb)[D]) {
  uint64_t r[D];
#pragma unroll
  for (int k = 0; k < D; ++k) {
    uint64_t acc = gl64::mul(a[0], b[k]);
#pragma unroll
    for (int i = 1; i < D; ++i) acc = gl64::add(acc, gl64::mul(a[i], i <= k ? b[k - i] : wb[k + D - i]));
    r[k] = acc;
  }
#pragma unroll
  for (int k = 0; k < D; ++k) c[k] = r[k];
}

template <int D>
NTT_F64_HD void mul(uint64_t (&c)[D], const uint64_t (&a)[D], const uint64_t (&b)[D], uint64_t w) {
  uint64_t wb[D];
  wb[0] = 0;
#pragma unroll
  for (int j = 1; j < D; ++j) wb[j] = gl64::mul(b[j], w);
  mul_pre<D>(c, a, b, wb);
}

template <int D>
NTT_F64_HD void scale(uint64_t (&c)[D], const uint64_t (&a)[D], uint64_t s) {
#pragma unroll
  for (int k = 0; k < D; ++k) c[k] = gl64::mul(a[k], s);
}
template <int D>
NTT_F64_HD void add(uint64_t (&c)[D], const uint64_t (&a)[D], const uint64_t (&b)[D]) {
#pragma unroll
  for (int k = 0; k < D; ++k) c[k] = gl64::add(a[k], b[k]);
}
template <int D>
NTT_F64_HD void sub(uint64_t (&c)[D], const uint64_t (&a)[D], const uint64_t (&b)[D]) {
#pragma unroll
  for (int k = 0; k < D; ++k) c[k] = gl64::sub(a[k], b[k]);
}

}  // namespace gl64x
}  // namespace ntt
