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
//
// The inverse (inv): D = 2 by the conjugate over the norm, 1 / (a0 + a1 X) = (a0 - a1 X) / (a0^2 - W a1^2);
// D = 4 as the quadratic tower over Y = X^2, a = A0 + X A1 with A0 = a0 + a2 Y, A1 = a1 + a3 Y in
// F_p[Y]/(Y^2 - W): 1 / a = (A0 - X A1) / (A0^2 - Y A1^2), the denominator inverted at D = 2; the base inverse
// is x^(p-2).  f31x::inv works on Montgomery-form coefficients.  xf (at the end) is one interface over both
// fields for code that serves both engines.
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

// a^-1 in the ring; 0 (and, where X^D - W is reducible, every other non-invertible element) gives some
// value and never a fault: the base inverse is x^(p-2), which is 0 at 0
NTT_F64_HD uint64_t inv_base(uint64_t x) {
  uint64_t acc = 1, b = x;
  for (uint64_t e = gl64::kP - 2; e; e >>= 1) {
    if (e & 1) acc = gl64::mul(acc, b);
    b = gl64::mul(b, b);
  }
  return acc;
}
template <int D>
NTT_F64_HD void inv(uint64_t (&c)[D], const uint64_t (&a)[D], uint64_t w) {
  static_assert(D == 1 || D == 2 || D == 4, "extension degree");
  if constexpr (D == 1) {
    c[0] = inv_base(a[0]);
  } else if constexpr (D == 2) {  // (a0 - a1 X) / (a0^2 - W a1^2)
    const uint64_t n = gl64::sub(gl64::mul(a[0], a[0]), gl64::mul(gl64::mul(a[1], a[1]), w));
    const uint64_t ni = inv_base(n);
    const uint64_t c0 = gl64::mul(a[0], ni), c1 = gl64::mul(gl64::sub(0, a[1]), ni);
    c[0] = c0;
    c[1] = c1;
  } else {  // a = A0 + X A1 over F_p[Y]/(Y^2 - W), Y = X^2: (A0 - X A1) / (A0^2 - Y A1^2)
    const uint64_t A0[2] = {a[0], a[2]}, A1[2] = {a[1], a[3]};
    uint64_t s0[2], s1[2], n[2], ni[2], b0[2], b1[2];
    mul<2>(s0, A0, A0, w);
    mul<2>(s1, A1, A1, w);
    n[0] = gl64::sub(s0[0], gl64::mul(s1[1], w));
    n[1] = gl64::sub(s0[1], s1[0]);
    inv<2>(ni, n, w);
    mul<2>(b0, A0, ni, w);
    mul<2>(b1, A1, ni, w);
    c[0] = b0[0];
    c[1] = gl64::sub(0, b1[0]);
    c[2] = b0[1];
    c[3] = gl64::sub(0, b1[1]);
  }
}

}  // namespace gl64x

// ---- f31x inverse (after gl64x only for the file's order: nothing of gl64x is used)
namespace f31x {

// Montgomery form in and out: x = v 2^32 gives v^-1 2^32; one = 2^32 mod p.  x^(p-2): 0 at 0.
NTT_F31_HD uint32_t inv_base(uint32_t x, uint32_t one, uint32_t p, uint32_t pinv) {
  uint32_t acc = one, b = x;
  for (uint32_t e = p - 2; e; e >>= 1) {
    if (e & 1) acc = f31::mulv(acc, b, p, pinv);
    b = f31::mulv(b, b, p, pinv);
  }
  return acc;
}
// a^-1 for a in Montgomery form (coefficient-wise v 2^32), the result in the same form; W = (w, ws) a
// Shoup pair.  Non-invertible elements (0 among them) give some value and never a fault.
template <int D>
NTT_F31_HD void inv(uint32_t (&c)[D], const uint32_t (&a)[D], uint32_t w, uint32_t ws, uint32_t one, uint32_t p,
                    uint32_t pinv) {
  static_assert(D == 1 || D == 2 || D == 4, "extension degree");
  if constexpr (D == 1) {
    c[0] = inv_base(a[0], one, p, pinv);
  } else if constexpr (D == 2) {  // (a0 - a1 X) / (a0^2 - W a1^2)
    const uint32_t n = f31::sub(f31::mulv(a[0], a[0], p, pinv), f31::mulc(f31::mulv(a[1], a[1], p, pinv), w, ws, p), p);
    const uint32_t ni = inv_base(n, one, p, pinv);
    const uint32_t c0 = f31::mulv(a[0], ni, p, pinv), c1 = f31::mulv(f31::sub(0, a[1], p), ni, p, pinv);
    c[0] = c0;
    c[1] = c1;
  } else {  // a = A0 + X A1 over F_p[Y]/(Y^2 - W), Y = X^2: (A0 - X A1) / (A0^2 - Y A1^2)
    const uint32_t A0[2] = {a[0], a[2]}, A1[2] = {a[1], a[3]};
    uint32_t s0[2], s1[2], n[2], ni[2], b0[2], b1[2];
    mul<2>(s0, A0, A0, w, ws, p, pinv);
    mul<2>(s1, A1, A1, w, ws, p, pinv);
    n[0] = f31::sub(s0[0], f31::mulc(s1[1], w, ws, p), p);
    n[1] = f31::sub(s0[1], s1[0], p);
    inv<2>(ni, n, w, ws, one, p, pinv);
    mul<2>(b0, A0, ni, w, ws, p, pinv);
    mul<2>(b1, A1, ni, w, ws, p, pinv);
    c[0] = b0[0];
    c[1] = f31::sub(0, b1[0], p);
    c[2] = b0[1];
    c[3] = f31::sub(0, b1[1], p);
  }
}

}  // namespace f31x

// ---- one interface over both fields (the DEEP calls: ntt_deep_impl.hpp on the device, plan_deep.hpp on the
// host).  A value is in its field's WORKING FORM: v 2^32 mod p on the 4-byte field (so that the Montgomery
// products below are plain products, and a product with data in either I/O form leaves the data's form),
// the plain value on Goldilocks.  K holds the field's constants; the functions are overloaded on the value type.
namespace xf {

struct K31 {
  uint32_t p, pinv;
  uint32_t one;    // 2^32 mod p: 1 in the working form
  uint32_t w, ws;  // W, a Shoup pair
};
struct K64 {
  uint64_t one;  // 1
  uint64_t w;    // W
};
NTT_F31_HD bool canonical(uint32_t x, const K31& k) { return x < k.p; }
NTT_F64_HD bool canonical(uint64_t x, const K64&) { return gl64::is_canonical(x); }
// canonical host word -> working form
NTT_F31_HD uint32_t to_work(uint64_t v, const K31& k) { return (uint32_t)((v << 32) % k.p); }
NTT_F64_HD uint64_t to_work(uint64_t v, const K64&) { return v; }
NTT_F31_HD uint32_t add(uint32_t a, uint32_t b, const K31& k) { return f31::add(a, b, k.p); }
NTT_F64_HD uint64_t add(uint64_t a, uint64_t b, const K64&) { return gl64::add(a, b); }
NTT_F31_HD uint32_t sub(uint32_t a, uint32_t b, const K31& k) { return f31::sub(a, b, k.p); }
NTT_F64_HD uint64_t sub(uint64_t a, uint64_t b, const K64&) { return gl64::sub(a, b); }
// a b with one operand in the working form: the other operand's form is the result's
NTT_F31_HD uint32_t mul(uint32_t a, uint32_t b, const K31& k) { return f31::mulv(a, b, k.p, k.pinv); }
NTT_F64_HD uint64_t mul(uint64_t a, uint64_t b, const K64&) { return gl64::mul(a, b); }
template <int D>
NTT_F31_HD void mul(uint32_t (&c)[D], const uint32_t (&a)[D], const uint32_t (&b)[D], const K31& k) {
  if constexpr (D == 1)
    c[0] = f31::mulv(a[0], b[0], k.p, k.pinv);
  else
    f31x::mul<D>(c, a, b, k.w, k.ws, k.p, k.pinv);
}
template <int D>
NTT_F64_HD void mul(uint64_t (&c)[D], const uint64_t (&a)[D], const uint64_t (&b)[D], const K64& k) {
  if constexpr (D == 1)
    c[0] = gl64::mul(a[0], b[0]);
  else
    gl64x::mul<D>(c, a, b, k.w);
}
// the extension element a times the base-field scalar s
template <int D>
NTT_F31_HD void scale(uint32_t (&c)[D], const uint32_t (&a)[D], uint32_t s, const K31& k) {
  f31x::scalev<D>(c, a, s, k.p, k.pinv);
}
template <int D>
NTT_F64_HD void scale(uint64_t (&c)[D], const uint64_t (&a)[D], uint64_t s, const K64&) {
  gl64x::scale<D>(c, a, s);
}
template <int D>
NTT_F31_HD void add(uint32_t (&c)[D], const uint32_t (&a)[D], const uint32_t (&b)[D], const K31& k) {
  f31x::add<D>(c, a, b, k.p);
}
template <int D>
NTT_F64_HD void add(uint64_t (&c)[D], const uint64_t (&a)[D], const uint64_t (&b)[D], const K64&) {
  gl64x::add<D>(c, a, b);
}
template <int D>
NTT_F31_HD void sub(uint32_t (&c)[D], const uint32_t (&a)[D], const uint32_t (&b)[D], const K31& k) {
  f31x::sub<D>(c, a, b, k.p);
}
template <int D>
NTT_F64_HD void sub(uint64_t (&c)[D], const uint64_t (&a)[D], const uint64_t (&b)[D], const K64&) {
  gl64x::sub<D>(c, a, b);
}
// working form in and out
template <int D>
NTT_F31_HD void inv(uint32_t (&c)[D], const uint32_t (&a)[D], const K31& k) {
  f31x::inv<D>(c, a, k.w, k.ws, k.one, k.p, k.pinv);
}
template <int D>
NTT_F64_HD void inv(uint64_t (&c)[D], const uint64_t (&a)[D], const K64& k) {
  gl64x::inv<D>(c, a, k.w);
}
// a^e by square and multiply, working form in and out (a^0 = 1)
template <int D, class V, class K>
#if defined(__HIPCC__) || defined(__HIP__)
__host__ __device__ __forceinline__
#else
static inline
#endif
void pow(V (&c)[D], const V (&a)[D], uint64_t e, const K& k) {
  V acc[D], b[D];
#pragma unroll
  for (int j = 0; j < D; ++j) {
    acc[j] = j ? V(0) : k.one;
    b[j] = a[j];
  }
  for (; e; e >>= 1) {
    if (e & 1) mul<D>(acc, acc, b, k);
    if (e > 1) mul<D>(b, b, b, k);
  }
#pragma unroll
  for (int j = 0; j < D; ++j) c[j] = acc[j];
}

}  // namespace xf
}  // namespace ntt
