// Host check of ntt_amd/csrc/fieldext.hpp (the binomial-extension arithmetic the FRI fold kernel runs): the
// product in F_p[X]/(X^D - W) in its three forms (constant operand with W b precomputed; both operands
// variable, Montgomery on the 31-bit fields; the element-format operand b R), the products by a base-field
// scalar, and add / sub, against schoolbook arithmetic in unsigned __int128, for (BabyBear, 4, 11),
// (BabyBear, 2, 11), (KoalaBear, 4, 3), (Goldilocks, 2, 7) and (1004535809, 2, 3).  Inputs: every pair of
// elements whose coordinates come from {0, 1, 2, p - 2, p - 1} (the full cross product over all 2 D
// positions), then 10^5 seeded random pairs.  The bounds the header documents are asserted beside the
// values: every result coordinate is canonical, and a replay of the accumulation shows each accumulator
// canonical after its addition with the raw sum below 2p <= 2^32, and x y < 2^32 p at every variable product.
// Exit status 0 when everything agrees; the first mismatches are printed otherwise.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "fieldext.hpp"

typedef unsigned __int128 u128;

static int g_bad = 0;
static void fail(const char* what, uint64_t p, int d) {
  if (g_bad++ < 20) fprintf(stderr, "p=%llu D=%d: %s\n", (unsigned long long)p, d, what);
}

static uint64_t powmod(uint64_t b, uint64_t e, uint64_t p) {
  u128 r = 1 % p, x = b % p;
  for (; e; e >>= 1, x = x * x % p)
    if (e & 1) r = r * x % p;
  return (uint64_t)r;
}
static uint64_t splitmix64(uint64_t& s) {
  uint64_t z = (s += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// c = a b in F_p[X]/(X^D - W), schoolbook, every term reduced in 128 bits
template <int D>
static void school(uint64_t (&c)[D], const uint64_t (&a)[D], const uint64_t (&b)[D], uint64_t w, uint64_t p) {
  for (int k = 0; k < D; ++k) {
    u128 lo = 0, hi = 0;
    for (int i = 0; i < D; ++i)
      for (int j = 0; j < D; ++j) {
        const u128 t = (u128)a[i] * b[j] % p;
        if (i + j == k) lo = (lo + t) % p;
        if (i + j == k + D) hi = (hi + t) % p;
      }
    c[k] = (uint64_t)((lo + hi * w % p) % p);
  }
}

template <int D>
struct Pair {
  uint64_t a[D], b[D];
};

// ------------------------------------------------------------------------------ 31-bit fields
template <int D>
static void check31(uint32_t p, uint32_t w, const Pair<D>& in) {
  namespace f = ntt::f31;
  namespace x = ntt::f31x;
  const uint64_t P = p;
  const uint32_t pinv = f::pinv32(p);
  const uint64_t r = (1ull << 32) % P, rinv = powmod(r, P - 2, P);
  uint64_t want[D];
  school<D>(want, in.a, in.b, w, P);
  uint32_t a[D], b[D], bs[D], wb[D], wbs[D], br[D], got[D];
  for (int j = 0; j < D; ++j) {
    a[j] = (uint32_t)in.a[j];
    b[j] = (uint32_t)in.b[j];
    bs[j] = f::shoup_companion(b[j], p);
    wb[j] = (uint32_t)((uint64_t)b[j] * w % P);
    wbs[j] = f::shoup_companion(wb[j], p);
    br[j] = (uint32_t)(in.b[j] * r % P);
  }
  const uint32_t ws = f::shoup_companion(w, p);
  // constant operand
  x::mul_pre<D>(got, a, b, bs, wb, wbs, p);
  for (int k = 0; k < D; ++k) {
    if (got[k] >= p) fail("mul_pre: result not canonical", P, D);
    if (got[k] != want[k]) fail("mul_pre differs from schoolbook", P, D);
  }
  // replay of the accumulation: every term canonical, every raw sum below 2p <= 2^32, every accumulator
  // canonical after its addition
  if (2 * P > (1ull << 32)) fail("2p > 2^32", P, D);
  for (int k = 0; k < D; ++k) {
    uint64_t acc = f::mulc(a[0], b[k], bs[k], p);
    if (acc >= P) fail("mulc term not canonical", P, D);
    for (int i = 1; i < D; ++i) {
      const uint64_t t = i <= k ? f::mulc(a[i], b[k - i], bs[k - i], p) : f::mulc(a[i], wb[k + D - i], wbs[k + D - i], p);
      if (t >= P || acc + t >= 2 * P) fail("raw sum reaches 2p", P, D);
      acc = f::add((uint32_t)acc, (uint32_t)t, p);
      if (acc >= P) fail("accumulator not canonical", P, D);
    }
    if (acc != want[k]) fail("replayed accumulation differs", P, D);
  }
  // both variable: Montgomery; x y < 2^32 p at every product (operands canonical, p < 2^32)
  for (int i = 0; i < D; ++i)
    for (int j = 0; j < D; ++j)
      if ((u128)a[i] * (j ? (uint64_t)wb[j] : (uint64_t)b[j]) >= ((u128)P << 32) || (u128)a[i] * b[j] >= ((u128)P << 32))
        fail("x y >= 2^32 p", P, D);
  x::mul<D>(got, a, b, w, ws, p, pinv);
  for (int k = 0; k < D; ++k) {
    if (got[k] >= p) fail("mul: result not canonical", P, D);
    if (got[k] != (uint64_t)((u128)want[k] * rinv % P)) fail("mul differs from schoolbook 2^-32", P, D);
  }
  // the operand in element format (b R): the plain product
  x::mul<D>(got, a, br, w, ws, p, pinv);
  for (int k = 0; k < D; ++k)
    if (got[k] != want[k]) fail("mul(a, b R) differs from schoolbook", P, D);
  // in place
  for (int k = 0; k < D; ++k) got[k] = a[k];
  x::mul_pre<D>(got, got, b, bs, wb, wbs, p);
  for (int k = 0; k < D; ++k)
    if (got[k] != want[k]) fail("mul_pre in place differs", P, D);
  // scalars: b_0 as the scalar
  x::scale<D>(got, a, b[0], bs[0], p);
  for (int k = 0; k < D; ++k)
    if (got[k] >= p || got[k] != in.a[k] * in.b[0] % P) fail("scale", P, D);
  x::scalev<D>(got, a, b[0], p, pinv);
  for (int k = 0; k < D; ++k)
    if (got[k] >= p || got[k] != (uint64_t)((u128)(in.a[k] * in.b[0] % P) * rinv % P)) fail("scalev", P, D);
  x::scalev<D>(got, a, br[0], p, pinv);
  for (int k = 0; k < D; ++k)
    if (got[k] != in.a[k] * in.b[0] % P) fail("scalev(a, s R)", P, D);
  x::add<D>(got, a, b, p);
  for (int k = 0; k < D; ++k)
    if (got[k] != (in.a[k] + in.b[k]) % P) fail("add", P, D);
  x::sub<D>(got, a, b, p);
  for (int k = 0; k < D; ++k)
    if (got[k] != (in.a[k] + P - in.b[k]) % P) fail("sub", P, D);
}

// ------------------------------------------------------------------------------ Goldilocks
template <int D>
static void check64(uint64_t w, const Pair<D>& in) {
  namespace x = ntt::gl64x;
  const uint64_t P = ntt::gl64::kP;
  uint64_t want[D], got[D], wb[D];
  school<D>(want, in.a, in.b, w, P);
  for (int j = 0; j < D; ++j) wb[j] = (uint64_t)((u128)in.b[j] * w % P);
  x::mul_pre<D>(got, in.a, in.b, wb);
  for (int k = 0; k < D; ++k) {
    if (got[k] >= P) fail("mul_pre: result not canonical", P, D);
    if (got[k] != want[k]) fail("mul_pre differs from schoolbook", P, D);
  }
  for (int k = 0; k < D; ++k) {  // replay: every term and accumulator canonical
    uint64_t acc = ntt::gl64::mul(in.a[0], in.b[k]);
    for (int i = 1; i < D; ++i) {
      const uint64_t t = ntt::gl64::mul(in.a[i], i <= k ? in.b[k - i] : wb[k + D - i]);
      if (t >= P || acc >= P) fail("term or accumulator not canonical", P, D);
      acc = ntt::gl64::add(acc, t);
    }
    if (acc >= P || acc != want[k]) fail("replayed accumulation differs", P, D);
  }
  x::mul<D>(got, in.a, in.b, w);
  for (int k = 0; k < D; ++k)
    if (got[k] >= P || got[k] != want[k]) fail("mul differs from schoolbook", P, D);
  for (int k = 0; k < D; ++k) got[k] = in.a[k];
  x::mul_pre<D>(got, got, in.b, wb);
  for (int k = 0; k < D; ++k)
    if (got[k] != want[k]) fail("mul_pre in place differs", P, D);
  x::scale<D>(got, in.a, in.b[0]);
  for (int k = 0; k < D; ++k)
    if (got[k] >= P || got[k] != (uint64_t)((u128)in.a[k] * in.b[0] % P)) fail("scale", P, D);
  x::add<D>(got, in.a, in.b);
  for (int k = 0; k < D; ++k)
    if (got[k] != (uint64_t)(((u128)in.a[k] + in.b[k]) % P)) fail("add", P, D);
  x::sub<D>(got, in.a, in.b);
  for (int k = 0; k < D; ++k)
    if (got[k] != (uint64_t)(((u128)in.a[k] + P - in.b[k]) % P)) fail("sub", P, D);
}

// every pair with coordinates from the edge set, then `nrand` seeded random pairs
template <int D, class F>
static void run_case(uint64_t p, F&& check) {
  const uint64_t edge[5] = {0, 1 % p, 2 % p, p - 2, p - 1};
  long total = 1;
  for (int i = 0; i < 2 * D; ++i) total *= 5;
  Pair<D> in;
  for (long c = 0; c < total; ++c) {
    long v = c;
    for (int i = 0; i < D; ++i, v /= 5) in.a[i] = edge[v % 5];
    for (int i = 0; i < D; ++i, v /= 5) in.b[i] = edge[v % 5];
    check(in);
  }
  uint64_t seed = 0x4672694578743031ull ^ p ^ (uint64_t)D;
  for (int n = 0; n < 100000; ++n) {
    for (int i = 0; i < D; ++i) in.a[i] = (uint64_t)((u128)splitmix64(seed) * p >> 64);
    for (int i = 0; i < D; ++i) in.b[i] = (uint64_t)((u128)splitmix64(seed) * p >> 64);
    check(in);
  }
}

int main() {
  run_case<4>(2013265921u, [](const Pair<4>& in) { check31<4>(2013265921u, 11, in); });
  run_case<2>(2013265921u, [](const Pair<2>& in) { check31<2>(2013265921u, 11, in); });
  run_case<4>(2130706433u, [](const Pair<4>& in) { check31<4>(2130706433u, 3, in); });
  run_case<2>(ntt::gl64::kP, [](const Pair<2>& in) { check64<2>(7, in); });
  run_case<2>(1004535809u, [](const Pair<2>& in) { check31<2>(1004535809u, 3, in); });
  // the base field as the degree-1 ring: the product is the field's own
  run_case<1>(2013265921u, [](const Pair<1>& in) { check31<1>(2013265921u, 11, in); });
  run_case<1>(ntt::gl64::kP, [](const Pair<1>& in) { check64<1>(7, in); });
  if (g_bad) {
    fprintf(stderr, "fieldext_check: %d mismatches\n", g_bad);
    return 1;
  }
  printf("fieldext_check: ok\n");
  return 0;
}
