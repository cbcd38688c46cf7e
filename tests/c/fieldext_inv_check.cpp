// Host check of the inverse in ntt_amd/csrc/fieldext.hpp (f31x::inv, gl64x::inv and the xf interface the DEEP
// calls use on the host and on the device): a a^-1 = 1 with the product taken by schoolbook arithmetic in
// unsigned __int128, never by the header's own product, on (BabyBear, 2, 11), (BabyBear, 4, 11),
// (KoalaBear, 4, 3), (Goldilocks, 2, 7), (Goldilocks, 4, 7) and (1811939329 > 2^30, 2, 13), each also at D = 1.  Inputs: 2 10^4 seeded random
// elements, base-field elements a = (v, 0, ..), a = X, and every element with coordinates from
// {0, 1, p - 1} but 0.  The inverse of 0 is 0 and returns; xf::pow agrees with repeated schoolbook products.
// Exit status 0 when everything agrees; the first mismatches are printed otherwise.
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "fieldext.hpp"

typedef unsigned __int128 u128;

static int g_bad = 0;
static void fail(const char* what, uint64_t p, int d) {
  if (g_bad++ < 20) fprintf(stderr, "p=%llu D=%d: %s\n", (unsigned long long)p, d, what);
}
static uint64_t splitmix64(uint64_t& s) {
  uint64_t z = (s += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
static uint64_t powmod(uint64_t b, uint64_t e, uint64_t p) {
  u128 r = 1 % p, x = b % p;
  for (; e; e >>= 1, x = x * x % p)
    if (e & 1) r = r * x % p;
  return (uint64_t)r;
}

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

// the field's side of the check: canonical <-> working form, the xf constants
struct F31 {
  typedef uint32_t V;
  typedef ntt::xf::K31 K;
  uint64_t p, r, rinv;
  K k;
  F31(uint32_t p_, uint32_t w) : p(p_) {
    r = (1ull << 32) % p;
    rinv = powmod(r, p - 2, p);
    k.p = p_;
    k.pinv = ntt::f31::pinv32(p_);
    k.one = (uint32_t)r;
    k.w = w;
    k.ws = ntt::f31::shoup_companion(w, p_);
  }
  V work(uint64_t v) const { return ntt::xf::to_work(v, k); }
  uint64_t plain(V v) const { return (uint64_t)((u128)v * rinv % p); }
};
struct F64 {
  typedef uint64_t V;
  typedef ntt::xf::K64 K;
  uint64_t p = ntt::gl64::kP;
  K k;
  explicit F64(uint64_t w) {
    k.one = 1;
    k.w = w;
  }
  V work(uint64_t v) const { return v; }
  uint64_t plain(V v) const { return v; }
};

// a a^-1 = 1 (must: the element is known to be invertible), canonical output; returns whether it held
template <int D, class F>
static bool check_one(const F& f, const uint64_t (&a)[D], uint64_t w, bool must) {
  typename F::V aw[D], iw[D];
  for (int j = 0; j < D; ++j) aw[j] = f.work(a[j]);
  ntt::xf::inv<D>(iw, aw, f.k);
  uint64_t inv[D], prod[D];
  bool ok = true;
  for (int j = 0; j < D; ++j) {
    if (!ntt::xf::canonical(iw[j], f.k)) fail("inverse not canonical", f.p, D);
    inv[j] = f.plain(iw[j]);
  }
  school<D>(prod, a, inv, w, f.p);
  for (int j = 0; j < D; ++j) ok = ok && prod[j] == (j ? 0u : 1u);
  if (must && !ok) fail("a a^-1 != 1", f.p, D);
  return ok;
}

template <int D, class F>
static void check_field(const F& f, uint64_t w, bool is_field) {
  uint64_t seed = 0x1234 + 17 * D + f.p;
  long invertible = 0;
  for (int it = 0; it < 20000; ++it) {
    uint64_t a[D];
    for (int j = 0; j < D; ++j) a[j] = splitmix64(seed) % f.p;
    invertible += check_one<D>(f, a, w, is_field);
  }
  if (invertible < 19000) fail("too few random elements inverted", f.p, D);
  for (int it = 0; it < 200; ++it) {  // the base field inside the extension
    uint64_t a[D] = {};
    a[0] = it < 3 ? (it == 0 ? 1 : it == 1 ? 2 : f.p - 1) : 1 + splitmix64(seed) % (f.p - 1);
    check_one<D>(f, a, w, true);
  }
  if (D > 1) {  // X: X^-1 = W^-1 X^(D-1)
    uint64_t a[D] = {};
    a[D > 1 ? 1 : 0] = 1;
    check_one<D>(f, a, w, true);
  }
  {  // coordinates from {0, 1, p - 1}
    const uint64_t edge[3] = {0, 1, f.p - 1};
    int n = 1;
    for (int j = 0; j < D; ++j) n *= 3;
    for (int code = 1; code < n; ++code) {
      uint64_t a[D];
      for (int j = 0, c = code; j < D; ++j, c /= 3) a[j] = edge[c % 3];
      check_one<D>(f, a, w, is_field);
    }
  }
  {  // 0 -> 0, and the call returns
    typename F::V z[D] = {}, out[D];
    ntt::xf::inv<D>(out, z, f.k);
    for (int j = 0; j < D; ++j)
      if (out[j] != 0) fail("inverse of 0 is not 0", f.p, D);
  }
  for (uint64_t e : {0ull, 1ull, 2ull, 5ull, 64ull, 1000ull}) {  // xf::pow against repeated schoolbook products
    uint64_t a[D], want[D] = {};
    typename F::V aw[D], pw[D];
    for (int j = 0; j < D; ++j) aw[j] = f.work(a[j] = splitmix64(seed) % f.p);
    want[0] = 1;
    for (uint64_t i = 0; i < e; ++i) {
      uint64_t t[D];
      school<D>(t, want, a, w, f.p);
      for (int j = 0; j < D; ++j) want[j] = t[j];
    }
    ntt::xf::pow<D>(pw, aw, e, f.k);
    for (int j = 0; j < D; ++j)
      if (f.plain(pw[j]) != want[j]) fail("pow", f.p, D);
  }
}

int main() {
  const F31 bb(2013265921u, 11), kb(2130706433u, 3), big(1811939329u, 13);
  const F64 gl(7);
  check_field<1>(bb, 11, true);
  check_field<2>(bb, 11, true);
  check_field<4>(bb, 11, true);
  check_field<1>(kb, 3, true);
  check_field<4>(kb, 3, true);
  check_field<1>(gl, 7, true);
  check_field<2>(gl, 7, true);
  check_field<4>(gl, 7, true);  // p = 1 mod 4 and 7 a non-residue: X^4 - 7 is irreducible
  check_field<1>(big, 13, true);
  check_field<2>(big, 13, true);
  if (g_bad) {
    fprintf(stderr, "fieldext_inv_check: %d mismatches\n", g_bad);
    return 1;
  }
  printf("fieldext_inv_check: ok\n");
  return 0;
}
