// Host check of ntt_amd/csrc/field31.hpp (the one-word arithmetic the Eng31 kernels run): add, sub,
// the twiddle product with its precomputed companion, the variable product and canonicalisation
// against uint64_t arithmetic mod p, with every intermediate bound the header documents asserted, for
// p = 2013265921 (BabyBear), 2130706433 (KoalaBear), 1004535809 (30 bits) and 3: the edge set's full
// cross product (reduced below p), then 10^6 seeded random pairs per modulus.
// Exit status 0 when everything agrees; the first mismatches are printed otherwise.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "field31.hpp"

namespace f = ntt::f31;

static int g_bad = 0;

static void expect(const char* what, uint32_t p, uint32_t a, uint32_t b, uint64_t got, uint64_t want) {
  if (got == want) return;
  if (g_bad++ < 20)
    fprintf(stderr, "p=%u %s(%u, %u) = %llu, expected %llu\n", p, what, a, b, (unsigned long long)got,
            (unsigned long long)want);
}
static void bound(const char* what, uint32_t p, uint32_t a, uint32_t b, bool ok) {
  if (ok) return;
  if (g_bad++ < 20) fprintf(stderr, "p=%u bound %s broken at (%u, %u)\n", p, what, a, b);
}

struct Field {
  uint32_t p, pinv;
  uint64_t r;     // 2^32 mod p
  uint64_t rinv;  // 2^-32 mod p
};

static uint64_t powmod(uint64_t b, uint64_t e, uint64_t p) {
  uint64_t r = 1 % p;
  b %= p;
  for (; e; e >>= 1, b = b * b % p)
    if (e & 1) r = r * b % p;
  return r;
}

// a, b canonical
static void check_pair(const Field& F, uint32_t a, uint32_t b) {
  const uint32_t p = F.p;
  const uint64_t P = p;
  // add: the raw sum stays below 2p < 2^32
  bound("a + b < 2p", p, a, b, (uint64_t)a + b < 2 * P && 2 * P <= (1ull << 32));
  expect("add", p, a, b, f::add(a, b, p), ((uint64_t)a + b) % P);
  // sub
  expect("sub", p, a, b, f::sub(a, b, p), ((uint64_t)a + P - b) % P);
  // sub_lazy: in [1, 2p - 1], congruent to a - b
  const uint32_t dl = f::sub_lazy(a, b, p);
  bound("sub_lazy in [1, 2p)", p, a, b, dl >= 1 && dl < 2 * P && (uint64_t)dl == (uint64_t)a + P - b);
  // twiddle product: b is the twiddle, ws its companion
  const uint32_t ws = f::shoup_companion(b, p);
  bound("ws = floor(w 2^32 / p)", p, a, b, ((uint64_t)b << 32) - (uint64_t)ws * P < P);
  const uint64_t ab = (uint64_t)a * b % P;
  {
    const uint64_t q = ((uint64_t)a * ws) >> 32;
    const uint64_t exact = (uint64_t)a * b - q * P;  // no wrap in 64 bits: q p <= a w
    bound("shoup q p <= x w", p, a, b, q * P <= (uint64_t)a * b);
    bound("shoup_lazy < 2p", p, a, b, exact < 2 * P);
    expect("shoup_lazy", p, a, b, f::shoup_lazy(a, b, ws, p), exact);
  }
  expect("mulc", p, a, b, f::mulc(a, b, ws, p), ab);
  // the same product fed with the butterfly's unreduced difference a - b + p (any 32-bit x is legal)
  {
    const uint32_t x = dl;
    const uint64_t q = ((uint64_t)x * ws) >> 32;
    const uint64_t exact = (uint64_t)x * b - q * P;
    bound("shoup_lazy(sub_lazy) < 2p", p, a, b, q * P <= (uint64_t)x * b && exact < 2 * P);
    expect("mulc(sub_lazy)", p, a, b, f::mulc(x, b, ws, p), (uint64_t)x % P * b % P);
  }
  // variable product: x y 2^-32, lazy value in (0, 2p)
  {
    const uint32_t ml = f::mont_lazy(a, b, p, F.pinv);
    const uint32_t lo = a * b, hi = (uint32_t)(((uint64_t)a * b) >> 32);
    const uint32_t m = lo * F.pinv, mh = (uint32_t)(((uint64_t)m * p) >> 32);
    bound("m p = lo mod 2^32", p, a, b, (uint32_t)(m * p) == lo);
    bound("hi < p, mh < p", p, a, b, hi < p && mh < p);
    bound("mont_lazy in (0, 2p)", p, a, b, ml > 0 && ml < 2 * P && (uint64_t)ml == (uint64_t)hi + P - mh);
    expect("mulv", p, a, b, f::mulv(a, b, p, F.pinv), ab * F.rinv % P);
  }
  // mulv by the element-format table entry w 2^32 mod p is the plain product
  expect("mulv(a, b R)", p, a, b, f::mulv(a, (uint32_t)(b * F.r % P), p, F.pinv), ab);
}

static uint64_t splitmix64(uint64_t& s) {
  uint64_t z = (s += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

static void check_field(uint32_t p) {
  Field F;
  F.p = p;
  F.pinv = f::pinv32(p);
  bound("p pinv = 1 mod 2^32", p, 0, 0, (uint32_t)(p * F.pinv) == 1u && f::modulus_ok(p));
  F.r = (1ull << 32) % p;
  F.rinv = powmod(F.r, (uint64_t)p - 2, p);
  bound("r rinv = 1", p, 0, 0, F.r * F.rinv % p == 1 % p);

  const uint64_t raw[] = {0, 1, 2, 1ull << 24, 1ull << 27, (1ull << 30) - 1, 1ull << 30, (1ull << 30) + 1,
                          ((uint64_t)p - 1) / 2, ((uint64_t)p + 1) / 2, (uint64_t)p - 2, (uint64_t)p - 1};
  std::vector<uint32_t> edge;
  for (uint64_t v : raw) edge.push_back((uint32_t)(v % p));
  for (uint32_t a : edge)
    for (uint32_t b : edge) check_pair(F, a, b);

  // canonicalisation: values below 2p come down once; canonical values stay
  for (uint32_t a : edge) {
    expect("canon2", p, a, 0, f::canon2(a, p), a);
    expect("canon2(+p)", p, a, 0, f::canon2(a + p, p), a);
    expect("is_canonical", p, a, 0, f::is_canonical(a, p) ? 1 : 0, 1);
  }
  const uint32_t bad[] = {p, p + 1, 0x80000000u, 0xFFFFFFFFu};
  for (uint32_t a : bad) expect("is_canonical", p, a, 0, f::is_canonical(a, p) ? 1 : 0, 0);
  // the twiddle product takes any 32-bit word
  for (uint32_t x : bad)
    for (uint32_t w : edge) {
      const uint32_t ws = f::shoup_companion(w, p);
      const uint64_t q = ((uint64_t)x * ws) >> 32;
      bound("shoup_lazy(any x) < 2p", p, x, w, q * p <= (uint64_t)x * w && (uint64_t)x * w - q * p < 2ull * p);
      expect("mulc(any x)", p, x, w, f::mulc(x, w, ws, p), (uint64_t)x % p * w % p);
    }

  uint64_t seed = 0x4261627942656172ull ^ p;
  for (int i = 0; i < 1000000; ++i) {
    const uint32_t a = (uint32_t)(splitmix64(seed) % p), b = (uint32_t)(splitmix64(seed) % p);
    check_pair(F, a, b);
  }
}

int main() {
  for (uint32_t p : {2013265921u, 2130706433u, 1004535809u, 3u}) check_field(p);
  if (g_bad) {
    fprintf(stderr, "field31_check: %d mismatches\n", g_bad);
    return 1;
  }
  printf("field31_check: ok\n");
  return 0;
}
