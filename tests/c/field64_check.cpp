// Host check of ntt_amd/csrc/field64.hpp (the Goldilocks arithmetic the Eng64G kernels run):
// add, sub, mul and canonicalisation against unsigned __int128 arithmetic mod p on the edge set's
// full cross product, the non-canonical patterns, and 10^6 seeded random pairs.
// Exit status 0 when everything agrees; the first mismatches are printed otherwise.
#include <cstdint>
#include <cstdio>

#include "field64.hpp"

using ntt::gl64::kEps;
using ntt::gl64::kP;
typedef unsigned __int128 u128;

static int g_bad = 0;

static void expect(const char* what, uint64_t a, uint64_t b, uint64_t got, uint64_t want) {
  if (got == want) return;
  if (g_bad++ < 20)
    fprintf(stderr, "%s(%016llx, %016llx) = %016llx, expected %016llx\n", what, (unsigned long long)a,
            (unsigned long long)b, (unsigned long long)got, (unsigned long long)want);
}

static void check_pair(uint64_t a, uint64_t b) {
  expect("add", a, b, ntt::gl64::add(a, b), (uint64_t)(((u128)a + b) % kP));
  expect("sub", a, b, ntt::gl64::sub(a, b), (uint64_t)(((u128)a + kP - b) % kP));
  expect("mul", a, b, ntt::gl64::mul(a, b), (uint64_t)(((u128)a * b) % kP));
}

static uint64_t splitmix64(uint64_t& s) {
  uint64_t z = (s += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

int main() {
  static_assert(kP == 0xFFFFFFFF00000001ull && kEps == 0xFFFFFFFFull, "modulus");
  const uint64_t edge[] = {0,
                           1,
                           2,
                           kEps - 1,
                           kEps,
                           kEps + 1,
                           1ull << 32,
                           (1ull << 32) + 1,
                           (1ull << 63) - 1,
                           1ull << 63,
                           (1ull << 63) + 1,
                           kP - kEps,
                           kP - 2,
                           kP - 1};
  for (uint64_t a : edge)
    for (uint64_t b : edge) check_pair(a, b);

  // raw patterns: canonical values stay, [p, 2^64) comes down by p
  for (uint64_t a : edge) {
    expect("canonical", a, 0, ntt::gl64::canonical(a), a);
    expect("is_canonical", a, 0, ntt::gl64::is_canonical(a) ? 1 : 0, 1);
  }
  const uint64_t raw[] = {kP, kP + 1, ~0ull};
  for (uint64_t a : raw) {
    expect("canonical", a, 0, ntt::gl64::canonical(a), a - kP);
    expect("is_canonical", a, 0, ntt::gl64::is_canonical(a) ? 1 : 0, 0);
  }
  // reduce128 on the extreme 128-bit values (a product never reaches them; the reduction takes any)
  const uint64_t words[] = {0, 1, kEps, 1ull << 32, kP - 1, kP, ~0ull};
  for (uint64_t lo : words)
    for (uint64_t hi : words)
      expect("reduce128", lo, hi, ntt::gl64::reduce128(lo, hi), (uint64_t)((((u128)hi << 64) | lo) % kP));

  uint64_t seed = 0x476F6C64696C6F63ull;
  for (int i = 0; i < 1000000; ++i) {
    const uint64_t a = splitmix64(seed) % kP, b = splitmix64(seed) % kP;
    check_pair(a, b);
  }
  if (g_bad) {
    fprintf(stderr, "field64_check: %d mismatches\n", g_bad);
    return 1;
  }
  printf("field64_check: ok\n");
  return 0;
}
