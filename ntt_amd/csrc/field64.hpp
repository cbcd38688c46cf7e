// Goldilocks field arithmetic, p = 2^64 - 2^32 + 1, on canonical 64-bit values (host + device).
//
// p > 2^63 leaves no lazy headroom in 64 bits, so every function takes and returns canonical values
// (in [0, p)).  With eps = 2^32 - 1 = 2^64 - p:
//   2^64 = eps (mod p)  and  2^96 = -1 (mod p),
// so a carry out of 64 bits is paid back by adding eps and a borrow by subtracting eps, and a 128-bit
// product lo + 2^64 (hl + 2^32 hh) reduces to lo - hh + hl eps with no multiplication (hl eps =
// (hl << 32) - hl).  Twiddles are plain canonical values: no Montgomery form, no Shoup quotient.
//
// The 64 x 64 -> 128 product is written on 32-bit halves so that each step is one 32 x 32 + 64
// multiply-add (v_mad_u64_u32 on gfx950): four of them per product.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#define NTT_F64_HD __host__ __device__ __forceinline__
#else
#define NTT_F64_HD static inline
#endif

namespace ntt {
namespace gl64 {

constexpr uint64_t kP = 0xFFFFFFFF00000001ull;  // 2^64 - 2^32 + 1
constexpr uint64_t kEps = 0xFFFFFFFFull;        // 2^64 - p

// a raw 64-bit pattern is a canonical element iff it is below p ([p, 2^64) holds eps patterns that are not)
NTT_F64_HD bool is_canonical(uint64_t x) { return x < kP; }
// any 64-bit pattern -> its canonical value (x < 2^64 < 2p: one subtraction; x - p = x + eps mod 2^64)
NTT_F64_HD uint64_t canonical(uint64_t x) { return x >= kP ? x + kEps : x; }

// a + b mod p.  The true sum is s + 2^64 c < 2p.  With a carry, s + 2^64 - p = s + eps (< p, so it does
// not wrap again); without one, s >= p needs s - p, which is s + eps mod 2^64 as well.
NTT_F64_HD uint64_t add(uint64_t a, uint64_t b) {
  const uint64_t s = a + b;
  const bool fix = (s < a) | (s >= kP);
  return fix ? s + kEps : s;
}

// a - b mod p.  With a borrow the stored difference is a - b + 2^64; a - b + p = that - eps (>= 1).
NTT_F64_HD uint64_t sub(uint64_t a, uint64_t b) {
  const uint64_t d = a - b;
  return a < b ? d - kEps : d;
}

// lo + 2^64 hi mod p for any 128-bit value
NTT_F64_HD uint64_t reduce128(uint64_t lo, uint64_t hi) {
  const uint64_t hh = hi >> 32, hl = hi & kEps;
  // t0 = lo - hh (2^96 = -1).  Borrow: the stored value is lo - hh + 2^64 >= 2^64 - 2^32 + 1, and
  // 2^64 = eps, so subtract eps (no second borrow).
  uint64_t t0 = lo - hh;
  if (lo < hh) t0 -= kEps;
  // t1 = hl eps <= (2^32 - 1)^2 < 2^64
  const uint64_t t1 = (hl << 32) - hl;
  // t2 = t0 + t1.  Carry: the stored value is t0 + t1 - 2^64 <= t0 - 2^33 + 1, so adding eps back
  // stays below 2^64.
  uint64_t t2 = t0 + t1;
  if (t2 < t0) t2 += kEps;
  // t2 is any 64-bit pattern congruent to the product: bring [p, 2^64) down
  return canonical(t2);
}

// a b mod p.  Partial products on 32-bit halves; no step overflows 64 bits:
// (2^32 - 1)^2 + 2 (2^32 - 1) = 2^64 - 1.
NTT_F64_HD uint64_t mul(uint64_t a, uint64_t b) {
  const uint32_t a0 = (uint32_t)a, a1 = (uint32_t)(a >> 32);
  const uint32_t b0 = (uint32_t)b, b1 = (uint32_t)(b >> 32);
  const uint64_t p00 = (uint64_t)a0 * b0;
  const uint64_t m1 = (uint64_t)a0 * b1 + (p00 >> 32);
  const uint64_t m2 = (uint64_t)a1 * b0 + (uint32_t)m1;
  const uint64_t hi = (uint64_t)a1 * b1 + (m1 >> 32) + (m2 >> 32);
  const uint64_t lo = (m2 << 32) | (uint32_t)p00;
  return reduce128(lo, hi);
}

}  // namespace gl64
}  // namespace ntt
