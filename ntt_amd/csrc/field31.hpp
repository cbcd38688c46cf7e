// One-word prime-field arithmetic for any odd prime p < 2^31 on canonical 32-bit values (host +
// device): BabyBear 2^31 - 2^27 + 1, KoalaBear 2^31 - 2^24 + 1 and every smaller odd prime.
//
// At p > 2^30 the sum of two lazy values below 2p no longer fits 32 bits, so every function takes and
// returns canonical values (in [0, p)) unless its name says `lazy`.  Bounds of every intermediate
// (all arithmetic is unsigned, modulo 2^32 where a difference is formed):
//   canon2(x)        x < 2p < 2^32            -> min(x, x - p): x - p wraps above x when x < p
//   add(a, b)        s = a + b < 2p < 2^32    -> canon2(s)
//   sub(a, b)        d = a - b mod 2^32; a >= b: d < p and d + p in [p, 2p) is the larger one;
//                    a < b: d >= 2^32 - p + 1 > 2^31 > d + p - 2^32 = a - b + p in [1, p)
//                                             -> min(d, d + p)
//   sub_lazy(a, b)   a - b + p in [1, 2p - 1], no wrap: an input of the Shoup product, which takes
//                    any 32-bit x
//   shoup_lazy(x, w, ws)   w < p, ws = floor(w 2^32 / p), so w 2^32 = ws p + e with 0 <= e < p.
//                    q = floor(x ws / 2^32) for ANY 32-bit x; x w - q p lies in
//                    [x e / 2^32, x e / 2^32 + p) within [0, 2p): it fits 32 bits, so the low words
//                    x w - q p mod 2^32 are the value itself
//   mulc(x, w, ws)   canon2(shoup_lazy): x w mod p
//   mont_lazy(x, y)  x y < 2^32 p (true for x, y < p < 2^32).  lo + 2^32 hi = x y, m = lo p^-1 mod
//                    2^32, so m p = lo (mod 2^32) and x y - m p = 2^32 (hi - mh), mh = floor(m p /
//                    2^32) < p, hi < p: hi - mh in (-p, p), plus p in (0, 2p)
//   mulv(x, y)       canon2(mont_lazy): x y 2^-32 mod p
// The twiddle tables hold Shoup pairs (w, ws); the element-format tables hold w 2^32 mod p, so that
// mulv by a table entry is a plain product.  4 + 2 VALU ops per twiddle product, 6 + 2 per
// variable product, 2 + 2 per addition or subtraction.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#define NTT_F31_HD __host__ __device__ __forceinline__
#else
#define NTT_F31_HD static inline
#endif

namespace ntt {
namespace f31 {

NTT_F31_HD uint32_t umin(uint32_t a, uint32_t b) { return a < b ? a : b; }
NTT_F31_HD uint32_t mulhi(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umulhi(a, b);
#else
  return (uint32_t)(((uint64_t)a * b) >> 32);
#endif
}

// the moduli this arithmetic serves
NTT_F31_HD bool modulus_ok(uint64_t p) { return (p & 1) && p >= 3 && p < (1ull << 31); }
NTT_F31_HD bool is_canonical(uint32_t x, uint32_t p) { return x < p; }
// x < 2p -> x mod p
NTT_F31_HD uint32_t canon2(uint32_t x, uint32_t p) { return umin(x, x - p); }

NTT_F31_HD uint32_t add(uint32_t a, uint32_t b, uint32_t p) { return canon2(a + b, p); }
NTT_F31_HD uint32_t sub(uint32_t a, uint32_t b, uint32_t p) {
  const uint32_t d = a - b;
  return umin(d, d + p);
}
// a - b + p in [1, 2p - 1]: congruent to a - b, not canonical
NTT_F31_HD uint32_t sub_lazy(uint32_t a, uint32_t b, uint32_t p) { return a - b + p; }

// p^-1 mod 2^32 (Newton: five steps double 1 correct bit to 32)
NTT_F31_HD uint32_t pinv32(uint32_t p) {
  uint32_t inv = 1;
  for (int i = 0; i < 5; ++i) inv *= 2 - p * inv;
  return inv;
}
// the precomputed companion of a twiddle w < p: floor(w 2^32 / p) < 2^32
NTT_F31_HD uint32_t shoup_companion(uint32_t w, uint32_t p) { return (uint32_t)(((uint64_t)w << 32) / p); }

// x w - floor(x ws / 2^32) p in [0, 2p) for any 32-bit x
NTT_F31_HD uint32_t shoup_lazy(uint32_t x, uint32_t w, uint32_t ws, uint32_t p) {
  const uint32_t q = mulhi(x, ws);
  return x * w - q * p;
}
NTT_F31_HD uint32_t mulc(uint32_t x, uint32_t w, uint32_t ws, uint32_t p) { return canon2(shoup_lazy(x, w, ws, p), p); }

// x y 2^-32 + (0 or p), in (0, 2p), for x y < 2^32 p
NTT_F31_HD uint32_t mont_lazy(uint32_t x, uint32_t y, uint32_t p, uint32_t pinv) {
  const uint32_t lo = x * y, hi = mulhi(x, y);
  const uint32_t m = lo * pinv;
  return hi - mulhi(m, p) + p;
}
NTT_F31_HD uint32_t mulv(uint32_t x, uint32_t y, uint32_t p, uint32_t pinv) { return canon2(mont_lazy(x, y, p, pinv), p); }

}  // namespace f31
}  // namespace ntt
