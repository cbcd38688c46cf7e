// The modulus-derived constants of Eng29<...>::Args (engines.hpp), computed on the host at plan
// creation: everything except the twiddles w8 / ninv and the debug pointer.  A header of its own so
// that the primitive-level probe (tests/c/field29_probe.hip) hands its kernels the very constants
// the plans hand theirs.  Host only.
#pragma once
#include <cmath>
#include <stdint.h>

#include "field29.hpp"

namespace ntt {

// A: an Eng29<L, ...>::Args (EA = its type, E29 the engine: the PC_* slots); p: the modulus as NH
// canonical little-endian 32-bit words.
template <class E29, int L, int NH, class EA>
inline void eng29_fill_consts(EA& A, const uint32_t* p) {
  uint32_t pw[NH];
  for (int i = 0; i < NH; ++i) pw[i] = p[i];
  pack29<L, NH>(A.M.p, pw);
  for (int i = 0; i < L; ++i) A.kp[0][i] = A.M.p[i];
  for (int j = 1; j < 5; ++j) {  // 2^j p: double the normalised limbs and renormalise
    for (int i = 0; i < L; ++i) A.kp[j][i] = A.kp[j - 1][i] << 1;
    norm_u<L>(A.kp[j]);
  }
  for (int i = 0; i < L; ++i) A.M.p2[i] = A.kp[1][i];
  neg29<L>(A.pbar, A.M.p);
  uint32_t inv = 1;
  for (int i = 0; i < 5; ++i) inv *= 2 - p[0] * inv;
  A.M.pinv = (0u - inv) & kMask29;
  const uint32_t ptop = A.M.p[L - 1];
  A.red_ok = ptop >= (1u << 18) ? 1u : 0u;
  A.red_inv = std::nextafter(1.0f / (float)(ptop + 1u), 0.0f);
  // padded offsets for the unnormalised butterflies (used only when red_ok: p_top >= 3)
  auto padded = [&](uint32_t K, uint32_t pad, uint32_t* c) {
    uint32_t kp[L];
    uint64_t carry = 0;
    for (int i = 0; i < L; ++i) {
      const uint64_t v = (uint64_t)A.M.p[i] * K + carry;
      kp[i] = (uint32_t)v & kMask29;
      carry = v >> 29;
    }
    kp[L - 1] += (uint32_t)(carry << 29);  // K p < 2^(29L): carry is 0 for the supported fields
    const uint32_t b = pad >> 29;
    c[0] = kp[0] + pad;
    for (int i = 1; i + 1 < L; ++i) c[i] = kp[i] + pad - b;
    c[L - 1] = kp[L - 1] - b;
  };
  padded(5, 1u << 29, A.pc[E29::PC_5_29]);
  padded(9, 1u << 30, A.pc[E29::PC_9_30]);
  padded(4, 1u << 29, A.pc[E29::PC_4_29]);
  padded(17, 1u << 29, A.pc[E29::PC_17_29]);
  padded(7, 1u << 30, A.pc[E29::PC_7_30]);
}

}  // namespace ntt
