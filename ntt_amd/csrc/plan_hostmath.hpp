// Host field arithmetic of the plans (table building) and each engine's encoding of table entries
// and kernel arguments.  Included by ntt_plan.cpp alone.
#pragma once
#include <array>
#include <cstdint>
#include <vector>

#include "eng29_args.hpp"
#include "ntt_kernels.hpp"

namespace {
using namespace ntt;

// ------------------------------------------------------------------------------ host field math
template <int N>
using Vec = std::array<uint32_t, N>;

template <int N>
struct HostField {
  Modulus<N> M;
  Vec<N> r1{}, r2{};  // R mod p, R^2 mod p

  Vec<N> mul(const Vec<N>& a, const Vec<N>& b) const {
    Vec<N> r;
    mont_mul_cios<N>(r.data(), a.data(), b.data(), M);
    return r;
  }
  Vec<N> add(const Vec<N>& a, const Vec<N>& b) const {
    Vec<N> r;
    add_mod<N>(r.data(), a.data(), b.data(), M);
    return r;
  }
  Vec<N> to_mont(const Vec<N>& a) const { return mul(a, r2); }
  Vec<N> from_mont(const Vec<N>& a) const {
    Vec<N> one{};
    one[0] = 1;
    return mul(a, one);
  }
  // base (Montgomery) ^ e, e given as 32-bit little-endian words
  Vec<N> pow(const Vec<N>& base, const std::vector<uint32_t>& e) const {
    Vec<N> acc = r1, b = base;
    for (size_t i = 0; i < e.size() * 32; ++i) {
      if ((e[i / 32] >> (i % 32)) & 1) acc = mul(acc, b);
      b = mul(b, b);
    }
    return acc;
  }
  Vec<N> pow_u64(const Vec<N>& base, uint64_t e) const {
    return pow(base, std::vector<uint32_t>{(uint32_t)e, (uint32_t)(e >> 32)});
  }
  bool below_p(const Vec<N>& a) const {
    for (int i = N - 1; i >= 0; --i)
      if (a[i] != M.p[i]) return a[i] < M.p[i];
    return false;
  }
  // limbs64 host words (64-bit, little-endian) -> the element they spell, as N 32-bit words (which may
  // reach past the caller's limbs: Goldilocks, N = 3 over one 64-bit limb).  False: a bit above the N
  // words is set, or the value is not below p.  Zero passes: the callers that refuse it check for it.
  bool canonical(const uint64_t* w, unsigned limbs64, Vec<N>& out) const {
    out = Vec<N>{};
    for (int i = 0; i < N && (unsigned)(i / 2) < limbs64; ++i) out[i] = (uint32_t)(w[i / 2] >> (32 * (i % 2)));
    for (unsigned i = (N + 1) / 2; i < limbs64; ++i)
      if (w[i]) return false;
    if ((N & 1) && (unsigned)(N / 2) < limbs64 && (w[N / 2] >> 32)) return false;
    return below_p(out);
  }
};

template <int N>
static bool vec_lt(const Vec<N>& a, const Vec<N>& b) {
  for (int i = N - 1; i >= 0; --i)
    if (a[i] != b[i]) return a[i] < b[i];
  return false;
}

// ------------------------------------------------------------------------------ engine encodings
// The host does all table arithmetic in 32-bit Montgomery form (HostField<NH>), produces canonical
// values, then encodes them in the engine's own Montgomery domain / limb layout.
template <class E>
struct EngHost;

template <int L, int W32, int S, int T>
struct EngHost<Eng29<L, W32, S, T>> {
  using E29 = Eng29<L, W32, S, T>;
  static constexpr int NH = W32;
  static constexpr int TW = E29::TW;
  using EA = typename E29::Args;
  HostField<NH> const* H = nullptr;
  Vec<NH> kR{};          // B = 2^(29L) mod p, canonical
  uint32_t pinvB[L] = {};  // p^-1 mod B
  void init(const HostField<NH>& h) {
    H = &h;
    Vec<NH> x{};
    x[0] = 1;
    for (int k = 0; k < 29 * L; ++k) x = h.add(x, x);
    kR = x;
    uint32_t pw[NH], pl[L];
    for (int i = 0; i < NH; ++i) pw[i] = h.M.p[i];
    pack29<L, NH>(pl, pw);
    inv_mod_B29<L>(pinvB, pl);
  }
  static void limbs(const Vec<NH>& c, uint32_t (&x)[L]) {
    uint32_t w[NH];
    for (int i = 0; i < NH; ++i) w[i] = c[i];
    pack29<L, NH>(x, w);
  }
  Vec<NH> times_B(const Vec<NH>& c) const { return H->mul(c, H->to_mont(kR)); }  // c B mod p
  // canonical c -> Shoup table entry (c, floor(c B / p)) as TW words
  void encode(const Vec<NH>& c, uint32_t* out) const {
    uint32_t w[L], wr[L], ws[L];
    limbs(c, w);
    limbs(times_B(c), wr);
    shoup_ws29<L>(ws, wr, pinvB);
    for (int i = 0; i < TW; ++i) out[i] = i < L ? w[i] : (i < 2 * L ? ws[i - L] : 0u);
  }
  // entry whose value is c R_e (R_e = B): the left factor of the two-level twiddle products
  void encode_scaled(const Vec<NH>& c, uint32_t* out) const { encode(times_B(c), out); }
  bool check_modulus(const uint32_t* p) const {
    // 2p fits the HBM words (p < 2^(32 W32 - 1)) and 64p <= B = 2^(29L) (lazy bounds up to 33p)
    int bits = 0;
    for (int i = NH - 1; i >= 0; --i)
      if (p[i]) { bits = 32 * i + 32 - __builtin_clz(p[i]); break; }
    return bits <= 32 * NH - 1 && bits <= 29 * L - 6;
  }
  void fill_args(EA& A, const uint32_t* p, const Vec<NH>* w8, const Vec<NH>& ninv) const {
    eng29_fill_consts<E29, L, NH>(A, p);  // eng29_args.hpp: everything but the twiddles
    uint32_t tmp[TW];
    auto to_tw = [&](const Vec<NH>& c, typename E29::Tw& t) {
      encode(c, tmp);
      for (int i = 0; i < L; ++i) {
        t.w[i] = tmp[i];
        t.ws[i] = tmp[L + i];
      }
    };
    for (int k = 0; k < 3; ++k) to_tw(w8[k], A.w8[k]);
    to_tw(ninv, A.ninv);
  }
};

// The one-word engines' arguments (Eng32, Eng31): w_8^k and n^-1 as the Shoup pairs of EH::encode
template <class EH, class EA, class V>
static void fill_tw_pairs(const EH& eh, EA& A, const V* w8, const V& ninv) {
  uint32_t t[2];
  auto tw = [&](const V& c, auto& e) {
    eh.encode(c, t);
    e.w[0] = t[0];
    e.ws = t[1];
  };
  for (int k = 0; k < 3; ++k) tw(w8[k], A.w8[k]);
  tw(ninv, A.ninv);
}

template <int N, int MEMW_, int SCR_>
struct EngHost<Eng32<N, MEMW_, SCR_>> {
  static constexpr int NH = N;
  using EA = typename Eng32<N, MEMW_, SCR_>::Args;
  HostField<NH> const* H = nullptr;
  void init(const HostField<NH>& h) { H = &h; }
  // canonical c -> Shoup pair (c, floor(c 2^32 / p))
  void encode(const Vec<NH>& c, uint32_t* out) const {
    out[0] = c[0];
    out[1] = (uint32_t)(((uint64_t)c[0] << 32) / H->M.p[0]);
  }
  // entry whose value is c R_e (R_e = 2^32, the Montgomery radix of Eng32::mulv): c's Montgomery form
  void encode_scaled(const Vec<NH>& c, uint32_t* out) const { encode(H->to_mont(c), out); }
  // lazy values up to 4p must fit 32 bits
  bool check_modulus(const uint32_t* p) const { return p[0] < (1u << 30); }
  void fill_args(EA& A, const uint32_t* p, const Vec<NH>* w8, const Vec<NH>& ninv) const {
    A.p = p[0];
    A.p2 = 2 * p[0];
    uint32_t inv = 1;
    for (int i = 0; i < 5; ++i) inv *= 2 - p[0] * inv;  // p^-1 mod 2^32 (Newton)
    A.pinv = inv;
    fill_tw_pairs(*this, A, w8, ninv);
  }
};

// Goldilocks: the host works on the modulus zero-padded to three 32-bit words (the no-carry host
// Montgomery product needs a top word below 2^31 - 1, and p's own top word is 2^32 - 1); the engine's
// values and table entries are the canonical low two words, and its radix R_e is 1.
constexpr uint64_t kGoldilocksP = 0xFFFFFFFF00000001ull;
template <>
struct EngHost<Eng64G> {
  static constexpr int NH = 3;
  using EA = Eng64G::Args;
  HostField<NH> const* H = nullptr;
  void init(const HostField<NH>& h) { H = &h; }
  void encode(const Vec<NH>& c, uint32_t* out) const {
    out[0] = c[0];
    out[1] = c[1];
  }
  void encode_scaled(const Vec<NH>& c, uint32_t* out) const { encode(c, out); }
  bool check_modulus(const uint32_t* p) const {
    return p[0] == (uint32_t)kGoldilocksP && p[1] == (uint32_t)(kGoldilocksP >> 32) && p[2] == 0u;
  }
  void fill_args(EA& A, const uint32_t*, const Vec<NH>* w8, const Vec<NH>& ninv) const {
    for (int k = 0; k < 3; ++k) encode(w8[k], A.w8[k].w);
    encode(ninv, A.ninv.w);
  }
};

// Eng31: one 32-bit host word; twiddle entries are Shoup pairs, element-format entries w 2^32 mod p (the
// Montgomery radix of Eng31::mulv), like the P path's, on any odd modulus below 2^31.
template <>
struct EngHost<Eng31> {
  static constexpr int NH = 1;
  using EA = Eng31::Args;
  HostField<NH> const* H = nullptr;
  void init(const HostField<NH>& h) { H = &h; }
  void encode(const Vec<NH>& c, uint32_t* out) const {
    out[0] = c[0];
    out[1] = f31::shoup_companion(c[0], H->M.p[0]);
  }
  void encode_scaled(const Vec<NH>& c, uint32_t* out) const { encode(H->to_mont(c), out); }
  bool check_modulus(const uint32_t* p) const { return f31::modulus_ok(p[0]); }
  void fill_args(EA& A, const uint32_t* p, const Vec<NH>* w8, const Vec<NH>& ninv) const {
    A.p = p[0];
    A.pinv = f31::pinv32(p[0]);
    fill_tw_pairs(*this, A, w8, ninv);
  }
};

}  // namespace
