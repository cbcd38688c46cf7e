// Host check of ntt_amd/csrc/poseidon2.hpp, the text the Merkle kernels run: the permutation, the sponge and the
// compression against the golden vectors of tests/golden/poseidon2_vectors.json (the integer oracle
// tests/poseidon2_ref.py; tests/test_poseidon2_host.py flattens them into the token file named on the command
// line), on canonical data and, on the 4-byte fields, on Montgomery-form data; and two algebraic pins that do not
// depend on the oracle, in unsigned __int128 arithmetic:
//   M_E equals the product with the explicit matrix circ(2 M4, M4, .., M4);
//   with rounds_f = 2, rounds_p = 0 and degree 3 the permutation is M_E((M_E((M_E s + c_0)^3) + c_1)^3).
// Token file: the number of cases, then per case
//   p t alpha rounds_f rounds_p  ext_rc[rounds_f t] int_rc[rounds_p] int_diag[t]
//   nstates {in[t] out[t]}  nrows {w row[w] digest[D]}  nleaves w {row[w]} nodes[(2 nleaves - 1) D]
// Exit status 0 when everything agrees; the first mismatches are printed otherwise.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "poseidon2.hpp"

typedef unsigned __int128 u128;
using namespace ntt;

static int g_bad = 0;
static void fail(const char* what, uint64_t p, uint64_t at) {
  if (g_bad++ < 20) fprintf(stderr, "p=%llu: %s (%llu)\n", (unsigned long long)p, what, (unsigned long long)at);
}
static uint64_t splitmix64(uint64_t& s) {
  uint64_t z = (s += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

static p2::P31 k31(uint64_t p, bool mont) {
  p2::P31 k{};
  const uint64_t r = (1ull << 32) % p;
  k.p = (uint32_t)p;
  k.pinv = f31::pinv32(k.p);
  k.one = (uint32_t)r;
  k.r2 = (uint32_t)(r * r % p);
  k.mont = mont ? 1u : 0u;
  return k;
}
static p2::P64 k64() {
  p2::P64 k{};
  k.one = 1;
  return k;
}
// canonical word -> the I/O form of the case
static uint32_t io(uint64_t v, const p2::P31& k) { return k.mont ? (uint32_t)((v << 32) % k.p) : (uint32_t)v; }
static uint64_t io(uint64_t v, const p2::P64&) { return v; }

struct Case {
  uint64_t p;
  unsigned t, alpha, rf, rp;
  std::vector<uint64_t> ext, irc, diag;
  std::vector<std::vector<uint64_t>> st_in, st_out, rows, digests, leaves;
  std::vector<uint64_t> nodes;
};

static std::vector<uint64_t> g_tok;
static size_t g_pos = 0;
static uint64_t next() {
  if (g_pos >= g_tok.size()) {
    fprintf(stderr, "token file too short\n");
    exit(2);
  }
  return g_tok[g_pos++];
}
static std::vector<uint64_t> take(size_t n) {
  std::vector<uint64_t> v(n);
  for (auto& x : v) x = next();
  return v;
}

template <int T, int A, class V, class K>
static void run_case(const Case& c, const K& k) {
  constexpr int D = T / 2;
  std::vector<V> tab(p2::Layout<T>::elems(c.rf, c.rp));
  if (!p2::pack<T>(tab.data(), c.p, c.rf, c.rp, c.ext.data(), c.irc.data(), c.diag.data(), k)) fail("pack refused", c.p, 0);
  for (size_t i = 0; i < c.st_in.size(); ++i) {
    V s[T];
    for (int j = 0; j < T; ++j) s[j] = p2::load_form(io(c.st_in[i][j], k), k);
    p2::permute<T, A>(s, tab.data(), c.rf, c.rp, k);
    for (int j = 0; j < T; ++j)
      if (p2::store_form(s[j], k) != io(c.st_out[i][j], k)) fail("permutation", c.p, i);
  }
  for (size_t i = 0; i < c.rows.size(); ++i) {
    std::vector<V> row(c.rows[i].size());
    for (size_t j = 0; j < row.size(); ++j) row[j] = io(c.rows[i][j], k);
    V dig[D];
    p2::hash_row<T, A>(dig, row.data(), row.size(), tab.data(), c.rf, c.rp, k);
    for (int j = 0; j < D; ++j)
      if (dig[j] != io(c.digests[i][j], k)) fail("leaf hash", c.p, i);
  }
  {  // the tree: leaves, then every layer by compress
    const size_t n = c.leaves.size();
    std::vector<V> nodes((2 * n - 1) * D);
    for (size_t i = 0; i < n; ++i) {
      std::vector<V> row(c.leaves[i].size());
      for (size_t j = 0; j < row.size(); ++j) row[j] = io(c.leaves[i][j], k);
      p2::hash_row<T, A>(&nodes[i * D], row.data(), row.size(), tab.data(), c.rf, c.rp, k);
    }
    for (size_t in = 0, out = n, m = n; m > 1; in += m, m >>= 1)
      for (size_t i = 0; i < m / 2; ++i, ++out)
        p2::compress<T, A>(&nodes[out * D], &nodes[(in + 2 * i) * D], &nodes[(in + 2 * i + 1) * D], tab.data(), c.rf, c.rp, k);
    for (size_t i = 0; i < nodes.size(); ++i)
      if (nodes[i] != io(c.nodes[i], k)) fail("tree node", c.p, i / D);
  }
}

template <int T, class V, class K>
static void run_alpha(const Case& c, const K& k) {
  if (c.alpha == 3) run_case<T, 3, V>(c, k);
  else if (c.alpha == 5) run_case<T, 5, V>(c, k);
  else if (c.alpha == 7) run_case<T, 7, V>(c, k);
  else fail("degree", c.p, c.alpha);
}

// ---- the pins
static const int kM4[4][4] = {{2, 3, 1, 1}, {1, 2, 3, 1}, {1, 1, 2, 3}, {3, 1, 1, 2}};
template <int T>
static void circ(uint64_t (&y)[T], const uint64_t (&x)[T], uint64_t p) {
  for (int i = 0; i < T; ++i) {
    u128 acc = 0;
    for (int j = 0; j < T; ++j) {
      const int f = (i / 4 == j / 4 ? 2 : 1) * kM4[i % 4][j % 4];
      acc = (acc + (u128)f * x[j]) % p;
    }
    y[i] = (uint64_t)acc;
  }
}
static uint64_t cube(uint64_t x, uint64_t p) { return (uint64_t)((u128)x * x % p * x % p); }

template <int T, class V, class K>
static void pins(uint64_t p, const K& k, uint64_t seed) {
  for (int it = 0; it < 200; ++it) {
    uint64_t x[T], y[T], c0[T], c1[T];
    for (int j = 0; j < T; ++j) {
      x[j] = it == 0 ? p - 1 : splitmix64(seed) % p;
      c0[j] = splitmix64(seed) % p;
      c1[j] = splitmix64(seed) % p;
    }
    // M_E is linear, so the canonical words serve in any form
    V s[T];
    for (int j = 0; j < T; ++j) s[j] = (V)x[j];
    p2::m_ext<T>(s, k);
    circ<T>(y, x, p);
    for (int j = 0; j < T; ++j)
      if (s[j] != (V)y[j]) fail("M_E is not circ(2 M4, M4, ..)", p, it);
    // rounds_f = 2, rounds_p = 0, degree 3, written out (an identity of polynomials: it holds where 3 | p - 1 too)
    uint64_t a[T], b[T], want[T];
    circ<T>(a, x, p);
    for (int j = 0; j < T; ++j) a[j] = cube((uint64_t)(((u128)a[j] + c0[j]) % p), p);
    circ<T>(b, a, p);
    for (int j = 0; j < T; ++j) b[j] = cube((uint64_t)(((u128)b[j] + c1[j]) % p), p);
    circ<T>(want, b, p);
    uint64_t ext[2 * T], diag[T];
    for (int j = 0; j < T; ++j) ext[j] = c0[j], ext[T + j] = c1[j], diag[j] = 1;
    if (p % 3 != 1 && !p2::shape_ok(p, 3, 2, 0)) fail("shape refused", p, 0);
    std::vector<V> tab(p2::Layout<T>::elems(2, 0));
    p2::pack<T>(tab.data(), p, 2, 0, ext, nullptr, diag, k);
    for (int j = 0; j < T; ++j) s[j] = p2::load_form(io(x[j], k), k);
    p2::permute<T, 3>(s, tab.data(), 2, 0, k);
    for (int j = 0; j < T; ++j)
      if (p2::store_form(s[j], k) != io(want[j], k)) fail("two degree-3 rounds", p, it);
  }
}

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: poseidon2_check TOKENS\n");
    return 2;
  }
  FILE* f = fopen(argv[1], "r");
  if (!f) {
    perror(argv[1]);
    return 2;
  }
  unsigned long long v;
  while (fscanf(f, "%llu", &v) == 1) g_tok.push_back(v);
  fclose(f);

  const uint64_t ncases = next();
  for (uint64_t ci = 0; ci < ncases; ++ci) {
    Case c;
    c.p = next(), c.t = (unsigned)next(), c.alpha = (unsigned)next(), c.rf = (unsigned)next(), c.rp = (unsigned)next();
    c.ext = take((size_t)c.rf * c.t), c.irc = take(c.rp), c.diag = take(c.t);
    if (!p2::shape_ok(c.p, c.alpha, c.rf, c.rp)) fail("shape refused", c.p, ci);
    const size_t d = c.t / 2;
    for (uint64_t n = next(); n--;) c.st_in.push_back(take(c.t)), c.st_out.push_back(take(c.t));
    for (uint64_t n = next(); n--;) {
      const size_t w = next();
      c.rows.push_back(take(w)), c.digests.push_back(take(d));
    }
    const size_t nl = next(), w = next();
    for (size_t i = 0; i < nl; ++i) c.leaves.push_back(take(w));
    c.nodes = take((2 * nl - 1) * d);
    if (c.t == 16 && c.p < (1ull << 31)) {
      run_alpha<16, uint32_t>(c, k31(c.p, false));
      run_alpha<16, uint32_t>(c, k31(c.p, true));
    } else if (c.t == 8 && c.p == gl64::kP) {
      run_alpha<8, uint64_t>(c, k64());
    } else {
      fail("no engine for the case", c.p, c.t);
    }
  }
  if (g_pos != g_tok.size()) fail("tokens left over", 0, g_tok.size() - g_pos);

  // a bad parameter set is refused
  if (p2::shape_ok(2013265921u, 3, 8, 13) || p2::shape_ok(2013265921u, 7, 7, 13) || p2::shape_ok(2013265921u, 7, 18, 13) ||
      p2::shape_ok(2013265921u, 7, 8, 65) || p2::shape_ok(gl64::kP, 5, 8, 22) || p2::shape_ok(2130706433u, 4, 8, 20))
    fail("a bad shape was accepted", 0, 0);

  pins<16, uint32_t>(2130706433u, k31(2130706433u, false), 11);
  pins<16, uint32_t>(2130706433u, k31(2130706433u, true), 12);
  pins<16, uint32_t>(2013265921u, k31(2013265921u, false), 13);
  pins<16, uint32_t>(1811939329u, k31(1811939329u, true), 14);
  pins<8, uint64_t>(gl64::kP, k64(), 15);

  if (g_bad) {
    fprintf(stderr, "poseidon2_check: %d mismatches\n", g_bad);
    return 1;
  }
  printf("poseidon2_check: ok (%llu cases)\n", (unsigned long long)ncases);
  return 0;
}
