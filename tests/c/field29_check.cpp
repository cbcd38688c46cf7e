// Host driver for ntt_amd/csrc/field29.hpp (the radix-2^29 arithmetic of the Eng29 kernels): runs the
// primitives on records read from a file and writes the raw result limbs; tests/test_field29_host.py
// generates the records and checks the results with exact integer arithmetic (tests/f29_ref.py).
//
//   field29_check <records> <results>
//
// records: a sequence of batches of uint32 words
//   op, L, W32, n, p[L], p2[L], pinv, pbar[L], then n records of the op's operand words
// results: per batch, n records of the op's result words (tables below), in the same order.
// Exit status 0 when every batch was understood; 2 on a malformed file.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "field29.hpp"

enum : uint32_t {
  OP_NORM_U = 1,    // x                -> x
  OP_NORM_S = 2,    // x                -> x, returned top limb
  OP_COND_SUB = 3,  // x, q             -> x
  OP_ADD = 4,       // a, b             -> add29
  OP_SUB_RAW = 5,   // a, b             -> sub29_raw
  OP_SUB = 6,       // a, b             -> sub29
  OP_MONT = 7,      // a, b             -> mont29, mont29_chain
  OP_MULC = 8,      // x, w, ws         -> mulc29, mulc29_cc, mulc29_blk
  OP_MULLO = 9,     // a, b             -> mullo29
  OP_NEG = 10,      // a                -> neg29
  OP_SHOUP_WS = 11, // wR, pinvB        -> shoup_ws29
  OP_INV_B = 12,    // p                -> inv_mod_B29
  OP_PACK = 13,     // w[W32]           -> pack29<L, W32>
  OP_UNPACK = 14    // x                -> unpack29<L, W32>
};

template <int L>
static void get(uint32_t (&x)[L], const uint32_t* s) {
  for (int i = 0; i < L; ++i) x[i] = s[i];
}
template <int L>
static void put(std::vector<uint32_t>& o, const uint32_t (&x)[L]) {
  o.insert(o.end(), x, x + L);
}

// operand / result words per record; 0: unknown op
static bool shape(uint32_t op, uint32_t L, uint32_t W, uint32_t& nin, uint32_t& nout) {
  switch (op) {
    case OP_NORM_U: nin = L; nout = L; return true;
    case OP_NORM_S: nin = L; nout = L + 1; return true;
    case OP_COND_SUB: case OP_ADD: case OP_SUB_RAW: case OP_SUB: case OP_MULLO: case OP_SHOUP_WS:
      nin = 2 * L; nout = L; return true;
    case OP_MONT: nin = 2 * L; nout = 2 * L; return true;
    case OP_MULC: nin = 3 * L; nout = 3 * L; return true;
    case OP_NEG: case OP_INV_B: nin = L; nout = L; return true;
    case OP_PACK: nin = W; nout = L; return true;
    case OP_UNPACK: nin = L; nout = W; return true;
  }
  return false;
}

template <int L, int W>
static void run_pack(uint32_t op, const uint32_t* in, std::vector<uint32_t>& out) {
  if (op == OP_PACK) {
    uint32_t w[W], x[L];
    get<W>(w, in);
    ntt::pack29<L, W>(x, w);
    put<L>(out, x);
  } else {
    uint32_t w[W], x[L];
    get<L>(x, in);
    ntt::unpack29<L, W>(w, x);
    put<W>(out, w);
  }
}

template <int L>
static bool run(uint32_t op, uint32_t W, const ntt::Mod29<L>& M, const uint32_t (&pbar)[L], const uint32_t* in,
                std::vector<uint32_t>& out) {
  uint32_t a[L], b[L], c[L], r[L];
  switch (op) {
    case OP_NORM_U:
      get<L>(a, in);
      ntt::norm_u<L>(a);
      put<L>(out, a);
      return true;
    case OP_NORM_S: {
      get<L>(a, in);
      const int32_t top = ntt::norm_s<L>(a);
      put<L>(out, a);
      out.push_back((uint32_t)top);
      return true;
    }
    case OP_COND_SUB:
      get<L>(a, in);
      get<L>(b, in + L);
      ntt::cond_sub<L>(a, b);
      put<L>(out, a);
      return true;
    case OP_ADD: case OP_SUB_RAW: case OP_SUB:
      get<L>(a, in);
      get<L>(b, in + L);
      if (op == OP_ADD) ntt::add29<L>(r, a, b, M);
      else if (op == OP_SUB_RAW) ntt::sub29_raw<L>(r, a, b, M);
      else ntt::sub29<L>(r, a, b, M);
      put<L>(out, r);
      return true;
    case OP_MONT:
      get<L>(a, in);
      get<L>(b, in + L);
      ntt::mont29<L>(r, a, b, M);
      put<L>(out, r);
      ntt::mont29_chain<L>(r, a, b, M);
      put<L>(out, r);
      return true;
    case OP_MULC:
      get<L>(a, in);
      get<L>(b, in + L);
      get<L>(c, in + 2 * L);
      ntt::mulc29<L>(r, a, b, c, pbar);
      put<L>(out, r);
      ntt::mulc29_cc<L>(r, a, b, c, pbar);
      put<L>(out, r);
      ntt::mulc29_blk<L>(r, a, b, c, pbar);
      put<L>(out, r);
      return true;
    case OP_MULLO:
      get<L>(a, in);
      get<L>(b, in + L);
      ntt::mullo29<L>(r, a, b);
      put<L>(out, r);
      return true;
    case OP_NEG:
      get<L>(a, in);
      ntt::neg29<L>(r, a);
      put<L>(out, r);
      return true;
    case OP_SHOUP_WS:
      get<L>(a, in);
      get<L>(b, in + L);
      ntt::shoup_ws29<L>(r, a, b);
      put<L>(out, r);
      return true;
    case OP_INV_B:
      get<L>(a, in);
      ntt::inv_mod_B29<L>(r, a);
      put<L>(out, r);
      return true;
    case OP_PACK: case OP_UNPACK:
      if (L == 9 && W == 8) run_pack<9, 8>(op, in, out);
      else if (L == 9 && W == 12) run_pack<9, 12>(op, in, out);
      else if (L == 14 && W == 12) run_pack<14, 12>(op, in, out);
      else return false;
      return true;
  }
  return false;
}

template <int L>
static bool batch(uint32_t op, uint32_t W, uint32_t n, uint32_t nin, const uint32_t* consts, const uint32_t* recs,
                  std::vector<uint32_t>& out) {
  ntt::Mod29<L> M;
  uint32_t pbar[L];
  get<L>(M.p, consts);
  get<L>(M.p2, consts + L);
  M.pinv = consts[2 * L];
  get<L>(pbar, consts + 2 * L + 1);
  for (uint32_t j = 0; j < n; ++j)
    if (!run<L>(op, W, M, pbar, recs + (size_t)j * nin, out)) return false;
  return true;
}

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: field29_check <records> <results>\n");
    return 2;
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<uint32_t> in;
  uint32_t buf[1 << 14];
  size_t got;
  while ((got = fread(buf, 4, 1 << 14, f)) > 0) in.insert(in.end(), buf, buf + got);
  fclose(f);
  std::vector<uint32_t> out;
  size_t pos = 0, batches = 0;
  while (pos < in.size()) {
    if (in.size() - pos < 4) return 2;
    const uint32_t op = in[pos], L = in[pos + 1], W = in[pos + 2], n = in[pos + 3];
    uint32_t nin = 0, nout = 0;
    if ((L != 9 && L != 14) || !shape(op, L, W, nin, nout)) return 2;
    const size_t nc = 3 * (size_t)L + 1, need = 4 + nc + (size_t)n * nin;
    if (in.size() - pos < need) return 2;
    const uint32_t* consts = in.data() + pos + 4;
    const uint32_t* recs = consts + nc;
    const bool ok = L == 9 ? batch<9>(op, W, n, nin, consts, recs, out) : batch<14>(op, W, n, nin, consts, recs, out);
    if (!ok) return 2;
    pos += need;
    ++batches;
  }
  f = fopen(argv[2], "wb");
  if (!f) return 2;
  const bool wrote = out.empty() || fwrite(out.data(), 4, out.size(), f) == out.size();
  if (fclose(f) != 0 || !wrote) return 2;
  printf("field29_check: %zu batches, %zu result words\n", batches, out.size());
  return 0;
}
