// GPU probe of the radix-2^29 engine's primitives (tests/test_gpu_field29.py): small kernels that run
// ONE primitive of Eng29 (engines.hpp), field29.hpp / field29_asm9.hpp or the register DFTs of
// ntt_kernels_impl.hpp per element and write the raw result limbs (L words per element, not
// canonical words), so the test can check limb bounds as well as values.  The Args constants come from
// eng29_fill_consts (eng29_args.hpp), the function the plans call.  Built by
// tests/field29_probe_build.py into tests/c/libf29probe.so; not part of libntt.
//
// Engines: 0 = Eng29<9,8>, 1 = Eng29<9,12>, 2 = Eng29<14,12>.  Every launcher takes the modulus as
// E::MEMW little-endian words (host pointer), device pointers for the data, n elements (a multiple of
// 64, at most 2^16: one wave per workgroup, every lane active), synchronises and returns the HIP
// status, or a negative number for an argument it refuses.
#define NTT_DEBUG_CHECKS 0
#include <hip/hip_runtime.h>

#include <cstring>

#include "eng29_args.hpp"
#include "ntt_kernels_impl.hpp"

namespace {
using namespace ntt;
using E0 = Eng29<9, 8>;
using E1 = Eng29<9, 12>;
using E2 = Eng29<14, 12>;

template <class E>
typename E::Args make_args(const uint32_t* p_words, const uint32_t* w8) {
  typename E::Args A{};
  eng29_fill_consts<E, E::W, E::MEMW>(A, p_words);
  if (w8)  // w8: 3 x (w[L], ws[L]) limbs
    for (int k = 0; k < 3; ++k)
      for (int i = 0; i < E::W; ++i) {
        A.w8[k].w[i] = w8[(2 * k) * E::W + i];
        A.w8[k].ws[i] = w8[(2 * k + 1) * E::W + i];
      }
  A.dbg = nullptr;
  return A;
}

template <int W>
__device__ __forceinline__ void ld(uint32_t (&x)[W], const uint32_t* s, size_t i) {
#pragma unroll
  for (int j = 0; j < W; ++j) x[j] = s[i * W + j];
}
template <int W>
__device__ __forceinline__ void st(uint32_t* d, size_t i, const uint32_t (&x)[W]) {
#pragma unroll
  for (int j = 0; j < W; ++j) d[i * W + j] = x[j];
}

// ---- products.  tw: per element (w[L], ws[L]) -- or y[L] in its first half for the variable products
enum { PR_MUL = 0, PR_MUL_U = 1, PR_MULC = 2, PR_MULC_CC = 3, PR_MULC_BLK = 4, PR_MULV = 5, PR_MONT = 6, PR_MONT_CHAIN = 7 };
template <class E>
__global__ __launch_bounds__(64) void k_prod(int mode, const uint32_t* x, const uint32_t* tw, const typename E::Tw tu,
                                             uint32_t* out, uint32_t n, const typename E::Args A) {
  constexpr int L = E::W;
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  uint32_t v[L], r[L];
  typename E::Tw t;
  ld<L>(v, x, i);
  ld<L>(t.w, tw, 2 * (size_t)i);
  ld<L>(t.ws, tw, 2 * (size_t)i + 1);
  switch (mode) {
    case PR_MUL: E::mul(v, t, A); break;
    case PR_MUL_U: E::mul_u(v, tu, A); break;
    case PR_MULC: mulc29<L>(r, v, t.w, t.ws, A.pbar); st<L>(out, i, r); return;
    case PR_MULC_CC: mulc29_cc<L>(r, v, t.w, t.ws, A.pbar); st<L>(out, i, r); return;
    case PR_MULC_BLK: mulc29_blk<L>(r, v, t.w, t.ws, A.pbar); st<L>(out, i, r); return;
    case PR_MULV: E::mulv(v, t.w, A); break;
    case PR_MONT: mont29<L>(r, v, t.w, A.M); st<L>(out, i, r); return;
    case PR_MONT_CHAIN: mont29_chain<L>(r, v, t.w, A.M); st<L>(out, i, r); return;
    default: break;
  }
  st<L>(out, i, v);
}

// ---- reductions to raw limbs.  code 0 / 1: reduce_top<true / false>; 2 / 3: cond_sub_rare by p / 2p;
// 100 + k: row k of the table (FROM, TO, FAST, R32) of reduce<> instances the pass kernels make
#define F29_REDUCE_TABLE(X) \
  X(0, 8, 4, false, true) X(1, 16, 4, false, true) X(2, 32, 4, false, true) \
  X(3, 8, 4, true, true) X(4, 16, 4, true, true) X(5, 32, 4, true, true) \
  X(6, 8, 4, true, false) X(7, 16, 4, true, false) X(8, 32, 4, true, false) \
  X(9, 4, 2, true, true) X(10, 4, 2, false, true) X(11, 4, 1, false, true)
template <class E>
__global__ __launch_bounds__(64) void k_red(int code, const uint32_t* x, uint32_t* out, uint32_t n,
                                            const typename E::Args A) {
  constexpr int L = E::W;
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  uint32_t v[L];
  ld<L>(v, x, i);
  switch (code) {
    case 0: E::template reduce_top<true>(v, A); break;
    case 1: E::template reduce_top<false>(v, A); break;
    case 2: E::cond_sub_rare(v, A.kp[0]); break;
    case 3: E::cond_sub_rare(v, A.kp[1]); break;
#define X(K, FROM, TO, FAST, R32)                                             \
  case 100 + K:                                                               \
    if constexpr (!FAST || E::FASTRED) E::template reduce<FROM, TO, FAST, R32>(v, A); \
    break;
      F29_REDUCE_TABLE(X)
#undef X
    default: break;
  }
  st<L>(out, i, v);
}

// ---- reduce + pack to HBM words.  code 0: put; 1 + 2 b + f: store<4 2^b, f> (b = 0..3);
// 9 + f: store_lazy<4, f>
template <class E, int MW>
__global__ __launch_bounds__(64) void k_store(int code, const uint32_t* x, uint32_t* out, uint32_t n,
                                              const typename E::Args A) {
  constexpr int L = E::W;
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  uint32_t v[L];
  ld<L>(v, x, i);
  switch (code) {
    case 0: E::template put<MW>(out, i, v); break;
    case 1: E::template store<4, false, MW>(out, i, v, A); break;
    case 3: E::template store<8, false, MW>(out, i, v, A); break;
    case 5: E::template store<16, false, MW>(out, i, v, A); break;
    case 7: E::template store<32, false, MW>(out, i, v, A); break;
    case 9: E::template store_lazy<4, false, MW>(out, i, v, A); break;
    default:
      if constexpr (E::FASTRED) {
        switch (code) {
          case 2: E::template store<4, true, MW>(out, i, v, A); break;
          case 4: E::template store<8, true, MW>(out, i, v, A); break;
          case 6: E::template store<16, true, MW>(out, i, v, A); break;
          case 8: E::template store<32, true, MW>(out, i, v, A); break;
          case 10: E::template store_lazy<4, true, MW>(out, i, v, A); break;
          default: break;
        }
      }
      break;
  }
}
template <class E, int MW>
__global__ __launch_bounds__(64) void k_load(const uint32_t* words, uint32_t* out, uint32_t n) {
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  uint32_t v[E::W];
  E::template load<MW>(v, words, i);
  st<E::W>(out, i, v);
}

// ---- butterflies and register DFTs: 8 slots of L limbs per element, in and out.
// 0..2: bfly_l<4 / 8 / 16> on slots 0, 1; 3..5: bfly_w_l<4> by w8[0..2]; 6: bfly_w_l<8> by w8[1];
// 10..12: dft_q<2 / 4 / 8>; 20..22: dft_q_fast<2 / 4 / 8>
template <class E>
__global__ __launch_bounds__(64) void k_dft(int code, const uint32_t* x, uint32_t* out, uint32_t n,
                                            const typename E::Args A) {
  constexpr int L = E::W;
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  uint32_t v[8][L];
#pragma unroll
  for (int s = 0; s < 8; ++s) ld<L>(v[s], x, 8 * (size_t)i + s);
  switch (code) {
    case 0: E::template bfly_l<4>(v[0], v[1], A); break;
    case 1: E::template bfly_l<8>(v[0], v[1], A); break;
    case 2: E::template bfly_l<16>(v[0], v[1], A); break;
    case 3: E::template bfly_w_l<4>(v[0], v[1], A.w8[0], A); break;
    case 4: E::template bfly_w_l<4>(v[0], v[1], A.w8[1], A); break;
    case 5: E::template bfly_w_l<4>(v[0], v[1], A.w8[2], A); break;
    case 6: E::template bfly_w_l<8>(v[0], v[1], A.w8[1], A); break;
    case 10: dft_q<E, 2, 0>(v, A); break;
    case 11: dft_q<E, 4, 0>(v, A); break;
    case 12: dft_q<E, 8, 0>(v, A); break;
    default:
      if constexpr (E::FASTRED) {
        if (code == 20) dft_q_fast<E, 2, 0>(v, A);
        else if (code == 21) dft_q_fast<E, 4, 0>(v, A);
        else if (code == 22) dft_q_fast<E, 8, 0>(v, A);
      }
      break;
  }
#pragma unroll
  for (int s = 0; s < 8; ++s) st<L>(out, 8 * (size_t)i + s, v[s]);
}

template <class F>
int with_engine(int eng, F&& f) {
  switch (eng) {
    case 0: return f(E0{});
    case 1: return f(E1{});
    case 2: return f(E2{});
  }
  return -1;
}
bool bad_n(uint32_t n) { return n == 0 || n % 64 != 0 || n > 65536; }
int finish() {
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipDeviceSynchronize();
  return (int)e;
}
}  // namespace

extern "C" {

// words per engine: L, MEMW, SCRW, TABW, FASTRED
int f29_engine_info(int eng, int* out) {
  return with_engine(eng, [&](auto e) {
    using E = decltype(e);
    out[0] = E::W; out[1] = E::MEMW; out[2] = E::SCRW; out[3] = E::TABW; out[4] = E::FASTRED ? 1 : 0;
    return 0;
  });
}

// The constants eng29_fill_consts produced, flattened: M.p[L], M.p2[L], M.pinv, kp[5][L], pbar[L],
// red_inv (its bits), red_ok, pc[5][L]: 13 L + 3 words.
int f29_args(int eng, const uint32_t* p_words, uint32_t* out) {
  return with_engine(eng, [&](auto e) {
    using E = decltype(e);
    constexpr int L = E::W;
    const typename E::Args A = make_args<E>(p_words, nullptr);
    uint32_t* o = out;
    for (int i = 0; i < L; ++i) *o++ = A.M.p[i];
    for (int i = 0; i < L; ++i) *o++ = A.M.p2[i];
    *o++ = A.M.pinv;
    for (int j = 0; j < 5; ++j)
      for (int i = 0; i < L; ++i) *o++ = A.kp[j][i];
    for (int i = 0; i < L; ++i) *o++ = A.pbar[i];
    uint32_t bits;
    memcpy(&bits, &A.red_inv, 4);
    *o++ = bits;
    *o++ = A.red_ok;
    for (int j = 0; j < 5; ++j)
      for (int i = 0; i < L; ++i) *o++ = A.pc[j][i];
    return 0;
  });
}

// x: n x L limbs; tw: n x 2L limbs (device); tu: the wave-uniform twiddle of PR_MUL_U, 2L limbs (host)
int f29_prod(int eng, int mode, const uint32_t* p_words, const uint32_t* x, const uint32_t* tw, const uint32_t* tu,
             uint32_t* out, uint32_t n) {
  if (bad_n(n) || mode < 0 || mode > PR_MONT_CHAIN) return -1;
  return with_engine(eng, [&](auto e) {
    using E = decltype(e);
    const typename E::Args A = make_args<E>(p_words, nullptr);
    typename E::Tw t{};
    for (int i = 0; i < E::W; ++i) {
      t.w[i] = tu[i];
      t.ws[i] = tu[E::W + i];
    }
    hipLaunchKernelGGL(k_prod<E>, dim3(n / 64), dim3(64), 0, 0, mode, x, tw, t, out, n, A);
    return finish();
  });
}

int f29_reduce(int eng, int code, const uint32_t* p_words, const uint32_t* x, uint32_t* out, uint32_t n) {
  if (bad_n(n)) return -1;
  return with_engine(eng, [&](auto e) {
    using E = decltype(e);
    bool known = code >= 0 && code <= 3, fast = code <= 1;
#define X(K, FROM, TO, FAST, R32) \
  if (code == 100 + K) known = true, fast = FAST;
    F29_REDUCE_TABLE(X)
#undef X
    const typename E::Args A = make_args<E>(p_words, nullptr);
    if (!known) return -1;
    if (fast && !(E::FASTRED && A.red_ok)) return -2;  // the quotient estimate needs p_top >= 2^18
    hipLaunchKernelGGL(k_red<E>, dim3(n / 64), dim3(64), 0, 0, code, x, out, n, A);
    return finish();
  });
}

// out: n x mw words
int f29_store(int eng, int mw, int code, const uint32_t* p_words, const uint32_t* x, uint32_t* out, uint32_t n) {
  if (bad_n(n) || code < 0 || code > 10) return -1;
  return with_engine(eng, [&](auto e) {
    using E = decltype(e);
    if (mw != E::MEMW && mw != E::SCRW && mw != E::TABW) return -1;
    const typename E::Args A = make_args<E>(p_words, nullptr);
    const bool fast = code != 0 && code % 2 == 0;
    if (fast && !(E::FASTRED && A.red_ok)) return -2;
    if (mw == E::MEMW)
      hipLaunchKernelGGL((k_store<E, E::MEMW>), dim3(n / 64), dim3(64), 0, 0, code, x, out, n, A);
    else if (mw == E::SCRW)
      hipLaunchKernelGGL((k_store<E, E::SCRW>), dim3(n / 64), dim3(64), 0, 0, code, x, out, n, A);
    else
      hipLaunchKernelGGL((k_store<E, E::TABW>), dim3(n / 64), dim3(64), 0, 0, code, x, out, n, A);
    return finish();
  });
}

// words: n x mw words; out: n x L limbs
int f29_load(int eng, int mw, const uint32_t* words, uint32_t* out, uint32_t n) {
  if (bad_n(n)) return -1;
  return with_engine(eng, [&](auto e) {
    using E = decltype(e);
    if (mw != E::MEMW && mw != E::SCRW && mw != E::TABW) return -1;
    if (mw == E::MEMW)
      hipLaunchKernelGGL((k_load<E, E::MEMW>), dim3(n / 64), dim3(64), 0, 0, words, out, n);
    else if (mw == E::SCRW)
      hipLaunchKernelGGL((k_load<E, E::SCRW>), dim3(n / 64), dim3(64), 0, 0, words, out, n);
    else
      hipLaunchKernelGGL((k_load<E, E::TABW>), dim3(n / 64), dim3(64), 0, 0, words, out, n);
    return finish();
  });
}

// x, out: n x 8 x L limbs; w8: 3 x (w[L], ws[L]) limbs (host)
int f29_dft(int eng, int code, const uint32_t* p_words, const uint32_t* w8, const uint32_t* x, uint32_t* out,
            uint32_t n) {
  if (bad_n(n) || 8 * (size_t)n > 65536) return -1;
  const bool plain = (code >= 0 && code <= 6) || (code >= 10 && code <= 12), fast = code >= 20 && code <= 22;
  if (!plain && !fast) return -1;
  return with_engine(eng, [&](auto e) {
    using E = decltype(e);
    const typename E::Args A = make_args<E>(p_words, w8);
    if (fast && !(E::FASTRED && A.red_ok)) return -2;
    hipLaunchKernelGGL(k_dft<E>, dim3(n / 64), dim3(64), 0, 0, code, x, out, n, A);
    return finish();
  });
}
}
