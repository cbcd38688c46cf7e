// Field engines: how an element lives in registers, LDS, HBM and twiddle tables, and the lazy
// butterfly arithmetic on it.  The NTT kernels are generic over the engine.
//
//   Eng29<L, W32[, SCR]>: radix-2^29 limbs (field29.hpp); HBM holds W32 canonical 32-bit words
//                  (cgbn_mem_t<32*W32>, reference cgbn_cuda.h:51-55).  L = 9 / W32 = 8 is the 256-bit
//                  class (BN254 Fr, BLS12-381 Fr, zero-padded P), L = 14 / W32 = 12 the 384-bit
//                  (6 x 64-bit limb) template.
//   Eng32<1>:      one 32-bit limb, HBM holds the reference's `long long` (P469762049 path).
//   Eng64G:        the Goldilocks field, p = 2^64 - 2^32 + 1, one canonical 64-bit limb (field64.hpp).
//   Eng31:         any odd prime p < 2^31 (BabyBear, KoalaBear) on canonical 4-byte elements (field31.hpp).
#pragma once
#include "field.hpp"
#include "field29.hpp"
#include "field29_asm9.hpp"
#include "field31.hpp"
#include "field64.hpp"

// Debug build (ntt_amd/libntt_debug.so, NTT_DEBUG_CHECKS=1): the pass kernels check every HBM index
// against its buffer, the caller's inputs for canonical form, the lazy bound (< 2p) of every
// intermediate and the canonical form of every output, and record violations in a per-plan status
// word that ntt_plan_device_status reports (bits below).  The product build compiles none of it.
#ifndef NTT_DEBUG_CHECKS
#define NTT_DEBUG_CHECKS 0
#endif
enum : uint32_t {
  NTT_DBG_BOUNDS = 1u << 8,  // an element index outside its buffer (the access is redirected to element 0)
  NTT_DBG_INPUT = 1u << 9,   // a caller input element >= p
  NTT_DBG_LAZY = 1u << 10,   // an intermediate (plan scratch) >= 2p
  NTT_DBG_OUTPUT = 1u << 11  // an output element >= p
};
__device__ __forceinline__ void ntt_dbg_flag(uint32_t* status, uint32_t bit) {
  if (status) __hip_atomic_fetch_or(status, bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
#ifndef NTT_WAVES_256
#define NTT_WAVES_256 4
#endif
// elements per thread in the pass kernels for the 256-bit class (4: radix-4 register sub-stages, 4
// waves/SIMD; 8: radix-8 sub-stages, 2 waves/SIMD)
#ifndef NTT_EPT_256
#define NTT_EPT_256 4
#endif
#ifndef NTT_256_PASS1_TABLE
#define NTT_256_PASS1_TABLE 1
#endif
#ifndef NTT_P_SCRATCH32
#define NTT_P_SCRATCH32 1
#endif
#ifndef NTT_P_NARROW_FIRST
#define NTT_P_NARROW_FIRST 1
#endif
#ifndef NTT_P_PASS1_TABLE
#define NTT_P_PASS1_TABLE 1
#endif
#ifndef NTT_P_LDS_TW
#define NTT_P_LDS_TW 1
#endif
#ifndef NTT_EPT_P
#define NTT_EPT_P 8  // elements per thread of the P path (16: two radix-8 register groups per thread)
#endif
#ifndef NTT_TILE_LOG_P
#define NTT_TILE_LOG_P 13
#endif
#ifndef NTT_MIN_COLS_LOG_P
#define NTT_MIN_COLS_LOG_P 4
#endif
#ifndef NTT_TILE_LOG_256
#define NTT_TILE_LOG_256 10
#endif
// Goldilocks engine (Eng64G): tile, elements per thread, pass-1 outer-twiddle table
#ifndef NTT_TILE_LOG_G
#define NTT_TILE_LOG_G 12
#endif
#ifndef NTT_EPT_G
#define NTT_EPT_G 8
#endif
#ifndef NTT_G_PASS1_TABLE
#define NTT_G_PASS1_TABLE 0
#endif
// 31-bit engine (Eng31): tile, elements per thread, narrowest column group, pass-1 outer-twiddle table
#ifndef NTT_TILE_LOG_31
#define NTT_TILE_LOG_31 13
#endif
#ifndef NTT_EPT_31
#define NTT_EPT_31 8
#endif
#ifndef NTT_MIN_COLS_LOG_31
#define NTT_MIN_COLS_LOG_31 4
#endif
#ifndef NTT_PREF_COLS_LOG_31
#define NTT_PREF_COLS_LOG_31 5
#endif
#ifndef NTT_31_PASS1_TABLE
#define NTT_31_PASS1_TABLE 1
#endif

namespace ntt {

// 16-B write-through vector store (sc1: the line leaves this XCD's L2 at once, so a workgroup on any
// XCD that acquires after the publishing counter reads it fresh; MI355X_MICROARCH.md § visibility,
// the R1 publish form).  The compiler does not count inline-asm stores: the publisher drains them
// with an explicit s_waitcnt vmcnt(0) before it signals.  s_nop 1: the store-data VGPR hazard.
__device__ __forceinline__ void store_wt16(uint4* p, uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
  typedef uint32_t v4u __attribute__((ext_vector_type(4)));
  const v4u v = {a, b, c, d};
  asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(p), "v"(v) : "memory");
}

// ------------------------------------------------------------------------------ 29-bit engine
// Twiddles are multiplied with Shoup's precomputed-quotient product (mulc29): a table entry holds
// the canonical w and ws = floor(w * B / p), B = 2^(29L).  143 MADs per product for L = 9 instead
// of the Montgomery product's 162, measured 14-18 % faster per product on MI355X
// (profiles/r01_mb_mont29_v2.txt).  Element x twiddle products are < 3p for any input < B.
//
// Lazy bounds (units of p): the in-register DFTs take inputs < IN p (IN = 4: products < 3p,
// reduced k = 0 outputs < 4p, HBM loads < p) and radix-2 stage s adds/subtracts with offset
// IN 2^(s-1) p, so a Q-point DFT returns values < IN Q p <= 32p < B for every supported field.
template <int L, int W32, int SCR_ = 0, int TL_ = 0>
struct Eng29 {
  static constexpr int W = L;                   // registers per element
  static constexpr int MEMW = W32;              // 32-bit words per element in HBM (canonical)
  // words per element of the plan's own scratch: 256-bit values (< 2p, p < 2^255) need 8 even in the
  // 48-B caller layout, so only the first read and the last write of a transform move 48 B per
  // element.  SCR_ != 0 forces it (Eng256wI: the caller's 48-B element, for NTT_PLAN_IN_PLACE plans,
  // whose intermediates live in the caller's buffer)
  static constexpr int SCRW = SCR_ ? SCR_ : ((L <= 9 && W32 > 8) ? 8 : W32);
  // words per entry of the element-format twiddle tables (values < p: 8 words for the 256-bit class)
  static constexpr int TABW = (L <= 9) ? 8 : W32;
  static constexpr int TW = (2 * L + 3) & ~3;   // words per twiddle-table entry: w, ws (16-B aligned)
  static constexpr int LDSW = L;                // words per element in LDS
  static constexpr int IN = 4;                  // DFT input bound (units of p)
  static constexpr int MUL_OUT = 4;             // bound used for twiddle products (they are < 3p)
  // Pass-kernel shape.  The products are long dependent v_mad_u64_u32 chains, so a SIMD needs 3-4
  // resident waves to keep its VALU busy (Shoup product: 851 SIMD cycles at 2 waves, 785 at 3-4;
  // profiles/r01_mb_mont29_v2.txt).  256-bit class: 4 elements per thread (radix-4 register
  // sub-stages), 1024-element tiles (36 KiB LDS), 4 workgroups = 4 waves per SIMD.  384-bit class:
  // 8 elements per thread, 1024-element tiles, 2 waves per SIMD.
  static constexpr int EPT = (L <= 9) ? NTT_EPT_256 : 8;
  // TL_ != 0 forces the tile: Eng256T's 4096-element tiles (one 1024-thread workgroup, 144 KiB of
  // LDS, per CU), which run 2^20 in two passes (10 + 10) instead of three (7 + 7 + 6)
  static constexpr int TILE_LOG = TL_ ? TL_ : ((L <= 9) ? (EPT == 8 ? 11 : NTT_TILE_LOG_256) : 10);
  static constexpr int WAVES_PER_EU = (L <= 9) ? (EPT == 4 ? NTT_WAVES_256 : 2) : 2;
  // column passes own >= 4 adjacent columns: >= 128-B runs.  The 4096-element tiles also take one
  // column per tile (radix 4096: 2^24 in two passes, 12 + 12, whose 32-B runs meet their three
  // neighbours on one XCD through the XCD-grouped tile order; ntt_plan.cpp make_wide_plan)
  static constexpr int MIN_COLS_LOG = TL_ == 12 ? 0 : 2;
  static constexpr bool PASS1_FULL_TABLE = NTT_256_PASS1_TABLE;  // VALU-bound: a table read beats a second product
  static constexpr bool NARROW_FIRST = false;  // near-equal radices
  // column passes after the first take their outer twiddles as Shoup pairs (w, ws) from L2-resident
  // tables (E::TW words per entry): 143 MADs per product instead of the Montgomery product's 162
  static constexpr bool SHOUP_OUTER = (L == 9);
  // no LDS twiddle staging: a radix-256 table of Shoup pairs (20 KiB) beside the 36-KiB tile would
  // halve the workgroups per CU
  static constexpr bool LDS_TW = false;
  // mul_u multiplies by a twiddle held in SGPRs (mulc29_a9u), so a sub-stage whose twiddle is the same
  // in every lane of a wave reads its table entries with scalar loads (tload_u); the 384-bit class's
  // mulc29_blk has no such form and keeps the per-lane loads
  static constexpr bool SGPR_TW = (L == 9);
  // quotient-estimate reduction needs p's top limb >= 2^18: possible only when 29L - 18 <= 255
  static constexpr bool FASTRED = 29 * L - 18 <= 255;
  struct Tw {
    uint32_t w[L];   // canonical twiddle
    uint32_t ws[L];  // floor(w * B / p)
  };
  struct Args {
    Mod29<L> M;           // p, 2p, -p^-1 mod 2^29 (Montgomery products of two variables)
    uint32_t kp[5][L];    // 2^j p, j = 0..4, normalised: lazy offsets and reductions
    uint32_t pbar[L];     // B - p (Shoup)
    Tw w8[3];             // w_8^1, w_8^2, w_8^3
    Tw ninv;              // n^-1
    float red_inv;        // 1 / (p_top + 1) rounded down (quotient-estimate reduction)
    uint32_t red_ok;      // p_top >= 2^18: the top-limb quotient estimate is within 1
    uint32_t pc[5][L];    // padded offsets K p for the unnormalised butterflies (PC_* below)
    uint32_t* dbg;        // debug builds: the plan's status word (NTT_DBG_*); null otherwise
  };
  // debug builds: x < q (x any limb representation of a non-negative value, q normalised)
  __device__ static bool dbg_below(const uint32_t (&x)[W], const uint32_t (&q)[L]) {
    uint32_t y[W];
#pragma unroll
    for (int i = 0; i < W; ++i) y[i] = x[i];
    norm_u<L>(y);
    for (int i = L - 1; i >= 0; --i)
      if (y[i] != q[i]) return y[i] < q[i];
    return false;
  }
  __device__ static bool dbg_canonical(const uint32_t (&x)[W], const Args& A) { return dbg_below(x, A.kp[0]); }
  // Padded offsets: value K p, limbs c_0 = kp_0 + P, c_i = kp_i + P - P/2^29 (0 < i < 8),
  // c_8 = kp_8 - P/2^29, so that c_0 >= P and c_i >= P - P/2^29 (with equality where a limb of K p is
  // zero, e.g. p = 2^250 + small) and a - b + C never goes negative limb-wise for b_i <= P - P/2^29:
  // normalised limbs (<= 2^29 - 1) under P = 2^29, sums of two of them (<= 2^30 - 2) under P = 2^30.
  // K = (value bound of b) + 1 keeps the top limb non-negative when p_top >= 3.
  enum : int { PC_5_29 = 0, PC_9_30 = 1, PC_4_29 = 2, PC_17_29 = 3, PC_7_30 = 4 };

  // The 256-bit class in the 48-B layout (W32 = 12) reads only the first 32 B of an element: its
  // values (canonical inputs < p < 2^255, lazy intermediates < 2p) leave words 8..11 zero.  Holding
  // 12 words per element in flight spilled 48 B per thread in pass 1 (12 B with 8 words).  The
  // checked build reads all 48 B, so a non-canonical input still raises its flag.
  template <int MW = W32>
  __device__ static __forceinline__ void load(uint32_t (&x)[W], const uint32_t* __restrict__ base, size_t idx) {
    constexpr int MR = (L <= 9 && MW > 8 && !NTT_DEBUG_CHECKS) ? 8 : MW;
    uint32_t w[MW];
    const uint4* p = reinterpret_cast<const uint4*>(base + idx * MW);
#pragma unroll
    for (int q = 0; q < MW / 4; ++q) {
      if (4 * q < MR) {
        const uint4 v = p[q];
        w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w;
      } else {
        w[4 * q] = w[4 * q + 1] = w[4 * q + 2] = w[4 * q + 3] = 0u;
      }
    }
    pack29<L, MW>(x, w);
  }
  // x < FROM p (power of two) -> x < TO p by conditional subtractions of FROM/2 p, ..., TO p
  template <int FROM, int TO>
  __device__ static __forceinline__ void reduce_chain(uint32_t (&x)[W], const Args& A) {
    static_assert(FROM <= 32 && TO >= 1, "lazy bound");
    if constexpr (FROM > TO) {
      constexpr int j = __builtin_ctz(FROM / 2);
      cond_sub<L>(x, A.kp[j]);
      reduce_chain<FROM / 2, TO>(x, A);
    }
  }
  // x < 64p -> [0, 2p): x - q p with q = floor(x_top / (p_top + 1)) (float estimate biased low by
  // 2^-15, more than its worst rounding overshoot 2^-17.9), which is floor(x / p) or one less when
  // p_top >= 2^18; it is one less only when x / p is within ~2^-14 below an integer, so the result
  // is < p for all but ~2^-14 of inputs.  x - q p = (x + q pbar) mod B.  9 MADs + ~30 simple ops
  // instead of up to four conditional subtractions.
  // The carry stays 32-bit: q <= 64 and pbar_i < 2^29, so every column is < 2^35.2 and its carry
  // c < 2^6.2; x_i + c < 2^32 for the input limbs (< 2^31.6).  Per limb one 32-bit add, one MAD
  // (q pbar_i + (x_i + c)), a mask and one v_alignbit (the carry) -- instead of a 64-bit shift and a
  // 64-bit add of the zero-extended limb, whose register pairs cost the compiler extra moves.
  // R32 = false: the 64-bit-carry form.  The radix-256 column passes took it while the 32-bit form
  // spilled there (3.6 % slower in pass 1); since their wave-uniform sub-stage holds its twiddles in
  // SGPRs the 32-bit form fits without scratch, and every pass takes it (NTT_COL_R32_BELOW).
  template <bool R32 = true>
  __device__ static __forceinline__ void reduce_top(uint32_t (&x)[W], const Args& A) {
    const float qf = __builtin_fmaf((float)x[L - 1], A.red_inv, -0x1p-15f);
    const uint32_t q = qf > 0.f ? (uint32_t)qf : 0u;
    if constexpr (R32) {
    uint32_t c = 0;
#pragma unroll
    for (int i = 0; i < L; ++i) {
      const uint64_t acc = (uint64_t)q * A.pbar[i] + (uint32_t)(x[i] + c);
      x[i] = (uint32_t)acc & kMask29;
      c = (uint32_t)(acc >> 29);
    }
    } else {
    uint64_t acc = 0;
#pragma unroll
    for (int i = 0; i < L; ++i) {
      acc = (acc >> 29) + x[i] + (uint64_t)q * A.pbar[i];
      x[i] = (uint32_t)acc & kMask29;
    }
    }
  }
  // FAST (a kernel template flag, chosen per plan from Args::red_ok): quotient-estimate reduction
  // for the large drops.  A runtime branch here makes the compiler sink the two paths' kp[] uses into
  // one dynamically indexed access and copy the kernel arguments to scratch, hence the template.
  // x < 2q (normalised) -> x < q, skipping the subtraction when no lane of the wave can need it
  // (top limb below q's: x < q for sure).  Wave-uniform branch.
  __device__ static __forceinline__ void cond_sub_rare(uint32_t (&x)[W], const uint32_t (&q)[L]) {
    if (__any(x[L - 1] >= q[L - 1])) cond_sub<L>(x, q);
  }
  template <int FROM, int TO, bool FAST = false, bool R32 = true>
  __device__ static __forceinline__ void reduce(uint32_t (&x)[W], const Args& A) {
    if constexpr (FAST && FROM > 4 && TO <= 4) {
      reduce_top<R32>(x, A);
      if constexpr (TO == 1) cond_sub_rare(x, A.kp[0]);
    } else if constexpr (FAST && FROM == 4 && TO == 2) {
      cond_sub_rare(x, A.kp[1]);  // products: < 1.6p for BN254 Fr, < 2.4p for BLS12-381 Fr
    } else {
      reduce_chain<FROM, TO>(x, A);
    }
  }
  // x < BOUND p -> x < 2p (fits the HBM words: p < 2^255) -> HBM.  Between passes only.
  // WT: write-through stores (the fused single-launch schedule hands the tile to other workgroups)
  template <int BOUND, bool FAST = false, int MW = W32, bool WT = false>
  __device__ static __forceinline__ void store_lazy(uint32_t* __restrict__ base, size_t idx, uint32_t (&x)[W],
                                                    const Args& A) {
    reduce<BOUND, 2, FAST>(x, A);
#if NTT_DEBUG_CHECKS
    if (!dbg_below(x, A.kp[1])) ntt_dbg_flag(A.dbg, NTT_DBG_LAZY);
#endif
    put<MW, WT>(base, idx, x);
  }
  // x < BOUND p -> canonical -> HBM
  template <int BOUND, bool FAST = false, int MW = W32>
  __device__ static __forceinline__ void store(uint32_t* __restrict__ base, size_t idx, uint32_t (&x)[W],
                                               const Args& A) {
    reduce<BOUND, 1, FAST>(x, A);
#if NTT_DEBUG_CHECKS
    if (!dbg_below(x, A.kp[0])) ntt_dbg_flag(A.dbg, NTT_DBG_OUTPUT);
#endif
    put<MW>(base, idx, x);
  }
  template <int MW = W32, bool WT = false>
  __device__ static __forceinline__ void put(uint32_t* __restrict__ base, size_t idx, const uint32_t (&x)[W]) {
    uint32_t w[MW];
    unpack29<L, MW>(w, x);
    uint4* p = reinterpret_cast<uint4*>(base + idx * MW);
#pragma unroll
    for (int q = 0; q < MW / 4; ++q) {
      if constexpr (WT)
        store_wt16(p + q, w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
      else
        p[q] = make_uint4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
    }
  }
  __device__ static __forceinline__ void tload(Tw& t, const uint32_t* __restrict__ tab, size_t idx) {
    const uint4* p = reinterpret_cast<const uint4*>(tab + idx * TW);
#pragma unroll
    for (int q = 0; q < TW / 4; ++q) {
      const uint4 v = p[q];
      const uint32_t vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = 4 * q + r;
        if (i < L) t.w[i] = vv[r];
        else if (i < 2 * L) t.ws[i - L] = vv[r];
      }
    }
  }
  // The entry at an index that is the same in every lane of the wave (formed from a
  // __builtin_amdgcn_readfirstlane value): read through the constant address space, so that the words
  // arrive by scalar loads into SGPRs, where mul_u takes them -- no vector-memory instruction and no
  // VGPR for the pair.  Only for tables that no store of this launch touches (the scalar cache is not
  // coherent with them): the plans' twiddle tables, written by an earlier launch.
  __device__ static __forceinline__ void tload_u(Tw& t, const uint32_t* __restrict__ tab, uint32_t idx) {
    typedef uint32_t V4 __attribute__((ext_vector_type(4)));
    typedef const __attribute__((address_space(4))) V4* CP;
    const CP p = (CP)(tab + (size_t)idx * TW);
#pragma unroll
    for (int q = 0; q < TW / 4; ++q) {
      const V4 v = p[q];
      const uint32_t vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = 4 * q + r;
        if (i < L) t.w[i] = vv[r];
        else if (i < 2 * L) t.ws[i - L] = vv[r];
      }
    }
  }
  // x <- x * w mod p, x any value < B (limbs < 2^31): result < 3p
  __device__ static __forceinline__ void mul(uint32_t (&x)[W], const Tw& t, const Args& A) {
    uint32_t r[W];
    if constexpr (L == 9)
      mulc29_a9(r, x, t.w, t.ws, A.pbar);
    else
      mulc29_blk<L>(r, x, t.w, t.ws, A.pbar);
#pragma unroll
    for (int i = 0; i < W; ++i) x[i] = r[i];
  }
  // the same product by a wave-uniform twiddle (the w_8^k constants of the in-register DFTs): its
  // words stay in SGPRs instead of being copied to VGPRs before every product
  __device__ static __forceinline__ void mul_u(uint32_t (&x)[W], const Tw& t, const Args& A) {
    uint32_t r[W];
    if constexpr (L == 9)
      mulc29_a9u(r, x, t.w, t.ws, A.pbar);
    else
      mulc29_blk<L>(r, x, t.w, t.ws, A.pbar);
#pragma unroll
    for (int i = 0; i < W; ++i) x[i] = r[i];
  }
  // x <- x * y / B mod p (Montgomery product of two variables), x < 32p, y < 4p: result < 3p
  __device__ static __forceinline__ void mulv(uint32_t (&x)[W], const uint32_t (&y)[W], const Args& A) {
    uint32_t r[W];
    if constexpr (L == 9)
      mont29_a9(r, x, y, A.M);
    else
      mont29<L>(r, x, y, A.M);
#pragma unroll
    for (int i = 0; i < W; ++i) x[i] = r[i];
  }
  // ---- lazy DIF butterflies: a, b < K p  ->  (a + b, a - b + K p), both < 2K p, normalised.
  __device__ static __forceinline__ void bfly_lk(uint32_t (&a)[W], uint32_t (&b)[W], const uint32_t (&q)[L]) {
#pragma unroll
    for (int i = 0; i < L; ++i) {
      const uint32_t x = a[i], y = b[i];
      a[i] = x + y;
      b[i] = x - y + q[i];
    }
    norm_u<L>(a);
    norm_s<L>(b);
  }
  template <int K>
  __device__ static __forceinline__ void bfly_l(uint32_t (&a)[W], uint32_t (&b)[W], const Args& A) {
    static_assert(K == 4 || K == 8 || K == 16, "lazy bound");
    bfly_lk(a, b, A.kp[__builtin_ctz(K)]);
  }
  template <int K>
  __device__ static __forceinline__ void bfly_w_l(uint32_t (&a)[W], uint32_t (&b)[W], const Tw& t,
                                                  const Args& A) {
    bfly_l<K>(a, b, A);
    mul_u(b, t, A);  // t: one of the w_8^k kernel arguments
  }
  // ---- unnormalised butterflies (FAST engines; limb/value bounds tracked in dft_q_fast)
  template <int CI>
  __device__ static __forceinline__ void bfly_raw(uint32_t (&a)[W], uint32_t (&b)[W], const Args& A) {
#pragma unroll
    for (int i = 0; i < L; ++i) {
      const uint32_t x = a[i], y = b[i];
      a[i] = x + y;
      b[i] = x - y + A.pc[CI][i];
    }
  }
  template <int CI>
  __device__ static __forceinline__ void bfly_raw_w(uint32_t (&a)[W], uint32_t (&b)[W], const Tw& t,
                                                    const Args& A) {
    bfly_raw<CI>(a, b, A);
    mul_u(b, t, A);  // t: one of the w_8^k kernel arguments
  }
  __device__ static __forceinline__ void norm(uint32_t (&x)[W]) {
    norm_u<L>(x);
  }
};

// ------------------------------------------------------------------------------ 32-bit engine
// One 32-bit limb: the P469762049 `long long` path (MEMW = 2), the reference's own field
// (GZKP-NTT.cu:7-8) and any odd modulus p < 2^30.  Values live in [0, 2p) between operations
// (Harvey's lazy butterflies: 4p < 2^32, so a + b and a - b + 2p never wrap) and are canonical in
// the caller's HBM buffers; the plan scratch holds the lazy value.
//   * twiddle x element: Shoup's product with a table entry (w, floor(w 2^32 / p)):
//     q = mulhi(x, w'), r = x w - q p (mod 2^32) in [0, 2p) for any 32-bit x -- 4 VALU ops
//     (v_mul_hi_u32, 2 x v_mul_lo_u32, v_sub_u32);
//   * variable x variable (outer-twiddle tables in the element format, pointwise products):
//     Montgomery with R = 2^32, r = hi(x y) - hi(m p) + p in (0, 2p) for x y < 2^32 p -- 6 ops;
//   * reduction 2p -> p (and 4p -> 2p): min(x, x - p) as unsigned -- 2 ops, no compare.
// The former CIOS / 64-bit-carry form took 127 VALU ops per element in a radix-256 column pass.
template <int N, int MEMW_, int SCR_ = 0>
struct Eng32 {
  static_assert(N == 1, "the 32-bit engine is the 1-limb path (p < 2^30)");
  static constexpr int W = 1;
  static constexpr int MEMW = MEMW_;
  // 1-limb P path: values < 2^31, so the plan's scratch and tables hold 4 B per element where the
  // caller's `long long` layout holds 8 (HBM-bound path: a third less traffic per transform).
  // SCR_ != 0 forces the scratch width (EngPI: the caller's 8 B, for NTT_PLAN_IN_PLACE)
  static constexpr int SCRW = SCR_ ? SCR_ : (NTT_P_SCRATCH32 ? 1 : MEMW_);
  // element-format twiddle tables (w R mod p < 2^31) take 4 B per entry whatever the scratch width:
  // the in-place plan's pass 1 streams a 2^26-entry table at the SSIP size
  static constexpr int TABW = 1;
  static constexpr int TW = 2;  // Shoup pair (w, floor(w 2^32 / p))
  static constexpr int LDSW = 1;
  static constexpr int IN = 4;       // bound hints of the generic kernels (every value here is < 2p)
  static constexpr int MUL_OUT = 4;
  static constexpr int EPT = NTT_EPT_P;
  // 8192-element tiles (32 KiB LDS, 1024 threads) and >= 16 columns per column-pass workgroup, so
  // every HBM run is >= 128 B; 2048-element tiles left 64-B runs at radix 256 and 32-B runs at
  // radix 512 (2.0-3.3 TB/s).
  static constexpr int TILE_LOG = NTT_TILE_LOG_P;
  static constexpr int MIN_COLS_LOG = NTT_MIN_COLS_LOG_P;
  // pass 1 streams its n-entry outer-twiddle table (4 B per entry: +33 % pass-1 bytes) instead of
  // forming the twiddle from the two-level tables: those are 64 KiB + 64 KiB of Shoup pairs gathered
  // per element, and the shorter arithmetic of this engine made pass 1 wait on them (2^26: 307 ->
  // 237 us with the table, profiles/r03_pab/)
  static constexpr bool PASS1_FULL_TABLE = NTT_P_PASS1_TABLE;
  // pass 1 (columns n / R_1 apart) takes a radix one below the rest: twice as wide runs (2^26: 8+9+9)
  static constexpr bool NARROW_FIRST = NTT_P_NARROW_FIRST;
  static constexpr bool SHOUP_OUTER = false;
  // the parallel-load stage (parallel-load.cu:114-193, re-derived): the pass's w_R^e table (R <= 512
  // Shoup pairs) is staged into LDS while the tile's HBM loads are in flight; sub-stages read their
  // twiddles from LDS instead of issuing L1/L2 loads beside the data stream
  static constexpr bool LDS_TW = NTT_P_LDS_TW;
  static constexpr bool SGPR_TW = false;  // no SGPR-twiddle product
  static constexpr int WAVES_PER_EU = 4;
  static constexpr bool FASTRED = false;
  struct Tw {
    uint32_t w[1];  // canonical w
    uint32_t ws;    // floor(w 2^32 / p)
  };
  struct Args {
    uint32_t p, p2;  // p, 2p
    uint32_t pinv;   // p^-1 mod 2^32 (Montgomery products)
    Tw w8[3];        // w_8^1, w_8^2, w_8^3
    Tw ninv;         // n^-1
    uint32_t* dbg;   // debug builds: the plan's status word (NTT_DBG_*); null otherwise
  };
  __device__ static __forceinline__ uint32_t red(uint32_t x, uint32_t m) {  // x < 2m -> x < m
    return min(x, x - m);
  }
  __device__ static bool dbg_canonical(const uint32_t (&x)[W], const Args& A) { return x[0] < A.p; }
  __device__ static __forceinline__ uint32_t shoup(uint32_t x, uint32_t w, uint32_t ws, uint32_t p) {
    const uint32_t q = __umulhi(x, ws);
    return x * w - q * p;  // [0, 2p)
  }
  template <int MW = MEMW_>
  __device__ static __forceinline__ void load(uint32_t (&x)[W], const uint32_t* __restrict__ base, size_t idx) {
    static_assert(MW == MEMW_ || MW == SCRW || MW == TABW, "HBM width");
    if constexpr (MW == 1)
      x[0] = base[idx];
    else
      x[0] = reinterpret_cast<const uint2*>(base)[idx].x;
  }
  template <int FROM, int TO, bool FAST = false, bool R32 = true>
  __device__ static __forceinline__ void reduce(uint32_t (&)[W], const Args&) {}  // always < 2p
  template <int MW = MEMW_>
  __device__ static __forceinline__ void put(uint32_t* __restrict__ base, size_t idx, uint32_t v) {
    static_assert(MW == MEMW_ || MW == SCRW || MW == TABW, "HBM width");
    if constexpr (MW == 1)
      base[idx] = v;
    else
      reinterpret_cast<uint2*>(base)[idx] = make_uint2(v, 0u);
  }
  // scratch between passes: the lazy value (< 2p < 2^31)
  template <int BOUND, bool FAST = false, int MW = MEMW_, bool WT = false>
  __device__ static __forceinline__ void store_lazy(uint32_t* __restrict__ base, size_t idx, uint32_t (&x)[W],
                                                    [[maybe_unused]] const Args& A) {
    static_assert(!WT, "write-through scratch stores: Eng29 engines only (fused schedule)");
#if NTT_DEBUG_CHECKS
    if (x[0] >= A.p2) ntt_dbg_flag(A.dbg, NTT_DBG_LAZY);
#endif
    put<MW>(base, idx, x[0]);
  }
  // canonical (< p)
  template <int BOUND, bool FAST = false, int MW = MEMW_>
  __device__ static __forceinline__ void store(uint32_t* __restrict__ base, size_t idx, uint32_t (&x)[W],
                                               const Args& A) {
    const uint32_t v = red(x[0], A.p);
#if NTT_DEBUG_CHECKS
    if (v >= A.p) ntt_dbg_flag(A.dbg, NTT_DBG_OUTPUT);
#endif
    put<MW>(base, idx, v);
  }
  __device__ static __forceinline__ void tload(Tw& t, const uint32_t* __restrict__ tab, size_t idx) {
    const uint2 v = reinterpret_cast<const uint2*>(tab)[idx];
    t.w[0] = v.x;
    t.ws = v.y;
  }
  __device__ static __forceinline__ void tload_lds(Tw& t, const uint32_t* lds_tw, uint32_t idx) {
    const uint2 v = reinterpret_cast<const uint2*>(lds_tw)[idx];
    t.w[0] = v.x;
    t.ws = v.y;
  }
  __device__ static __forceinline__ void mul(uint32_t (&x)[W], const Tw& t, const Args& A) {
    x[0] = shoup(x[0], t.w[0], t.ws, A.p);
  }
  __device__ static __forceinline__ void mul_u(uint32_t (&x)[W], const Tw& t, const Args& A) { mul(x, t, A); }
  // x y / 2^32 mod p in (0, 2p) for x y < 2^32 p (x, y < 2p: 4p^2 < 2^32 p)
  __device__ static __forceinline__ void mulv(uint32_t (&x)[W], const uint32_t (&y)[W], const Args& A) {
    const uint32_t lo = x[0] * y[0], hi = __umulhi(x[0], y[0]);
    const uint32_t m = lo * A.pinv;
    x[0] = hi - __umulhi(m, A.p) + A.p;
  }
  // lazy DIF butterfly: a, b < 2p -> (a + b, a - b), both reduced to < 2p
  template <int K>
  __device__ static __forceinline__ void bfly_l(uint32_t (&a)[W], uint32_t (&b)[W], const Args& A) {
    const uint32_t s = a[0] + b[0], d = a[0] - b[0] + A.p2;
    a[0] = red(s, A.p2);
    b[0] = red(d, A.p2);
  }
  template <int K>
  __device__ static __forceinline__ void bfly_w_l(uint32_t (&a)[W], uint32_t (&b)[W], const Tw& t, const Args& A) {
    const uint32_t s = a[0] + b[0], d = a[0] - b[0] + A.p2;  // d < 4p: any 32-bit x is fine for Shoup
    a[0] = red(s, A.p2);
    b[0] = shoup(d, t.w[0], t.ws, A.p);
  }
};

// ------------------------------------------------------------------------------ Goldilocks engine
// p = 2^64 - 2^32 + 1 on 8-byte elements (field64.hpp).  p > 2^63 leaves no room for lazy values in
// 64 bits, so every value is canonical between operations: in registers, LDS, scratch and tables.
// An element is two 32-bit words (low, high) everywhere; a twiddle is the plain canonical value
// (8 B per table entry), and the one product serves twiddles and variables alike (R_e = 1).
//   * add / sub: one 64-bit add or subtract, the carry or borrow paid back with eps = 2^32 - 1;
//   * mul: four v_mad_u64_u32, then lo - hh + hl eps (2^64 = eps, 2^96 = -1): no multiplication in
//     the reduction, ~20 VALU ops per product.
// The lazy bounds of the generic kernels (IN, MUL_OUT, the butterflies' K) are all 1 and `reduce`
// does nothing.
struct Eng64G {
  static constexpr int W = 2;
  static constexpr int MEMW = 2;
  static constexpr int SCRW = 2;
  static constexpr int TABW = 2;
  static constexpr int TW = 2;
  static constexpr int LDSW = 2;  // two 4-B planes: consecutive lanes hit consecutive banks
  static constexpr int IN = 1;
  static constexpr int MUL_OUT = 1;
  static constexpr int EPT = NTT_EPT_G;
  // 4096-element tiles (32 KiB LDS, 512 threads, two or more workgroups per CU) and >= 16 columns per
  // column-pass workgroup: every HBM run is >= 128 B
  static constexpr int TILE_LOG = NTT_TILE_LOG_G;
  static constexpr int MIN_COLS_LOG = 4;
  // pass 1 forms its outer twiddle from the L2-resident two-level tables (one more product per
  // element) instead of streaming an n-entry table of 8-B entries beside the 8-B data
  static constexpr bool PASS1_FULL_TABLE = NTT_G_PASS1_TABLE;
  static constexpr bool NARROW_FIRST = true;  // HBM-bound like the P path: pass 1 reads wider runs
  static constexpr bool SHOUP_OUTER = false;
  static constexpr bool LDS_TW = false;
  static constexpr bool SGPR_TW = false;
  static constexpr int WAVES_PER_EU = 4;
  static constexpr bool FASTRED = false;
  struct Tw {
    uint32_t w[2];  // canonical w (low, high)
  };
  struct Args {
    Tw w8[3];       // w_8^1, w_8^2, w_8^3
    Tw ninv;        // n^-1
    uint32_t* dbg;  // debug builds: the plan's status word (NTT_DBG_*); null otherwise
  };
  __device__ static __forceinline__ uint64_t u64(const uint32_t (&x)[W]) { return ((uint64_t)x[1] << 32) | x[0]; }
  __device__ static __forceinline__ void set(uint32_t (&x)[W], uint64_t v) {
    x[0] = (uint32_t)v;
    x[1] = (uint32_t)(v >> 32);
  }
  __device__ static bool dbg_canonical(const uint32_t (&x)[W], const Args&) { return gl64::is_canonical(u64(x)); }
  template <int MW = MEMW>
  __device__ static __forceinline__ void load(uint32_t (&x)[W], const uint32_t* __restrict__ base, size_t idx) {
    static_assert(MW == 2, "HBM width");
    const uint2 v = reinterpret_cast<const uint2*>(base)[idx];
    x[0] = v.x;
    x[1] = v.y;
  }
  template <int FROM, int TO, bool FAST = false, bool R32 = true>
  __device__ static __forceinline__ void reduce(uint32_t (&)[W], const Args&) {}  // always canonical
  template <int MW = MEMW, bool WT = false>
  __device__ static __forceinline__ void put(uint32_t* __restrict__ base, size_t idx, const uint32_t (&x)[W]) {
    static_assert(MW == 2 && !WT, "HBM width; write-through stores: Eng29 engines only");
    reinterpret_cast<uint2*>(base)[idx] = make_uint2(x[0], x[1]);
  }
  // scratch between passes: canonical like everything else (the "lazy" check of the debug build
  // degenerates to the canonical one)
  template <int BOUND, bool FAST = false, int MW = MEMW, bool WT = false>
  __device__ static __forceinline__ void store_lazy(uint32_t* __restrict__ base, size_t idx, uint32_t (&x)[W],
                                                    [[maybe_unused]] const Args& A) {
#if NTT_DEBUG_CHECKS
    if (!gl64::is_canonical(u64(x))) ntt_dbg_flag(A.dbg, NTT_DBG_LAZY);
#endif
    put<MW, WT>(base, idx, x);
  }
  template <int BOUND, bool FAST = false, int MW = MEMW>
  __device__ static __forceinline__ void store(uint32_t* __restrict__ base, size_t idx, uint32_t (&x)[W],
                                               [[maybe_unused]] const Args& A) {
#if NTT_DEBUG_CHECKS
    if (!gl64::is_canonical(u64(x))) ntt_dbg_flag(A.dbg, NTT_DBG_OUTPUT);
#endif
    put<MW>(base, idx, x);
  }
  __device__ static __forceinline__ void tload(Tw& t, const uint32_t* __restrict__ tab, size_t idx) {
    const uint2 v = reinterpret_cast<const uint2*>(tab)[idx];
    t.w[0] = v.x;
    t.w[1] = v.y;
  }
  __device__ static __forceinline__ void tload_lds(Tw& t, const uint32_t* lds_tw, uint32_t idx) {
    const uint2 v = reinterpret_cast<const uint2*>(lds_tw)[idx];
    t.w[0] = v.x;
    t.w[1] = v.y;
  }
  __device__ static __forceinline__ void mul(uint32_t (&x)[W], const Tw& t, const Args&) {
    set(x, gl64::mul(u64(x), u64(t.w)));
  }
  __device__ static __forceinline__ void mul_u(uint32_t (&x)[W], const Tw& t, const Args& A) { mul(x, t, A); }
  __device__ static __forceinline__ void mulv(uint32_t (&x)[W], const uint32_t (&y)[W], const Args&) {
    set(x, gl64::mul(u64(x), u64(y)));
  }
  // DIF butterfly on canonical values: (a + b, a - b)
  template <int K>
  __device__ static __forceinline__ void bfly_l(uint32_t (&a)[W], uint32_t (&b)[W], const Args&) {
    const uint64_t x = u64(a), y = u64(b);
    set(a, gl64::add(x, y));
    set(b, gl64::sub(x, y));
  }
  template <int K>
  __device__ static __forceinline__ void bfly_w_l(uint32_t (&a)[W], uint32_t (&b)[W], const Tw& t, const Args&) {
    const uint64_t x = u64(a), y = u64(b);
    set(a, gl64::add(x, y));
    set(b, gl64::mul(gl64::sub(x, y), u64(t.w)));
  }
};

// ------------------------------------------------------------------------------ 31-bit engine
// Any odd prime p < 2^31 on 4-byte elements (field31.hpp): BabyBear, KoalaBear, and NTT_PLAN_ELEM32
// custom plans.  2p no longer leaves room for a second lazy value in 32 bits, so every value is
// canonical between operations: in registers, LDS, scratch and tables (IN = MUL_OUT = 1, `reduce`
// does nothing).  One word per element everywhere: the caller's buffers, the scratch, the
// element-format tables (w 2^32 mod p) and LDS; twiddle tables hold Shoup pairs (w, floor(w 2^32 / p)).
//   * add / sub: one add or subtract and one min (v_min_u32 against the value shifted by p);
//   * twiddle product: Shoup's, 4 VALU ops, then one min;
//   * variable product: Montgomery with R = 2^32, 6 ops, then one min;
//   * the twiddled butterfly feeds a - b + p (< 2p: any 32-bit value is a valid Shoup input) to the
//     product unreduced: 2 + 4 + 2 ops for its second output.
// Shape: the P path's (8192-element tiles, 8 elements per thread, 1024 threads, 4 waves per SIMD, the
// pass's w_R^e table staged in LDS, pass 1 a radix narrower).  DESIGN section 7 has the measurements.
struct Eng31 {
  static constexpr int W = 1;
  static constexpr int MEMW = 1;
  static constexpr int SCRW = 1;
  static constexpr int TABW = 1;
  static constexpr int TW = 2;  // Shoup pair (w, floor(w 2^32 / p))
  static constexpr int LDSW = 1;
  static constexpr int IN = 1;
  static constexpr int MUL_OUT = 1;
  static constexpr int EPT = NTT_EPT_31;
  static constexpr int TILE_LOG = NTT_TILE_LOG_31;
  // 2^4 columns of 4 B are 64-B runs; 2^5 (128-B runs) caps the radix at 2^8, which leaves 2^17
  // without a valid radix sequence on 8192-element tiles (r_1 + r_p >= 13 and r_{p-1} + r_p >= 13 need
  // 18 bits in three passes, and two passes stop at 16)
  static constexpr int MIN_COLS_LOG = NTT_MIN_COLS_LOG_31;
  // ... so the kernels are instantiated down to 2^4 columns (radix 2^9) and the planner prefers 2^5
  // (radices <= 2^8) wherever that costs no extra pass: 2^16 runs 8 + 8 instead of 7 + 9 (measured 15 %
  // faster in a batch of 64) and 2^24 8 + 8 + 8 instead of 7 + 8 + 9 (within 2 %);
  // 2^17 and 2^18 keep 8 + 9 and 9 + 9 (ntt_plan.cpp schedule_for)
  static constexpr int PREF_COLS_LOG = NTT_PREF_COLS_LOG_31 > NTT_MIN_COLS_LOG_31 ? NTT_PREF_COLS_LOG_31 : NTT_MIN_COLS_LOG_31;
  static constexpr bool PASS1_FULL_TABLE = NTT_31_PASS1_TABLE;
  static constexpr bool NARROW_FIRST = true;
  static constexpr bool SHOUP_OUTER = false;
  static constexpr bool LDS_TW = true;
  static constexpr bool SGPR_TW = false;
  static constexpr int WAVES_PER_EU = 4;
  static constexpr bool FASTRED = false;
  struct Tw {
    uint32_t w[1];  // canonical w
    uint32_t ws;    // floor(w 2^32 / p)
  };
  struct Args {
    uint32_t p;
    uint32_t pinv;  // p^-1 mod 2^32 (Montgomery products)
    Tw w8[3];       // w_8^1, w_8^2, w_8^3
    Tw ninv;        // n^-1
    uint32_t* dbg;  // debug builds: the plan's status word (NTT_DBG_*); null otherwise
  };
  __device__ static bool dbg_canonical(const uint32_t (&x)[W], const Args& A) { return f31::is_canonical(x[0], A.p); }
  template <int MW = MEMW>
  __device__ static __forceinline__ void load(uint32_t (&x)[W], const uint32_t* __restrict__ base, size_t idx) {
    static_assert(MW == 1, "HBM width");
    x[0] = base[idx];
  }
  template <int FROM, int TO, bool FAST = false, bool R32 = true>
  __device__ static __forceinline__ void reduce(uint32_t (&)[W], const Args&) {}  // always canonical
  // scratch between passes: canonical like everything else (the "lazy" check of the debug build
  // degenerates to the canonical one)
  template <int BOUND, bool FAST = false, int MW = MEMW, bool WT = false>
  __device__ static __forceinline__ void store_lazy(uint32_t* __restrict__ base, size_t idx, uint32_t (&x)[W],
                                                    [[maybe_unused]] const Args& A) {
    static_assert(MW == 1 && !WT, "HBM width; write-through stores: Eng29 engines only");
#if NTT_DEBUG_CHECKS
    if (!f31::is_canonical(x[0], A.p)) ntt_dbg_flag(A.dbg, NTT_DBG_LAZY);
#endif
    base[idx] = x[0];
  }
  template <int BOUND, bool FAST = false, int MW = MEMW>
  __device__ static __forceinline__ void store(uint32_t* __restrict__ base, size_t idx, uint32_t (&x)[W],
                                               [[maybe_unused]] const Args& A) {
    static_assert(MW == 1, "HBM width");
#if NTT_DEBUG_CHECKS
    if (!f31::is_canonical(x[0], A.p)) ntt_dbg_flag(A.dbg, NTT_DBG_OUTPUT);
#endif
    base[idx] = x[0];
  }
  __device__ static __forceinline__ void tload(Tw& t, const uint32_t* __restrict__ tab, size_t idx) {
    const uint2 v = reinterpret_cast<const uint2*>(tab)[idx];
    t.w[0] = v.x;
    t.ws = v.y;
  }
  __device__ static __forceinline__ void tload_lds(Tw& t, const uint32_t* lds_tw, uint32_t idx) {
    const uint2 v = reinterpret_cast<const uint2*>(lds_tw)[idx];
    t.w[0] = v.x;
    t.ws = v.y;
  }
  // any 32-bit x (a caller's non-canonical word included): x w mod p
  __device__ static __forceinline__ void mul(uint32_t (&x)[W], const Tw& t, const Args& A) {
    x[0] = f31::mulc(x[0], t.w[0], t.ws, A.p);
  }
  __device__ static __forceinline__ void mul_u(uint32_t (&x)[W], const Tw& t, const Args& A) { mul(x, t, A); }
  // x y 2^-32 mod p for x y < 2^32 p
  __device__ static __forceinline__ void mulv(uint32_t (&x)[W], const uint32_t (&y)[W], const Args& A) {
    x[0] = f31::mulv(x[0], y[0], A.p, A.pinv);
  }
  // DIF butterfly on canonical values: (a + b, a - b)
  template <int K>
  __device__ static __forceinline__ void bfly_l(uint32_t (&a)[W], uint32_t (&b)[W], const Args& A) {
    const uint32_t x = a[0], y = b[0];
    a[0] = f31::add(x, y, A.p);
    b[0] = f31::sub(x, y, A.p);
  }
  template <int K>
  __device__ static __forceinline__ void bfly_w_l(uint32_t (&a)[W], uint32_t (&b)[W], const Tw& t, const Args& A) {
    const uint32_t x = a[0], y = b[0];
    a[0] = f31::add(x, y, A.p);
    b[0] = f31::mulc(f31::sub_lazy(x, y, A.p), t.w[0], t.ws, A.p);
  }
};

// ------------------------------------------------------------------------------ LDS (any engine)
// An element of LDSW words is split into 16-byte planes ([plane][idx]) plus a 4-byte plane per
// leftover word, so lanes reading consecutive indices hit consecutive slots.  E: elements per plane.
template <int LDSW, int E>
__device__ __forceinline__ void lds_put(uint32_t* lds, uint32_t idx, const uint32_t (&x)[LDSW]) {
  constexpr int Q = LDSW / 4;
  uint4* l4 = reinterpret_cast<uint4*>(lds);
#pragma unroll
  for (int q = 0; q < Q; ++q) l4[q * E + idx] = make_uint4(x[4 * q], x[4 * q + 1], x[4 * q + 2], x[4 * q + 3]);
  uint32_t* l1 = lds + 4 * Q * E;
#pragma unroll
  for (int r = 4 * Q; r < LDSW; ++r) l1[(r - 4 * Q) * E + idx] = x[r];
}
template <int LDSW, int E>
__device__ __forceinline__ void lds_get(uint32_t (&x)[LDSW], const uint32_t* lds, uint32_t idx) {
  constexpr int Q = LDSW / 4;
  const uint4* l4 = reinterpret_cast<const uint4*>(lds);
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const uint4 v = l4[q * E + idx];
    x[4 * q] = v.x; x[4 * q + 1] = v.y; x[4 * q + 2] = v.z; x[4 * q + 3] = v.w;
  }
  const uint32_t* l1 = lds + 4 * Q * E;
#pragma unroll
  for (int r = 4 * Q; r < LDSW; ++r) x[r] = l1[(r - 4 * Q) * E + idx];
}

}  // namespace ntt
