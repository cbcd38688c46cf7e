// HIP kernels for the MI355X NTT (gfx950), generic over the field engine (engines.hpp).
// See DESIGN.md for the decomposition.
//
// A forward transform of n = 2^L elements is p passes of radix R_i = 2^r_i (sum r_i = L):
//   * passes 1..p-1 ("column passes", KIND_COLUMN): in a block of length N_i the element at
//     c + s_i*d (c < s_i = N_i/R_i, d < R_i) takes part in a length-R_i DFT over d; output k is
//     multiplied by w_{N_i}^{c*k} and stored at c + s_i*k (four-step DIF, in place).  A workgroup
//     owns T = TILE/R_i adjacent columns, so every global access is a T*S-byte contiguous run.
//   * pass p ("final pass", KIND_FINAL): length-R_p DFTs over contiguous runs, written to the
//     digit-reversed (= natural) output position, src -> dst (out of place).  This replaces the
//     reference's SSIP stage-2 mirror-pair trick (GZKP-NTT.cu:1359-1449) with a plan-owned
//     ping-pong buffer: 288 GB of HBM makes an n*S scratch free, and both reads and writes stay
//     fully coalesced.
//   * n <= TILE: one workgroup per transform (KIND_SINGLE).
// Inside a workgroup the R-point DFT is sub-stages of radix 8 (last 2/4/8) in registers with
// LDS exchanges (16-B planes) in between: the wave64 replacement for the reference's shared-memory
// radix-2 rounds (SSIP_NTT_stage1 GZKP-NTT.cu:1297-1357) and its cub::WarpExchange /
// parallel-load staging (test-cub-WarpExchange.cu:6-64, parallel-load.cu:114-193).
// This header: the pass tile, k_pass and its launchers, nothing else.  Every other kernel family has a
// header of its own beside it: the single-launch schedules in ntt_fused_impl.hpp, the row-major matrix
// passes in ntt_mat_impl.hpp, the PRO_LDE launchers in ntt_lde_impl.hpp, the in-place final pass and
// digit reversal in ntt_inplace_impl.hpp, the table builders in ntt_tables_impl.hpp, the rival
// schedules in ntt_rivals_impl.hpp, the element-wise kernels in ntt_elementwise_impl.hpp and the FRI
// fold in ntt_fold_impl.hpp.
#pragma once
#include <cstdlib>
#include <utility>

#include "ntt_kernels.hpp"

namespace ntt {


// Compile-time loop: f(std::integral_constant<int, I>{}) for I in [0, N).  Register arrays indexed
// by I stay in VGPRs (a loop the unroller gives up on would send x[][] to scratch).
template <class F, int... I>
__device__ __forceinline__ void static_for_impl(F&& f, std::integer_sequence<int, I...>) {
  (f(std::integral_constant<int, I>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
  static_for_impl(f, std::make_integer_sequence<int, N>{});
}

// The launchers' radix dispatch: f(std::integral_constant<int, R>{}) for the run-time logr = R in
// [LO, HI], hipErrorInvalidValue outside.  (Host code: static_for above is the device's.)
template <int LO, class F, int... I>
hipError_t with_radix_impl(int logr, F&& f, std::integer_sequence<int, I...>) {
  hipError_t e = hipErrorInvalidValue;
  (void)((logr == LO + I ? (e = f(std::integral_constant<int, LO + I>{}), true) : false) || ...);
  return e;
}
template <int LO, int HI, class F>
hipError_t with_radix(int logr, F&& f) {
  return with_radix_impl<LO>(logr, f, std::make_integer_sequence<int, HI - LO + 1>{});
}

__host__ __device__ constexpr int brev_bits(int v, int bits) {
  int r = 0;
  for (int i = 0; i < bits; ++i) r |= ((v >> i) & 1) << (bits - 1 - i);
  return r;
}

// Sub-stage schedule of one radix-2^LOGR pass: register DFTs of radix 2^QB (QB = log2 of the
// elements per thread), the last one smaller when QB does not divide LOGR.
template <int LOGR, int QB>
struct Sched {
  static constexpr int nsub = (LOGR + QB - 1) / QB;
  static constexpr int qb(int s) { return (LOGR - QB * s) >= QB ? QB : (LOGR - QB * s); }
  static constexpr int logN(int s) { return LOGR - QB * s; }      // log2 N_s
  static constexpr int logsig(int s) { return logN(s) - qb(s); }  // log2 sigma_s
};
template <class E>
constexpr int ept_log() { return E::EPT >= 8 ? 3 : (E::EPT == 4 ? 2 : 1); }  // register DFTs of <= 8 points

// natural index of in-workgroup position pi after all sub-stages (digit reversal)
template <int LOGR, int QB>
__device__ __forceinline__ uint32_t natural_index(uint32_t pi) {
  using S = Sched<LOGR, QB>;
  uint32_t k = 0;
#pragma unroll
  for (int s = 0; s < S::nsub; ++s) {
    const uint32_t ks = (pi >> S::logsig(s)) & ((1u << S::qb(s)) - 1);
    k |= ks << (QB * s);
  }
  return k;
}

// In-register DFT of size Q in {2,4,8} over x[base + d], d < Q (DIF radix-2 network): output X_k
// lands in slot base + brev(k).  Lazy bounds (engines.hpp): inputs < IN p, stage s offsets by
// IN 2^(s-1) p, outputs < IN Q p.
template <class E, int Q, int base, int N>
__device__ __forceinline__ void dft_q(uint32_t (&x)[N][E::W], const typename E::Args& F) {
  constexpr int K1 = E::IN, K2 = 2 * E::IN, K3 = 4 * E::IN;
  if constexpr (Q == 2) {
    E::template bfly_l<K1>(x[base], x[base + 1], F);
  } else if constexpr (Q == 4) {
    E::template bfly_l<K1>(x[base], x[base + 2], F);
    E::template bfly_w_l<K1>(x[base + 1], x[base + 3], F.w8[1], F);
    E::template bfly_l<K2>(x[base], x[base + 1], F);
    E::template bfly_l<K2>(x[base + 2], x[base + 3], F);
  } else {
    static_assert(Q == 8, "radix");
    E::template bfly_l<K1>(x[base], x[base + 4], F);
    E::template bfly_w_l<K1>(x[base + 1], x[base + 5], F.w8[0], F);
    E::template bfly_w_l<K1>(x[base + 2], x[base + 6], F.w8[1], F);
    E::template bfly_w_l<K1>(x[base + 3], x[base + 7], F.w8[2], F);
    E::template bfly_l<K2>(x[base], x[base + 2], F);
    E::template bfly_w_l<K2>(x[base + 1], x[base + 3], F.w8[1], F);
    E::template bfly_l<K2>(x[base + 4], x[base + 6], F);
    E::template bfly_w_l<K2>(x[base + 5], x[base + 7], F.w8[1], F);
    E::template bfly_l<K3>(x[base], x[base + 1], F);
    E::template bfly_l<K3>(x[base + 2], x[base + 3], F);
    E::template bfly_l<K3>(x[base + 4], x[base + 5], F);
    E::template bfly_l<K3>(x[base + 6], x[base + 7], F);
  }
}

// The same DFTs with unnormalised butterflies (FAST Eng29 engines): limbs grow past 29 bits and are
// carry-normalised only where a later stage could overflow 32 bits.  (limb bound, value bound / p)
// per slot, inputs (2^29, 4):
//   Q = 8  stage 1: s (2^30, 8), d (1.5 2^30, 9), d * w -> (2^29, 3)
//          stage 2: x0,x1 (2^31, 16)  x2 (2.5 2^30, 17)  x4 (2^31, 12)  x5 (2^30, 6)  x6 (2.5 2^30, 13)
//          normalise x0 x1 x2 x4 x6; stage 3 outputs <= (2^31, 33)
//   Q = 4  stage 2 outputs <= (2.5 2^30, 17); Q = 2: (1.5 2^30, 9)
// Products accept limbs < 2^31.6 (64-bit column sums) and values < B = 2^261 (33p < 2^260).
template <class E, int Q, int base, int N>
__device__ __forceinline__ void dft_q_fast(uint32_t (&x)[N][E::W], const typename E::Args& F) {
  if constexpr (Q == 2) {
    E::template bfly_raw<E::PC_5_29>(x[base], x[base + 1], F);
  } else if constexpr (Q == 4) {
    E::template bfly_raw<E::PC_5_29>(x[base], x[base + 2], F);
    E::template bfly_raw_w<E::PC_5_29>(x[base + 1], x[base + 3], F.w8[1], F);
    E::template bfly_raw<E::PC_9_30>(x[base], x[base + 1], F);
    E::template bfly_raw<E::PC_4_29>(x[base + 2], x[base + 3], F);
  } else {
    static_assert(Q == 8, "radix");
    E::template bfly_raw<E::PC_5_29>(x[base], x[base + 4], F);
    E::template bfly_raw_w<E::PC_5_29>(x[base + 1], x[base + 5], F.w8[0], F);
    E::template bfly_raw_w<E::PC_5_29>(x[base + 2], x[base + 6], F.w8[1], F);
    E::template bfly_raw_w<E::PC_5_29>(x[base + 3], x[base + 7], F.w8[2], F);
    E::template bfly_raw<E::PC_9_30>(x[base], x[base + 2], F);
    E::template bfly_raw_w<E::PC_9_30>(x[base + 1], x[base + 3], F.w8[1], F);
    E::template bfly_raw<E::PC_4_29>(x[base + 4], x[base + 6], F);
    E::template bfly_raw_w<E::PC_4_29>(x[base + 5], x[base + 7], F.w8[1], F);
    E::norm(x[base]);
    E::norm(x[base + 1]);
    E::norm(x[base + 2]);
    E::norm(x[base + 4]);
    E::norm(x[base + 6]);
    E::template bfly_raw<E::PC_17_29>(x[base], x[base + 1], F);
    E::template bfly_raw<E::PC_4_29>(x[base + 2], x[base + 3], F);
    E::template bfly_raw<E::PC_7_30>(x[base + 4], x[base + 5], F);
    E::template bfly_raw<E::PC_4_29>(x[base + 6], x[base + 7], F);
  }
}
template <class E, int Q, int base, bool FAST, int N>
__device__ __forceinline__ void dft(uint32_t (&x)[N][E::W], const typename E::Args& F) {
  if constexpr (FAST)
    dft_q_fast<E, Q, base>(x, F);
  else
    dft_q<E, Q, base>(x, F);
}

template <class E>
__device__ __forceinline__ void twiddle_mul(uint32_t (&x)[E::W], const uint32_t* tab, uint32_t e,
                                            const typename E::Args& F) {
  typename E::Tw w;
  E::tload(w, tab, e);
  E::mul(x, w, F);
}
// the same from the LDS copy of the table (E::LDS_TW engines: E::TW words per entry)
template <class E>
__device__ __forceinline__ void twiddle_mul_lds(uint32_t (&x)[E::W], const uint32_t* lds_tw, uint32_t e,
                                                const typename E::Args& F) {
  typename E::Tw w;
  E::tload_lds(w, lds_tw, e);
  E::mul(x, w, F);
}

// LDS slot of (local column/block c, in-column position pi): column-minor like HBM, with c XOR-ed
// by the low bits of pi so that both lane orders used (c fastest, or pi fastest) hit distinct
// 16-byte slots (the final pass writes with pi fastest: 8-way conflicts without the swizzle).  A
// swizzle that also removed the wave-uniform sub-stage's read conflicts cost more address VALU than
// the conflicts (+0.8 %).
// One column per tile (T = 1, radix 4096 on 4096-element tiles): consecutive lanes step pi by 1, 4, 16
// or 64, so pi's 16-B slot is XOR-ed by bits 4..7 and 8..11 of pi (tools/lds_t1_sim.py: 0 extra
// cycles per ds_read_b128 and 1.6 per ds_write_b128 against 26 / 22 unswizzled, measured 23).
template <int T>
__device__ __forceinline__ uint32_t lds_slot(uint32_t c, uint32_t pi) {
  if constexpr (T == 1)
    return pi ^ (((pi >> 4) ^ (pi >> 8)) & 15u);
  else
    return (c ^ (pi & (T - 1))) + T * pi;
}

// Wave-uniform trivial twiddles.  Sub-stage s multiplies its outputs k = 1..Q-1 by w^(cp k) with
// cp = g mod sigma_s.  When sigma_s divides the wave count, every cp class is whole waves: wave w
// takes cp = (w + rot) mod sigma_s (rot = the tile index, so that each SIMD -- which holds the same wave
// slot of several workgroups -- gets its share of the cp = 0 waves), and the cp = 0 waves skip their
// products (w^0 = 1) with a scalar branch.  NTT_UNIFORM_CP=0 keeps the lane-order mapping.
#ifndef NTT_UNIFORM_CP
#define NTT_UNIFORM_CP 1
#endif
template <int LOGR, int QB, int NT, int s>
struct Uniform {
  using S = Sched<LOGR, QB>;
  static constexpr int sb = S::logsig(s);
  static constexpr bool on = NTT_UNIFORM_CP && s > 0 && s + 1 < S::nsub && sb >= 1 && (1 << sb) <= NT / 64;
};
// (local column c, group g) of thread t's j-th group in sub-stage s
template <int LOGR, int QB, int T, int NT, int EPT, int s>
__device__ __forceinline__ void sub_map(uint32_t t, int j, uint32_t rot, uint32_t& c, uint32_t& g) {
  using U = Uniform<LOGR, QB, NT, s>;
  if constexpr (U::on) {
    constexpr int sb = U::sb, G = EPT >> Sched<LOGR, QB>::qb(s);
    const uint32_t wave = t >> 6, lane = t & 63;
    const uint32_t cp = (wave + rot) & ((1u << sb) - 1);
    const uint32_t u = ((((wave >> sb) << 6) | lane)) + (uint32_t)(NT >> sb) * (uint32_t)j;
    (void)G;
    c = u % T;
    g = ((u / T) << sb) | cp;
  } else {
    const uint32_t lam = t + NT * j;
    c = lam % T;
    g = lam / T;
  }
}

// One LDS exchange + in-register radix-Q sub-stage s (s >= 1).
template <class E, int LOGR, int T, int TE, int NT, int s, bool FAST, bool R32, bool LTW>
__device__ __forceinline__ void substage(uint32_t (&x)[E::EPT][E::W], uint32_t (&cl)[E::EPT / 2],
                                         uint32_t (&pil)[E::EPT / 2], uint32_t* lds, const PassArgs<E>& A, int t,
                                         const uint32_t* lds_tw, uint32_t rot) {
  using S = Sched<LOGR, ept_log<E>()>;
  constexpr int EPT = E::EPT;
  constexpr int pqb = S::qb(s - 1), PQ = 1 << pqb, PG = EPT / PQ, psb = S::logsig(s - 1), plN = S::logN(s - 1);
  constexpr int qb = S::qb(s), Q = 1 << qb, G = EPT / Q, sb = S::logsig(s), lN = S::logN(s);
  // The exchange stays inside one lambda of its own.  Written straight into this function it is the same
  // program, but the compiler then forms the LDS addresses of the radix-256 tiles of 73 kernels with other
  // instructions (tools/kernel_manifest.py), and a refactor does not change device code.
  static_for<1>([&](auto) {
    if constexpr (s > 1) __syncthreads();  // everyone finished reading the previous round
    static_for<PG>([&](auto J) {
      constexpr int j = J;
      const uint32_t g = pil[j];
      const uint32_t rho = g >> psb, cp = g & ((1u << psb) - 1);
      static_for<PQ>([&](auto K) {
        constexpr int k = K;
        const uint32_t pi = (rho << plN) + cp + (k << psb);
        lds_put<E::LDSW, TE>(lds, lds_slot<T>(cl[j], pi), x[j * PQ + brev_bits(k, pqb)]);
      });
    });
    __syncthreads();
    static_for<G>([&](auto J) {
      constexpr int j = J;
      uint32_t c, g;
      sub_map<LOGR, ept_log<E>(), T, NT, EPT, s>(t, j, rot, c, g);
      const uint32_t rho = g >> sb, cp = g & ((1u << sb) - 1);
      static_for<Q>([&](auto D) {
        constexpr int d = D;
        const uint32_t pi = (rho << lN) + cp + (d << sb);
        lds_get<E::LDSW, TE>(x[j * Q + d], lds, lds_slot<T>(c, pi));
      });
    });
  });
  static_for<G>([&](auto J) {
    constexpr int j = J;
    uint32_t c, g;
    sub_map<LOGR, ept_log<E>(), T, NT, EPT, s>(t, j, rot, c, g);
    cl[j] = c;
    pil[j] = g;
  });
  static_for<G>([&](auto J) {
    constexpr int j = J;
    dft<E, Q, j * Q, FAST>(x, A.F);
    if constexpr (s + 1 < S::nsub) {
      E::template reduce<E::IN * Q, E::IN, FAST, R32>(x[j * Q], A.F);  // k = 0: the only output not multiplied
      const uint32_t cp = pil[j] & ((1u << sb) - 1);
      auto twiddles = [&]() {
        static_for<Q - 1>([&](auto K1) {
          constexpr int k = K1 + 1;
          if constexpr (LTW)
            twiddle_mul_lds<E>(x[j * Q + brev_bits(k, qb)], lds_tw, (cp * k) << (LOGR - lN), A.F);
          else
            twiddle_mul<E>(x[j * Q + brev_bits(k, qb)], A.tw_int, (cp * k) << (LOGR - lN), A.F);
        });
      };
      if constexpr (Uniform<LOGR, ept_log<E>(), NT, s>::on) {
        const uint32_t cps = __builtin_amdgcn_readfirstlane(cp);  // the wave's class, in an SGPR
        if (cps == 0) {  // wave-uniform: w^0 = 1, only bring the bounds down
          static_for<Q - 1>([&](auto K1) {
            E::template reduce<E::IN * Q, E::IN, FAST, R32>(x[j * Q + brev_bits(K1 + 1, qb)], A.F);
          });
        } else if constexpr (E::SGPR_TW && !LTW) {
          // one table entry per wave: scalar address, scalar loads, the pair stays in SGPRs.  One
          // entry at a time: three at once are 54 SGPRs beside pbar, pc and the w_8 words.
          static_for<Q - 1>([&](auto K1) {
            constexpr int k = K1 + 1;
            typename E::Tw w;
            E::tload_u(w, A.tw_int, (cps * k) << (LOGR - lN));
            E::mul_u(x[j * Q + brev_bits(k, qb)], w, A.F);
          });
        } else {
          twiddles();
        }
      } else {
        twiddles();
      }
    }
  });
}

// PRO: load prologue of a fused first column pass (FAST engines with full tables only).
//   PRO_PW:    polynomial multiply.  The pass reads the two forward transforms src and A.src2 and
//              starts from their Montgomery product a b / R_e; R_e is folded into the pass's
//              outer-twiddle table together with n^-1 (PlanImpl::ensure_polymul_table).
//   PRO_COSET: coset forward, x_j <- x_j c^j with j = col + s d: x_j u^d (u = c^s, Shoup table
//              A.tw_in over the in-column index d) and c^col folded into the outer-twiddle table
//              (PlanImpl::coset).
//   PRO_LDE:   low-degree extension (ntt_lde_batch), in the pass that reads the caller's buffer (the
//              first column pass, or KIND_SINGLE).  Transform b's input is the A.src_stride / MEMW
//              coefficients at src + b A.src_stride; a position at or above that length is the
//              engine's zero and is not loaded.  The shift's c^j rides at load: with a full table the
//              PRO_COSET way (u^d here, c^col in the table), else from the two-level tables
//              A.tw_in (lo_s) and A.tw_in_hi as k_scale_pow does (A.tw_in null: no shift), where
//              lde_mul_at_load(); the other passes read inputs that k_lde_scale has scaled.
enum : int { PRO_NONE = 0, PRO_PW = 1, PRO_COSET = 2, PRO_LDE = 3 };
// FSM: four-step addressing (PassArgs::fs) compiled in: 0 = plain batched transforms (every
// product path), 1 = chunk maps / interleave, 2 = the same plus the output twiddle epilogue.
// SHTW: the column pass's full outer-twiddle table holds Shoup pairs (PassArgs::tw_sh).
// Column passes of radix < 2^NTT_COL_R32_BELOW also take the 32-bit-carry reduce_top: -1.0 % on 2^28's
// four radix-128 passes (profiles/r02_uni/col_r32_ab_*.txt).  Radix 256 used to spill with it (28 B, 3.6 %
// slower in pass 1) and stayed on the 64-bit-carry form until the wave-uniform sub-stage took its
// twiddles in SGPRs: with 18 VGPRs fewer live there, every radix-256 column pass compiles to 119-123
// VGPRs and no scratch (16-40 B with the 64-bit form), -1.3 % at 2^24 (profiles/r07_sgpr_tw/).  So 9: all
// the tile's column radices; 8 rebuilds the former split.
#ifndef NTT_COL_R32_BELOW
#define NTT_COL_R32_BELOW 9
#endif
// ---- in-place final pass with the digit reversal fused (NTT_PLAN_IN_PLACE; k_final_ipn, ntt_inplace_impl.hpp).
// The final pass's outputs of slab `mid` belong in slab `midrev` (the palindromic schedule makes the
// digit reversal an involution), so a tile may store only after every tile of slab midrev has READ
// its elements (an anti-dependency: nothing handed-off is loaded, so no acquire is needed).  Reads
// are counted per slab; the slab's last reader raises the slab's ready word.  Slab m's two words live
// on a 128-B line of their own (ipn_sync[32 (1 + m)]), the ticket / exit / watchdog words on line 0.
template <class E>
__device__ __forceinline__ void ipn_signal_read(const PassArgs<E>& A, uint32_t mid) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every wave's loads have returned
  __syncthreads();
  uint32_t* line = A.ipn_sync + 32 * (1 + mid);  // [0] reads done, [1] ready
  if (threadIdx.x == 0 && __hip_atomic_fetch_add(line, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == A.ipn_strips - 1)
    __hip_atomic_store(line + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// A wait gave up (Watchdog, ntt_kernels.hpp): the launch's abort word, then the plan's host-mapped
// report word (system scope: the host reads it at the plan's next call without a device query).
__device__ __forceinline__ void watchdog_trip(const Watchdog& wd) {
  if (wd.abort) __hip_atomic_store(wd.abort, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (wd.report) __hip_atomic_store(wd.report, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
// One lane's bounded poll of `word` with relaxed agent-scope global loads (no read-modify-write
// polls: DESIGN §4), sleeping S0 below N0 polls, S1 below N1, S2 after.  True once the word is
// non-zero; false when the wait gave up: wd.spins polls without it (this lane trips the watchdog) or
// another workgroup of the launch gave up first (its abort word, checked every 256 polls, is set).
template <int S0, uint32_t N0, int S1, uint32_t N1, int S2>
__device__ __forceinline__ bool poll_bounded(uint32_t* word, const Watchdog& wd) {
  typedef __attribute__((address_space(1))) uint32_t gu32;  // a global (not flat) access
  gu32* const g = (gu32*)word;
  gu32* const ab = (gu32*)wd.abort;
  for (uint32_t spins = 0;; ++spins) {
    if (__hip_atomic_load(g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return true;
    if (spins >= wd.spins) {
      watchdog_trip(wd);
      return false;
    }
    if ((spins & 255u) == 255u && ab && __hip_atomic_load(ab, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return false;
    if (spins < N0) __builtin_amdgcn_s_sleep(S0);
    else if (spins < N1) __builtin_amdgcn_s_sleep(S1);
    else __builtin_amdgcn_s_sleep(S2);
  }
}
// True (workgroup-uniform) once slab midrev has been read; false when the wait gave up, and the tile
// must then not store: its outputs would overwrite elements of midrev that are still unread.
template <class E>
__device__ __forceinline__ bool ipn_wait_mirror(const PassArgs<E>& A, uint32_t midrev) {
  __shared__ uint32_t s_ok;
  if (threadIdx.x == 0)
    s_ok = poll_bounded<4, 8, 32, 8, 32>(A.ipn_sync + 32 * (1 + midrev) + 1, A.wd) ? 1u : 0u;
  __syncthreads();
  return __builtin_amdgcn_readfirstlane(s_ok) != 0u;  // wave-uniform: scalar branches around it
}

// Grid-wide barrier k of a launch (k = 1, 2, ...), the guide's R1 publish (MI355X_MICROARCH.md
// § visibility): every wave drains its (write-through) stores, a workgroup barrier, then one lane's
// agent-scope add.  The arrivals are sharded: workgroup b adds to shard b mod 8 (8 counters, each on a
// 128-B line of its own, cumulative: shard s completes barrier k at k n_s arrivals, n_s = its
// workgroups), and the last arrival of each shard adds to the top counter, whose last arrival (k S,
// S = non-empty shards) raises the barrier's go word.  One counter taking all G arrivals serialises
// them (the guide's fan-in: ~12 ns per atomic, ~12 us at G = 1024); eight shards take them in
// parallel.  The sharding is by block index, so it is correct under any placement; under the observed
// round-robin dealing a shard is one XCD.  Then one lane polls the go word (bounded, Watchdog), ONE
// agent-scope acquire, and the workgroup barrier releases every wave.  False (workgroup-uniform) when
// the wait gave up: the workgroup then skips what is left of the launch.
__device__ __forceinline__ bool grid_barrier_words(uint32_t* top, uint32_t* shards, uint32_t* go, uint32_t k,
                                                   const Watchdog& wd) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's stores (and loads) are done
  __syncthreads();
  __shared__ uint32_t s_ok;
  if (threadIdx.x == 0) {
    const uint32_t G = gridDim.x, sh = blockIdx.x & 7u;
    const uint32_t ns = (G + 7u - sh) >> 3, nsh = G < 8u ? G : 8u;
    if (__hip_atomic_fetch_add(shards + 32 * sh, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == k * ns - 1 &&
        __hip_atomic_fetch_add(top, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == k * nsh - 1)
      __hip_atomic_store(go, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_ok = poll_bounded<4, 16, 32, 16, 32>(go, wd) ? 1u : 0u;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  __syncthreads();
  return __builtin_amdgcn_readfirstlane(s_ok) != 0u;
}
// The in-place single launch's last barrier (the K-th of the launch: FUSED3BI_BARRIERS in k_fused3bi,
// FUSED2BI_BARRIERS in k_fused2bi), between every final tile's loads and any store (PassArgs: ipn_sync = the top counter,
// ipn_shards = the shard lines, ipn_go = the go word)
template <uint32_t K, class E>
__device__ __forceinline__ bool ipn_grid_barrier(const PassArgs<E>& A) {
  return grid_barrier_words(A.ipn_sync, A.ipn_shards, A.ipn_go, K, A.wd);
}

// Residency of an in-place single launch (k_fused2bi, k_fused3bi).  Their grid barriers need every
// workgroup resident at once, which a plain launch promises only on a device nobody else holds CUs of
// (another process, or a persistent kernel of the caller's on another stream).  Were a workgroup left
// waiting for a CU, the resident ones would trip the watchdog after pass 1 had already overwritten the
// caller's buffer.  So every workgroup arrives at kernel start (grid barrier 1 of the launch, no wait),
// and before its FIRST store waits until all G have arrived.  The go word is decided once, by
// compare-exchange: the last arrival sets it 0 -> 1 (go), a waiter whose bounded poll ran out sets it
// 0 -> 2 (abandon: no workgroup of the launch stores anything, the caller's buffer is unchanged, and
// the call is reported through the watchdog as NTT_ERR_DEVICE).  Arriving costs one atomic per
// workgroup; the wait is normally satisfied at its first poll, a whole pass-1 tile after the last
// workgroup started.
__device__ __forceinline__ void residency_arrive(uint32_t* top, uint32_t* shards, uint32_t* go) {
  if (threadIdx.x == 0) {
    const uint32_t G = gridDim.x, sh = blockIdx.x & 7u;
    const uint32_t ns = (G + 7u - sh) >> 3, nsh = G < 8u ? G : 8u;
    if (__hip_atomic_fetch_add(shards + 32 * sh, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == ns - 1 &&
        __hip_atomic_fetch_add(top, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == nsh - 1) {
      uint32_t zero = 0u;
      __hip_atomic_compare_exchange_strong(go, &zero, 1u, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}
// True (workgroup-uniform) when the launch's go word says go; false when it was abandoned.
__device__ __forceinline__ bool residency_wait(uint32_t* go, const Watchdog& wd) {
  __shared__ uint32_t s_go;
  if (threadIdx.x == 0) {
    typedef __attribute__((address_space(1))) uint32_t gu32;
    uint32_t v = 0;
    for (uint32_t spins = 0;; ++spins) {
      v = __hip_atomic_load((gu32*)go, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (v) break;
      if (spins >= wd.spins) {
        uint32_t cur = 0u;
        if (__hip_atomic_compare_exchange_strong(go, &cur, 2u, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT)) {
          watchdog_trip(wd);
          v = 2u;
        } else {
          v = cur;  // decided meanwhile
        }
        break;
      }
      if (spins < 16) __builtin_amdgcn_s_sleep(4);
      else __builtin_amdgcn_s_sleep(32);
    }
    s_go = v;
  }
  __syncthreads();
  return __builtin_amdgcn_readfirstlane(s_go) == 1u;
}
// Once a workgroup has passed its residency_wait the go word is final (1 or 2) until the launch's
// last workgroup out clears it: the kernel reads the decision there.
__device__ __forceinline__ bool residency_went(uint32_t* go) {
  __shared__ uint32_t s_go;
  if (threadIdx.x == 0) s_go = __hip_atomic_load(go, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __syncthreads();
  return __builtin_amdgcn_readfirstlane(s_go) == 1u;
}

// LDS of one pass tile (words), and whether the pass stages its w_R^e table in LDS: E::LDS_TW
// (parallel-load stage), not in a first pass with two-level outer twiddles (the P path's pass 1),
// where it measured slower (profiles/r02_ldstw/)
template <class E, int LOGR, int KIND>
__host__ __device__ constexpr int pass_tile_te() {
  return (KIND == KIND_SINGLE) ? (1 << LOGR) : (1 << tile_log_of<E>());  // KIND_ROWS: TILE / 2^LOGR transforms
}
template <class E, int LOGR, int KIND>
__host__ __device__ constexpr int pass_lds_words() {
  return pass_tile_te<E, LOGR, KIND>() * E::LDSW;
}
template <class E, int KIND, bool FULLTW>
__host__ __device__ constexpr bool pass_ltw() {
  return E::LDS_TW && !(KIND == KIND_COLUMN && !FULLTW);
}

// One workgroup tile of one pass: tile w (the workgroup index of a k_pass launch) of transform bq
// (its blockIdx.y).  lds: pass_lds_words() words, lds_tw: 2^LOGR E::TW words when pass_ltw().  k_pass runs
// one tile per workgroup; the fused single-launch schedule (k_fused3, ntt_fused_impl.hpp) runs several
// passes' tiles in one persistent workgroup.
// LOOPED (persistent workgroups, k_fused3): the thread index is re-read per tile through an opaque
// copy, so that the compiler does not hoist every lane-dependent address out of the tile loop (held in
// VGPRs across the whole loop, they spilled 200-380 B per thread; per tile they cost a few VALU ops).
// IPN (final pass of an in-place plan): outputs go to their natural positions in the same buffer.
// IPN_SLAB (k_final_ipn): a tile's loads are counted in per slab, and its stores wait until the mirror
// slab has been read.  IPN_FUSED3 / IPN_FUSED2 (k_fused3bi / k_fused2bi, every final tile resident):
// a grid barrier, the launch's last, between all loads and all stores.  IPN_RESIDENCY (pass 1 of
// k_fused3bi / k_fused2bi): the stores wait for the launch's residency decision (residency_wait) and
// are skipped when it was abandoned.
// MAT (k_pass_mat in ntt_mat_impl.hpp, the ntt_*_matrix calls): the strip form.  The tile is Mode I with il = A.il on strip
// bq of a row-major [n][A.mat_w] matrix: (TILE >> il) transform positions by 2^il adjacent columns, the
// interleaved index P = row 2^il + bl standing for element (row, bq 2^il + bl) at row A.mat_w + that
// column -- a multiply where Mode I shifts.  Twiddle indices depend on the row alone.  Columns at and
// past A.mat_w (the last strip of a row) do not exist: their lanes load nothing, carry zeros through
// the tile and store nothing.
enum : int { IPN_NONE = 0, IPN_SLAB = 1, IPN_FUSED3 = 2, IPN_FUSED2 = 3, IPN_RESIDENCY = 4 };
// Names for pass_tile's options, in the order of its template parameters: no call site passes a bare
// true / false / 0.  (They stay positional values of the types below.  Gathering them into one options
// type, or calling through a wrapper that takes one, changed the register allocation of 29-bit-engine
// kernels -- tools/kernel_manifest.py -- and was taken out again.)
constexpr bool TW_FULL = true, TW_TWO_LEVEL = false;    // FULLTW: a full outer-twiddle table / the two-level tables
constexpr bool RED_FAST = true, RED_GENERIC = false;    // FAST: unnormalised butterflies and fast reductions
constexpr bool SRC_CALLER = true, SRC_SCRATCH = false;  // SRC_USER: a column pass's source layout
enum : int { FSM_NONE = 0, FSM_MAPS = 1, FSM_EPILOGUE = 2 };  // FSM
constexpr bool OUTER_SHOUP = true, OUTER_MONT = false;  // SHTW: the full table holds Shoup pairs / w R_e
constexpr bool STORE_WT = true, STORE_PLAIN = false;    // WT: write-through stores (read by another workgroup)
constexpr bool TILE_LOOPED = true, TILE_ONCE = false;   // LOOPED: several tiles per workgroup
constexpr bool STRIP_FORM = true;                       // MAT
template <class E, int LOGR, int KIND, bool FULLTW, bool FAST, int PRO = PRO_NONE, bool SRC_USER = true,
          int FSM = 0, bool SHTW = false, bool WT = false, bool LOOPED = false, int IPN = 0, bool MAT = false>
__device__ __forceinline__ void pass_tile(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst,
                                          const PassArgs<E>& A, const uint32_t w, const uint32_t bq,
                                          uint32_t* __restrict__ lds, uint32_t* __restrict__ lds_tw) {
  static_assert(!SHTW || (FULLTW && KIND == KIND_COLUMN), "Shoup pairs: a column pass's full table");
  static_assert(!WT || KIND == KIND_COLUMN, "write-through stores: scratch");
  static_assert(IPN == IPN_NONE || (IPN == IPN_RESIDENCY ? KIND == KIND_COLUMN && WT : KIND == KIND_FINAL), "IPN forms");
  constexpr int QB = ept_log<E>(), EPT = E::EPT;
  using S = Sched<LOGR, QB>;
  constexpr bool COLLIKE = KIND == KIND_COLUMN || KIND == KIND_STOCKHAM || KIND == KIND_DIT;  // column groups
  constexpr bool ROWS = KIND == KIND_ROWS;  // T whole transforms per workgroup: transform w T + c
  constexpr int TE = pass_tile_te<E, LOGR, KIND>();
  constexpr int T = TE >> LOGR;  // columns (column pass) or blocks (final / single) per workgroup
  // reduce_top form (engines.hpp): radix-256 column passes are at the VGPR cap and keep the 64-bit one
  constexpr bool R32 = KIND != KIND_COLUMN || LOGR < NTT_COL_R32_BELOW;
  constexpr int NT = TE / EPT;   // threads
  static_assert(LOGR >= QB && T >= 1, "radix");
  constexpr bool LTW = pass_ltw<E, KIND, FULLTW>();

  // HBM words per element: the caller's buffers hold E::MEMW, the plan's scratch and outer-twiddle
  // tables E::SCRW (8 for 256-bit values in the 48-B layout).  Column passes read the caller's
  // buffer (pass 1, SRC_USER) or scratch and write scratch; the final pass reads scratch.
  // (Stockham passes ping-pong between caller-format buffers: E::MEMW words both ways)
  constexpr int SW = (KIND == KIND_COLUMN) ? (SRC_USER ? E::MEMW : E::SCRW) : (KIND == KIND_FINAL ? E::SCRW : E::MEMW);
  constexpr int DW = (KIND == KIND_COLUMN) ? E::SCRW : E::MEMW;

  int t = threadIdx.x;
  if constexpr (LOOPED) asm volatile("" : "+v"(t));
  if (t >= NT) return;
  // Four-step addressing (PassArgs::fs, ntt_rplan_*): the first pass may read and the last pass may
  // write through the per-peer chunk maps, and Mode I runs 2^il interleaved transforms.  All flags
  // are kernel arguments (wave-uniform branches); fs == 0 is the plain batched transform.
  constexpr bool IN_USER = (KIND == KIND_COLUMN && SRC_USER) || KIND == KIND_SINGLE || ROWS;
  constexpr bool EPI = FSM == 2 && KIND != KIND_COLUMN;
  static_assert(!MAT || ((KIND == KIND_COLUMN || KIND == KIND_FINAL) && FSM == 1 && !FULLTW && IPN == 0), "strip form");
  const bool fs_il = MAT || (FSM > 0 && (A.fs & FS_IL) != 0);
  const bool map_in = !MAT && FSM > 0 && IN_USER && (A.fs & FS_MAP_IN);
  const bool map_out = !MAT && FSM > 0 && KIND != KIND_COLUMN && (A.fs & FS_MAP_OUT);
  // one interleaved transform per workgroup (KIND_ROWS: T adjacent ones, runs of T elements)
  const bool single_il = (KIND == KIND_SINGLE || ROWS) && fs_il;
  const size_t tstride = A.batch_stride / E::MEMW;  // elements between batched transforms
  const size_t bidx = MAT ? 0 : (size_t)bq * tstride;  // first element of this transform (KIND_ROWS: bq = 0; MAT: bq is the strip)
  if constexpr (MAT) {}
  else if constexpr (PRO == PRO_LDE) src += (size_t)bq * A.src_stride;  // the inputs are shorter than the outputs
  else if (!map_in && !single_il) src += bidx * SW;
  if (!map_out && !single_il) dst += bidx * DW;
  const size_t boff = bidx * E::MEMW;  // caller-buffer words (src2)
  // input element `pos` of transform b (= bq, or w T + c in KIND_ROWS; Mode I column passes: the
  // interleaved linear index)
  auto in_pos = [&](size_t pos, size_t b) -> size_t {
    if (single_il) pos = (pos << A.il) + b;
    else if (ROWS && !map_in) pos += b * tstride;
    if (!map_in) return pos;
    return A.min(pos, fs_il ? 0 : b);
  };
  // output element (pre-map position as above) -> address; epilogue-table index of the same element
  auto out_pos = [&](size_t pos, size_t b) -> size_t {
    if (single_il) pos = (pos << A.il) + b;
    else if (ROWS && !map_out) pos += b * tstride;
    if (!map_out) return pos;
    return A.mout(pos, fs_il ? 0 : b);
  };
  auto epi_idx = [&](size_t pos, size_t b) -> size_t {
    if (!fs_il) return (b << A.log_n) + pos;
    if (single_il) pos = (pos << A.il) + b;
    return (A.fs & FS_MAP_EPI) ? A.mepi(pos, 0) : pos;
  };
  // MAT: the address of interleaved index P of this strip; false: the column does not exist.  rev (the
  // load of the first pass, the store of the last: MAT_REV_IN / MAT_REV_OUT): the row is stored at its
  // log_n-bit reversal -- another row, the same run of columns within it
  auto mat_at = [&](size_t P, size_t& at, bool rev = false) -> bool {
    const uint32_t col = (bq << A.il) + (uint32_t)(P & ((1u << A.il) - 1));
    uint32_t row = (uint32_t)(P >> A.il);
    if (rev) row = __builtin_bitreverse32(row) >> (32 - A.log_n);  // log_n >= 3 in a pass
    at = (size_t)row * A.mat_w + col;
    return col < A.mat_w;
  };
  // MAT_MUL_OUT: natural output row j times c^-j, the two-level product of the load side (PRO_LDE)
  auto mat_mul_out = [&]([[maybe_unused]] uint32_t (&v)[E::W], [[maybe_unused]] uint32_t row) {
    if constexpr (MAT) {
      typename E::Tw tl, th;
      E::tload(tl, A.tw_in, row & ((1u << A.lo_bits) - 1));
      E::tload(th, A.tw_in_hi, row >> A.lo_bits);
      E::mul(tl.w, th, A.F);
      E::mulv(v, tl.w, A.F);
    }
  };
  // debug builds: an index outside its buffer is recorded and redirected to element 0
  auto ck = [&](size_t i, [[maybe_unused]] size_t lim) -> size_t {
#if NTT_DEBUG_CHECKS
    if (i >= lim) {
      ntt_dbg_flag(A.F.dbg, NTT_DBG_BOUNDS);
      return 0;
    }
#endif
    return i;
  };

  // ------------------------------------------------------------------ workgroup geometry
  size_t colbase = 0;  // column pass: first element of this WG's column group
  uint32_t col0 = 0;   // column pass: column index (within block) of local column 0
  uint32_t mid = 0, k10 = 0, midrev = 0;  // final pass
  uint32_t b0 = 0, tb_log = 0;            // final pass, Mode I: first transform, log2 transforms per WG
  if constexpr (COLLIKE) {
    const uint32_t log_s = A.log_blk - LOGR;
    const uint32_t groups_log = log_s - __builtin_ctz(T);  // column groups per block (log)
    const size_t blk = w >> groups_log;
    col0 = (w & ((1u << groups_log) - 1)) * T;
    colbase = (blk << A.log_blk) + col0;
  } else if constexpr (KIND == KIND_FINAL) {
    const uint32_t w1_log = A.log_n - A.r1 - LOGR;  // W1 = n / (R_1 R_p)
    mid = w & ((1u << w1_log) - 1);
    if (fs_il) {
      // T = (adjacent transforms) x (adjacent k_1 values): as many transforms as the interleave has
      constexpr uint32_t tl = __builtin_ctz(T);
      tb_log = tl < A.il ? tl : A.il;
      const uint32_t tk_log = tl - tb_log;
      const uint32_t rest = w >> w1_log;
      k10 = (rest & ((1u << (A.r1 - tk_log)) - 1)) << tk_log;
      b0 = (rest >> (A.r1 - tk_log)) << tb_log;
    } else {
      k10 = (w >> w1_log) * T;
    }
    uint32_t m = mid;
    for (uint32_t i = 0; i < A.nmid; ++i) {
      const uint32_t d = m & ((1u << A.mid_bits[i]) - 1);
      m >>= A.mid_bits[i];
      midrev |= d << A.mid_off[i];
    }
  }
  const uint32_t log_s = COLLIKE ? (A.log_blk - LOGR) : 0u;

  uint32_t x[EPT][E::W];
  uint32_t cl[EPT / 2];   // local column/block of each group (<= EPT/2 groups per thread)
  uint32_t pil[EPT / 2];  // group index of each group

  // ------------------------------------------------------------------ sub-stage 0: global -> regs
  // E::LDS_TW: this pass's w_R^e words, loaded ahead of the tile (L2 hits) and stored to LDS after
  // sub-stage 0 (which still multiplies from the global table)
  constexpr int TWWORDS = LTW ? (1 << LOGR) * E::TW : 1;  // the staged table, E::TW words per entry
  uint32_t stw[LTW ? (TWWORDS + NT - 1) / NT : 1];
  if constexpr (LTW && S::nsub > 1) {
    static_for<(TWWORDS + NT - 1) / NT>([&](auto I) {
      constexpr int i = I;
      stw[i] = (t + NT * i < TWWORDS) ? A.tw_int[t + NT * i] : 0u;
    });
  }
  {
    constexpr int qb = S::qb(0), Q = 1 << qb, G = EPT / Q, sb = S::logsig(0);
    static_for<G>([&](auto J) {
      constexpr int j = J;
      const uint32_t lam = t + NT * j;
      uint32_t c, g;
      if constexpr (COLLIKE) {
        c = lam % T;
        g = lam / T;
      } else {
        g = lam & ((1u << sb) - 1);
        c = lam >> sb;
      }
      cl[j] = c;
      pil[j] = g;
      static_for<Q>([&](auto D) {
        constexpr int d = D;
        const uint32_t pi = g + (d << sb);
        size_t pos;
        if constexpr (COLLIKE) {
          pos = colbase + c + ((size_t)pi << log_s);
        } else if constexpr (KIND == KIND_FINAL) {
          if (fs_il) {
            const uint32_t k1 = k10 + (c >> tb_log), b = b0 + (c & ((1u << tb_log) - 1));
            const size_t beta = ((size_t)k1 << (A.log_n - A.r1 - LOGR)) + mid;
            pos = (((beta << LOGR) + pi) << A.il) + b;
          } else {
            const size_t beta = ((size_t)(k10 + c) << (A.log_n - A.r1 - LOGR)) + mid;
            pos = (beta << LOGR) + pi;
          }
        } else {
          pos = pi;
        }
        const size_t b = ROWS ? (size_t)w * T + c : (size_t)bq;  // this element's transform
        if constexpr (PRO == PRO_LDE) {
          static_assert((FSM == 0 || MAT) && SRC_USER && (KIND == KIND_SINGLE || KIND == KIND_COLUMN), "PRO_LDE passes");
          // pos is the position in the transform (pass 1 has one block; MAT: row 2^il + bl, the input
          // being the matrix's first rows).  Zeros past the input's end come from registers; a tile with
          // no input at all still runs and stores its zeros over whatever the scratch or the caller's
          // buffer held.
          size_t at = pos;
          bool have = true;
          if constexpr (MAT) {
            have = mat_at(pos, at);
            pos >>= A.il;  // the row: c^row below
          }
          if (have && pos < A.src_stride / E::MEMW) {
            E::template load<SW>(x[j * Q + d], src, ck(at, A.dbg_src_n));
#if NTT_DEBUG_CHECKS
            if (!E::dbg_canonical(x[j * Q + d], A.F)) ntt_dbg_flag(A.F.dbg, NTT_DBG_INPUT);
#endif
            if constexpr (KIND == KIND_COLUMN && FULLTW) {
              if (A.tw_in) {  // c^pos = c^col (outer table) u^pi; null: no shift, the plan's own table
                typename E::Tw u;
                E::tload(u, A.tw_in, pi);
                E::mul(x[j * Q + d], u, A.F);  // < 3p, normalised
              }
            } else if constexpr (lde_mul_at_load<E, KIND>()) {
              if (A.tw_in) {  // c^pos = lo_s[pos mod 2^lo_bits] hi[pos >> lo_bits]
                typename E::Tw tl, th;
                E::tload(tl, A.tw_in, (uint32_t)(pos & ((1u << A.lo_bits) - 1)));
                E::tload(th, A.tw_in_hi, (uint32_t)(pos >> A.lo_bits));
                E::mul(tl.w, th, A.F);
                E::mulv(x[j * Q + d], tl.w, A.F);
              }
            }
          } else {
#pragma unroll
            for (int l = 0; l < E::W; ++l) x[j * Q + d][l] = 0u;
          }
        } else if constexpr (MAT) {
          size_t at;
          if (mat_at(pos, at, KIND == KIND_COLUMN && (A.mat_ops & MAT_REV_IN))) {
            E::template load<SW>(x[j * Q + d], src, ck(at, A.dbg_src_n));
#if NTT_DEBUG_CHECKS
            if (KIND == KIND_COLUMN && A.src_user) {
              if (!E::dbg_canonical(x[j * Q + d], A.F)) ntt_dbg_flag(A.F.dbg, NTT_DBG_INPUT);
            }
#endif
          } else {
#pragma unroll
            for (int l = 0; l < E::W; ++l) x[j * Q + d][l] = 0u;
          }
        } else {
          E::template load<SW>(x[j * Q + d], src, ck(IN_USER ? in_pos(pos, b) : pos, A.dbg_src_n));
#if NTT_DEBUG_CHECKS
          // the caller's elements must be canonical (the reference's BAD LIMB trap); a column pass reads
          // them only when A.src_user (one SRC_USER instance also serves later passes when the scratch
          // and caller layouts agree)
          if (KIND == KIND_SINGLE || ROWS || (KIND == KIND_COLUMN && A.src_user)) {
            if (!E::dbg_canonical(x[j * Q + d], A.F)) ntt_dbg_flag(A.F.dbg, NTT_DBG_INPUT);
          }
#endif
        }
        if constexpr ((KIND == KIND_STOCKHAM || KIND == KIND_DIT) && FULLTW) {
          // bellperson's input twiddle (GZKP-NTT.cu:348-354): element pi of group k = index mod p is
          // multiplied by w_n^((n >> lgp >> deg) k pi), from a [k / T][pi][k mod T] table (p >= T).
          // KIND_DIT (GZKP(B, G), in place after the bit reversal): column c < s = 2^lgp of a block of
          // N = s R, input d multiplied by w_N^(c d) -- the same table shape with k = c
          uint32_t tw[E::W];
          const uint32_t k0 = col0 & ((1u << A.lgp) - 1);
          E::template load<E::TABW>(tw, A.tw_full, ((size_t)k0 << LOGR) + pi * T + c);
          E::mulv(x[j * Q + d], tw, A.F);
        }
        if constexpr (PRO == PRO_PW) {
          uint32_t y[E::W];
          E::load(y, A.src2 + boff, in_pos(pos, b));  // src2 has src's layout (a four-step piece: mapped)
          E::mulv(x[j * Q + d], y, A.F);  // canonical inputs: < 3p, normalised
        } else if constexpr (PRO == PRO_COSET) {
          typename E::Tw u;
          E::tload(u, A.tw_in, pi);
          E::mul(x[j * Q + d], u, A.F);  // < 3p, normalised
        }
      });
    });
    static_for<G>([&](auto J) {
      constexpr int j = J;
      dft<E, Q, j * Q, FAST>(x, A.F);
      if constexpr (S::nsub > 1) {
        E::template reduce<E::IN * Q, E::IN, FAST, R32>(x[j * Q], A.F);  // k = 0: the only output not multiplied
        static_for<Q - 1>([&](auto K1) {
          constexpr int k = K1 + 1;
          twiddle_mul<E>(x[j * Q + brev_bits(k, qb)], A.tw_int, pil[j] * k, A.F);
        });
      }
    });
    if constexpr (LTW && S::nsub > 1) {
      // parallel-load stage: the table words loaded with the tile (above) go to LDS now; the first
      // exchange's barrier publishes them to sub-stages 1.. (no barrier of its own)
      static_for<(TWWORDS + NT - 1) / NT>([&](auto I) {
        constexpr int i = I;
        if (t + NT * i < TWWORDS) lds_tw[t + NT * i] = stw[i];
      });
    }
  }

  if constexpr (IPN == IPN_SLAB) ipn_signal_read(A, mid);  // this tile's elements are in registers now

  // ------------------------------------------------------------------ sub-stages 1..nsub-1 via LDS
  if constexpr (S::nsub > 1) substage<E, LOGR, T, TE, NT, 1, FAST, R32, LTW>(x, cl, pil, lds, A, t, lds_tw, w);
  if constexpr (S::nsub > 2) substage<E, LOGR, T, TE, NT, 2, FAST, R32, LTW>(x, cl, pil, lds, A, t, lds_tw, w);
  if constexpr (S::nsub > 3) substage<E, LOGR, T, TE, NT, 3, FAST, R32, LTW>(x, cl, pil, lds, A, t, lds_tw, w);
  if constexpr (S::nsub > 4) substage<E, LOGR, T, TE, NT, 4, FAST, R32, LTW>(x, cl, pil, lds, A, t, lds_tw, w);
  if constexpr (S::nsub > 5) substage<E, LOGR, T, TE, NT, 5, FAST, R32, LTW>(x, cl, pil, lds, A, t, lds_tw, w);
  static_assert(S::nsub <= 6, "sub-stages");

  // ------------------------------------------------------------------ output
  if constexpr (IPN == IPN_SLAB) {  // the slab this tile writes into has been read (or the wait gave up: no stores)
    if (!ipn_wait_mirror(A, midrev)) return;
  } else if constexpr (IPN == IPN_FUSED3 || IPN == IPN_FUSED2) {  // in-place single launch: every final tile has read
    if (!ipn_grid_barrier<IPN == IPN_FUSED3 ? FUSED3BI_BARRIERS : FUSED2BI_BARRIERS>(A)) return;
  } else if constexpr (IPN == IPN_RESIDENCY) {  // in-place single launch, pass 1: every workgroup is resident (A.ipn_go)
    if (!residency_wait(A.ipn_go, A.wd)) return;
  }
  {
    constexpr int ls = S::nsub - 1;
    constexpr int qb = S::qb(ls), Q = 1 << qb, G = EPT / Q, sb = S::logsig(ls), lN = S::logN(ls);
    static_for<G>([&](auto J) {
      constexpr int j = J;
      const uint32_t g = pil[j];
      const uint32_t rho = g >> sb, cp = g & ((1u << sb) - 1);
      const uint32_t c = cl[j];
      static_for<Q>([&](auto K) {
        constexpr int k = K;
        uint32_t(&v)[E::W] = x[j * Q + brev_bits(k, qb)];
        const uint32_t pi = (rho << lN) + cp + (k << sb);
        const uint32_t kn = natural_index<LOGR, QB>(pi);
        size_t pos;
        if constexpr (KIND == KIND_DIT) {
          // in place (GZKP-NTT.cu:157-158): output k of column c back to c + s k of its block
          pos = colbase + c + ((size_t)kn << log_s);
          E::template store<E::IN * Q, FAST, DW>(dst, ck(pos, A.dbg_dst_n), v, A.F);
        } else if constexpr (KIND == KIND_STOCKHAM) {
          // autosort store (GZKP-NTT.cu:378-384): y[((index - k) << deg) + k + kn p], k = index mod p
          const uint32_t idx = col0 + c, kk = idx & ((1u << A.lgp) - 1);
          pos = ((size_t)(idx - kk) << LOGR) + kk + ((size_t)kn << A.lgp);
          E::template store<E::IN * Q, FAST, DW>(dst, ck(pos, A.dbg_dst_n), v, A.F);
        } else if constexpr (KIND == KIND_COLUMN) {
          if constexpr (FULLTW) {
            // outer twiddle w_{N_i}^{col * kn} R_e from the per-pass table (HBM element format,
            // column-group-major [col / T][kn][col mod T], so one workgroup's entries are one
            // contiguous T * R run: HBM-streamed for pass 1, L2-resident later); the Montgomery
            // product removes R_e.  32 B per entry instead of a 80-B Shoup pair.
            uint32_t tw[E::W];
            size_t ti = ((size_t)col0 << LOGR) + (kn * T + c);
            if (fs_il) {  // Mode I: transform columns (col0 + c) >> il, in the table's column-group-major layout
              const uint32_t tc = (col0 + c) >> A.il;
              ti = ((size_t)(tc & ~(uint32_t)(T - 1)) << LOGR) + kn * T + (tc & (T - 1));
            }
            if constexpr (SHTW) {  // Shoup pair (w, floor(w B / p)), E::TW words: 143 MADs, no R_e
              typename E::Tw tws;
              E::tload(tws, A.tw_full, ti);
              E::mul(v, tws, A.F);
            } else {
              E::template load<E::TABW>(tw, A.tw_full, ti);
              E::mulv(v, tw, A.F);
            }
          } else {
            // outer twiddle w_{N_i}^{col * kn} = w_n^{(col * kn) << log_m} from the two-level
            // tables: t = (lo R_e) * hi, then the Montgomery product v * t / R_e = v * lo * hi
            const size_t e = ((size_t)((col0 + c) >> A.il) * kn) << A.log_m;  // il = 0 unless Mode I
            typename E::Tw tl, th;
            E::tload(tl, A.tw_lo, (uint32_t)(e & ((1u << A.lo_bits) - 1)));
            E::tload(th, A.tw_hi, (uint32_t)(e >> A.lo_bits));
            E::mul(tl.w, th, A.F);
            E::mulv(v, tl.w, A.F);
          }
          pos = colbase + c + ((size_t)kn << log_s);
          if constexpr (MAT) {  // scratch (or, for a transform of one pass, the caller's buffer) in the matrix's own layout
            // a transform of one pass: its rows are the natural outputs (the c^-j epilogue, the row map)
            size_t at;
            if (mat_at(pos, at, (A.mat_ops & MAT_REV_OUT) != 0)) {
              if constexpr (PRO == PRO_NONE) {
                if (A.mat_ops & MAT_MUL_OUT) mat_mul_out(v, (uint32_t)(pos >> A.il));
              }
              E::template store_lazy<E::MUL_OUT, FAST, DW, WT>(dst, ck(at, A.dbg_dst_n), v, A.F);
            }
          } else {
            E::template store_lazy<E::MUL_OUT, FAST, DW, WT>(dst, ck(pos, A.dbg_dst_n), v, A.F);  // scratch: < 2p, read by the next pass
          }
        } else if constexpr (KIND == KIND_FINAL) {
          if (fs_il) {
            const uint32_t k1 = k10 + (c >> tb_log), b = b0 + (c & ((1u << tb_log) - 1));
            pos = (((size_t)k1 + ((size_t)midrev << A.r1) + ((size_t)kn << (A.log_n - LOGR))) << A.il) + b;
          } else if (!IPN && (A.flags & 2u)) {  // NTT_PLAN_IN_PLACE: the input's own position; k_digitrev_swap follows
            pos = ((size_t)(k10 + c) << (A.log_n - A.r1)) + ((size_t)mid << LOGR) + kn;
          } else {
            pos = (size_t)(k10 + c) + ((size_t)midrev << A.r1) + ((size_t)kn << (A.log_n - LOGR));
          }
          if constexpr (EPI) {  // four-step twiddle w_n^(j1 k2) of this output (ntt_rplan), then the pack map
            uint32_t tw[E::W];
            E::template load<E::TABW>(tw, A.tw_epi, epi_idx(pos, bq));
            E::mulv(v, tw, A.F);
            E::template store<E::MUL_OUT, FAST, DW>(dst, ck(out_pos(pos, bq), A.dbg_dst_n), v, A.F);
          } else if constexpr (MAT) {
            size_t at;
            if (mat_at(pos, at, (A.mat_ops & MAT_REV_OUT) != 0)) {
              if (A.mat_ops & MAT_MUL_OUT) {
                mat_mul_out(v, (uint32_t)(pos >> A.il));
                E::template store<E::MUL_OUT, FAST, DW>(dst, ck(at, A.dbg_dst_n), v, A.F);
              } else {
                E::template store<E::IN * Q, FAST, DW>(dst, ck(at, A.dbg_dst_n), v, A.F);
              }
            }
          } else {
            E::template store<E::IN * Q, FAST, DW>(dst, ck(out_pos(pos, bq), A.dbg_dst_n), v, A.F);
          }
        } else {  // KIND_SINGLE, KIND_ROWS
          pos = kn;
          const size_t b = ROWS ? (size_t)w * T + c : (size_t)bq;
          if constexpr (EPI) {
            if (A.flags & 1u) E::mul(v, A.F.ninv, A.F);
            uint32_t tw[E::W];
            E::template load<E::TABW>(tw, A.tw_epi, epi_idx(pos, b));
            E::mulv(v, tw, A.F);
            E::template store<E::MUL_OUT, FAST>(dst, ck(out_pos(pos, b), A.dbg_dst_n), v, A.F);
          } else if (A.flags & 1u) {
            E::mul(v, A.F.ninv, A.F);
            E::template store<E::MUL_OUT, FAST>(dst, ck(out_pos(pos, b), A.dbg_dst_n), v, A.F);
          } else {
            E::template store<E::IN * Q, FAST>(dst, ck(out_pos(pos, b), A.dbg_dst_n), v, A.F);
          }
        }
      });
    });
  }
}

template <class E, int LOGR, int KIND, bool FULLTW, bool FAST, int PRO = PRO_NONE, bool SRC_USER = true,
          int FSM = 0, bool SHTW = false>
__global__ __launch_bounds__((1 << E::TILE_LOG) / E::EPT) __attribute__((amdgpu_waves_per_eu(E::WAVES_PER_EU)))
void k_pass(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, const PassArgs<E> A) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[pass_lds_words<E, LOGR, KIND>()];
  __shared__ __attribute__((aligned(16))) uint32_t lds_tw[pass_ltw<E, KIND, FULLTW>() ? (1 << LOGR) * E::TW : 1];
  // flags bit 2: workgroups are dealt round-robin over the 8 XCDs (b and b + 8 share one, for speed
  // only), so tile (b mod 8) G/8 + b / 8 puts neighbouring tiles -- which share 128-B lines when a
  // pass's runs are 64 B -- on one XCD's L2 at about the same time
  uint32_t w = blockIdx.x;
  if (A.flags & 4u) {
    const uint32_t G = gridDim.x;
    if ((G & 7u) == 0) w = (w & 7u) * (G >> 3) + (w >> 3);
  }
  pass_tile<E, LOGR, KIND, FULLTW, FAST, PRO, SRC_USER, FSM, SHTW>(src, dst, A, w, blockIdx.y, lds, lds_tw);
}

// ---------------------------------------------------------------------------- launchers
// Radices the planner can emit: column/final passes use 3 <= r <= tile_log - MIN_COLS_LOG, single-workgroup
// transforms 3 <= r <= tile_log.  Only those are instantiated.
// Plain (no prologue) pass launch; later column passes of engines whose scratch is narrower than the
// caller's layout read scratch (SRC_USER = false).
template <class E, int LOGR, int KIND, bool FULLTW, bool FAST, int FSM>
static hipError_t launch_plain(const uint32_t* src, uint32_t* dst, const PassArgs<E>& A, dim3 g, dim3 b,
                               hipStream_t st) {
  if constexpr (KIND == KIND_COLUMN && FULLTW && FAST && E::SHOUP_OUTER) {
    if (A.tw_sh) {  // Shoup-pair outer twiddles: later column passes, or pass 1 of a small plan
      constexpr bool SU = E::SCRW == E::MEMW;  // one instance when scratch and caller layouts agree
      if (A.src_user && !SU) return hipErrorInvalidValue;
      hipLaunchKernelGGL((k_pass<E, LOGR, KIND, true, true, PRO_NONE, SU, FSM, true>), g, b, 0, st, src, dst, A);
      return hipGetLastError();
    }
  }
  if (A.tw_sh) return hipErrorInvalidValue;
  if constexpr (KIND == KIND_COLUMN && E::SCRW != E::MEMW) {
    if (!A.src_user) {
      hipLaunchKernelGGL((k_pass<E, LOGR, KIND, FULLTW, FAST, PRO_NONE, false, FSM>), g, b, 0, st, src, dst, A);
      return hipGetLastError();
    }
  }
  hipLaunchKernelGGL((k_pass<E, LOGR, KIND, FULLTW, FAST, PRO_NONE, true, FSM>), g, b, 0, st, src, dst, A);
  return hipGetLastError();
}

// FSM (four-step addressing) instance for this pass: column passes need it only for a mapped input
// (first pass) or Mode I twiddles; final / single passes for a mapped output, Mode I or the epilogue.
template <class E, int KIND, int LOGR, bool FULLTW, bool FAST>
static hipError_t launch_fsm(const uint32_t* src, uint32_t* dst, const PassArgs<E>& A, dim3 g, dim3 b,
                             hipStream_t st) {
  if constexpr (KIND == KIND_STOCKHAM || KIND == KIND_DIT) {
    if (A.fs || A.tw_epi) return hipErrorInvalidValue;
    return launch_plain<E, LOGR, KIND, FULLTW, FAST, 0>(src, dst, A, g, b, st);
  }
  if (A.fs == 0 && !A.tw_epi) return launch_plain<E, LOGR, KIND, FULLTW, FAST, 0>(src, dst, A, g, b, st);
  if constexpr (KIND != KIND_COLUMN) {
    if (A.tw_epi) return launch_plain<E, LOGR, KIND, FULLTW, FAST, 2>(src, dst, A, g, b, st);
  }
  return launch_plain<E, LOGR, KIND, FULLTW, FAST, 1>(src, dst, A, g, b, st);
}

template <class E, int KIND, int LOGR>
static hipError_t launch_pass_r(const uint32_t* src, uint32_t* dst, const PassArgs<E>& A, uint32_t grid,
                                uint32_t batch, hipStream_t st) {
  constexpr int TL = tile_log_of<E>();
  constexpr int MAXR = (KIND == KIND_SINGLE || KIND == KIND_ROWS) ? TL : TL - E::MIN_COLS_LOG;
  // KIND_ROWS: the engines and radices the ntt_*_rows.hip units instantiate (>= 2 transforms per tile);
  // the quotient-estimate engines only in their FAST form
  constexpr bool ROWS_OFF = KIND == KIND_ROWS && (!HasRows<E>::value || LOGR < kRowsMinLog ||
                                                  LOGR > rows_max_log<E>() || LOGR >= TL);
  if constexpr (LOGR > MAXR || ROWS_OFF || ((KIND == KIND_STOCKHAM || KIND == KIND_DIT) && !HasStockham<E>::value)) {
    return hipErrorInvalidValue;
  } else {
    constexpr int TE = (KIND == KIND_SINGLE) ? (1 << LOGR) : (1 << TL);
    constexpr int NT = TE / E::EPT;
    const dim3 g(grid, batch), b(NT < 64 ? 64 : NT);
    if constexpr (E::FASTRED) {
      if (A.F.red_ok) {
        if constexpr (KIND == KIND_STOCKHAM || KIND == KIND_DIT) {
          return A.tw_full ? launch_fsm<E, KIND, LOGR, true, true>(src, dst, A, g, b, st)
                           : launch_fsm<E, KIND, LOGR, false, true>(src, dst, A, g, b, st);
        }
        if constexpr (KIND == KIND_COLUMN) {
          if (A.tw_full && A.src2) {
            if (A.fs)  // Mode I polymul inverse (ntt_rplan)
              hipLaunchKernelGGL((k_pass<E, LOGR, KIND, true, true, PRO_PW, true, 1>), g, b, 0, st, src, dst, A);
            else
              hipLaunchKernelGGL((k_pass<E, LOGR, KIND, true, true, PRO_PW>), g, b, 0, st, src, dst, A);
            return hipGetLastError();
          }
          if (A.tw_full && A.tw_in) {
            if (A.fs) return hipErrorInvalidValue;
            hipLaunchKernelGGL((k_pass<E, LOGR, KIND, true, true, PRO_COSET>), g, b, 0, st, src, dst, A);
            return hipGetLastError();
          }
          if (A.tw_full) return launch_fsm<E, KIND, LOGR, true, true>(src, dst, A, g, b, st);
        }
        if (A.src2 || A.tw_in) return hipErrorInvalidValue;  // fused prologues: FAST column + full tables
        return launch_fsm<E, KIND, LOGR, false, true>(src, dst, A, g, b, st);
      }
    }
    if (A.src2 || A.tw_in) return hipErrorInvalidValue;
    if constexpr (KIND == KIND_ROWS && E::FASTRED) {
      return hipErrorInvalidValue;  // fast reductions only (the caller runs KIND_SINGLE otherwise)
    } else {
      if constexpr (KIND == KIND_COLUMN || KIND == KIND_STOCKHAM || KIND == KIND_DIT) {
        if (A.tw_full) return launch_fsm<E, KIND, LOGR, true, false>(src, dst, A, g, b, st);
      }
      return launch_fsm<E, KIND, LOGR, false, false>(src, dst, A, g, b, st);
    }
  }
}

template <class E, int KIND>
hipError_t launch_pass_kind(int logr, const uint32_t* src, uint32_t* dst, const PassArgs<E>& A, uint32_t grid,
                                uint32_t batch, hipStream_t st) {
  return with_radix<3, 13>(logr, [&](auto R) { return launch_pass_r<E, KIND, R>(src, dst, A, grid, batch, st); });
}

template <class E>
hipError_t launch_pass(int kind, int logr, const uint32_t* src, uint32_t* dst, const PassArgs<E>& A, uint32_t grid,
                       uint32_t batch, hipStream_t st) {
  if (kind == KIND_COLUMN) return launch_pass_kind<E, KIND_COLUMN>(logr, src, dst, A, grid, batch, st);
  if (kind == KIND_FINAL) return launch_pass_kind<E, KIND_FINAL>(logr, src, dst, A, grid, batch, st);
  if (kind == KIND_STOCKHAM || kind == KIND_DIT) {
    if constexpr (HasStockham<E>::value) {
      if (kind == KIND_DIT) return launch_pass_kind<E, KIND_DIT>(logr, src, dst, A, grid, batch, st);
      return launch_pass_kind<E, KIND_STOCKHAM>(logr, src, dst, A, grid, batch, st);
    }
    return hipErrorInvalidValue;
  }
  if (kind == KIND_ROWS) {  // grid = batch / (TILE / 2^logr) workgroups, batch argument 1
    if constexpr (HasRows<E>::value) return launch_pass_kind<E, KIND_ROWS>(logr, src, dst, A, grid, batch, st);
    return hipErrorInvalidValue;
  }
  return launch_pass_kind<E, KIND_SINGLE>(logr, src, dst, A, grid, batch, st);
}

// One pass kind of one engine per translation unit (the kernels dominate compile time).
#define NTT_INSTANTIATE_KIND(E, KIND)                                                                          \
  template hipError_t launch_pass_kind<E, KIND>(int, const uint32_t*, uint32_t*, const PassArgs<E>&, uint32_t, \
                                                uint32_t, hipStream_t);

#define NTT_EXTERN_KIND(E, KIND)                                                                                     \
  extern template hipError_t launch_pass_kind<E, KIND>(int, const uint32_t*, uint32_t*, const PassArgs<E>&, uint32_t, \
                                                       uint32_t, hipStream_t);

// The pass-level dispatch of one engine (ntt_*_misc.hip): the kinds live in units of their own
#define NTT_INSTANTIATE(E)                                                                                         \
  NTT_EXTERN_KIND(E, KIND_COLUMN)                                                                                  \
  NTT_EXTERN_KIND(E, KIND_FINAL)                                                                                   \
  NTT_EXTERN_KIND(E, KIND_SINGLE)                                                                                  \
  NTT_EXTERN_KIND(E, KIND_STOCKHAM)                                                                                \
  NTT_EXTERN_KIND(E, KIND_DIT)                                                                                     \
  template hipError_t launch_pass<E>(int, int, const uint32_t*, uint32_t*, const PassArgs<E>&, uint32_t, uint32_t, \
                                     hipStream_t);

}  // namespace ntt
