// The single-launch schedules (NTT_PLAN_SINGLE_LAUNCH): a whole transform as ONE kernel of pass tiles
// (pass_tile, ntt_kernels_impl.hpp).  Three passes on Eng256 (k_fused3, k_fused3b, in place k_fused3bi) and
// two on the 4096-element tiles of Eng256T (k_fused2b, in place k_fused2bi).  Included by
// ntt_e256_fused.hip and ntt_e256t_fused.hip alone.  The host side's arithmetic (sync-word layout, the
// dataflow form's counters) is plan_fused.hpp.
#pragma once
#include "ntt_kernels_impl.hpp"

namespace ntt {

// ---------------------------------------------------------------------------- fused 3-pass launch
// BASELINE config 2 asks for the 2^20 transform as a single kernel (the reference's SSIP schedule is
// 4 launches at 2^20, GZKP-NTT.cu:1509-1545).  k_fused3 runs the three passes of a 3-pass schedule in
// ONE persistent launch.  Workgroups take tiles from one ticket counter in pass-major order (pass 1's
// tiles, then pass 2's, then the final pass's); a tile waits only for the tiles it reads, through
// counters keyed by the dependency structure of the four-step passes:
//   * pass-2 tile (block k1, column group g) reads columns g T2 + [0, T2) + s2 j2 of every j2 < R2,
//     written by the pass-1 tiles whose columns mod s2 (= 2^r3) fall in the same U-column unit
//     (U = max(T1, T2)): s2 / U counters, each reached by (U / T1) R2 pass-1 tiles;
//   * a final tile (T3 adjacent k1, one k2) reads every column of those k1 blocks: counters keyed by
//     k1 >> log T3 (R1 / T3 of them), each reached by T3 (s2 / T2) pass-2 tiles.
// Deadlock-free at any residency: a tile waits only for tiles with smaller tickets, which are held
// by running workgroups whose own waits are on smaller tickets still (pass 1 waits on nothing).
// Hand-off (MI355X_MICROARCH.md § visibility, publish form R1): scratch stores are write-through
// (sc1), every wave drains them (s_waitcnt vmcnt(0)), a workgroup barrier, then one lane's agent-scope
// counter add; the group's last arrival raises a ready word; the consumer polls it, takes ONE
// agent-scope acquire, waits, barrier, plain loads.
// Every dependency wait is bounded (Watchdog: a workgroup whose wait gives up runs no further tile,
// the launch's other waits give up at once, and the plan's next call returns NTT_ERR_DEVICE), so every
// wave reaches the exit; the last workgroup out re-zeroes the counters for the next launch.
// Producer: every wave drains its write-through stores, a barrier, then one lane counts the tile in;
// the group's last arrival (told by the value its add returns) raises the group's ready word, which
// lies on a 128-B line of its own.  Consumers poll only that word: 128 pollers on the counter itself
// queued the producers' adds behind their polls (2^20: 350-450 us per transform instead of 160).
__device__ __forceinline__ void fused_publish(uint32_t* cnt, uint32_t* ready, uint32_t need) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every wave: its write-through stores are done
  __syncthreads();
  if (threadIdx.x == 0 && __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == need - 1)
    __hip_atomic_store(ready, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// Consumer: one lane polls the ready word with relaxed agent-scope loads (compare-exchange polls,
// read-modify-writes at the memory side, queued the producers' updates behind them: 2^20 single
// launch 0.162 -> see DESIGN §4), sleeping 60 ns .. 1 us between polls; then ONE agent-scope acquire, its wait, and
// the workgroup barrier before any load of the handed-off tile.  Bounded (Watchdog): false
// (workgroup-uniform) when the wait gave up; the workgroup then runs no further tile.
__device__ __forceinline__ bool fused_wait(uint32_t* ready, const FusedArgs& F) {
  if (F.dbg & 1u) return true;  // diagnostics only: no dependency waits (wrong output)
  __shared__ uint32_t s_ok;
  if (threadIdx.x == 0) {
    s_ok = poll_bounded<2, 4, 8, 16, 32>(ready, F.wd) ? 1u : 0u;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  __syncthreads();
  return __builtin_amdgcn_readfirstlane(s_ok) != 0u;
}

template <class E>
struct FusedKArgs {
  const uint32_t* src;
  uint32_t* scratch;
  uint32_t* dst;
  PassArgs<E> A1, A2, A3;
  FusedArgs F;
};
static_assert(sizeof(FusedKArgs<Eng256>) <= 4096, "kernel argument segment");
// The kernel arguments re-addressed per tile through an opaque copy of the kernarg pointer, so that
// the persistent loops do not keep every pass's uniform arguments live across the loop (with the
// LOOPED thread index above: 0-16 B of spills instead of 200-380 B).
template <class E>
__device__ __forceinline__ const FusedKArgs<E>& fused_kargs() {
  typedef const __attribute__((address_space(4))) FusedKArgs<E>* KP;
  KP p = (KP)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(p));
  return *(const FusedKArgs<E>*)p;
}

// pass_tile's options in these kernels: FAST tiles of persistent workgroups.  Passes 1 and 2 are column
// passes with full tables (pass 2: Shoup pairs) whose stores another workgroup reads (write-through); the
// in-place forms append what their stores wait for (IPN_*).
#define NTT_FUSED_PASS1 TW_FULL, RED_FAST, PRO_NONE, SRC_CALLER, FSM_NONE, OUTER_MONT, STORE_WT, TILE_LOOPED
#define NTT_FUSED_PASS2 TW_FULL, RED_FAST, PRO_NONE, SRC_CALLER, FSM_NONE, OUTER_SHOUP, STORE_WT, TILE_LOOPED
#define NTT_FUSED_FINAL TW_TWO_LEVEL, RED_FAST, PRO_NONE, SRC_CALLER, FSM_NONE, OUTER_MONT, STORE_PLAIN, TILE_LOOPED
// what the kernels below assume of their engine; fused3_engine / fused2_engine (ntt_kernels.hpp) name the
// engines they are instantiated for
template <class E>
constexpr bool fused3_props() {
  return E::FASTRED && E::SHOUP_OUTER && !E::LDS_TW && E::TILE_LOG == 10 && E::EPT == 4;
}
static_assert(fused3_props<Eng256>() && fused3_engine<Eng256>(), "the engine of ntt_e256_fused.hip");

template <class E, int R1, int R2, int R3>
__global__ __launch_bounds__((1 << E::TILE_LOG) / E::EPT) __attribute__((amdgpu_waves_per_eu(E::WAVES_PER_EU)))
void k_fused3(const FusedKArgs<E> K) {
  static_assert(fused3_props<E>(), "fused schedule: FAST 256-bit engines");
  constexpr int LW = pass_lds_words<E, R1, KIND_COLUMN>();
  static_assert(LW == pass_lds_words<E, R3, KIND_FINAL>(), "one tile size");
  __shared__ __attribute__((aligned(16))) uint32_t lds[LW];
  __shared__ uint32_t lds_tw[1];
  __shared__ uint32_t s_ticket;
  const FusedArgs& F = K.F;
  uint32_t* const cnt12 = F.sync + 4;
  uint32_t* const cnt23 = F.sync + 4 + F.n12;
  const uint32_t t = threadIdx.x, total = 3 * F.tiles;
  // Tile order: every tile is a ticket sync[0]++, the first taken at start, each later one while the
  // previous tile's stores drain, i.e. in completion order.  (A ticket prefetched at tile START let
  // the first workgroups to start take two or three pass-1 tiles each while later ones idled on
  // pass-2 tiles: 4x slower at 2^20.)
  uint32_t stat = blockIdx.x;  // dbg bit 2: static order b, b + nwg, ...
  auto ticket = [&]() -> uint32_t {
    if (F.dbg & 4u) return stat += F.nwg;
    return t == 0 ? __hip_atomic_fetch_add(F.sync, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
  };
  if (t == 0) s_ticket = (F.dbg & 4u) ? blockIdx.x : ticket();
  __syncthreads();
  uint32_t tk = s_ticket;
  auto advance = [&](uint32_t next) {
    __syncthreads();  // every wave is done with this tile's LDS and s_ticket
    if (t == 0) s_ticket = next;
    __syncthreads();
    tk = s_ticket;
  };
  // tickets only grow per workgroup and are handed out pass-major: one loop per pass
  while (tk < F.tiles) {  // pass 1: the caller's buffer -> scratch
    const uint32_t w = tk;
    const FusedKArgs<E>& L = fused_kargs<E>();
    pass_tile<E, R1, KIND_COLUMN, NTT_FUSED_PASS1>(L.src, L.scratch, L.A1, w, 0, lds, lds_tw);
    const uint32_t next = ticket();  // issued before the drain of this tile's stores
    const uint32_t key = (w & F.k1_mask) >> F.k1_shift;
    fused_publish(cnt12 + key, F.sync + F.rbase + 32 * key, F.need12);
    advance(next);
  }
  while (tk < 2 * F.tiles) {  // pass 2: scratch in place (Shoup-pair outer twiddles)
    const uint32_t w = tk - F.tiles, g = w & ((1u << F.cg_log) - 1);
    if (!fused_wait(F.sync + F.rbase + 32 * (g >> F.k2_shift), F)) {
      tk = total;  // gave up (watchdog): no further tile, straight to the exit
      break;
    }
    const FusedKArgs<E>& L = fused_kargs<E>();
    pass_tile<E, R2, KIND_COLUMN, NTT_FUSED_PASS2>(L.scratch, L.scratch, L.A2, w, 0, lds, lds_tw);
    const uint32_t next = ticket();
    const uint32_t key = (w >> F.cg_log) >> F.t3_log;
    fused_publish(cnt23 + key, F.sync + F.rbase + 32 * (F.n12 + key), F.need23);
    advance(next);
  }
  while (tk < total) {  // final pass: scratch -> the caller's buffer, natural order
    const uint32_t w = tk - 2 * F.tiles;
    if (!fused_wait(F.sync + F.rbase + 32 * (F.n12 + (w >> F.r2)), F)) break;
    const FusedKArgs<E>& L = fused_kargs<E>();
    pass_tile<E, R3, KIND_FINAL, NTT_FUSED_FINAL>(L.scratch, L.dst, L.A3, w, 0, lds, lds_tw);
    advance(ticket());
  }
  if (t == 0 && __hip_atomic_fetch_add(F.sync + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == F.nwg - 1) {
    // the last workgroup out: nobody touches the counters again in this launch
    const uint32_t words = F.rbase + 32 * (F.n12 + F.n23);
    for (uint32_t i = 0; i < words; ++i) __hip_atomic_store(F.sync + i, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (F.wd.abort) __hip_atomic_store(F.wd.abort, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// The same three passes with two grid-wide barriers instead of per-tile hand-offs (FusedArgs::mode 1,
// a plain launch of at most the workgroups the device holds at once).  Each workgroup runs tiles b, b + G, ... of a
// pass, then the barrier.  The barrier (the guide's R1 publish, MI355X_MICROARCH.md § visibility):
// * scratch stores are write-through (sc1), so no release fence: every wave drains them, then a
//   workgroup barrier, then one lane counts the workgroup in;
// * the last of the G arrivals raises the barrier's go word (its own 128-B line);
// * one lane per workgroup polls that word with relaxed global loads (bounded: then the watchdog
//   word), takes ONE agent-scope acquire, and the workgroup barrier releases every wave.
// A/B: plain stores with an agent-scope release per workgroup were slower at 2^20
// (every release writes back its XCD's L2), and compare-exchange polls of one word by 1024
// workgroups made each barrier cost ~0.15 ms.
// The arrival counter is cumulative (barrier k completes at k G arrivals); the last workgroup out
// re-zeroes the words for the next launch.
// False (workgroup-uniform) when the wait gave up (Watchdog): the workgroup then skips the passes left.
__device__ __forceinline__ bool fused_grid_barrier(const FusedArgs& F, uint32_t k) {
  return grid_barrier_words(F.sync, F.shards, F.sync + F.rbase + kSyncLine * (k - 1), k, F.wd);
}

// The exit of a form with K grid barriers.  The last workgroup out -- every other one has passed (or given
// up at) all K barriers -- re-zeroes the launch's words for the next launch: the counter line, the abort
// word, the K go words and the shards (plan_fused.hpp has the layout).
template <uint32_t K>
__device__ __forceinline__ void fused_last_out(const FusedArgs& F, const uint32_t G) {
  if (threadIdx.x == 0 && __hip_atomic_fetch_add(F.sync + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == G - 1) {
    __hip_atomic_store(F.sync, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(F.sync + 1, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (F.wd.abort) __hip_atomic_store(F.wd.abort, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (uint32_t k = 0; k < K; ++k)
      __hip_atomic_store(F.sync + F.rbase + kSyncLine * k, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (uint32_t sh = 0; sh < kSyncShards; ++sh)
      __hip_atomic_store(F.shards + kSyncLine * sh, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

template <class E, int R1, int R2, int R3>
__global__ __launch_bounds__((1 << E::TILE_LOG) / E::EPT) __attribute__((amdgpu_waves_per_eu(E::WAVES_PER_EU)))
void k_fused3b(const FusedKArgs<E> K) {
  static_assert(fused3_props<E>(), "fused schedule: FAST 256-bit engines");
  constexpr int LW = pass_lds_words<E, R1, KIND_COLUMN>();
  static_assert(LW == pass_lds_words<E, R3, KIND_FINAL>(), "one tile size");
  __shared__ __attribute__((aligned(16))) uint32_t lds[LW];
  __shared__ uint32_t lds_tw[1];
  const FusedArgs& F = K.F;
  const uint32_t G = gridDim.x;
  for (uint32_t w = blockIdx.x; w < F.tiles; w += G) {  // pass 1: the caller's buffer -> scratch
    const FusedKArgs<E>& L = fused_kargs<E>();
    pass_tile<E, R1, KIND_COLUMN, NTT_FUSED_PASS1>(L.src, L.scratch, L.A1, w, 0, lds, lds_tw);
    __syncthreads();  // every wave is done with this tile's LDS
  }
  bool ok = fused_grid_barrier(F, 1);
  for (uint32_t w = blockIdx.x; ok && w < F.tiles; w += G) {  // pass 2: scratch in place
    const FusedKArgs<E>& L = fused_kargs<E>();
    pass_tile<E, R2, KIND_COLUMN, NTT_FUSED_PASS2>(L.scratch, L.scratch, L.A2, w, 0, lds, lds_tw);
    __syncthreads();
  }
  ok = ok && fused_grid_barrier(F, 2);  // a workgroup that gave up does not arrive: the others give up too
  for (uint32_t w = blockIdx.x; ok && w < F.tiles; w += G) {  // final pass: scratch -> the caller's buffer
    const FusedKArgs<E>& L = fused_kargs<E>();
    pass_tile<E, R3, KIND_FINAL, NTT_FUSED_FINAL>(L.scratch, L.dst, L.A3, w, 0, lds, lds_tw);
    __syncthreads();
  }
  fused_last_out<FUSED3B_BARRIERS>(F, G);
}

// The single-launch schedule of an NTT_PLAN_IN_PLACE plan (FusedArgs::mode 2; BASELINE config 2's
// "single-kernel self-sort-in-place"): no scratch, every pass in the caller's buffer.  Passes 1 and 2
// write the positions they read (write-through, as k_fused3b); the final pass of the palindromic
// schedule writes its outputs to their natural positions, which lie in the mirror slab, so every final
// tile loads and transforms, a third grid barrier makes sure every tile has read, and only then do the
// tiles store (IPN = 2 in pass_tile).  That needs every final tile resident at once: one tile per
// workgroup, nwg == tiles (n <= 2^20 at 4 workgroups per CU), and a residency check before the first
// store (residency_arrive / residency_wait: barrier 1), so that a launch whose workgroups are not all
// resident stores nothing.
template <class E, int R1, int R2, int R3>
__global__ __launch_bounds__((1 << E::TILE_LOG) / E::EPT) __attribute__((amdgpu_waves_per_eu(E::WAVES_PER_EU)))
void k_fused3bi(const FusedKArgs<E> K) {
  static_assert(fused3_props<E>() && E::SCRW == E::MEMW, "fused in place: 256-bit engines");
  constexpr int LW = pass_lds_words<E, R1, KIND_COLUMN>();
  static_assert(LW == pass_lds_words<E, R3, KIND_FINAL>(), "one tile size");
  __shared__ __attribute__((aligned(16))) uint32_t lds[LW];
  __shared__ uint32_t lds_tw[1];
  const FusedArgs& F = K.F;
  const uint32_t G = gridDim.x;
  uint32_t* const go1 = F.sync + F.rbase;  // residency: grid barrier 1 (residency_arrive)
  residency_arrive(F.sync, F.shards, go1);
  for (uint32_t w = blockIdx.x; w < F.tiles; w += G) {  // pass 1, in place; its stores wait for residency
    const FusedKArgs<E>& L = fused_kargs<E>();
    pass_tile<E, R1, KIND_COLUMN, NTT_FUSED_PASS1, IPN_RESIDENCY>(L.dst, L.dst, L.A1, w, 0, lds, lds_tw);
    __syncthreads();
  }
  bool ok = residency_went(go1) && fused_grid_barrier(F, 2);
  for (uint32_t w = blockIdx.x; ok && w < F.tiles; w += G) {  // pass 2, in place
    const FusedKArgs<E>& L = fused_kargs<E>();
    pass_tile<E, R2, KIND_COLUMN, NTT_FUSED_PASS2>(L.dst, L.dst, L.A2, w, 0, lds, lds_tw);
    __syncthreads();
  }
  ok = ok && fused_grid_barrier(F, 3);
  if (ok && blockIdx.x < F.tiles) {  // final pass: load, transform, barrier 4 (inside), natural-order stores
    const FusedKArgs<E>& L = fused_kargs<E>();
    pass_tile<E, R3, KIND_FINAL, NTT_FUSED_FINAL, IPN_FUSED3>(L.dst, L.dst, L.A3, blockIdx.x, 0, lds, lds_tw);
  }
  fused_last_out<FUSED3BI_BARRIERS>(F, G);
}

// BASELINE config 2 as ONE kernel on 4096-element tiles (the reference's 2^20
// schedule is 4 launches, GZKP-NTT.cu:1509-1545): the two passes (10 + 10) of Eng256T with ONE grid
// barrier between them.  2^20 is 256 tiles per pass, one 1024-thread workgroup per CU, so each
// workgroup runs one tile of each pass.  A plain launch (no cooperative launch: its ~20 us per call
// was most of the 3-pass single launch's deficit) of at most the occupancy query's
// workgroups; the barrier is bounded (Watchdog), so a device shared with another persistent kernel
// ends in NTT_ERR_DEVICE, never a hang.
//   k_fused2b  (FusedArgs::mode 3): pass 1 caller -> scratch (write-through), barrier, final pass
//              scratch -> caller, natural order.
//   k_fused2bi (FusedArgs::mode 4): NTT_PLAN_IN_PLACE, the palindromic 10 + 10: pass 1 in place (its
//              stores wait for the residency decision, barrier 1), barrier 2, the final pass loads and
//              transforms every tile, barrier 3 (every tile has read: all 256 final tiles are
//              resident), then the stores to the natural positions in the mirror slab (pass_tile
//              IPN = 3).  No scratch.
// FusedArgs::trace (diagnostics, NTT_FUSED_TRACE): per workgroup the wall clock (100 MHz) at start,
// after pass 1, after the pass barrier and at the end.
__device__ __forceinline__ void fused_trace(const FusedArgs& F, uint32_t at) {
  if (F.trace && threadIdx.x == 0) F.trace[4 * blockIdx.x + at] = (unsigned long long)wall_clock64();
}
template <class E, int R1, int R2>
__global__ __launch_bounds__((1 << E::TILE_LOG) / E::EPT) __attribute__((amdgpu_waves_per_eu(E::WAVES_PER_EU)))
void k_fused2b(const FusedKArgs<E> K) {
  static_assert(E::FASTRED && !E::LDS_TW, "fused schedule: FAST 256-bit engines");
  constexpr int LW = pass_lds_words<E, R1, KIND_COLUMN>();
  static_assert(LW == pass_lds_words<E, R2, KIND_FINAL>(), "one tile size");
  __shared__ __attribute__((aligned(16))) uint32_t lds[LW];
  __shared__ uint32_t lds_tw[1];
  const FusedArgs& F = K.F;
  const uint32_t G = gridDim.x;
  fused_trace(F, 0);
  for (uint32_t w = blockIdx.x; w < F.tiles; w += G) {  // pass 1: the caller's buffer -> scratch
    const FusedKArgs<E>& L = fused_kargs<E>();
    pass_tile<E, R1, KIND_COLUMN, NTT_FUSED_PASS1>(L.src, L.scratch, L.A1, w, 0, lds, lds_tw);
    __syncthreads();
  }
  fused_trace(F, 1);
  const bool ok = fused_grid_barrier(F, 1);
  fused_trace(F, 2);
  for (uint32_t w = blockIdx.x; ok && w < F.tiles; w += G) {  // final pass: scratch -> the caller's buffer
    const FusedKArgs<E>& L = fused_kargs<E>();
    pass_tile<E, R2, KIND_FINAL, NTT_FUSED_FINAL>(L.scratch, L.dst, L.A3, w, 0, lds, lds_tw);
    __syncthreads();
  }
  fused_trace(F, 3);
  fused_last_out<FUSED2B_BARRIERS>(F, G);
}

template <class E, int R>
__global__ __launch_bounds__((1 << E::TILE_LOG) / E::EPT) __attribute__((amdgpu_waves_per_eu(E::WAVES_PER_EU)))
void k_fused2bi(const FusedKArgs<E> K) {
  static_assert(E::FASTRED && !E::LDS_TW && E::SCRW == E::MEMW, "fused in place: 256-bit engines");
  constexpr int LW = pass_lds_words<E, R, KIND_COLUMN>();
  static_assert(LW == pass_lds_words<E, R, KIND_FINAL>(), "one tile size");
  __shared__ __attribute__((aligned(16))) uint32_t lds[LW];
  __shared__ uint32_t lds_tw[1];
  const FusedArgs& F = K.F;
  const uint32_t G = gridDim.x;
  uint32_t* const go1 = F.sync + F.rbase;  // residency: grid barrier 1 (residency_arrive)
  fused_trace(F, 0);
  residency_arrive(F.sync, F.shards, go1);
  for (uint32_t w = blockIdx.x; w < F.tiles; w += G) {  // pass 1, in place; its stores wait for residency
    const FusedKArgs<E>& L = fused_kargs<E>();
    pass_tile<E, R, KIND_COLUMN, NTT_FUSED_PASS1, IPN_RESIDENCY>(L.dst, L.dst, L.A1, w, 0, lds, lds_tw);
    __syncthreads();
  }
  fused_trace(F, 1);
  const bool ok = residency_went(go1) && fused_grid_barrier(F, 2);
  fused_trace(F, 2);
  if (ok && blockIdx.x < F.tiles) {  // final pass: load, transform, barrier 3 (inside), natural-order stores
    const FusedKArgs<E>& L = fused_kargs<E>();
    pass_tile<E, R, KIND_FINAL, NTT_FUSED_FINAL, IPN_FUSED2>(L.dst, L.dst, L.A3, blockIdx.x, 0, lds, lds_tw);
  }
  fused_trace(F, 3);
  fused_last_out<FUSED2BI_BARRIERS>(F, G);
}

// ---- instances and launchers.  One list per family says which (mode, radices) has a kernel; the launcher
// launches what it returns and the capacity query asks the occupancy of what it returns, so the plan
// never sizes a grid from another kernel's occupancy.
template <class E>
using FusedKernel = void (*)(const FusedKArgs<E>);
template <int V>
constexpr std::integral_constant<int, V> rdx{};  // a radix as a value whose type carries it

// k_fused3 (mode 0, and what the launcher has always taken any other mode for), k_fused3b (mode 1),
// k_fused3bi (mode 2); null: no instance
template <class E>
FusedKernel<E> fused3_kernel(uint32_t mode, int r1, int r2, int r3) {
  FusedKernel<E> k = nullptr;
  [[maybe_unused]] auto scratch = [&](auto A, auto B, auto C) {
    if (mode != 2 && r1 == A && r2 == B && r3 == C) k = mode == 1 ? &k_fused3b<E, A, B, C> : &k_fused3<E, A, B, C>;
  };
  [[maybe_unused]] auto inplace = [&](auto A, auto B, auto C) {  // one workgroup per tile
    if (mode == 2 && r1 == A && r2 == B && r3 == C) k = &k_fused3bi<E, A, B, C>;
  };
  if constexpr (fused3_engine<E>()) {
    scratch(rdx<6>, rdx<6>, rdx<6>);
    scratch(rdx<7>, rdx<6>, rdx<6>);
    scratch(rdx<7>, rdx<7>, rdx<6>);
    scratch(rdx<7>, rdx<7>, rdx<7>);
    scratch(rdx<8>, rdx<7>, rdx<7>);
    scratch(rdx<8>, rdx<8>, rdx<7>);
    scratch(rdx<8>, rdx<8>, rdx<8>);
    inplace(rdx<6>, rdx<6>, rdx<6>);
    inplace(rdx<6>, rdx<7>, rdx<6>);
    inplace(rdx<7>, rdx<6>, rdx<7>);
  }
  return k;
}
// k_fused2b (mode 3), k_fused2bi (mode 4): 2^20 = 10 + 10 on the 4096-element tiles
template <class E>
FusedKernel<E> fused2_kernel(uint32_t mode, int r1, int r2) {
  if constexpr (fused2_engine<E>()) {
    if (r1 == 10 && r2 == 10 && mode == 3) return &k_fused2b<E, 10, 10>;
    if (r1 == 10 && r2 == 10 && mode == 4) return &k_fused2bi<E, 10>;
  }
  return nullptr;
}

// The grid-barrier forms are plain launches of at most the occupancy query's workgroups (the plan
// checks that the grid fits the device, fused_capacity); the plan serialises its single launches
// per device (ntt_plan.cpp FusedSerial), and the in-place forms check residency before their first
// store.  Round 6 retired the cooperative launch: ~20 us more per call, and every
// rocprofv3-traced process that had made one crashed in the runtime's exit handlers.
template <class E>
hipError_t fused_launch(FusedKernel<E> k, const FusedKArgs<E>& K, hipStream_t st) {
  if (!k) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k, dim3(K.F.nwg), dim3((1 << E::TILE_LOG) / E::EPT), 0, st, K);
  return hipGetLastError();
}
// workgroups of kernel k resident at once on `device` (occupancy query x CUs)
template <class E>
hipError_t fused_capacity(FusedKernel<E> k, int device, uint32_t* wgs) {
  int cus = 0, per = 0;
  if (!k || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess)
    return hipErrorInvalidValue;
  const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, reinterpret_cast<const void*>(k),
                                                                    (1 << E::TILE_LOG) / E::EPT, 0);
  if (e != hipSuccess) return e;
  *wgs = (uint32_t)(cus * per);
  return hipSuccess;
}

template <class E>
hipError_t launch_fused2(int r1, int r2, const uint32_t* src, uint32_t* scratch, uint32_t* dst, const PassArgs<E>& A1,
                         const PassArgs<E>& A2, const FusedArgs& F, hipStream_t st) {
  return fused_launch<E>(fused2_kernel<E>(F.mode, r1, r2), FusedKArgs<E>{src, scratch, dst, A1, A1, A2, F}, st);
}
template <class E>
hipError_t fused2_capacity(int r1, int r2, int device, uint32_t* wgs, uint32_t mode) {
  return fused_capacity<E>(fused2_kernel<E>(mode, r1, r2), device, wgs);
}

template <class E>
hipError_t launch_fused3(int r1, int r2, int r3, const uint32_t* src, uint32_t* scratch, uint32_t* dst,
                         const PassArgs<E>& A1, const PassArgs<E>& A2, const PassArgs<E>& A3, const FusedArgs& F,
                         hipStream_t st) {
  return fused_launch<E>(fused3_kernel<E>(F.mode, r1, r2, r3), FusedKArgs<E>{src, scratch, dst, A1, A2, A3, F}, st);
}
template <class E>
hipError_t fused3_capacity(int r1, int r2, int r3, int device, uint32_t* wgs, uint32_t mode) {
  return fused_capacity<E>(fused3_kernel<E>(mode, r1, r2, r3), device, wgs);
}

#undef NTT_FUSED_PASS1
#undef NTT_FUSED_PASS2
#undef NTT_FUSED_FINAL

#define NTT_INSTANTIATE_FUSED(E)                                                                                \
  template hipError_t launch_fused3<E>(int, int, int, const uint32_t*, uint32_t*, uint32_t*, const PassArgs<E>&,     \
                                       const PassArgs<E>&, const PassArgs<E>&, const FusedArgs&, hipStream_t);      \
  template hipError_t fused3_capacity<E>(int, int, int, int, uint32_t*, uint32_t);

#define NTT_INSTANTIATE_FUSED2(E)                                                                                 \
  template hipError_t launch_fused2<E>(int, int, const uint32_t*, uint32_t*, uint32_t*, const PassArgs<E>&,           \
                                       const PassArgs<E>&, const FusedArgs&, hipStream_t);                          \
  template hipError_t fused2_capacity<E>(int, int, int, uint32_t*, uint32_t);

}  // namespace ntt
