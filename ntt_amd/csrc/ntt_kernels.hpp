// Kernel-facing argument structs and launcher declarations (host + device).
#pragma once
#include <type_traits>
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "engines.hpp"
#include "fieldext.hpp"
#include "plan_fused.hpp"
#include "poseidon2.hpp"
#include "scan_shape.hpp"

namespace ntt {

// KIND_STOCKHAM: the rival schedule of the reference's bellperson / improved_NTT_v1..v4 family
// (GZKP-NTT.cu:324-386, 556-1296): Stockham autosort passes, input-side twiddles, no final
// permutation (ntt_plan_create_ex flag NTT_PLAN_STOCKHAM).
// KIND_DIT: the GZKP(B, G) rival (GZKP-NTT.cu:115-165): in-place DIT column passes with input-side
// twiddles w_N^(c d) over bit-reversed data (ntt_plan_create_ex flag NTT_PLAN_GZKP).
// KIND_ROWS: a batch of short single-tile transforms (below one wave each: n <= 2^7 on the 256-bit
// engines, 2^6 on P), TILE / n of them per workgroup (the final pass's block layout), instead of one
// per workgroup (KIND_SINGLE): batched short transforms and the four-step's row transforms
// (ntt_rplan) of such n.  At n = 2^8 / 2^9 on the 256-bit engines one transform per one- / two-wave
// workgroup is as fast or faster.
enum : int { KIND_COLUMN = 0, KIND_FINAL = 1, KIND_SINGLE = 2, KIND_STOCKHAM = 3, KIND_DIT = 4, KIND_ROWS = 5 };
// engines with KIND_STOCKHAM instances (ntt_e256_stk.hip, ntt_ep_stk.hip)
template <class E>
struct HasStockham {
  static constexpr bool value = false;
};
// engines with KIND_ROWS instances (ntt_e256_rows.hip, ntt_e256w_rows.hip, ntt_ep_rows.hip) and the radices they cover
template <class E>
struct HasRows {
  static constexpr bool value = false;
};
constexpr int kRowsMinLog = 3;
// the largest KIND_ROWS radix of an engine, measured (profiles/r05_rows/): 2^7 on the
// 256-bit engines (1024-element tiles, 256-thread workgroups); 2^6 on P, whose 8192-element tiles
// make 1024-thread workgroups that lose to one transform per workgroup from 2^7 up (+20 %, 2^8 +180 %)
// (Goldilocks, W = 2: 4096-element tiles and 512-thread workgroups, the P path's shape; its limit is
// taken from P, not measured; Eng31, W = 1: P's own shape, its limit taken from P as well)
template <class E>
constexpr int rows_max_log() {
  return E::W <= 2 ? 6 : 7;
}

// Elements per workgroup tile of the multi-pass kernels (engines.hpp: E::TILE_LOG, E::EPT per thread).
template <class E>
__host__ __device__ constexpr int tile_log_of() { return E::TILE_LOG; }

using Eng256 = Eng29<9, 8>;    // 4 x 64-bit limbs in HBM
using Eng384 = Eng29<14, 12>;  // 6 x 64-bit limbs in HBM, moduli up to 2^383
using Eng256w = Eng29<9, 12>;  // 6 x 64-bit limbs in HBM, moduli < 2^255 (256-bit arithmetic)
using Eng256wI = Eng29<9, 12, 12>;  // the same with 48-B intermediates: NTT_PLAN_IN_PLACE plans (C3 in place)
using Eng256T = Eng29<9, 8, 0, 12>;  // 4 x 64-bit limbs, 4096-element tiles: single 2^20 transforms (C2)
using EngP = Eng32<1, 2>;      // P469762049, `long long` in HBM
using EngPI = Eng32<1, 2, 2>;  // the same with 8-B scratch elements: NTT_PLAN_IN_PLACE plans of P
template <class E>
struct IsEng32 : std::false_type {};
template <int N, int M, int S>
struct IsEng32<Eng32<N, M, S>> : std::true_type {};
template <>
struct HasStockham<Eng256> {
  static constexpr bool value = true;
};
template <>
struct HasStockham<EngP> {
  static constexpr bool value = true;
};
template <>
struct HasRows<Eng256> {
  static constexpr bool value = true;
};
template <>
struct HasRows<Eng256w> {  // the 6 x 64-bit layout of 256-bit moduli (BLS12-381 C3), ntt_e256w_rows.hip
  static constexpr bool value = true;
};
template <>
struct HasRows<EngP> {  // P469762049 (the reference's own field), ntt_ep_rows.hip
  static constexpr bool value = true;
};
template <>
struct HasRows<Eng64G> {  // Goldilocks, ntt_eg_rows.hip
  static constexpr bool value = true;
};
template <>
struct HasRows<Eng31> {  // primes below 2^31 on 4-B elements, ntt_e31_rows.hip
  static constexpr bool value = true;
};
// engines with low-degree-extension instances (PRO_LDE first passes, ntt_*_lde.hip): every engine a
// default plan runs on; not the NTT_PLAN_IN_PLACE engines nor the 4096-element tiles
template <class E>
struct HasLde {
  static constexpr bool value = std::is_same_v<E, Eng256> || std::is_same_v<E, Eng384> || std::is_same_v<E, Eng256w> ||
                                std::is_same_v<E, EngP> || std::is_same_v<E, Eng64G> || std::is_same_v<E, Eng31>;
};

// a modulus as W little-endian 32-bit words (canonical-range checks)
template <int W>
struct ModWords {
  uint32_t w[W];
};
template <class E>
hipError_t launch_count_noncanonical(const uint32_t* d, size_t n, const ModWords<E::MEMW>& p,
                                     unsigned long long* bad, hipStream_t st);

// Four-step position map (PassArgs::min / mout / mepi): p -> (p >> lc) ps + ((p mod 2^lc) >> lc2) ps2
// + (b << lc2) + (p mod 2^lc2); lc2 = lc (and ps2 = 0) is the one-level map of round 2.
struct FsMap {
  uint32_t lc, lc2;
  uint64_t ps, ps2;
  __host__ __device__ size_t operator()(size_t p, size_t b) const {
    const size_t m = ((size_t)1 << lc) - 1, m2 = ((size_t)1 << lc2) - 1;
    return (p >> lc) * ps + ((p & m) >> lc2) * ps2 + (b << lc2) + (p & m2);
  }
};

// Every inter-workgroup wait (k_final_ipn, k_fused3, k_fused3b, k_fused3bi) is bounded.  A wait that
// reaches `spins` polls gives up: it raises the launch's own abort word (which the launch's other
// waits check every 256 polls, so they give up too and every wave reaches the exit), the workgroup
// skips its remaining stores, and the plan's
// host-mapped report word `report` is set (system scope).  The next call on the plan returns
// NTT_ERR_DEVICE without any device query (ntt_plan_device_status reads and clears the report).
// spins = 0 gives up at once (ntt_plan_set_watchdog: a test hook).
struct Watchdog {
  uint32_t* report;  // host-mapped word of the plan (null: none)
  uint32_t* abort;   // the launch's abort word, on a 128-B line of its own (pollers of a line that also
                     // holds a counter queue the counter's atomic adds: DESIGN §4); zeroed by the last
                     // workgroup out
  uint32_t spins;    // poll limit, ~1 us per poll after the first few (default 2^21, ~2 s)
};

template <class E>
struct PassArgs {
  typename E::Args F;
  const uint32_t* tw_int;  // w_R^e, e < R (this pass's radix), engine table format
  const uint32_t* tw_lo;   // outer twiddles w_n^e = tw_lo[e mod 2^lo_bits] * tw_hi[e >> lo_bits]
  const uint32_t* tw_hi;
  const uint32_t* tw_full;  // column pass: per-pass outer twiddle table (HBM element format) or null
  const uint32_t* src2;     // first column pass of a fused polymul inverse: x <- mont(src, src2) at load
  const uint32_t* tw_in;    // first column pass of a fused coset forward: x_d <- x_d u^d (Shoup table, d < R);
                            // PRO_LDE without a full table, where lde_mul_at_load(): the shift's two-level
                            // lo_s table (null: no shift, or the inputs are already scaled)
  uint32_t lo_bits;
  uint32_t log_n;
  uint32_t log_blk;  // column pass: log2 of the block length N_i
  uint32_t log_m;    // column pass: log2(n / N_i)
  uint32_t r1;       // final pass: log2 R_1
  uint32_t nmid;     // final pass: number of middle digits (p - 2)
  uint32_t mid_bits[4];  // final pass: middle digit widths, least significant (k_{p-1}) first
  uint32_t mid_off[4];   // final pass: output bit offset (relative to R_1) of those digits
  uint32_t flags;        // bit 0: multiply outputs by ninv (single-pass inverse); bit 1: final pass
                         // writes each output to its input's position (NTT_PLAN_IN_PLACE); bit 2:
                         // XCD-grouped tile order (tiles t and t + 1 on one XCD, k_pass)
  uint32_t src_user;     // column pass: src is the caller's buffer (E::MEMW words/element), not scratch (E::SCRW)
  size_t batch_stride;   // 32-bit words between batched transforms in the caller's buffers (n * E::MEMW)
  // ---- distributed four-step addressing (ntt_rplan_*); fs == 0: plain batched transforms.
  // Mode B (fs & FS_IL == 0): transform b (= blockIdx.y) of a batch, position p (the row transforms:
  //   packed output of the forward, exchanged input of the inverse).
  // Mode I (fs & FS_IL): 2^il transforms interleaved, element j of transform b at P = j 2^il + b (the
  //   [n1][c] column layout and the exchanged blocks); every pass groups T adjacent transforms, so
  //   runs stay contiguous.  b = 0 in the maps below (P carries it).
  // A map (FsMap) sends p to (p >> lc) ps + ((p mod 2^lc) >> lc2) ps2 + (b << lc2) + (p mod 2^lc2):
  //   peer blocks of ps elements, within them column pieces of ps2 elements (lc2 = lc: no pieces).
  //   min: the first pass's input (FS_MAP_IN, src and src2), mout: the last pass's output
  //   (FS_MAP_OUT), mepi: the Mode I epilogue-table index (FS_MAP_EPI).
  uint32_t lgp;          // KIND_STOCKHAM: log2 of the number of groups p already combined (bellperson `lgp`)
  uint32_t fs;           // FS_* bits
  uint32_t il;           // Mode I: log2 of the interleave
  FsMap min, mout, mepi;
  const uint32_t* tw_epi;  // final pass: multiply output k of transform b by this table's entry (w R_e,
                           // E::SCRW words; index b N + k in Mode B, k 2^il + b in Mode I) or null
  uint32_t tw_sh;          // column pass: tw_full holds Shoup pairs (canonical w, floor(w B / p); E::TW words
                           // per entry, E::SHOUP_OUTER engines) instead of w R_e in the element format
  // ---- in-place final pass with the digit reversal fused (k_final_ipn, NTT_PLAN_IN_PLACE):
  uint32_t* ipn_sync;        // [0] tile ticket, [1] workgroups exited; slab m: reads done at [32 (1 + m)],
                             // ready at [32 (1 + m) + 1] (one 128-B line per slab)
  const uint32_t* ipn_order; // slab (middle-digit value) of the i-th slab in ticket order (pairs adjacent)
  uint32_t ipn_strips;       // workgroups per slab (R_1 / T)
  uint32_t* ipn_go;          // k_fused3bi (the in-place single launch): the final pass's barrier go word
  uint32_t* ipn_shards;      //   and its arrival shard lines (ipn_sync: the top counter)
  Watchdog wd;               // bounded waits (k_final_ipn, k_fused3bi)
  // debug builds (NTT_DEBUG_CHECKS): element extents of src / dst from this transform's first element
  // (~0: not checked, e.g. four-step maps into the caller's exchange blocks)
  size_t dbg_src_n, dbg_dst_n;
  // ---- low-degree extension (PRO_LDE, ntt_lde_batch): the pass that reads the caller's buffer takes
  // transform b's input at src + b src_stride, src_stride / E::MEMW elements long; positions at and
  // above that length are zero and never loaded (batch_stride stays the destination's stride)
  size_t src_stride;        // 32-bit words between the batch's inputs (n_in * E::MEMW)
  const uint32_t* tw_in_hi; // the shift's two-level hi table (with tw_in = lo_s: c^j at load)
  // ---- row-major matrix transforms (k_pass_mat, ntt_*_matrix): the pass runs on strips of 2^il adjacent
  // columns of a [n][mat_w] matrix, element (row, col) at row mat_w + col; workgroup g of the launch is
  // strip g mod mat_ns of tile g / mat_ns (the strips of one tile share lines: they run together)
  uint32_t mat_w;   // columns of the matrix
  uint32_t mat_ns;  // strips per row: ceil(mat_w / 2^il)
  uint32_t mat_ops; // MAT_* bits (ntt_*_matrix_ex): row maps of the first / last pass, the c^-j epilogue
};
enum : uint32_t { FS_MAP_IN = 1u, FS_MAP_OUT = 2u, FS_IL = 4u, FS_MAP_EPI = 8u };
// PassArgs::mat_ops.  A row map changes which row a strip's run of columns belongs to, never the run:
//   MAT_REV_IN   the pass that reads the caller's matrix loads natural row j from row bitrev_log_n(j);
//   MAT_REV_OUT  the pass that writes the caller's matrix stores natural row k at row bitrev_log_n(k);
//   MAT_MUL_OUT  that pass multiplies natural output row j by tw_in[j mod 2^lo_bits] tw_in_hi[j >> lo_bits]
//                (the shift's inverse tables: c^-j) before the store; tw_in is then not a load-side table.
enum : uint32_t { MAT_REV_IN = 1u, MAT_REV_OUT = 2u, MAT_MUL_OUT = 4u };

// Fused single-launch schedule of a 3-pass transform (k_fused3, BASELINE config 2's "single-kernel"):
// one persistent launch runs pass 1's, pass 2's and the final pass's tiles, handed between
// workgroups through counters instead of kernel boundaries.  Word layout of `sync` (zero before the
// first launch; the last workgroup to leave re-zeroes it): [0] tile ticket, [1] workgroups exited,
// [2], [3] spare, [4, 4 + n12) pass 1 -> 2 counters,
// [4 + n12, 4 + n12 + n23) pass 2 -> final counters, then one ready word per counter (rbase); FusedSync
// (plan_fused.hpp) has the layout of every form.
struct FusedArgs {
  uint32_t* sync;
  uint32_t tiles;      // tiles per pass (n / TILE)
  uint32_t nwg;        // workgroups launched
  uint32_t k1_mask, k1_shift;  // pass-1 tile w: counter (w & k1_mask) >> k1_shift
  uint32_t cg_log;             // pass-2 tile w: column group w mod 2^cg_log, block k1 = w >> cg_log
  uint32_t k2_shift;           //   waits on counter (w mod 2^cg_log) >> k2_shift
  uint32_t t3_log;             //   signals counter n12 + (k1 >> t3_log)
  uint32_t r2;                 // final tile w: waits on counter n12 + (w >> r2)
  uint32_t n12, n23;
  uint32_t need12, need23;     // arrivals per counter
  uint32_t rbase;              // ready word of counter i at sync[rbase + 32 i] (one 128-B line each)
  uint32_t dbg;                // diagnostics only (NTT_FUSED_DBG): bit 0 no dependency waits (wrong
                               // output), bit 2 static tile order (needs every workgroup resident)
  uint32_t mode;               // 0: dataflow hand-offs between tiles (k_fused3); 1: two grid barriers
                               // (k_fused3b); 2: the NTT_PLAN_IN_PLACE form, residency + three grid
                               // barriers, one workgroup per tile (k_fused3bi); 3: two passes on
                               // 4096-element tiles, one barrier (k_fused2b); 4: the same in place,
                               // residency + two barriers (k_fused2bi)
  Watchdog wd;                 // bounded waits
  uint32_t* shards;            // grid barriers (modes 1..4): 8 arrival shards, one 128-B line each
  unsigned long long* trace;   // diagnostics (NTT_FUSED_TRACE, modes 3 and 4): 4 timestamps per workgroup
};
// the engines k_fused3 / k_fused3b / k_fused3bi are instantiated for: those whose fused unit is in build.py's
// SOURCES (ntt_e256_fused.hip).  The kernels assert the properties they need of it (fused3_props).
template <class E>
__host__ __device__ constexpr bool fused3_engine() {
  return std::is_same_v<E, Eng256>;
}
template <class E>
hipError_t launch_fused3(int r1, int r2, int r3, const uint32_t* src, uint32_t* scratch, uint32_t* dst,
                         const PassArgs<E>& A1, const PassArgs<E>& A2, const PassArgs<E>& A3, const FusedArgs& F,
                         hipStream_t st);
// workgroups one launch of k_fused3<E, r1, r2, r3> (mode 0) or k_fused3b (mode 1) keeps resident on
// `device` (occupancy query x CUs)
template <class E>
hipError_t fused3_capacity(int r1, int r2, int r3, int device, uint32_t* wgs, uint32_t mode = 0);

// The two-pass single launch on 4096-element tiles (k_fused2b, FusedArgs::mode 3; in place:
// k_fused2bi, mode 4): 2^20 = 10 + 10 on Eng256T with one grid barrier, a plain launch
// the engines k_fused2b / k_fused2bi are instantiated for (radices 10 + 10: 2^20 on 4096-element tiles)
template <class E>
__host__ __device__ constexpr bool fused2_engine() {
  return E::FASTRED && !E::LDS_TW && E::TILE_LOG == 12 && E::EPT == 4 && E::W == 9 && E::MEMW == 8;
}
template <class E>
hipError_t launch_fused2(int r1, int r2, const uint32_t* src, uint32_t* scratch, uint32_t* dst, const PassArgs<E>& A1,
                         const PassArgs<E>& A2, const FusedArgs& F, hipStream_t st);
template <class E>
hipError_t fused2_capacity(int r1, int r2, int device, uint32_t* wgs, uint32_t mode);

// The in-place final pass with the digit reversal fused (NTT_PLAN_IN_PLACE, batch 1): A.ipn_* set,
// grid = n / TILE workgroups, src == dst.  See k_final_ipn.
template <class E>
hipError_t launch_final_ipn(int logr, uint32_t* data, const PassArgs<E>& A, uint32_t grid, hipStream_t st);
// workgroups of k_final_ipn<E, logr> resident at once on `device` (0: unknown)
template <class E>
uint32_t launch_final_ipn_capacity(int logr, int device);

template <class E, int KIND>
hipError_t launch_pass_kind(int logr, const uint32_t* src, uint32_t* dst, const PassArgs<E>& A, uint32_t grid,
                            uint32_t batch, hipStream_t st);
template <class E>
hipError_t launch_pass(int kind, int logr, const uint32_t* src, uint32_t* dst, const PassArgs<E>& A, uint32_t grid,
                       uint32_t batch, hipStream_t st);
// PRO_LDE passes without the shift in their outer table: is the two-level product c^j = lo_s * hi
// compiled in at the load?  Yes on the one- and two-word engines; on the 9-limb engines in
// KIND_SINGLE only; never on the 14-limb engine.  Elsewhere the two table entries and their product
// do not fit beside the tile (the pass would spill where its plain sibling does not), and
// the shift is applied by launch_lde_scale over the inputs first.
template <class E, int KIND>
__host__ __device__ constexpr bool lde_mul_at_load() {
  return E::W <= 2 || (E::W <= 9 && KIND == KIND_SINGLE);
}
// PRO_LDE instances that exist.  A few passes that sit at their register cap spill with the padded
// load where their plain sibling does not: the 14-limb engine's radix-8 column pass and its
// 8- and 16-point single tiles, and the 9-limb engines' radix-64 column pass in the generic (non-FAST)
// form.  They are not instantiated; ntt_lde_batch runs such a plan through the zero-padded staging
// route (PlanImpl::lde_staged).  fast: the FAST form (A.F.red_ok on a fast-reduction engine).
template <class E>
__host__ __device__ constexpr bool lde_pass_available(int kind, int logr, bool fast) {
  if (E::W > 9) return !((kind == KIND_COLUMN && logr == 3) || (kind == KIND_SINGLE && logr <= 4));
  if (E::W == 9) return !(kind == KIND_COLUMN && logr == 6 && !fast);
  return true;
}
// dst[v n_in + j] = src[v n_in + j] c^j (j < n_in, v < batch; canonical in and out), c^j from the
// shift's two-level tables: the inputs of a low-degree extension whose first pass cannot take the
// product at load.  Engines with HasLde only.
template <class E>
hipError_t launch_lde_scale(const uint32_t* src, uint32_t* dst, size_t n_in, uint32_t batch, const uint32_t* lo_s,
                            const uint32_t* hi, uint32_t lo_bits, const typename E::Args& F, hipStream_t st);
// The pass of a low-degree extension that reads the caller's buffer (PRO_LDE): kind = KIND_COLUMN (the
// first pass of a multi-pass size) or KIND_SINGLE (sizes up to one tile).  Engines with HasLde only.
template <class E>
hipError_t launch_lde_pass(int kind, int logr, const uint32_t* src, uint32_t* dst, const PassArgs<E>& A, uint32_t grid,
                           uint32_t batch, hipStream_t st);
// ---- row-major matrix transforms (ntt_forward_matrix / ntt_inverse_matrix / ntt_lde_matrix): the
// transforms run over the columns of a [n][width] matrix in the strip form of the pass tile (MAT in
// ntt_kernels_impl.hpp).  Engines with instances (ntt_eg_mat.hip, ntt_e31_mat.hip): the two a STARK
// prover's plans run on; nothing is instantiated for the others.
template <class E>
struct HasMat {
  static constexpr bool value = std::is_same_v<E, Eng64G> || std::is_same_v<E, Eng31>;
};
// A strip is at least 64 contiguous bytes per row (half a 128-byte line): 2^4 columns of 4 B, 2^3 of 8 B
template <class E>
__host__ __device__ constexpr int mat_min_strip_log() {
  return E::MEMW == 1 ? 4 : 3;
}
// ... which caps a matrix pass's radix at TILE >> that (2^9 on both engines)
template <class E>
__host__ __device__ constexpr int mat_max_radix_log() {
  return E::TILE_LOG - mat_min_strip_log<E>();
}
// One pass of a matrix transform: kind = KIND_COLUMN (two-level outer twiddles; a transform of one pass
// is a column pass whose columns are the strip's: its outer twiddles are w^0, its output natural) or
// KIND_FINAL; 3 <= logr <= mat_max_radix_log.  A.il = log2 of the strip's columns, A.mat_w, A.mat_ns set;
// grid = tiles x strips workgroups.  lde: the pass reads the first A.src_stride / E::MEMW rows only and
// multiplies row j by c^j at the load (A.tw_in / A.tw_in_hi, null: no shift); KIND_COLUMN only.
template <class E>
hipError_t launch_mat_pass(int kind, int logr, bool lde, const uint32_t* src, uint32_t* dst, const PassArgs<E>& A,
                           uint32_t grid, hipStream_t st);
// Matrix transforms of 2 and 4 rows, O(n^2): out[k][b] = sum_{j < n_in} in[j][b] c^j w^(jk), times n^-1
// when A.flags bit 0; A.tw_int holds w^e (e < n), A.tw_in / A.tw_in_hi the shift's tables or null.
// src == dst is allowed when n_in = n (each thread owns one column).
template <class E>
hipError_t launch_mat_naive(const uint32_t* src, uint32_t* dst, const PassArgs<E>& A, uint32_t n_in, hipStream_t st);

// ---- FRI fold of bit-reversed coset evaluations (ntt_fri_fold; k_fri_fold in ntt_fold_impl.hpp, instances
// in ntt_eg_fold.hip and ntt_e31_fold.hip: the HasMat engines).  Every constant of a call is wave-uniform
// and travels in the kernel arguments as a twiddle (E::Tw: a Shoup pair on Eng31, the value on Eng64G).
template <class E>
struct FoldArgs {
  typename E::Args F;   // p, p^-1, the checked build's status word
  const uint32_t* lo_s; // w_n^-e two-level tables of the plan: lo scaled by R_e, and
  const uint32_t* hi;   // the plain hi table (no n^-1)
  uint32_t lo_bits;
  uint32_t tab_shift;   // log_n - log_rows: w_N^-e = w_n^-(e << tab_shift)
  uint32_t log_m;       // log_rows - log_arity: the output has 2^log_m rows
  uint32_t vec;         // d_in and d_out are 16-byte aligned: vector loads and stores
  size_t src_words;     // 32-bit words of d_in (N d E::MEMW) and
  size_t dst_words;     // of d_out (M d E::MEMW)
  typename E::Tw cinv;      // c^-1
  typename E::Tw scale;     // 2^-log_arity
  typename E::Tw zeta[8];   // zeta^-e, zeta = w_N^M of order 2^log_arity, e < 2^(log_arity - 1)
  typename E::Tw beta[4][4];   // [s][j]: coefficient j of beta^(2^s), and
  typename E::Tw wbeta[4][4];  // of W beta^(2^s) (j >= 1)
};
// One launch: log_arity 1..4, ext_degree 1, 2 or 4; staged: the fibres reach their threads through LDS
// (16 B per lane at consecutive addresses; needs A.vec), else each thread loads its own fibre.
template <class E>
hipError_t launch_fri_fold(unsigned log_arity, unsigned ext_degree, bool staged, const uint32_t* in, uint32_t* out,
                           const FoldArgs<E>& A, hipStream_t st);

// ---- DEEP openings and quotients of a row-major coset evaluation matrix (ntt_deep_points, ntt_matrix_open,
// ntt_deep_quotient; kernels in ntt_deep_impl.hpp, instances in ntt_eg_deep.hip and ntt_e31_deep.hip: the HasMat
// engines).  Host scalars travel in the kernel arguments in the field's working form
// (fieldext.hpp xf: v 2^32 mod p on Eng31, the value on Eng64G).
template <class E>
using deep_val_t = std::conditional_t<std::is_same_v<E, Eng31>, uint32_t, uint64_t>;
template <class E>
using deep_k_t = std::conditional_t<std::is_same_v<E, Eng31>, xf::K31, xf::K64>;
// The shape decisions, shared by the launchers, the kernels and ntt_deep_info.  memw = E::MEMW.
struct DeepShape {
  static constexpr unsigned BT = 256;          // threads of every DEEP workgroup
  static constexpr unsigned RUN_WORDS = 16;    // points: each thread owns 64 B of consecutive output rows
  static constexpr unsigned UNROLL = 4;        // open: rows a thread has in flight
  static constexpr unsigned TARGET_WGS = 2048; // open: workgroups wanted (256 CUs x 8)
  static constexpr unsigned MAX_CHUNKS = 1024; // open: row chunks at most, whatever N
  static constexpr unsigned FIN_COLS = 16;     // open, second launch: columns per workgroup (x BT / 16 chunk lanes)
  static constexpr unsigned TAB_COLS = 512;    // quotient: columns of the scale alpha^j table held in LDS
  static constexpr unsigned SCR_TAB = 4;       // quotient scratch: V in elements [0, d), the table from element 4
  __host__ __device__ static constexpr unsigned ceil_log2(unsigned v) {
    unsigned l = 0;
    while (l < 32 && (1ull << l) < v) ++l;
    return l;
  }
  // open: log2 of a strip's columns: the width rounded up to a power of two, at least 64 B per row, at most a wave
  __host__ __device__ static constexpr unsigned strip_log(unsigned width, int memw) {
    const unsigned lo = memw == 1 ? 4u : 3u, l = ceil_log2(width);
    return l < lo ? lo : (l > 6 ? 6u : l);
  }
  __host__ __device__ static constexpr unsigned strips(unsigned width, int memw) {
    const unsigned l = strip_log(width, memw);
    return (unsigned)(((uint64_t)width + (1u << l) - 1) >> l);
  }
  // open: rows per chunk (a multiple of the rows one workgroup step covers); the chunks are ceil(N / that):
  // enough of them for TARGET_WGS workgroups, at most MAX_CHUNKS, none empty
  __host__ __device__ static constexpr uint64_t open_chunk_rows(unsigned width, unsigned log_rows, int memw) {
    const uint64_t n = 1ull << log_rows, step = (uint64_t)(BT >> strip_log(width, memw)) * UNROLL;
    const unsigned ns = strips(width, memw);
    uint64_t want = (TARGET_WGS + ns - 1) / ns;
    if (want > MAX_CHUNKS) want = MAX_CHUNKS;
    if (want < 1) want = 1;
    const uint64_t rows = (n + want - 1) / want;
    return (rows + step - 1) / step * step;
  }
  __host__ __device__ static constexpr unsigned open_chunks(unsigned width, unsigned log_rows, int memw) {
    const uint64_t n = 1ull << log_rows, cr = open_chunk_rows(width, log_rows, memw);
    return (unsigned)((n + cr - 1) / cr);
  }
  // quotient: log2 of the lanes that share a row.  Rows shorter than 64 B: one lane per row (a wave then reads
  // 64 consecutive rows, one contiguous run); otherwise a quarter of the largest power of two up to the width
  // (four columns a lane: the cross-lane sum is paid once per row, whatever the lane's share), 64 B of lanes at
  // least (16 on 4-byte elements, 8 on 8-byte ones), a wave at most
  __host__ __device__ static constexpr unsigned lanes_log(unsigned width, int memw) {
    if ((uint64_t)width * 4 * memw < 64) return 0;
    const unsigned lo = memw == 1 ? 4u : 3u;
    unsigned l = 0;
    while (l < 8 && (2u << l) <= width) ++l;
    l = l >= 2 ? l - 2 : 0;
    return l < lo ? lo : (l > 6 ? 6u : l);
  }
};
template <class E>
struct DeepArgs {
  typename E::Args F;  // p, p^-1, the checked build's status word
  deep_k_t<E> K;       // the field's constants with W
  uint32_t log_rows, width;
  uint32_t vec;    // the call's row buffers are 16-byte aligned and whole 16-byte words long: vector access
  uint32_t flags;  // quotient: NTT_DEEP_ACCUMULATE
  size_t mat_elems, inv_elems, val_elems, out_elems, scr_elems;  // checked build: elements of each buffer
  // points: x_i = c w_n^(sigma(i) << tab_shift) from the forward two-level tables (lo scaled by R_e, plain hi)
  const uint32_t* lo_s;
  const uint32_t* hi;
  uint32_t lo_bits, tab_shift, bitrev;
  typename E::Tw c;
  deep_val_t<E> z[4];  // z (points and the open's second launch)
  // open
  uint32_t strip_log, chunks;
  uint64_t chunk_rows;
  deep_val_t<E> k[4];  // (z^N - c^N) / (N c^N)
  // quotient
  uint32_t lanes_log;
  deep_val_t<E> alpha[4], scale[4];
};
// ext_degree 1, 2 or 4 in each.  points: d_inv [N][d].  open: mat [N][width], inv -> part (chunks (d + 1) width
// elements of plan scratch), then part -> values [width][d].  quotient: values -> scr (SCR_TAB + width d
// elements of plan scratch), then mat, inv, scr -> out [N][d].
template <class E>
hipError_t launch_deep_points(unsigned d, uint32_t* inv, const DeepArgs<E>& A, hipStream_t st);
template <class E>
hipError_t launch_deep_open(unsigned d, const uint32_t* mat, const uint32_t* inv, uint32_t* part, const DeepArgs<E>& A,
                            hipStream_t st);
template <class E>
hipError_t launch_deep_open_fin(unsigned d, const uint32_t* part, uint32_t* values, const DeepArgs<E>& A, hipStream_t st);
template <class E>
hipError_t launch_deep_qpro(unsigned d, const uint32_t* values, uint32_t* scr, const DeepArgs<E>& A, hipStream_t st);
template <class E>
hipError_t launch_deep_quotient(unsigned d, const uint32_t* mat, const uint32_t* inv, const uint32_t* scr, uint32_t* out,
                                const DeepArgs<E>& A, hipStream_t st);

// ---- Poseidon2 Merkle commitments and openings of a row-major matrix (ntt_poseidon2_permute, ntt_merkle_commit,
// ntt_merkle_open; kernels in ntt_hash_impl.hpp, instances in ntt_eg_hash.hip and ntt_e31_hash.hip: the HasMat
// engines).  The permutation and its constant table: poseidon2.hpp.
template <class E>
using hash_k_t = std::conditional_t<std::is_same_v<E, Eng31>, p2::P31, p2::P64>;
// The shape decisions, shared by the launchers, the kernels and ntt_merkle_info.  memw = E::MEMW.
struct MerkleShape {
  static constexpr unsigned BT = 256;       // threads of a leaf, layer, tail or permute workgroup: a row, parent or state each
  static constexpr unsigned TAIL_LOG = 9;   // the tail workgroup takes a layer of 2^9 nodes: BT parents in its first step
  static constexpr unsigned OPEN_BT = 64;   // open: one wave per query
  __host__ __device__ static constexpr unsigned width_t(int memw) { return memw == 1 ? 16u : 8u; }  // the permutation's width
  // leaf: columns of a row tile in LDS (128 B of a row: four absorptions), rows at a pitch of one element more
  __host__ __device__ static constexpr unsigned chunk_cols(int memw) { return memw == 1 ? 32u : 16u; }
  __host__ __device__ static constexpr unsigned tail_log(unsigned log_rows) { return log_rows < TAIL_LOG ? log_rows : TAIL_LOG; }
  // the leaf launch, one per layer above the tail, the tail
  __host__ __device__ static constexpr unsigned launches(unsigned log_rows) {
    return 1 + (log_rows - tail_log(log_rows)) + (log_rows ? 1u : 0u);
  }
  // first node of layer l of a tree over 2^log_rows leaves
  __host__ __device__ static constexpr uint64_t layer_start(unsigned log_rows, unsigned l) {
    return (2ull << log_rows) - ((2ull << log_rows) >> l);
  }
};
template <class E>
struct HashArgs {
  hash_k_t<E> K;   // the field's constants and the I/O form
  uint32_t* dbg;   // checked build: the plan's status word
  uint32_t rounds_f, rounds_p;
  uint32_t log_rows, width;
  uint32_t vec;       // permute: the states, leaf: the matrix is 16-byte aligned and a row is whole 16-byte words: vector access
  uint32_t vec_tree;  // the tree is 16-byte aligned
  uint32_t layers; // tail: the layers it runs
  uint32_t nq;
  uint64_t count;  // permute: states; layer: parents
  uint64_t in_node, out_node;  // layer and tail: first node of the children's layer and of the parents'
  size_t mat_elems, tree_elems, st_elems, idx_elems, rows_elems, paths_elems;  // checked build: elements of each buffer
};
// sbox_degree 3, 5 or 7 in each; tab: the plan's constant table (poseidon2.hpp Layout).
// permute: states [count][T] in place.  leaf: mat [N][width] -> layer 0 of tree.  layer: count parents at out_node
// from the children at in_node.  tail: `layers` layers from the 2^layers nodes at in_node, one workgroup.
// open: rows (null: none) and paths of nq queries.
template <class E>
hipError_t launch_p2_permute(unsigned sbox_degree, uint32_t* states, const deep_val_t<E>* tab, const HashArgs<E>& A,
                             hipStream_t st);
template <class E>
hipError_t launch_merkle_leaf(unsigned sbox_degree, const uint32_t* mat, uint32_t* tree, const deep_val_t<E>* tab,
                              const HashArgs<E>& A, hipStream_t st);
template <class E>
hipError_t launch_merkle_layer(unsigned sbox_degree, uint32_t* tree, const deep_val_t<E>* tab, const HashArgs<E>& A,
                               hipStream_t st);
template <class E>
hipError_t launch_merkle_tail(unsigned sbox_degree, uint32_t* tree, const deep_val_t<E>* tab, const HashArgs<E>& A,
                              hipStream_t st);
template <class E>
hipError_t launch_merkle_open(const uint32_t* mat, const uint32_t* tree, const uint32_t* index, uint32_t* rows,
                              uint32_t* paths, const HashArgs<E>& A, hipStream_t st);

// ---- batch inversion and running sums / products down the columns of a row-major matrix (ntt_batch_inverse,
// ntt_matrix_scan; kernels in ntt_scan_impl.hpp, instances in ntt_eg_scan.hip and ntt_e31_scan.hip: the HasMat
// engines).  The shape decisions: scan_shape.hpp (ScanShape, InvShape).
template <class E>
struct ScanArgs {
  deep_k_t<E> K;          // the field's constants with W
  uint32_t* dbg;          // checked build: the plan's status word
  deep_val_t<E> ident;    // coordinate 0 of the operation's identity in the plan's I/O form
  deep_val_t<E> r2;       // conv: 2^64 mod p, which brings a canonical value to the working form by one product
  deep_val_t<E> rinv;     // conv: 2^-32 mod p, which brings the inverse of a run's product to the canonical form
  uint32_t conv;          // 4-byte canonical plans: one operand of every product goes to the working form first
  uint32_t vec;           // the caller's buffers are 16-byte aligned and whole 16-byte words long: vector access
  uint32_t excl;          // scan: NTT_SCAN_EXCLUSIVE
  uint32_t mid_cols, mid_run;  // scan, second launch (ScanShape::mid_cols, mid_run)
  ScanShape S;            // scan: the shape
  uint64_t rows;          // scan
  uint64_t count;         // inverse: elements
  size_t io_elems, buf_elems, tot_elems;  // checked build: base elements of d_in / d_out, the plan's buffer, d_totals
};
// inverse: d_in, d_out [count][d], form < InvShape::FORMS.  scan: the three launches; prod: the ring product of
// degree-d elements, else the sum, whose d is 1 (the caller folds the degree into the columns).  reduce: in ->
// buf [chunk][column][d]; mid: buf -> its exclusive scan in place, and totals (null: none); chunk: in, buf -> out,
// and totals when the shape has one chunk (buf is then not read).
template <class E>
hipError_t launch_batch_inverse(unsigned d, unsigned form, const uint32_t* in, uint32_t* out, const ScanArgs<E>& A,
                                hipStream_t st);
template <class E>
hipError_t launch_scan_reduce(unsigned d, bool prod, const uint32_t* in, uint32_t* buf, const ScanArgs<E>& A, hipStream_t st);
template <class E>
hipError_t launch_scan_mid(unsigned d, bool prod, uint32_t* buf, uint32_t* totals, const ScanArgs<E>& A, hipStream_t st);
template <class E>
hipError_t launch_scan_chunk(unsigned d, bool prod, const uint32_t* in, uint32_t* out, const uint32_t* buf, uint32_t* totals,
                             const ScanArgs<E>& A, hipStream_t st);

template <class E>
hipError_t launch_build_tw(uint32_t* out, size_t count, uint32_t log_r, uint32_t log_t, uint32_t log_m,
                           const uint32_t* lo, const uint32_t* hi, uint32_t lo_bits, const typename E::Args& F,
                           hipStream_t st, const uint32_t* clo = nullptr, const uint32_t* chi = nullptr);
// The same table as Shoup pairs (w, floor(w B / p)) in the engine's twiddle format (E::TW words per
// entry); pinvB = p^-1 mod B (E::W limbs, device memory).  E::SHOUP_OUTER engines only.
template <class E>
hipError_t launch_build_tw_sh(uint32_t* out, size_t count, uint32_t log_r, uint32_t log_t, uint32_t log_m,
                              const uint32_t* lo, const uint32_t* hi, uint32_t lo_bits, const typename E::Args& F,
                              const uint32_t* pinvB, hipStream_t st);
// NTT_PLAN_NAIVE: the power table w_n^i R_e (i < count, E::TABW words per entry) and one radix-2
// DIT round (stride 2^log_s) of the reference's `naive` rival over a bit-reversed vector
template <class E>
hipError_t launch_build_pow(uint32_t* out, size_t count, const uint32_t* lo, const uint32_t* hi, uint32_t lo_bits,
                            const typename E::Args& F, hipStream_t st);
// NTT_PLAN_NO_SWAP: one radix-2 Stockham round (stride 2^log_s) of the reference's `naive_no_swap`
template <class E>
hipError_t launch_noswap_round(const uint32_t* src, uint32_t* dst, uint32_t log_n, uint32_t log_s, const uint32_t* pw,
                               const typename E::Args& F, hipStream_t st);
// The reference's bealto.com radix-2^deg Stockham family (ntt.h NTT_PLAN_BELLPERSON,
// NTT_PLAN_IMPROVED_V1..V4): one round of 2^deg-point groups, 2^log_g groups per workgroup
// (A: tw_lo / tw_hi / lo_bits two-level tables for the input twiddles, tw_int the pq table of
// w_{2^max_deg}^j Shoup pairs, j < 2^(max_deg - 1)).  Engines with HasStockham only.
enum : int { BEALTO_BELLPERSON = 0, BEALTO_V1 = 1, BEALTO_V2 = 2, BEALTO_V3 = 3, BEALTO_V4 = 4 };
struct BealtoArgs {
  uint32_t log_n, lgp, deg, log_g, max_deg;
};
template <class E>
hipError_t launch_bealto(int variant, const uint32_t* src, uint32_t* dst, const PassArgs<E>& A, const BealtoArgs& B,
                         hipStream_t st);
template <class E>
hipError_t launch_naive_round(const uint32_t* src, uint32_t* dst, uint32_t log_n, uint32_t log_s, const uint32_t* pw,
                              const typename E::Args& F, hipStream_t st);
// dst[i] = src[digit reversal of i] over 2^log_n elements of E::MEMW words, digits of digits[q] bits
// in pass order (the GZKP rival's `rearrange`); nd = 0: the bit reversal (the naive rival's)
template <class E>
hipError_t launch_bitrev(const uint32_t* src, uint32_t* dst, uint32_t log_n, const uint32_t* digits, uint32_t nd,
                         hipStream_t st);
// scale (E::TW words, a twiddle) or null: every entry is also multiplied by it
template <class E>
hipError_t launch_build_fs_tw(uint32_t* out, uint32_t log_rows, uint32_t log_cols, uint64_t row0, uint64_t col0,
                              uint32_t log_n, const uint32_t* lo, const uint32_t* hi, uint32_t lo_bits,
                              const typename E::Args& F, hipStream_t st, const uint32_t* scale = nullptr);
template <class E>
hipError_t launch_naive(const uint32_t* src, uint32_t* dst, const PassArgs<E>& A, uint32_t batch, hipStream_t st);
// Fill local element i with the synthetic value of global index
// j = row0 + (i >> log_inner) + ((i mod 2^log_inner) << log_stride)   (log_inner = 64: j = i).
template <class E>
hipError_t launch_fill(int kind, uint32_t* dst, size_t n, uint64_t seed, uint32_t nrand, uint32_t top_bits,
                       uint64_t row0, uint32_t log_inner, uint32_t log_stride, hipStream_t st);
template <class E>
hipError_t launch_twiddle_pack(const uint32_t* src, uint32_t* dst, uint32_t log_rows, uint32_t log_len,
                               uint32_t log_bw, uint64_t row0, uint32_t log_n, const uint32_t* lo, const uint32_t* hi,
                               uint32_t lo_bits, const typename E::Args& F, uint64_t peer_stride, hipStream_t st);
template <class E>
hipError_t launch_transpose(const uint32_t* src, uint32_t* dst, uint32_t log_rows, uint32_t log_cols,
                            uint32_t log_blk_rows, uint64_t blk_stride, hipStream_t st);
// In-place digit reversal of a palindromic schedule (NTT_PLAN_IN_PLACE): position
// (k1, mid, kn) = k1 2^(log_n - R) + mid 2^R + kn  <->  (kn, midrev, k1), tiles of 2^tb_log x 2^tb_log.
struct DrevArgs {
  uint32_t log_n, R, tb_log, nmid;
  uint32_t diag;         // workgroup -> tile-pair order: 1 diagonal, 0 row-major
  uint32_t mid_bits[4];  // middle digit widths of `mid`, least significant first (PassArgs::mid_bits)
  uint32_t mid_off[4];   // their bit offsets in midrev (PassArgs::mid_off)
  size_t batch_stride;   // 32-bit words between batched transforms
  uint64_t unit0;        // first tile pair of this launch (launch_digitrev_swap chunks the grid)
};
template <class E>
hipError_t launch_digitrev_swap(uint32_t* data, const DrevArgs& A, uint32_t batch, hipStream_t st);
// data[j] *= c^j (coset / low-degree-extension scale), c^j = lo_s[j & mask] * hi[j >> lo_bits]
template <class E>
hipError_t launch_scale_pow(uint32_t* data, uint32_t log_n, uint32_t batch, const uint32_t* lo_s, const uint32_t* hi,
                            uint32_t lo_bits, const typename E::Args& F, hipStream_t st);
// c = a * b (canonical in/out): mont(mont(a, b), R^2) with r2 in the engine table format; in_map:
// element j of a and b is read at (*in_map)(j, 0) (a four-step piece of the column layout)
template <class E>
hipError_t launch_pointwise(const uint32_t* a, const uint32_t* b, uint32_t* c, size_t n, const typename E::Args& F,
                            const uint32_t* d_r2, hipStream_t st, const FsMap* in_map = nullptr);

}  // namespace ntt
