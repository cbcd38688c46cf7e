// Batch inversion and running sums / products down the columns of a row-major matrix (ntt_batch_inverse,
// ntt_matrix_scan).  Included by ntt_eg_scan.hip and ntt_e31_scan.hip alone.
//
// Forms.  The data are in the plan's I/O form.  A product is fieldext.hpp's xf::mul, which on the 4-byte field is
// the Montgomery product a b 2^-32: of two Montgomery-form values it is the Montgomery form of the product; on
// canonical 4-byte plans (A.conv) one operand goes to the working form first (ScanOp::work: one product by
// 2^64 mod p per coordinate).  Goldilocks has one form.
//
//   k_batch_inv  A thread owns a run of RW / (D E::MEMW) consecutive elements (RW 32-bit words); the workgroup's
//                words reach LDS with lane l on 16 B at base + 16 l, each thread's run at a pitch of RW + 4
//                words.  The thread multiplies up its run (a zero element counts as one), keeping the prefix
//                products in registers, inverts the last one (xf::inv), and walks back re-reading its elements
//                from LDS and writing the inverses over them (zero where the element was zero); the words
//                leave as they came.  The arithmetic treats every word as a Montgomery representative, so a
//                run's inverse comes out as 2^64 / v: on canonical plans it is multiplied by 2^-32 mod p once
//                per run, which scales every output of the run.  WAVE: the threads' run products meet in a
//                prefix and a suffix product scan across the wave (shuffles) and the wave's product is inverted
//                once; a thread's own inverse is that times the product of the later lanes' runs.
//   k_scan       A workgroup is rps thread rows x strip_cols columns (thread (r, c) = r strip_cols + c) and owns a
//                strip of columns x a chunk of rows, which it walks in tiles of rps RUN rows: thread (r, c) holds
//                rows [r RUN, (r + 1) RUN) of column c of the tile in registers, chains them, and the threads of
//                a column meet in an LDS scan (col_scan); the carry of the tiles before stays in registers.
//                REDUCE: the chunk's aggregate per column into the plan's buffer at [chunk][column].  Else: the
//                tile's scan from the chunk's prefix (the buffer after k_scan_mid; the identity when the shape has
//                one chunk, and then the totals are stored here).  A thread stores only what its workgroup has
//                loaded before, so d_out may be d_in.
//                NARROW (rows shorter than 64 B): the strip is the whole row and a tile one contiguous byte range,
//                which reaches LDS and leaves it with lane l on 16 B at base + 16 l; a thread row's words sit at
//                a pitch of 4 words more than their count.
//   k_scan_mid   mid_cols columns x BT / mid_cols chunk lanes per workgroup: a lane sums a run of consecutive
//                chunks, the lanes of a column meet in col_scan, and the lane writes the exclusive prefixes back
//                over its chunks; lane 0 stores the column's total.
// No atomics and no wait of one workgroup on another: the same bits every run.
// Checked build: an index outside its buffer sets 0x100 and goes to element 0, a non-canonical input element
// 0x200, a non-canonical output 0x800.
#pragma once
#include <type_traits>

#include "fieldext.hpp"
#include "ntt_kernels.hpp"

namespace ntt {

// checked build: `count` words from word index `at` against a buffer of `total` words
template <class E>
__device__ __forceinline__ size_t scan_idx(size_t at, [[maybe_unused]] size_t count, [[maybe_unused]] size_t total,
                                           [[maybe_unused]] const ScanArgs<E>& A) {
#if NTT_DEBUG_CHECKS
  if (at + count > total) {
    ntt_dbg_flag(A.dbg, NTT_DBG_BOUNDS);
    return 0;
  }
#endif
  return at;
}
template <class E>
__device__ __forceinline__ void scan_check([[maybe_unused]] deep_val_t<E> v, [[maybe_unused]] uint32_t bit,
                                           [[maybe_unused]] const ScanArgs<E>& A) {
#if NTT_DEBUG_CHECKS
  if (!xf::canonical(v, A.K)) ntt_dbg_flag(A.dbg, bit);
#endif
}
// one element of D coefficients from / to N = D E::MEMW words
template <class E, int D>
__device__ __forceinline__ void scan_unpack(deep_val_t<E> (&x)[D], const uint32_t (&w)[D * E::MEMW]) {
#pragma unroll
  for (int j = 0; j < D; ++j) {
    if constexpr (E::MEMW == 1)
      x[j] = w[j];
    else
      x[j] = ((uint64_t)w[2 * j + 1] << 32) | w[2 * j];
  }
}
template <class E, int D>
__device__ __forceinline__ void scan_pack(uint32_t (&w)[D * E::MEMW], const deep_val_t<E> (&x)[D]) {
#pragma unroll
  for (int j = 0; j < D; ++j) {
    if constexpr (E::MEMW == 1) {
      w[j] = x[j];
    } else {
      w[2 * j] = (uint32_t)x[j];
      w[2 * j + 1] = (uint32_t)(x[j] >> 32);
    }
  }
}
// N words at word index `at` (a multiple of N): 16-byte accesses when vec, 8-byte ones where the words are
// 8-byte aligned (elements of 8 bytes, or vec)
template <class E, int N>
__device__ __forceinline__ void scan_ldw(uint32_t (&w)[N], const uint32_t* base, size_t at, bool vec) {
  if (vec && N % 4 == 0) {
    const uint4* p4 = reinterpret_cast<const uint4*>(base + at);
#pragma unroll
    for (int q = 0; q < N / 4; ++q) {
      const uint4 v = p4[q];
      w[4 * q] = v.x, w[4 * q + 1] = v.y, w[4 * q + 2] = v.z, w[4 * q + 3] = v.w;
    }
  } else if (N % 2 == 0 && (E::MEMW == 2 || vec)) {
    const uint2* p2 = reinterpret_cast<const uint2*>(base + at);
#pragma unroll
    for (int q = 0; q < N / 2; ++q) {
      const uint2 v = p2[q];
      w[2 * q] = v.x, w[2 * q + 1] = v.y;
    }
  } else {
#pragma unroll
    for (int q = 0; q < N; ++q) w[q] = base[at + q];
  }
}
template <class E, int N>
__device__ __forceinline__ void scan_stw(uint32_t* base, size_t at, const uint32_t (&w)[N], bool vec) {
  if (vec && N % 4 == 0) {
    uint4* p4 = reinterpret_cast<uint4*>(base + at);
#pragma unroll
    for (int q = 0; q < N / 4; ++q) p4[q] = make_uint4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
  } else if (N % 2 == 0 && (E::MEMW == 2 || vec)) {
    uint2* p2 = reinterpret_cast<uint2*>(base + at);
#pragma unroll
    for (int q = 0; q < N / 2; ++q) p2[q] = make_uint2(w[2 * q], w[2 * q + 1]);
  } else {
#pragma unroll
    for (int q = 0; q < N; ++q) base[at + q] = w[q];
  }
}
// an element at element index e of a buffer of `total` words; the checked build looks at the index and the values
template <class E, int D>
__device__ __forceinline__ void scan_ld_elem(deep_val_t<E> (&x)[D], const uint32_t* base, size_t e, size_t total, bool vec,
                                             const ScanArgs<E>& A) {
  constexpr int DW = D * E::MEMW;
  uint32_t w[DW];
  scan_ldw<E, DW>(w, base, scan_idx<E>(e * DW, DW, total, A), vec);
  scan_unpack<E, D>(x, w);
#pragma unroll
  for (int j = 0; j < D; ++j) scan_check<E>(x[j], NTT_DBG_INPUT, A);
}
template <class E, int D>
__device__ __forceinline__ void scan_st_elem(uint32_t* base, size_t e, size_t total, const deep_val_t<E> (&x)[D], bool vec,
                                             const ScanArgs<E>& A) {
  constexpr int DW = D * E::MEMW;
  uint32_t w[DW];
#pragma unroll
  for (int j = 0; j < D; ++j) scan_check<E>(x[j], NTT_DBG_OUTPUT, A);
  scan_pack<E, D>(w, x);
  scan_stw<E, DW>(base, scan_idx<E>(e * DW, DW, total, A), w, vec);
}

// The workgroup's words [gb, gb + nw) of a buffer of `total` words <-> LDS, word f of them at lds[(f / grp) pitch +
// f % grp]: lane l on 16 B at base + 16 l when vec (grp, pitch and gb multiples of 4, total too), else word by word
template <class E>
__device__ __forceinline__ void scan_stage_in(uint32_t* lds, const uint32_t* src, size_t gb, uint32_t nw, uint32_t grp,
                                              uint32_t pitch, size_t total, const ScanArgs<E>& A) {
  const uint32_t tid = threadIdx.x;
  if (A.vec) {
    const uint4* s4 = reinterpret_cast<const uint4*>(src);
    uint4* l4 = reinterpret_cast<uint4*>(lds);
    for (uint32_t f = 4 * tid; f < nw; f += 4 * ScanShape::BT) l4[((f / grp) * pitch + f % grp) / 4] = s4[scan_idx<E>(gb + f, 4, total, A) / 4];
  } else {
    for (uint32_t f = tid; f < nw; f += ScanShape::BT) lds[(f / grp) * pitch + f % grp] = src[scan_idx<E>(gb + f, 1, total, A)];
  }
}
template <class E>
__device__ __forceinline__ void scan_stage_out(uint32_t* dst, const uint32_t* lds, size_t gb, uint32_t nw, uint32_t grp,
                                               uint32_t pitch, size_t total, const ScanArgs<E>& A) {
  const uint32_t tid = threadIdx.x;
  if (A.vec) {
    uint4* d4 = reinterpret_cast<uint4*>(dst);
    const uint4* l4 = reinterpret_cast<const uint4*>(lds);
    for (uint32_t f = 4 * tid; f < nw; f += 4 * ScanShape::BT) d4[scan_idx<E>(gb + f, 4, total, A) / 4] = l4[((f / grp) * pitch + f % grp) / 4];
  } else {
    for (uint32_t f = tid; f < nw; f += ScanShape::BT) dst[scan_idx<E>(gb + f, 1, total, A)] = lds[(f / grp) * pitch + f % grp];
  }
}

// The operation of a scan on elements of D coefficients: the field sum, or the ring product
template <class E, int D, bool PROD>
struct ScanOp {
  using V = deep_val_t<E>;
  // b in the I/O form -> the form op takes its right operand in
  static __device__ __forceinline__ void work(V (&o)[D], const V (&b)[D], const ScanArgs<E>& A) {
#pragma unroll
    for (int j = 0; j < D; ++j) o[j] = b[j];
    if constexpr (PROD && E::MEMW == 1) {
      if (A.conv) {
#pragma unroll
        for (int j = 0; j < D; ++j) o[j] = xf::mul(b[j], A.r2, A.K);
      }
    }
  }
  // a op bw in a's form
  static __device__ __forceinline__ void op(V (&c)[D], const V (&a)[D], const V (&bw)[D], const ScanArgs<E>& A) {
    if constexpr (PROD)
      xf::mul<D>(c, a, bw, A.K);
    else
      xf::add<D>(c, a, bw, A.K);
  }
  static __device__ __forceinline__ void ident(V (&o)[D], const ScanArgs<E>& A) {  // the I/O form
#pragma unroll
    for (int j = 0; j < D; ++j) o[j] = j ? V(0) : A.ident;
  }
  static __device__ __forceinline__ void ident_work(V (&o)[D], const ScanArgs<E>& A) {  // as work() gives it
#pragma unroll
    for (int j = 0; j < D; ++j) o[j] = (PROD && j == 0) ? A.K.one : V(0);
  }
};

// The threads (r, c) = r cs + c, r < nr, of the workgroup hold x: before <- op of x over the thread rows below r of
// column c (the identity at r = 0), total <- over all of them.  Every thread of the workgroup calls it.
template <class E, int D, bool PROD>
__device__ __forceinline__ void col_scan(deep_val_t<E> (&before)[D], deep_val_t<E> (&total)[D], const deep_val_t<E> (&x)[D],
                                         deep_val_t<E> (*sc)[ScanShape::BT], uint32_t r, uint32_t cs, uint32_t nr,
                                         const ScanArgs<E>& A) {
  using V = deep_val_t<E>;
  using Op = ScanOp<E, D, PROD>;
  const uint32_t tid = threadIdx.x;
  V cur[D];
#pragma unroll
  for (int j = 0; j < D; ++j) cur[j] = x[j], sc[j][tid] = x[j];
  for (uint32_t off = 1; off < nr; off <<= 1) {
    __syncthreads();
    const bool has = r >= off && r < nr;
    V o[D];
    if (has) {
#pragma unroll
      for (int j = 0; j < D; ++j) o[j] = sc[j][tid - off * cs];
    }
    __syncthreads();
    if (has) {
      V ow[D];
      Op::work(ow, o, A);
      Op::op(cur, cur, ow, A);
#pragma unroll
      for (int j = 0; j < D; ++j) sc[j][tid] = cur[j];
    }
  }
  __syncthreads();
  Op::ident(before, A);
  if (r > 0 && r < nr) {
#pragma unroll
    for (int j = 0; j < D; ++j) before[j] = sc[j][tid - cs];
  }
#pragma unroll
  for (int j = 0; j < D; ++j) total[j] = sc[j][(nr - 1) * cs + tid % cs];
  __syncthreads();
}

// ------------------------------------------------------------------------------ scan
template <class E, int D, bool PROD, bool REDUCE, bool NARROW>
__global__ __launch_bounds__(ScanShape::BT) void k_scan(const uint32_t* in, uint32_t* out, uint32_t* buf, uint32_t* totals,
                                                        const ScanArgs<E> A) {
  using V = deep_val_t<E>;
  using Op = ScanOp<E, D, PROD>;
  constexpr uint32_t BT = ScanShape::BT, DW = D * E::MEMW, RUN = ScanShape::RUN_WORDS / DW;
  __shared__ V sc[D][BT];
  __shared__ uint4 stage4[NARROW ? ScanShape::MAX_LDS_WORDS / 4 : 1];
  uint32_t* stage = reinterpret_cast<uint32_t*>(stage4);
  const uint32_t tid = threadIdx.x, cs = A.S.strip_cols, rps = A.S.rps, ns = A.S.strips, cols = A.S.cols;
  const uint32_t strip = blockIdx.x % ns, chunk = blockIdx.x / ns;
  const uint32_t c = tid % cs, r = tid / cs;
  const size_t col = (size_t)strip * cs + c;
  const bool live = r < rps && col < cols;
  const uint64_t r0 = (uint64_t)chunk * A.S.chunk_rows;
  const uint64_t r1 = r0 + A.S.chunk_rows < A.rows ? r0 + A.S.chunk_rows : A.rows;
  const size_t io_words = A.io_elems * E::MEMW, buf_words = A.buf_elems * E::MEMW, tot_words = A.tot_elems * E::MEMW;
  const bool vec = A.vec != 0;
  const uint32_t grp = ScanShape::RUN_WORDS * cs, pitch = grp + ScanShape::LDS_PAD;  // NARROW: a thread row's words in LDS
  const size_t rw = (size_t)cols * DW;                                               // words of a matrix row

  V carry[D];
  Op::ident(carry, A);
  if (!REDUCE && live && A.S.chunks > 1) scan_ld_elem<E, D>(carry, buf, (size_t)chunk * cols + col, buf_words, true, A);

  for (uint64_t t0 = r0; t0 < r1; t0 += A.S.tile_rows) {
    const uint64_t left = r1 - t0;
    const uint32_t trows = left < A.S.tile_rows ? (uint32_t)left : A.S.tile_rows;
    if constexpr (NARROW) {
      scan_stage_in<E>(stage, in, (size_t)t0 * rw, (uint32_t)(trows * rw), grp, pitch, io_words, A);
      __syncthreads();
    }
    V a[RUN][D];
#pragma unroll
    for (uint32_t k = 0; k < RUN; ++k) {
      const uint32_t tr = r * RUN + k;
      if (k == 0 || !PROD)
        Op::ident(a[k], A);
      else
        Op::ident_work(a[k], A);
      if (live && tr < trows) {
        if constexpr (NARROW) {
          uint32_t w[DW];
#pragma unroll
          for (uint32_t q = 0; q < DW; ++q) w[q] = stage[r * pitch + (k * cs + c) * DW + q];
          scan_unpack<E, D>(a[k], w);
#pragma unroll
          for (int j = 0; j < D; ++j) scan_check<E>(a[k][j], NTT_DBG_INPUT, A);
        } else {
          scan_ld_elem<E, D>(a[k], in, (size_t)(t0 + tr) * cols + col, io_words, vec, A);
        }
        if (k) Op::work(a[k], a[k], A);
      }
    }
    // a[k] <- a[0] op .. op a[k]
#pragma unroll
    for (uint32_t k = 1; k < RUN; ++k) Op::op(a[k], a[k - 1], a[k], A);
    if constexpr (REDUCE) {
      V w[D];
      Op::work(w, a[RUN - 1], A);
      Op::op(carry, carry, w, A);
    } else {
      V before[D], total[D], base[D], bw[D], w[D];
      col_scan<E, D, PROD>(before, total, a[RUN - 1], sc, r, cs, rps, A);
      Op::work(w, before, A);
      Op::op(base, carry, w, A);
      Op::work(bw, base, A);
      Op::work(w, total, A);
      Op::op(carry, carry, w, A);
#pragma unroll
      for (int k = 0; k < (int)RUN; ++k) {
        V o[D];
        if (A.excl) {
          if (k == 0) {
#pragma unroll
            for (int j = 0; j < D; ++j) o[j] = base[j];
          } else {
            Op::op(o, a[k - 1], bw, A);
          }
        } else {
          Op::op(o, a[k], bw, A);
        }
        const uint32_t tr = r * RUN + k;
        if (live && tr < trows) {
          if constexpr (NARROW) {
            uint32_t ow[DW];
#pragma unroll
            for (int j = 0; j < D; ++j) scan_check<E>(o[j], NTT_DBG_OUTPUT, A);
            scan_pack<E, D>(ow, o);
#pragma unroll
            for (uint32_t q = 0; q < DW; ++q) stage[r * pitch + (k * cs + c) * DW + q] = ow[q];
          } else {
            scan_st_elem<E, D>(out, (size_t)(t0 + tr) * cols + col, io_words, o, vec, A);
          }
        }
      }
      if constexpr (NARROW) {
        __syncthreads();
        scan_stage_out<E>(out, stage, (size_t)t0 * rw, (uint32_t)(trows * rw), grp, pitch, io_words, A);
      }
    }
    if constexpr (NARROW) __syncthreads();  // the next tile's words replace these
  }
  if constexpr (REDUCE) {
    V before[D], total[D];
    col_scan<E, D, PROD>(before, total, carry, sc, r, cs, rps, A);
    if (r == 0 && live) scan_st_elem<E, D>(buf, (size_t)chunk * cols + col, buf_words, total, true, A);
  } else {
    if (A.S.chunks == 1 && totals && r == 0 && live) scan_st_elem<E, D>(totals, col, tot_words, carry, vec, A);
  }
}

template <class E, int D, bool PROD>
__global__ __launch_bounds__(ScanShape::BT) void k_scan_mid(uint32_t* buf, uint32_t* totals, const ScanArgs<E> A) {
  using V = deep_val_t<E>;
  using Op = ScanOp<E, D, PROD>;
  constexpr uint32_t BT = ScanShape::BT;
  __shared__ V sc[D][BT];
  const uint32_t tid = threadIdx.x, mc = A.mid_cols, lanes = BT / mc, cols = A.S.cols, chunks = A.S.chunks;
  const uint32_t c = tid % mc, l = tid / mc;
  const size_t col = (size_t)blockIdx.x * mc + c;
  const bool live = col < cols;
  const uint32_t ch0 = l * A.mid_run < chunks ? l * A.mid_run : chunks;
  const uint32_t ch1 = ch0 + A.mid_run < chunks ? ch0 + A.mid_run : chunks;
  const size_t buf_words = A.buf_elems * E::MEMW, tot_words = A.tot_elems * E::MEMW;
  V acc[D], before[D], total[D];
  Op::ident(acc, A);
  if (live) {
    for (uint32_t ch = ch0; ch < ch1; ++ch) {
      V v[D];
      scan_ld_elem<E, D>(v, buf, (size_t)ch * cols + col, buf_words, true, A);
      Op::work(v, v, A);
      Op::op(acc, acc, v, A);
    }
  }
  col_scan<E, D, PROD>(before, total, acc, sc, l, mc, lanes, A);
  if (!live) return;
  for (uint32_t ch = ch0; ch < ch1; ++ch) {
    V v[D];
    scan_ld_elem<E, D>(v, buf, (size_t)ch * cols + col, buf_words, true, A);
    scan_st_elem<E, D>(buf, (size_t)ch * cols + col, buf_words, before, true, A);
    Op::work(v, v, A);
    Op::op(before, before, v, A);
  }
  if (l == 0 && totals) scan_st_elem<E, D>(totals, col, tot_words, total, A.vec != 0, A);
}

// ------------------------------------------------------------------------------ batch inverse
template <class E, int D, int RW, bool WAVE>
__global__ __launch_bounds__(InvShape::BT) void k_batch_inv(const uint32_t* in, uint32_t* out, const ScanArgs<E> A) {
  using V = deep_val_t<E>;
  constexpr uint32_t BT = InvShape::BT, DW = D * E::MEMW, R = RW / DW, STRIDE = RW + 4;
  __shared__ uint4 lds4[BT * STRIDE / 4];
  uint32_t* lds = reinterpret_cast<uint32_t*>(lds4);
  const uint32_t tid = threadIdx.x;
  const size_t total = (size_t)A.count * DW, gb = (size_t)blockIdx.x * BT * RW;
  const uint32_t nw = total - gb < (size_t)BT * RW ? (uint32_t)(total - gb) : BT * RW;
  scan_stage_in<E>(lds, in, gb, nw, RW, STRIDE, A.io_elems * E::MEMW, A);
  for (uint32_t f = nw + tid; f < BT * RW; f += BT) lds[(f / RW) * STRIDE + f % RW] = 0;  // past the end: zeros
  __syncthreads();
  uint32_t* my = lds + tid * STRIDE;

  // the element at position k of the run, one where it is zero (past the end too); zero: it was zero
  auto element = [&](V(&x)[D], uint32_t k, bool& zero) {
    uint32_t w[DW];
#pragma unroll
    for (uint32_t q = 0; q < DW; ++q) w[q] = my[k * DW + q];
    scan_unpack<E, D>(x, w);
    zero = true;
#pragma unroll
    for (int j = 0; j < D; ++j) {
      scan_check<E>(x[j], NTT_DBG_INPUT, A);
      zero = zero && x[j] == 0;
    }
    if (zero) x[0] = A.K.one;
  };

  V pre[R][D];
  {
    bool z;
    element(pre[0], 0, z);
#pragma unroll
    for (uint32_t k = 1; k < R; ++k) {
      V x[D];
      element(x, k, z);
      xf::mul<D>(pre[k], pre[k - 1], x, A.K);
    }
  }
  V t[D];
  if constexpr (WAVE) {
    // up <- the product of the runs of lanes <= this one, down <- of the lanes after it
    V up[D], down[D], one[D];
    const uint32_t lane = tid & 63;
#pragma unroll
    for (int j = 0; j < D; ++j) up[j] = down[j] = pre[R - 1][j], one[j] = j ? V(0) : A.K.one;
#pragma unroll
    for (uint32_t off = 1; off < 64; off <<= 1) {
      V o[D], q[D];
#pragma unroll
      for (int j = 0; j < D; ++j) o[j] = (V)__shfl_up(up[j], off), q[j] = (V)__shfl_down(down[j], off);
      if (lane < off) {
#pragma unroll
        for (int j = 0; j < D; ++j) o[j] = one[j];
      }
      if (lane + off > 63) {
#pragma unroll
        for (int j = 0; j < D; ++j) q[j] = one[j];
      }
      xf::mul<D>(up, up, o, A.K);
      xf::mul<D>(down, down, q, A.K);
    }
    V all[D], after[D];
#pragma unroll
    for (int j = 0; j < D; ++j) {
      all[j] = (V)__shfl(up[j], 63);
      after[j] = (V)__shfl_down(down[j], 1);
      if (lane == 63) after[j] = one[j];
    }
    xf::inv<D>(t, all, A.K);
    // 1 / (runs up to this lane) = 1 / all x (runs after it); 1 / (this run) = that x (runs before it)
    V before[D];
#pragma unroll
    for (int j = 0; j < D; ++j) {
      before[j] = (V)__shfl_up(up[j], 1);
      if (lane == 0) before[j] = one[j];
    }
    xf::mul<D>(t, t, after, A.K);
    xf::mul<D>(t, t, before, A.K);
  } else {
    xf::inv<D>(t, pre[R - 1], A.K);
  }
  if constexpr (E::MEMW == 1) {
    if (A.conv) {
#pragma unroll
      for (int j = 0; j < D; ++j) t[j] = xf::mul(t[j], A.rinv, A.K);
    }
  }
#pragma unroll
  for (int k = R - 1; k >= 0; --k) {
    V x[D], res[D];
    bool zero;
    element(x, k, zero);
    if (k > 0) {
      xf::mul<D>(res, t, pre[k - 1], A.K);
      xf::mul<D>(t, t, x, A.K);
    } else {
#pragma unroll
      for (int j = 0; j < D; ++j) res[j] = t[j];
    }
    uint32_t w[DW];
#pragma unroll
    for (int j = 0; j < D; ++j) {
      if (zero) res[j] = 0;
      scan_check<E>(res[j], NTT_DBG_OUTPUT, A);
    }
    scan_pack<E, D>(w, res);
#pragma unroll
    for (uint32_t q = 0; q < DW; ++q) my[k * DW + q] = w[q];
  }
  __syncthreads();
  scan_stage_out<E>(out, lds, gb, nw, RW, STRIDE, A.io_elems * E::MEMW, A);
}

// ------------------------------------------------------------------------------ launchers
#define NTT_SCAN_SWITCH_D(d, CALL)        \
  switch (d) {                            \
    case 1: CALL(1); break;               \
    case 2: CALL(2); break;               \
    case 4: CALL(4); break;               \
    default: return hipErrorInvalidValue; \
  }

template <class E>
hipError_t launch_batch_inverse(unsigned d, unsigned form, const uint32_t* in, uint32_t* out, const ScanArgs<E>& A,
                                hipStream_t st) {
  if (form >= InvShape::FORMS) return hipErrorInvalidValue;
  const dim3 grid((unsigned)InvShape::grid(A.count, form, d * E::MEMW)), block(InvShape::BT);
#define NTT_SCAN_CALL(DD)                                                                                   \
  switch (form) {                                                                                           \
    case 0: hipLaunchKernelGGL((k_batch_inv<E, DD, 16, false>), grid, block, 0, st, in, out, A); break;     \
    case 1: hipLaunchKernelGGL((k_batch_inv<E, DD, 32, false>), grid, block, 0, st, in, out, A); break;     \
    default: hipLaunchKernelGGL((k_batch_inv<E, DD, 16, true>), grid, block, 0, st, in, out, A); break;     \
  }
  NTT_SCAN_SWITCH_D(d, NTT_SCAN_CALL)
#undef NTT_SCAN_CALL
  return hipGetLastError();
}

// the sum has d = 1 (its degree is in the columns)
template <class E, bool REDUCE>
static hipError_t launch_scan_tiles(unsigned d, bool prod, const uint32_t* in, uint32_t* out, uint32_t* buf, uint32_t* totals,
                                    const ScanArgs<E>& A, hipStream_t st) {
  const dim3 grid((unsigned)A.S.grid()), block(ScanShape::BT);
  if (!prod) {
    if (d != 1) return hipErrorInvalidValue;
    if (A.S.narrow)
      hipLaunchKernelGGL((k_scan<E, 1, false, REDUCE, true>), grid, block, 0, st, in, out, buf, totals, A);
    else
      hipLaunchKernelGGL((k_scan<E, 1, false, REDUCE, false>), grid, block, 0, st, in, out, buf, totals, A);
    return hipGetLastError();
  }
#define NTT_SCAN_CALL(DD)                                                                                       \
  if (A.S.narrow)                                                                                               \
    hipLaunchKernelGGL((k_scan<E, DD, true, REDUCE, true>), grid, block, 0, st, in, out, buf, totals, A);       \
  else                                                                                                          \
    hipLaunchKernelGGL((k_scan<E, DD, true, REDUCE, false>), grid, block, 0, st, in, out, buf, totals, A)
  NTT_SCAN_SWITCH_D(d, NTT_SCAN_CALL)
#undef NTT_SCAN_CALL
  return hipGetLastError();
}
template <class E>
hipError_t launch_scan_reduce(unsigned d, bool prod, const uint32_t* in, uint32_t* buf, const ScanArgs<E>& A, hipStream_t st) {
  return launch_scan_tiles<E, true>(d, prod, in, nullptr, buf, nullptr, A, st);
}
template <class E>
hipError_t launch_scan_chunk(unsigned d, bool prod, const uint32_t* in, uint32_t* out, const uint32_t* buf, uint32_t* totals,
                             const ScanArgs<E>& A, hipStream_t st) {
  return launch_scan_tiles<E, false>(d, prod, in, out, const_cast<uint32_t*>(buf), totals, A, st);
}
template <class E>
hipError_t launch_scan_mid(unsigned d, bool prod, uint32_t* buf, uint32_t* totals, const ScanArgs<E>& A, hipStream_t st) {
  const dim3 grid((A.S.cols + A.mid_cols - 1) / A.mid_cols), block(ScanShape::BT);
  if (!prod) {
    if (d != 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL((k_scan_mid<E, 1, false>), grid, block, 0, st, buf, totals, A);
    return hipGetLastError();
  }
#define NTT_SCAN_CALL(DD) hipLaunchKernelGGL((k_scan_mid<E, DD, true>), grid, block, 0, st, buf, totals, A)
  NTT_SCAN_SWITCH_D(d, NTT_SCAN_CALL)
#undef NTT_SCAN_CALL
  return hipGetLastError();
}

#define NTT_INSTANTIATE_SCAN(E)                                                                                            \
  template hipError_t launch_batch_inverse<E>(unsigned, unsigned, const uint32_t*, uint32_t*, const ScanArgs<E>&,          \
                                              hipStream_t);                                                                \
  template hipError_t launch_scan_reduce<E>(unsigned, bool, const uint32_t*, uint32_t*, const ScanArgs<E>&, hipStream_t);  \
  template hipError_t launch_scan_mid<E>(unsigned, bool, uint32_t*, uint32_t*, const ScanArgs<E>&, hipStream_t);           \
  template hipError_t launch_scan_chunk<E>(unsigned, bool, const uint32_t*, uint32_t*, const uint32_t*, uint32_t*,         \
                                           const ScanArgs<E>&, hipStream_t);

}  // namespace ntt
