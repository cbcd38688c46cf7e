// The shape decisions of ntt_matrix_scan and ntt_batch_inverse, shared by the launchers,
// the kernels, ntt_scan_info and tests/c/scan_shape_check.cpp.  Standard C++ only: it compiles without HIP.
//
// A scan of M = [rows][cols] elements of dw 32-bit words each (cols = width and dw = d memw for the product;
// cols = width d and dw = memw for the sum, which scans base columns).  A workgroup of BT threads is a grid of
// rps thread rows x strip_cols columns, thread (r, c) = r strip_cols + c; it walks its chunk of rows in tiles of
// rps run_rows rows, thread (r, c) owning rows [r run_rows, (r + 1) run_rows) of column c of the tile.
//   Rows of at least 64 bytes: strips of strip_cols adjacent columns, a power of two: the columns rounded up
//     to one, at least 64 B and at most 256 B of a row; the last strip is masked.
//   Rows shorter than 64 bytes: one strip of all the columns (any count); a tile is one contiguous byte range
//     and reaches its threads through LDS.
// run_rows: 64 bytes of a column per thread.  chunk_rows: a multiple of the tile's rows, so that
// ceil(TARGET_WGS / strips) chunks (MAX_CHUNKS at most) cover the rows; chunks = ceil(rows / chunk_rows), none
// empty.  The plan-owned buffer holds chunks cols elements, at most buf_bound(), whatever the rows.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__HIP__)
#define NTT_SCAN_HD __host__ __device__ inline
#else
#define NTT_SCAN_HD inline
#endif

namespace ntt {

struct ScanShape {
  static constexpr unsigned BT = 256;           // threads of every scan and inverse workgroup
  static constexpr unsigned RUN_WORDS = 16;     // scan: 32-bit words of a column a thread holds per tile
  static constexpr unsigned TARGET_WGS = 2048;  // workgroups wanted (256 CUs x 8)
  static constexpr unsigned MAX_CHUNKS = 1024;  // row chunks at most, whatever the rows
  static constexpr unsigned NARROW_BYTES = 64;  // rows shorter than this take the narrow layout
  static constexpr unsigned STRIP_BYTES = 256;  // a strip's bytes of a row at most
  static constexpr unsigned LDS_PAD = 4;        // narrow layout: words of padding after each thread row's words

  // the decisions at one shape
  uint32_t cols = 0, dw = 0;   // columns scanned and 32-bit words of one element
  uint32_t narrow = 0;         // 1: the narrow layout
  uint32_t strip_cols = 0, strips = 0, rps = 0;
  uint32_t run_rows = 0, tile_rows = 0;
  uint64_t chunk_rows = 0;
  uint32_t chunks = 0, launches = 0;

  NTT_SCAN_HD static unsigned ceil_log2(uint64_t v) {
    unsigned l = 0;
    while (l < 63 && (1ull << l) < v) ++l;
    return l;
  }
  // cols x dw words per element, rows >= 1, cols >= 1, rows cols dw < 2^32 words / memw (the caller checks)
  NTT_SCAN_HD static ScanShape make(uint64_t rows, uint32_t cols, uint32_t dw) {
    ScanShape s;
    s.cols = cols, s.dw = dw;
    const uint64_t row_bytes = (uint64_t)cols * dw * 4;
    s.narrow = row_bytes < NARROW_BYTES ? 1u : 0u;
    if (s.narrow) {
      s.strip_cols = cols;
      s.strips = 1;
    } else {
      const unsigned lo = ceil_log2((NARROW_BYTES + dw * 4 - 1) / (dw * 4));
      unsigned hi = ceil_log2(STRIP_BYTES / (dw * 4));
      if (hi < lo) hi = lo;
      unsigned l = ceil_log2(cols);
      l = l < lo ? lo : (l > hi ? hi : l);
      s.strip_cols = 1u << l;
      s.strips = (uint32_t)(((uint64_t)cols + s.strip_cols - 1) >> l);
    }
    s.rps = BT / s.strip_cols;
    s.run_rows = RUN_WORDS / dw;
    s.tile_rows = s.rps * s.run_rows;
    uint64_t want = ((uint64_t)TARGET_WGS + s.strips - 1) / s.strips;
    if (want > MAX_CHUNKS) want = MAX_CHUNKS;
    const uint64_t per = (rows + want - 1) / want;
    s.chunk_rows = (per + s.tile_rows - 1) / s.tile_rows * s.tile_rows;
    s.chunks = (uint32_t)((rows + s.chunk_rows - 1) / s.chunk_rows);
    s.launches = s.chunks > 1 ? 3u : 1u;
    return s;
  }
  // elements of the plan-owned buffer at most, whatever the rows: chunks <= TARGET_WGS / strips + 1
  NTT_SCAN_HD static uint64_t buf_bound(uint32_t cols, uint32_t dw) {
    const ScanShape s = make(1, cols, dw);
    return (uint64_t)TARGET_WGS * s.strip_cols + cols + s.strip_cols;
  }
  NTT_SCAN_HD uint64_t buf_elems() const { return (uint64_t)chunks * cols; }
  NTT_SCAN_HD uint64_t grid() const { return (uint64_t)strips * chunks; }
  // the second launch: mid_cols columns x BT / mid_cols chunk lanes per workgroup, a lane a run of chunks
  NTT_SCAN_HD uint32_t mid_cols() const {
    const unsigned l = ceil_log2(chunks < BT ? chunks : BT);
    return BT >> l;
  }
  NTT_SCAN_HD uint32_t mid_run() const {
    const uint32_t lanes = BT / mid_cols();
    return (chunks + lanes - 1) / lanes;
  }
  // narrow layout: LDS words of one tile (a thread row's run_rows strip_cols dw words, then LDS_PAD)
  NTT_SCAN_HD uint32_t lds_words() const { return rps * (RUN_WORDS * strip_cols + LDS_PAD); }
  static constexpr unsigned MAX_LDS_WORDS = BT * (RUN_WORDS + LDS_PAD);  // strip_cols rps <= BT, rps <= BT
};

// ntt_batch_inverse: the ways of sharing one inversion.  A thread owns run_words(form)
// 32-bit words of consecutive elements: 16 (form 0, the run of k_deep_points), 32 (form 1), or 16 behind a
// cross-lane product scan with one inversion per wave (form 2).
struct InvShape {
  static constexpr unsigned BT = 256;
  static constexpr unsigned FORMS = 3;
  static constexpr unsigned DEFAULT_FORM = 1;
  NTT_SCAN_HD static unsigned run_words(unsigned form) { return form == 1 ? 32u : 16u; }
  NTT_SCAN_HD static unsigned run(unsigned form, unsigned dw) { return run_words(form) / dw; }
  NTT_SCAN_HD static uint64_t grid(uint64_t count, unsigned form, unsigned dw) {
    const uint64_t per = (uint64_t)BT * run(form, dw);
    return (count + per - 1) / per;
  }
};

}  // namespace ntt
