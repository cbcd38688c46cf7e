// Stand-alone host check of ntt_amd/csrc/scan_shape.hpp (built with -fsanitize=address,undefined by
// tests/test_scan_host.py): the shape decisions of ntt_matrix_scan over rows {1..70, 2^k +- 1 up to 2^32 - 1},
// widths {1, 2, 3, 4, 15, 16, 17, 37, 300, 2^16}, d {1, 2, 4}, both element sizes and both operations.
// Arithmetic that would overflow is done in unsigned __int128 and compared with what the launcher forms.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "scan_shape.hpp"

using ntt::InvShape;
using ntt::ScanShape;
typedef unsigned __int128 u128;

static void fail(const char* what, uint64_t rows, unsigned width, unsigned d, unsigned memw, int prod) {
  std::printf("scan_shape_check: %s at rows=%llu width=%u d=%u memw=%u prod=%d\n", what, (unsigned long long)rows, width, d,
              memw, prod);
  std::exit(1);
}

int main() {
  std::vector<uint64_t> rows;
  for (uint64_t r = 1; r <= 70; ++r) rows.push_back(r);
  for (unsigned k = 7; k <= 32; ++k) {
    rows.push_back((1ull << k) - 1);
    if (k < 32) rows.push_back((1ull << k) + 1);
  }
  const unsigned widths[] = {1, 2, 3, 4, 15, 16, 17, 37, 300, 1u << 16};
  unsigned long long cases = 0;
  for (unsigned memw = 1; memw <= 2; ++memw)
    for (unsigned d : {1u, 2u, 4u})
      for (int prod = 0; prod <= 1; ++prod)
        for (unsigned width : widths)
          for (uint64_t r : rows) {
            if ((u128)r * width * d >= ((u128)1 << 32)) continue;  // NTT_ERR_ARG before any shape
            const uint32_t cols = prod ? width : width * d, dd = prod ? d : 1, dw = dd * memw;
            const ScanShape s = ScanShape::make(r, cols, dw);
#define NEED(c, what) \
  if (!(c)) fail(what, r, width, d, memw, prod)
            NEED(s.chunks >= 1 && s.chunk_rows >= 1, "a chunk");
            NEED((u128)s.chunks * s.chunk_rows >= r && (u128)(s.chunks - 1) * s.chunk_rows < r, "an empty chunk");
            NEED(s.chunks == 1 || s.chunk_rows % s.run_rows == 0, "chunk_rows is no multiple of run_rows");
            NEED(s.chunk_rows % s.tile_rows == 0, "chunk_rows is no multiple of the tile");
            NEED(s.chunks <= ScanShape::MAX_CHUNKS, "chunks above the cap");
            NEED(s.launches == (s.chunks > 1 ? 3u : 1u), "launches");
            NEED(s.buf_elems() <= ScanShape::buf_bound(cols, dw), "the buffer above its bound");
            NEED((u128)s.buf_elems() * dd * memw * 4 < ((u128)1 << 40), "the buffer's bytes");
            const uint64_t row_bytes = (uint64_t)cols * dw * 4;
            NEED(s.narrow == (row_bytes < 64 ? 1u : 0u), "the layout");
            NEED(row_bytes < 64 || (uint64_t)s.strip_cols * dw * 4 >= 64, "a strip below 64 B");
            NEED(row_bytes < 64 || (uint64_t)s.strip_cols * dw * 4 <= 256 || s.strip_cols == 1, "a strip above 256 B");
            NEED((u128)s.strips * s.strip_cols >= cols && (u128)(s.strips - 1) * s.strip_cols < cols, "the strips");
            NEED(s.rps >= 1 && (uint64_t)s.rps * s.strip_cols <= ScanShape::BT, "threads");
            NEED(s.run_rows * dw == ScanShape::RUN_WORDS && s.tile_rows == s.rps * s.run_rows, "the tile");
            NEED(s.chunk_rows < (1ull << 32), "chunk_rows does not fit its 32-bit report");
            NEED(s.grid() < (1ull << 31), "the grid");
            NEED(!s.narrow || s.lds_words() <= ScanShape::MAX_LDS_WORDS, "the narrow tile's LDS");
            NEED(!s.narrow || (u128)s.tile_rows * cols * dw < ((u128)1 << 32), "the tile's words");
            // the products the launcher and the kernels form in 64 bits
            NEED((u128)(s.chunks - 1) * s.chunk_rows + s.chunk_rows < ((u128)1 << 64), "chunk * chunk_rows");
            NEED((u128)r * cols * dw < ((u128)1 << 63), "the matrix's words");
            const uint32_t mc = s.mid_cols(), lanes = ScanShape::BT / mc;
            NEED(mc >= 1 && mc * lanes == ScanShape::BT && (uint64_t)lanes * s.mid_run() >= s.chunks, "the second launch");
#undef NEED
            ++cases;
          }
  for (unsigned form = 0; form < InvShape::FORMS; ++form)
    for (unsigned dw : {1u, 2u, 4u, 8u}) {
      if (InvShape::run(form, dw) < 1 || InvShape::run(form, dw) * dw != InvShape::run_words(form)) fail("inverse run", 0, 0, dw, form, 0);
      for (uint64_t count : {1ull, 2ull, 255ull, (1ull << 32) / dw - 1}) {
        const uint64_t g = InvShape::grid(count, form, dw), per = (uint64_t)InvShape::BT * InvShape::run(form, dw);
        if ((u128)g * per < count || (u128)(g - 1) * per >= count || g >= (1ull << 31)) fail("inverse grid", count, 0, dw, form, 0);
      }
    }
  std::printf("scan_shape_check: ok (%llu shapes)\n", cases);
  return 0;
}
