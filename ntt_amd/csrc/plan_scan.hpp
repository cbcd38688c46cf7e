// Batch inversion and running sums / products down matrix columns (ntt_batch_inverse, ntt_matrix_scan,
// ntt_scan_info): the host side.  The shape of a call is scan_shape.hpp's (ScanShape::make, a header without HIP
// that tests/c/scan_shape_check.cpp sweeps on the host).  The one buffer the calls own holds the scan's chunk
// aggregates [chunk][column][d]; it is allocated at the first scan of more than one chunk and is bounded by
// ScanShape::buf_bound, whatever the rows.
// A Prover (plan_prover.hpp) owns one Scan and hands it a reference to itself: X, whose checks and field
// constants the calls share with the other features, and through it the plan P.  Included by plan_prover.hpp alone.
#pragma once

namespace {

template <class E, class Plan>
struct Scan {
  static constexpr int MEMW = E::MEMW;
  Prover<E, Plan>& X;
  Plan& P;
  DevBuf d_buf;  // the chunk aggregates, then their exclusive scan
  explicit Scan(Prover<E, Plan>& prover) : X(prover), P(prover.P) {}

  // the constants every kernel of the two calls takes; prod: the ring product (the sum has identity 0)
  ScanArgs<E> base_args(const deep_k_t<E>& k, bool prod) const {
    ScanArgs<E> A{};
    A.K = k;
    A.dbg = P.Ff.dbg;
    if constexpr (std::is_same_v<E, Eng31>) {
      const auto c = X.constants();
      const uint64_t p = c.p;
      uint64_t rinv = 1, b = c.one;
      for (uint64_t e = p - 2; e; e >>= 1) {  // (2^32)^(p-2)
        if (e & 1) rinv = rinv * b % p;
        b = b * b % p;
      }
      A.conv = c.mont ? 0u : 1u;
      A.r2 = c.r2;
      A.rinv = (uint32_t)rinv;
      A.ident = prod ? (A.conv ? 1u : c.one) : 0u;
    } else {
      A.ident = prod ? 1u : 0u;
    }
    return A;
  }

  int inverse(const void* in, void* out, uint64_t count, unsigned d, uint64_t ext_w, hipStream_t st) {
    deep_k_t<E> k{};
    if (!in || !out || count == 0 || !degree_ok(d) || count >= (1ull << 32) || count * d >= (1ull << 32) ||
        !X.ext_constants(d, ext_w, k))
      return NTT_ERR_ARG;
    const size_t bytes = (size_t)count * d * MEMW * 4;
    if (in != out && overlaps(in, bytes, out, bytes)) return NTT_ERR_ARG;
    ScanArgs<E> A = base_args(k, true);
    A.count = count;
    A.io_elems = (size_t)count * d;
    A.vec = aligned16(in, out) && (A.io_elems * MEMW) % 4 == 0;
    const int knob = knob::inv_form();
    const unsigned form = knob >= 0 && knob < (int)InvShape::FORMS ? (unsigned)knob : InvShape::DEFAULT_FORM;
    P.begin(st);
    const hipError_t e = launch_batch_inverse<E>(d, form, static_cast<const uint32_t*>(in), static_cast<uint32_t*>(out), A, st);
    P.mark(st, "v");
    return Plan::rc_of(e);
  }

  // the shape at (rows, width, d, op); false: NTT_ERR_ARG.  The sum scans width d base columns.
  bool shape(uint64_t rows, unsigned width, unsigned d, unsigned op, ScanShape& S) const {
    if (rows == 0 || width == 0 || !degree_ok(d) || op > NTT_SCAN_PRODUCT) return false;
    const uint64_t row_elems = (uint64_t)width * d;
    if (rows >= (1ull << 32) || row_elems >= (1ull << 32) || rows * row_elems >= (1ull << 32)) return false;
    const bool prod = op == NTT_SCAN_PRODUCT;
    S = ScanShape::make(rows, prod ? width : (uint32_t)row_elems, (prod ? d : 1u) * MEMW);
    return true;
  }

  int scan(const void* in, void* out, uint64_t rows, unsigned width, unsigned d, uint64_t ext_w, unsigned op, unsigned flags,
           void* totals, hipStream_t st) {
    deep_k_t<E> k{};
    ScanShape S;
    if (!in || !out || (flags & ~NTT_SCAN_EXCLUSIVE) || !shape(rows, width, d, op, S)) return NTT_ERR_ARG;
    const bool prod = op == NTT_SCAN_PRODUCT;
    const unsigned dd = prod ? d : 1u;  // the degree the kernels see
    if (!X.ext_constants(dd, ext_w, k)) return NTT_ERR_ARG;
    const size_t eb = (size_t)MEMW * 4, bytes = (size_t)rows * width * d * eb, tot_bytes = (size_t)width * d * eb;
    if (in != out && overlaps(in, bytes, out, bytes)) return NTT_ERR_ARG;
    if (totals && (overlaps(in, bytes, totals, tot_bytes) || overlaps(out, bytes, totals, tot_bytes))) return NTT_ERR_ARG;
    ScanArgs<E> A = base_args(k, prod);
    A.S = S;
    A.rows = rows;
    A.excl = flags & NTT_SCAN_EXCLUSIVE ? 1u : 0u;
    A.mid_cols = S.mid_cols();
    A.mid_run = S.mid_run();
    A.io_elems = (size_t)rows * width * d;
    A.tot_elems = (size_t)width * d;
    A.buf_elems = (size_t)S.buf_elems() * dd;
    A.vec = aligned16(in, out, totals) && (A.io_elems * MEMW) % 4 == 0;
    if (S.chunks > 1 && !d_buf.grow(A.buf_elems * eb)) return NTT_ERR_HIP;
    const uint32_t* src = static_cast<const uint32_t*>(in);
    uint32_t* tot = static_cast<uint32_t*>(totals);
    P.begin(st);
    hipError_t e = hipSuccess;
    if (S.chunks > 1) {
      e = launch_scan_reduce<E>(dd, prod, src, d_buf.get(), A, st);
      P.mark(st, "t");
      if (e == hipSuccess) {
        e = launch_scan_mid<E>(dd, prod, d_buf.get(), tot, A, st);
        P.mark(st, "k");
      }
    }
    if (e == hipSuccess) {
      e = launch_scan_chunk<E>(dd, prod, src, static_cast<uint32_t*>(out), d_buf.get(), tot, A, st);
      P.mark(st, "y");
    }
    return Plan::rc_of(e);
  }

  // the shape alone: a twiddle-only plan answers too
  int info(uint64_t rows, unsigned width, unsigned d, unsigned op, unsigned* strip_cols, unsigned* run_rows,
           unsigned* chunk_rows, unsigned* chunks, unsigned* launches) const {
    ScanShape S;
    if (!strip_cols || !run_rows || !chunk_rows || !chunks || !launches || !shape(rows, width, d, op, S)) return NTT_ERR_ARG;
    *strip_cols = S.strip_cols;
    *run_rows = S.run_rows;
    *chunk_rows = (unsigned)S.chunk_rows;
    *chunks = S.chunks;
    *launches = S.launches;
    return NTT_OK;
  }
};

}  // namespace
