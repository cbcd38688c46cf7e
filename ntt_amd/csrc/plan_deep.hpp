// DEEP openings and quotients (ntt_deep_points, ntt_matrix_open, ntt_deep_quotient, ntt_deep_info): the host
// side.  Every scalar of a call (z, alpha, scale, c, (z^N - c^N) / (N c^N)) is computed here per call with
// fieldext.hpp's xf arithmetic -- the text the kernels run -- and travels in the kernel arguments in the
// field's working form; x_i comes from the plan's own forward two-level tables (lo scaled by R_e, the plain
// hi) at stride 2^(log_n - log_rows), so no table is built and the shift cache of the other calls stays as it
// is.  The one buffer the calls own holds the open's per-chunk sums or the quotient's scale alpha^j table; it is
// allocated at the first call that needs it and grows with the width, never with N.
// A Prover (plan_prover.hpp) owns one Deep and hands it a reference to itself: X, whose checks and field
// constants the calls share with the other features, and through it the plan P.  Included by plan_prover.hpp alone.
#pragma once

namespace {

template <class E, class Plan>
struct Deep {
  static constexpr int MEMW = E::MEMW;
  using V = deep_val_t<E>;
  Prover<E, Plan>& X;
  Plan& P;
  DevBuf d_scr;  // open: [chunk][d + 1][width] sums; quotient: V, then the table [width][d]
  explicit Deep(Prover<E, Plan>& prover) : X(prover), P(prover.P) {}

  // z^N and c^N (working form); false: z is a base-field point of the coset c<w_N> (z_0^N = c^N)
  template <class K>
  bool off_domain(const V (&z)[4], unsigned d, V c, unsigned log_rows, const K& k, V (&zn)[4], V& cn) const {
    const uint64_t n = 1ull << log_rows;
    V c1[1] = {c}, cn1[1];
    xf::pow<1>(cn1, c1, n, k);
    cn = cn1[0];
    for (unsigned j = 0; j < 4; ++j) zn[j] = 0;
    if (d == 1) {
      V a[1] = {z[0]}, r[1];
      xf::pow<1>(r, a, n, k);
      zn[0] = r[0];
    } else if (d == 2) {
      V a[2] = {z[0], z[1]}, r[2];
      xf::pow<2>(r, a, n, k);
      zn[0] = r[0], zn[1] = r[1];
    } else {
      V a[4] = {z[0], z[1], z[2], z[3]}, r[4];
      xf::pow<4>(r, a, n, k);
      for (unsigned j = 0; j < 4; ++j) zn[j] = r[j];
    }
    const bool base = z[1] == 0 && z[2] == 0 && z[3] == 0;
    return !(base && zn[0] == cn);
  }
  DeepArgs<E> base_args(unsigned log_rows, unsigned width, const deep_k_t<E>& k) const {
    DeepArgs<E> A{};
    A.F = P.Ff;
    A.K = k;
    A.log_rows = log_rows;
    A.width = width;
    return A;
  }

  int points(void* inv, unsigned log_rows, unsigned d, uint64_t ext_w, const uint64_t* z, const uint64_t* shift,
             unsigned order, hipStream_t st) {
    deep_k_t<E> k{};
    if (!inv || !z || (order & ~NTT_MATRIX_BITREV_OUT) || log_rows > P.log_n || log_rows > 32 ||
        !X.ext_constants(d, ext_w, k))
      return NTT_ERR_ARG;
    V zw[4], zn[4], c, cn;
    typename E::Tw ctw;
    if (!X.words(z, d, zw, k) || !X.shift_of(shift, k, c, &ctw) || !off_domain(zw, d, c, log_rows, k, zn, cn))
      return NTT_ERR_ARG;
    DeepArgs<E> A = base_args(log_rows, 0, k);
    const size_t n = (size_t)1 << log_rows;
    A.inv_elems = n * d;
    A.vec = aligned16(inv) && (n * d * MEMW) % 4 == 0;
    A.lo_s = P.outer_lo(0);
    A.hi = P.outer_hi(0, 1);
    A.lo_bits = P.lo_bits;
    A.tab_shift = P.log_n - log_rows;
    A.bitrev = order & NTT_MATRIX_BITREV_OUT ? 1u : 0u;
    A.c = ctw;
    for (unsigned j = 0; j < 4; ++j) A.z[j] = zw[j];
    P.begin(st);
    const hipError_t e = launch_deep_points<E>(d, static_cast<uint32_t*>(inv), A, st);
    P.mark(st, "z");
    return Plan::rc_of(e);
  }

  int open(const void* mat, unsigned width, unsigned log_rows, const void* inv, unsigned d, uint64_t ext_w,
           const uint64_t* z, const uint64_t* shift, unsigned order, void* values, hipStream_t st) {
    deep_k_t<E> k{};
    if (!mat || !inv || !values || !z || (order & ~NTT_MATRIX_BITREV_OUT) || !X.shape_ok(width, log_rows) ||
        !X.ext_constants(d, ext_w, k))
      return NTT_ERR_ARG;
    V zw[4], zn[4], c, cn;
    if (!X.words(z, d, zw, k) || !X.shift_of(shift, k, c, nullptr) || !off_domain(zw, d, c, log_rows, k, zn, cn))
      return NTT_ERR_ARG;
    const size_t eb = (size_t)MEMW * 4, n = (size_t)1 << log_rows;
    if (overlaps(mat, n * width * eb, values, (size_t)width * d * eb) || overlaps(inv, n * d * eb, values, (size_t)width * d * eb))
      return NTT_ERR_ARG;
    DeepArgs<E> A = base_args(log_rows, width, k);
    A.mat_elems = n * width;
    A.inv_elems = n * d;
    A.val_elems = (size_t)width * d;
    A.vec = aligned16(inv, values);
    A.strip_log = DeepShape::strip_log(width, MEMW);
    A.chunk_rows = DeepShape::open_chunk_rows(width, log_rows, MEMW);
    A.chunks = DeepShape::open_chunks(width, log_rows, MEMW);
    A.scr_elems = (size_t)A.chunks * (d + 1) * width;
    {  // K = (z^N - c^N) / (N c^N)
      V den[1] = {xf::mul(xf::to_work((uint64_t)n % X.modulus(), k), cn, k)}, di[1];
      xf::inv<1>(di, den, k);
      zn[0] = xf::sub(zn[0], cn, k);
      for (unsigned j = 0; j < 4; ++j) A.k[j] = j < d ? xf::mul(zn[j], di[0], k) : V(0);
    }
    for (unsigned j = 0; j < 4; ++j) A.z[j] = zw[j];
    if (!d_scr.grow(A.scr_elems * eb)) return NTT_ERR_HIP;
    P.begin(st);
    hipError_t e = launch_deep_open<E>(d, static_cast<const uint32_t*>(mat), static_cast<const uint32_t*>(inv),
                                       d_scr.get(), A, st);
    P.mark(st, "o");
    if (e == hipSuccess) {
      e = launch_deep_open_fin<E>(d, d_scr.get(), static_cast<uint32_t*>(values), A, st);
      P.mark(st, "e");
    }
    return Plan::rc_of(e);
  }

  int quotient(const void* mat, unsigned width, unsigned log_rows, const void* inv, const void* values, unsigned d,
               uint64_t ext_w, const uint64_t* alpha, const uint64_t* scale, unsigned flags, void* out, hipStream_t st) {
    deep_k_t<E> k{};
    if (!mat || !inv || !values || !alpha || !out || (flags & ~NTT_DEEP_ACCUMULATE) || !X.shape_ok(width, log_rows) ||
        !X.ext_constants(d, ext_w, k))
      return NTT_ERR_ARG;
    DeepArgs<E> A = base_args(log_rows, width, k);
    const uint64_t one[4] = {1, 0, 0, 0};
    if (!X.words(alpha, d, A.alpha, k) || !X.words(scale ? scale : one, d, A.scale, k)) return NTT_ERR_ARG;
    const size_t eb = (size_t)MEMW * 4, n = (size_t)1 << log_rows, ob = n * d * eb;
    if (overlaps(mat, n * width * eb, out, ob) || overlaps(inv, n * d * eb, out, ob) ||
        overlaps(values, (size_t)width * d * eb, out, ob))
      return NTT_ERR_ARG;
    A.mat_elems = n * width;
    A.inv_elems = A.out_elems = n * d;
    A.val_elems = (size_t)width * d;
    A.vec = aligned16(inv, values, out);
    A.flags = flags;
    A.lanes_log = DeepShape::lanes_log(width, MEMW);
    A.scr_elems = DeepShape::SCR_TAB + (size_t)width * d;
    if (!d_scr.grow(A.scr_elems * eb)) return NTT_ERR_HIP;
    P.begin(st);
    hipError_t e = launch_deep_qpro<E>(d, static_cast<const uint32_t*>(values), d_scr.get(), A, st);
    P.mark(st, "a");
    if (e == hipSuccess) {
      e = launch_deep_quotient<E>(d, static_cast<const uint32_t*>(mat), static_cast<const uint32_t*>(inv), d_scr.get(),
                                  static_cast<uint32_t*>(out), A, st);
      P.mark(st, "q");
    }
    return Plan::rc_of(e);
  }

  // the shape alone: a twiddle-only plan answers too
  int info(unsigned width, unsigned log_rows, unsigned d, unsigned* open_row_chunks, unsigned* quotient_lanes_per_row) const {
    if (!open_row_chunks || !quotient_lanes_per_row || !X.shape_ok(width, log_rows) || !degree_ok(d)) return NTT_ERR_ARG;
    *open_row_chunks = DeepShape::open_chunks(width, log_rows, MEMW);
    *quotient_lanes_per_row = 1u << DeepShape::lanes_log(width, MEMW);
    return NTT_OK;
  }
};

}  // namespace
