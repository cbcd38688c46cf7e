// Row-major matrix transforms (ntt_forward_matrix / ntt_inverse_matrix / ntt_lde_matrix and their _ex
// forms): the transforms run down the columns of a [n][width] matrix on a schedule of their own
// (plan_schedule.hpp schedule_matrix: radices up to TILE >> strip, a strip of columns per pass), every
// pass in the strip form of the pass tile (k_pass_mat).  Column passes take their outer twiddles from the
// plan's two-level tables; the w_R^e tables of the matrix radices are built at the first matrix call.
// A Prover (plan_prover.hpp) owns one Matrix and hands it a reference to itself: X, whose checks the calls
// share with the other features, and through it the plan P; the shift's tables are the plan's shift cache
// (plan_shift.hpp).  Included by plan_prover.hpp alone.
#pragma once
#include <vector>

namespace {

template <class E, class Plan>
struct Matrix {
  static constexpr int MEMW = E::MEMW, SCRW = E::SCRW;
  Prover<E, Plan>& X;
  Plan& P;
  explicit Matrix(Prover<E, Plan>& prover) : X(prover), P(prover.P) {}

  Lazy mat_state;  // ready: d_mat_tab holds the tables below
  DevBuf d_mat_tab;
  unsigned mat_r[8] = {0}, mat_p = 0;
  size_t mat_int[2][8] = {};  // [dir][pass]: word offset of w_{R_i}^e (naive sizes: pass 0 = w_n^e, e < n)
  bool build_mat() {
    unsigned tb[8];
    if (!schedule_matrix(P.log_n, E::TILE_LOG, mat_min_strip_log<E>(), 1, mat_r, tb, mat_p)) return false;
    std::vector<uint32_t> host;
    for (int dir = 0; dir < 2; ++dir) {
      if (mat_p == 0) mat_int[dir][0] = P.push_powers_to(host, P.wn_m[dir], P.n, nullptr, false);
      for (unsigned i = 0; i < mat_p; ++i)
        mat_int[dir][i] =
            P.push_powers_to(host, P.H.pow_u64(P.wn_m[dir], P.n >> mat_r[i]), 1ull << mat_r[i], nullptr, false);
    }
    return d_mat_tab.alloc(host.size() * 4) &&
           hipMemcpy(d_mat_tab.get(), host.data(), host.size() * 4, hipMemcpyHostToDevice) == hipSuccess;
  }
  int info(unsigned width, unsigned* npasses, unsigned* radix_log) const {
    unsigned rr[8] = {0}, tb[8], p = 0;
    if (!X.usable() || !X.shape_ok(width, P.log_n)) return NTT_ERR_ARG;
    if (!schedule_matrix(P.log_n, E::TILE_LOG, mat_min_strip_log<E>(), width, rr, tb, p)) return NTT_ERR_ARG;
    if (npasses) *npasses = p;
    if (radix_log)
      for (int i = 0; i < 8; ++i) radix_log[i] = rr[i];
    return NTT_OK;
  }
  // in: [n_in = n >> log_blowup][width] (is_lde) or the matrix itself (in == out); out: [n][width]
  // The _ex forms change addresses and one product, never the schedule: a forward shift is the lde's
  // product at the first pass's load (PRO_LDE with every row present: it loads what the plain pass loads,
  // all of it ahead of the tile's first store, so a transform of one pass stays safe in place); an inverse
  // shift is c^-j at the last pass's store; BITREV_IN permutes the rows the first pass loads, BITREV_OUT
  // the rows the last pass stores.
  int run(const void* in, void* out, unsigned width, bool inverse, bool is_lde, unsigned log_blowup,
          const uint64_t* shift, unsigned limbs64, unsigned order, hipStream_t st) {
    const uint64_t n = P.n;
    const unsigned log_n = P.log_n;
    if (!in || !out || !X.usable()) return NTT_ERR_ARG;
    if (!X.shape_ok(width, log_n)) return NTT_ERR_ARG;  // element indices are 32-bit in places
    if (is_lde && log_blowup > log_n) return NTT_ERR_ARG;
    if (order & ~(inverse ? NTT_MATRIX_BITREV_IN : NTT_MATRIX_BITREV_OUT)) return NTT_ERR_ARG;
    const size_t n_in = is_lde ? (size_t)(n >> log_blowup) : (size_t)n, eb = (size_t)MEMW * 4;
    // the first pass reads d_in while later tiles write d_out
    if (is_lde && overlaps(in, n_in * width * eb, out, (size_t)n * width * eb)) return NTT_ERR_ARG;
    if (shift)
      if (int rc = P.shift.ensure_tables(shift, limbs64)) return rc;
    unsigned tb[8] = {0}, rr[8], p = 0;
    if (!schedule_matrix(log_n, E::TILE_LOG, mat_min_strip_log<E>(), width, rr, tb, p)) return NTT_ERR_ARG;
    if (!mat_state.ready([&] { return build_mat(); })) return NTT_ERR_HIP;
    const uint32_t* src = static_cast<const uint32_t*>(in);
    uint32_t* dst = static_cast<uint32_t*>(out);
    if (log_n == 0) {  // one row: the transform of one point, c^0 = 1
      if (dst != src && hipMemcpyAsync(dst, src, width * eb, hipMemcpyDeviceToDevice, st) != hipSuccess) return NTT_ERR_HIP;
      return NTT_OK;
    }
    const int dir = inverse ? 1 : 0;
    // forward: c^j at the first pass's load (the lde's pass, here maybe with n_in = n and in == out);
    // inverse: c^-j at the last pass's store
    const bool mul_in = !inverse && shift, mul_out = inverse && shift;
    const bool pro_lde = is_lde || mul_in;
    const unsigned last = mat_p == 0 ? 0 : mat_p - 1;
    auto mat_args = [&](unsigned i) {
      PassArgs<E> A = P.base_args(inverse);
      A.tw_int = d_mat_tab.get() + mat_int[dir][i];
      A.mat_w = width;
      A.il = tb[i];
      A.mat_ns = (uint32_t)(((uint64_t)width + (1u << tb[i]) - 1) >> tb[i]);
      A.dbg_src_n = A.dbg_dst_n = (size_t)n * width;
      if (i == 0 && pro_lde) {
        A.src_stride = n_in * MEMW;
        A.dbg_src_n = n_in * width;
        if (mul_in) {
          A.tw_in = P.shift.lo(0);
          A.tw_in_hi = P.shift.hi(0);
        }
      }
      if (i == 0 && (order & NTT_MATRIX_BITREV_IN)) A.mat_ops |= MAT_REV_IN;
      if (i == last && (order & NTT_MATRIX_BITREV_OUT)) A.mat_ops |= MAT_REV_OUT;
      if (i == last && mul_out) {
        A.mat_ops |= MAT_MUL_OUT;
        A.tw_in = P.shift.lo(1);
        A.tw_in_hi = P.shift.hi(1);
      }
      return A;
    };
    hipError_t e = hipSuccess;
    P.begin(st);
    if (mat_p == 0) {
      PassArgs<E> A = mat_args(0);
      A.flags = inverse ? 1u : 0u;
      e = launch_mat_naive<E>(src, dst, A, (uint32_t)n_in, st);
      P.mark(st, "n");
      return Plan::rc_of(e);
    }
    uint32_t* work = dst;
    if (mat_p >= 2) {  // n width elements, not the next power of two
      if (!P.d_scratch.grow((size_t)n * width * SCRW * 4)) return NTT_ERR_HIP;
      work = P.d_scratch.get();
    }
    unsigned blk = log_n;
    const unsigned ncol = mat_p == 1 ? 1 : mat_p - 1;  // column passes (a transform of one pass is one)
    for (unsigned i = 0; i < ncol && e == hipSuccess; ++i) {
      PassArgs<E> A = mat_args(i);
      A.tw_lo = P.outer_lo(dir);
      A.tw_hi = P.outer_hi(dir, i);  // the inverse's pass 1 carries n^-1
      A.log_blk = blk + tb[i];
      A.log_m = log_n - blk;
      A.src_user = i == 0 ? 1u : 0u;
      const uint32_t grid = (uint32_t)(((n << tb[i]) >> E::TILE_LOG) * A.mat_ns);
      e = launch_mat_pass<E>(KIND_COLUMN, (int)mat_r[i], i == 0 && pro_lde, i == 0 ? src : work, work, A, grid, st);
      P.mark(st, mat_p == 1 ? "s" : "c", mat_r[i]);
      blk -= mat_r[i];
    }
    if (mat_p >= 2 && e == hipSuccess) {
      const unsigned i = mat_p - 1;
      PassArgs<E> A = mat_args(i);
      A.r1 = mat_r[0];
      A.nmid = mat_p - 2;
      mid_digits(mat_r, mat_p, A.mid_bits, A.mid_off);
      const uint32_t grid = (uint32_t)(((n << tb[i]) >> E::TILE_LOG) * A.mat_ns);
      e = launch_mat_pass<E>(KIND_FINAL, (int)mat_r[i], false, work, dst, A, grid, st);
      P.mark(st, "f", mat_r[i]);
    }
    return Plan::rc_of(e);
  }
};

}  // namespace
