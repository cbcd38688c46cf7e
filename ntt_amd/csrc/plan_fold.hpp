// FRI fold (ntt_fri_fold): one launch of k_fri_fold.  Every constant is computed here, on the host,
// per call -- c^-1 (one inversion), 2^-k, the 2^(k-1) twiddles zeta^-e, and beta^(2^s), W beta^(2^s) for
// the k stages -- and travels in the kernel arguments; x0^-1's variable part w_N^-rev(i') comes from the
// plan's own inverse two-level tables (lo scaled by R_e, the plain hi: not the one carrying n^-1) at
// stride 2^(log_n - log_rows).  Nothing is cached, so the coset tables of the other calls stay as they are.
// The data keep their form: with t R_e as the variable operand mulv(x, t R_e) = x t whatever form x has,
// and the other products are by constants, so a NTT_PLAN_MONTGOMERY_IO plan runs the same code.
// A Prover (plan_prover.hpp) owns one Fold and hands it a reference to itself: X, whose checks the call shares
// with the other features, and through it the plan P.  The arithmetic here is the host field's (Vec<NH>, in
// Montgomery form), since every constant leaves as a twiddle.  Included by plan_prover.hpp alone.
#pragma once

namespace {

template <class E, class Plan>
struct Fold {
  static constexpr int NH = EngHost<E>::NH, MEMW = E::MEMW, TW = E::TW;
  Prover<E, Plan>& X;
  Plan& P;
  explicit Fold(Prover<E, Plan>& prover) : X(prover), P(prover.P) {}

  // the load form of k_fri_fold without the knob: each thread loads its own fibre.  Measured faster than the
  // form through LDS in five of six cases at 2^22 rows: the kernel is bound by its
  // arithmetic, not by the lines its loads touch, and the staging costs occupancy
  static constexpr bool kFoldStagedDefault = false;

  int run(const void* in, void* out, unsigned log_rows, unsigned log_arity, unsigned ext_degree, uint64_t ext_w,
          const uint64_t* beta, const uint64_t* shift, hipStream_t st) {
    const auto& H = P.H;
    const unsigned log_n = P.log_n;
    if (!in || !out || !beta || !X.usable()) return NTT_ERR_ARG;
    if (log_arity < 1 || log_arity > 4 || log_arity > log_rows || log_rows > log_n) return NTT_ERR_ARG;
    if (!degree_ok(ext_degree)) return NTT_ERR_ARG;
    const unsigned d = ext_degree, k = log_arity;
    Vec<NH> wc{}, cc{}, bc[4];
    if (d > 1 && (!H.canonical(&ext_w, 1, wc) || wc == Vec<NH>{})) return NTT_ERR_ARG;
    for (unsigned j = 0; j < d; ++j)
      if (!H.canonical(beta + j, 1, bc[j])) return NTT_ERR_ARG;
    if (shift && (!H.canonical(shift, 1, cc) || cc == Vec<NH>{})) return NTT_ERR_ARG;
    const size_t eb = (size_t)MEMW * 4, n_in = (size_t)1 << log_rows, n_out = n_in >> k;
    if (overlaps(in, n_in * d * eb, out, n_out * d * eb)) return NTT_ERR_ARG;  // other workgroups still read d_in
    FoldArgs<E> A{};
    A.F = P.Ff;
    A.lo_s = P.outer_lo(1);
    A.hi = P.outer_hi(1, 1);  // the plain hi table (pass 1's carries n^-1)
    A.lo_bits = P.lo_bits;
    A.tab_shift = log_n - log_rows;
    A.log_m = log_rows - k;
    A.vec = aligned16(in, out);
    A.src_words = n_in * d * MEMW;
    A.dst_words = n_out * d * MEMW;
    auto tw = [&](const Vec<NH>& m, typename E::Tw& t) {  // Montgomery-form host value -> twiddle
      uint32_t enc[TW];
      P.EH.encode(H.from_mont(m), enc);
      static_assert(sizeof(typename E::Tw) == TW * 4, "a twiddle is its table entry");
      memcpy(&t, enc, sizeof t);
    };
    tw(shift ? H.pow(H.to_mont(cc), P.pm2_) : H.r1, A.cinv);
    {
      Vec<NH> two{};
      two[0] = 2;
      tw(H.pow_u64(H.pow(H.to_mont(two), P.pm2_), k), A.scale);
    }
    {
      const Vec<NH> zi = H.pow_u64(P.wn_m[1], P.n >> k);  // zeta^-1 = w_n^-(n / 2^k)
      Vec<NH> acc = H.r1;
      for (unsigned e = 0; e < 8; ++e) {
        tw(acc, A.zeta[e]);
        acc = H.mul(acc, zi);
      }
    }
    {
      const Vec<NH> wm = d > 1 ? H.to_mont(wc) : H.r1;
      Vec<NH> b[4] = {}, zero{};
      for (unsigned j = 0; j < d; ++j) b[j] = H.to_mont(bc[j]);
      for (unsigned s = 0; s < 4; ++s) {
        for (unsigned j = 0; j < 4; ++j) {
          tw(j < d ? b[j] : zero, A.beta[s][j]);
          tw(j < d ? H.mul(b[j], wm) : zero, A.wbeta[s][j]);
        }
        // b <- b^2 in F_p[X]/(X^d - W)
        Vec<NH> lo[4] = {}, hi[4] = {};
        for (unsigned i = 0; i < d; ++i)
          for (unsigned j = 0; j < d; ++j) {
            Vec<NH>& acc = i + j < d ? lo[i + j] : hi[i + j - d];
            acc = H.add(acc, H.mul(b[i], b[j]));
          }
        for (unsigned j = 0; j < d; ++j) b[j] = H.add(lo[j], H.mul(hi[j], wm));
      }
    }
    const int want = knob::fold_staged();
    const bool staged = want < 0 ? kFoldStagedDefault : want != 0;
    P.begin(st);
    const hipError_t e =
        launch_fri_fold<E>(k, d, staged, static_cast<const uint32_t*>(in), static_cast<uint32_t*>(out), A, st);
    P.mark(st, "x", k);
    return Plan::rc_of(e);
  }
};

}  // namespace
