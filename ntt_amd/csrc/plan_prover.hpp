// The prover-stage calls of a plan -- the row-major matrix transforms, the FRI fold, the DEEP openings and
// quotients, the Poseidon2 Merkle commitments, batch inversion and the column scans -- behind one front.  They
// exist on the HasMat engines only (Goldilocks and the 4-byte fields), so only those engines' plans hold a
// Prover (PlanImpl::prover), and the C entry points reach it without a virtual call (ProverEngines in
// ntt_plan.cpp).  A Prover owns the five features, each in a header of its own with a reference to the Prover (X)
// and to the plan (P), and what they share: the field's modulus and constants, the checks of a degree, a shape
// and a host word, and the conversion of host words to the field's working form.  The predicates that need no
// plan (degree_ok, aligned16, fits32) are plan_schedule.hpp's.  Included by ntt_plan.cpp alone.
#pragma once
#include <cstring>

#include "ntt_kernels.hpp"
#include "plan_devmem.hpp"
#include "plan_hostmath.hpp"
#include "plan_knobs.hpp"
#include "plan_schedule.hpp"

namespace {
template <class E, class Plan>
struct Prover;
}  // namespace

#include "plan_deep.hpp"    // Deep<E, Plan>: DEEP openings and quotients of evaluation matrices
#include "plan_fold.hpp"    // Fold<E, Plan>: ntt_fri_fold
#include "plan_hash.hpp"    // Hash<E, Plan>: Poseidon2 Merkle commitments and openings
#include "plan_matrix.hpp"  // Matrix<E, Plan>: the row-major matrix transforms
#include "plan_scan.hpp"    // Scan<E, Plan>: batch inversion, running sums and products down matrix columns

namespace {

template <class E, class Plan>
struct Prover {
  static_assert(HasMat<E>::value, "the prover-stage kernels are instantiated for the HasMat engines only");
  static constexpr bool k31 = std::is_same_v<E, Eng31>;
  static constexpr int NH = EngHost<E>::NH;
  Plan& P;
  explicit Prover(Plan& plan) : P(plan) {}
  Matrix<E, Plan> mat{*this};
  Fold<E, Plan> fold{*this};
  Deep<E, Plan> deep{*this};
  Hash<E, Plan> hash{*this};
  Scan<E, Plan> scan{*this};

  bool usable() const { return !(P.flags & NTT_PLAN_TWIDDLE_ONLY); }
  uint64_t modulus() const {
    if constexpr (k31) return P.H.M.p[0];
    else return kGoldilocksP;
  }
  bool canon(uint64_t v) const { return v < modulus(); }
  // 2^log_rows rows of the plan's domain or of a smaller one, by width: every element index fits 32 bits
  bool shape_ok(unsigned width, unsigned log_rows) const { return log_rows <= P.log_n && fits32(width, log_rows); }

  // The field's constants without W.  A value travels to the kernels in the field's WORKING FORM (fieldext.hpp):
  // v 2^32 mod p on the 4-byte fields, whose constants are derived here and nowhere else on the host, with the
  // plan's I/O form beside them; the plain value on Goldilocks.
  hash_k_t<E> constants() const {
    hash_k_t<E> k{};
    if constexpr (k31) {
      const uint64_t p = P.H.M.p[0], r = (1ull << 32) % p;
      k.p = (uint32_t)p;
      k.pinv = f31::pinv32(k.p);
      k.one = (uint32_t)r;
      k.r2 = (uint32_t)(r * r % p);
      k.mont = (P.flags & NTT_PLAN_MONTGOMERY_IO) ? 1u : 0u;
    } else {
      k.one = 1;
    }
    return k;
  }
  // ... with W, for elements of F_p[X]/(X^d - W); false (NTT_ERR_ARG): a twiddle-only plan, a degree other than
  // 1, 2, 4, or W zero or not canonical
  bool ext_constants(unsigned d, uint64_t ext_w, deep_k_t<E>& k) const {
    if (!usable() || !degree_ok(d)) return false;
    if (d > 1 && (ext_w == 0 || !canon(ext_w))) return false;
    k = constants();
    k.w = (deep_val_t<E>)(d > 1 ? ext_w : 0);
    if constexpr (k31) k.ws = f31::shoup_companion(k.w, k.p);
    return true;
  }
  // d canonical host words -> working form; false: a word is not canonical
  template <class V, class K>
  bool words(const uint64_t* src, unsigned d, V (&dst)[4], const K& k) const {
    for (unsigned j = 0; j < 4; ++j) dst[j] = 0;
    for (unsigned j = 0; j < d; ++j) {
      if (!canon(src[j])) return false;
      dst[j] = xf::to_work(src[j], k);
    }
    return true;
  }
  // shift -> c (working form) and its twiddle; false: not canonical or zero
  template <class V, class K>
  bool shift_of(const uint64_t* shift, const K& k, V& c, typename E::Tw* tw) const {
    const uint64_t cv = shift ? *shift : 1;
    if (cv == 0 || !canon(cv)) return false;
    c = xf::to_work(cv, k);
    if (tw) {
      Vec<NH> cc{};
      cc[0] = (uint32_t)cv;
      if (NH > 1) cc[1] = (uint32_t)(cv >> 32);
      uint32_t enc[E::TW];
      P.EH.encode(cc, enc);
      static_assert(sizeof(typename E::Tw) == E::TW * 4, "a twiddle is its table entry");
      memcpy(tw, enc, sizeof *tw);
    }
    return true;
  }
};

}  // namespace
