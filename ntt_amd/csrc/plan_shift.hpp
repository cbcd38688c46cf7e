// Coset transforms and low-degree extensions: the tables of the cached shift c and the calls that use
// them (ntt_forward_coset / ntt_inverse_coset, ntt_lde_batch).  A plan owns one Shift and hands it a
// reference to itself; the matrix transforms read the cached tables through the plan.  Included by
// ntt_plan.cpp alone.
#pragma once
#include <vector>

#include "ntt_kernels.hpp"
#include "plan_devmem.hpp"
#include "plan_hostmath.hpp"
#include "plan_schedule.hpp"

namespace {

template <class E, class Plan>
struct Shift {
  static constexpr int NH = EngHost<E>::NH, MEMW = E::MEMW, TABW = E::TABW;
  Plan& P;
  explicit Shift(Plan& plan) : P(plan) {}

  // ---- the shift cache: data[j] *= c^j before the forward, c^-j after the inverse
  std::vector<uint32_t> coset_key;  // shift c (NH words) of the cached tables
  DevBuf d_coset;
  DevBuf d_coset_full;  // fused coset forward: pass-1 outer twiddles x c^col (n entries)
  bool coset_full_ok = false;
  size_t coset_off[2][3] = {};  // [dir][lo_s, hi, u^d (forward only)] word offsets into d_coset
  DevBuf d_lde_stage;           // ntt_lde_batch: scaled inputs of the engines without the product at load

  // the two-level tables of c^j (dir 0) / c^-j (dir 1): lo scaled by R_e, hi
  const uint32_t* lo(int dir) const { return d_coset.get() + coset_off[dir][0]; }
  const uint32_t* hi(int dir) const { return d_coset.get() + coset_off[dir][1]; }
  const uint32_t* u_pow() const { return d_coset.get() + coset_off[0][2]; }  // u^d, u = c^(n / R_1), d < R_1

  // The cached c^j tables (d_coset) of `shift`: checked (canonical, nonzero) and rebuilt when it changed
  int ensure_tables(const uint64_t* shift, unsigned limbs64) {
    Vec<NH> c{};
    if (!P.H.canonical(shift, limbs64, c) || c == Vec<NH>{}) return NTT_ERR_ARG;
    const std::vector<uint32_t> key(c.begin(), c.end());
    if (key != coset_key) {
      d_coset.reset();
      coset_key.clear();
      std::vector<uint32_t> host;
      const unsigned lo_bits = P.lo_bits;
      const Vec<NH> cm = P.H.to_mont(c);
      const Vec<NH> cim = P.H.pow(cm, P.pm2_);
      for (int dir = 0; dir < 2; ++dir) {
        const Vec<NH>& b = dir ? cim : cm;
        coset_off[dir][0] = P.push_powers_to(host, b, 1ull << lo_bits, nullptr, true);
        const Vec<NH> step = P.H.pow_u64(b, 1ull << lo_bits);
        coset_off[dir][1] = P.push_powers_to(host, step, 1ull << (P.log_n - lo_bits), nullptr, false);
      }
      // fused forward: u^d, u = c^s (s = n / R_1 columns of pass 1), d < R_1, Shoup entries
      if (P.npass >= 2)
        coset_off[0][2] = P.push_powers_to(host, P.H.pow_u64(cm, P.n >> P.r[0]), 1ull << P.r[0], nullptr, false);
      coset_full_ok = false;
      if (!d_coset.alloc(host.size() * 4)) return NTT_ERR_HIP;
      if (hipMemcpy(d_coset.get(), host.data(), host.size() * 4, hipMemcpyHostToDevice) != hipSuccess) return NTT_ERR_HIP;
      coset_key = key;
    }
    return NTT_OK;
  }
  // Pass-1 outer-twiddle table of the fused coset forward for the cached shift c: entry (col, k) =
  // w_n^(col k) c^col R_e, layout of d_full (built on the device once per shift).
  int ensure_full() {
    if (coset_full_ok) return NTT_OK;
    if (!d_coset_full && !d_coset_full.alloc((size_t)P.n * TABW * 4)) return NTT_ERR_HIP;
    if (launch_build_tw<E>(d_coset_full.get(), P.n, P.r[0], tile_log_of<E>() - P.r[0], 0, P.outer_lo(0), P.outer_hi(0, 0),
                           P.lo_bits, P.Ff, nullptr, lo(0), hi(0)) != hipSuccess ||
        hipDeviceSynchronize() != hipSuccess)
      return NTT_ERR_HIP;
    coset_full_ok = true;
    return NTT_OK;
  }
  // the scale rides in pass 1: u^d at load, c^col in the outer twiddles
  bool fusable() const { return P.use_full && P.npass >= 2 && Plan::fast(P.Ff); }

  int coset(void* d, const uint64_t* shift, unsigned limbs64, bool inverse, hipStream_t st) {
    if (!d || !shift || (P.flags & NTT_PLAN_TWIDDLE_ONLY)) return NTT_ERR_ARG;
    if (int rc = ensure_tables(shift, limbs64)) return rc;
    const int dir = inverse ? 1 : 0;
    auto scale = [&]() {
      return Plan::rc_of(launch_scale_pow<E>(static_cast<uint32_t*>(d), P.log_n, 1, lo(dir), hi(dir), P.lo_bits, P.Ff, st));
    };
    if (!inverse) {
      if (fusable()) {
        if (int rc = ensure_full()) return rc;
        uint32_t* x = static_cast<uint32_t*>(d);
        return P.run_io(x, x, 1, false, st, FirstPass::coset(d_coset_full.get(), u_pow()));
      }
      if (int rc = scale()) return rc;
      return P.run(d, 1, false, st);
    }
    if (int rc = P.run(d, 1, true, st)) return rc;
    return scale();
  }

  // Low-degree extension: the first pass (PRO_LDE) reads the n_in = n >> log_blowup coefficients of
  // each input and takes the padding from registers.  The shift's c^j is applied at that load: the
  // fused coset's way (u^d at load, c^col in the cached outer table) where fusable(), else from
  // the shift's two-level tables where the pass has room (lde_mul_at_load), else by one launch over the
  // inputs into the plan's staging buffer (recorded as an unlabelled launch).  Without a shift nothing
  // of the shift cache is touched: a fusable plan's pass then takes the plan's own pass-1 table.
  // The few passes without a PRO_LDE instance (lde_pass_available), 2- and 4-point plans, and fast-
  // reduction plans that could not build their full tables go through lde_staged.
  int lde(const void* in, void* out, unsigned log_blowup, const uint64_t* shift, unsigned limbs64, unsigned batch,
          hipStream_t st) {
    if constexpr (!HasLde<E>::value) {
      return NTT_ERR_ARG;
    } else {
      const unsigned log_n = P.log_n, npass = P.npass;
      if (!in || !out || batch == 0 || log_blowup > log_n) return NTT_ERR_ARG;
      if (P.flags & (NTT_PLAN_TWIDDLE_ONLY | NTT_PLAN_IN_PLACE)) return NTT_ERR_ARG;
      const size_t n_in = (size_t)(P.n >> log_blowup), eb = (size_t)MEMW * 4;
      // the first pass reads d_in while later tiles write d_out
      if (overlaps(in, (size_t)batch * n_in * eb, out, (size_t)batch * (size_t)P.n * eb)) return NTT_ERR_ARG;
      if (shift)
        if (int rc = ensure_tables(shift, limbs64)) return rc;
      const uint32_t* src = static_cast<const uint32_t*>(in);
      uint32_t* dst = static_cast<uint32_t*>(out);
      if (log_n == 0) {  // one coefficient, one evaluation: c^0 = 1
        if (hipMemcpyAsync(dst, src, (size_t)batch * eb, hipMemcpyDeviceToDevice, st) != hipSuccess) return NTT_ERR_HIP;
        return NTT_OK;
      }
      const bool fastred = Plan::fast(P.Ff), fuse = fusable();
      const int kind = npass == 1 ? KIND_SINGLE : KIND_COLUMN;
      if (npass == 0 || !lde_pass_available<E>(kind, (int)P.r[0], fastred) || (fastred && npass >= 2 && !fuse))
        return lde_staged(src, dst, n_in, shift != nullptr, batch, st);
      if (fuse) {
        if (!shift && !P.d_fulls[0]) return lde_staged(src, dst, n_in, false, batch, st);
        if (!shift)  // the plan's own pass-1 table (element format), no product at load
          return P.run_io(src, dst, batch, false, st, FirstPass::lde_plan_table(n_in, P.d_fulls[0].get() + P.full_off[0] * TABW));
        if (int rc = ensure_full()) return rc;
        return P.run_io(src, dst, batch, false, st, FirstPass::lde_coset(n_in, d_coset_full.get(), u_pow()));
      }
      if (!shift) return P.run_io(src, dst, batch, false, st, FirstPass::lde_at_load(n_in));
      const bool at_load = npass == 1 ? lde_mul_at_load<E, KIND_SINGLE>() : lde_mul_at_load<E, KIND_COLUMN>();
      if (at_load) return P.run_io(src, dst, batch, false, st, FirstPass::lde_at_load(n_in, lo(0), hi(0)));
      // the multi-limb engines' first pass has no room for the two table entries: one launch over
      // the batch n_in inputs scales them into the plan's staging buffer, which the pass then reads
      if (!d_lde_stage.grow((size_t)batch * n_in * eb)) return NTT_ERR_HIP;
      return P.run_io(src, dst, batch, false, st, FirstPass::lde_staged(n_in, lo(0), hi(0), d_lde_stage.get()));
    }
  }

  // The zero-padded route of a low-degree extension, for the plans whose first pass has no PRO_LDE
  // form: the padded vectors are staged in d_out (memset, strided copy), scaled by c^j there
  // (k_scale_pow over the N-sized vectors) and transformed in place by the plan's plain forward.
  int lde_staged(const uint32_t* src, uint32_t* dst, size_t n_in, bool shifted, unsigned batch, hipStream_t st) {
    const size_t eb = (size_t)MEMW * 4, n = (size_t)P.n;
    if (hipMemsetAsync(dst, 0, (size_t)batch * n * eb, st) != hipSuccess ||
        hipMemcpy2DAsync(dst, n * eb, src, n_in * eb, n_in * eb, batch, hipMemcpyDeviceToDevice, st) != hipSuccess)
      return NTT_ERR_HIP;
    if (shifted && launch_scale_pow<E>(dst, P.log_n, batch, lo(0), hi(0), P.lo_bits, P.Ff, st) != hipSuccess)
      return NTT_ERR_HIP;
    return P.run_io(dst, dst, batch, false, st, FirstPass::plain());
  }
};

}  // namespace
