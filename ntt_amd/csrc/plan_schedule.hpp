// The radix scheduler: which pass radices a transform of 2^log_n points takes on an engine, given the
// engine's parameters as plain numbers (engines.hpp: TILE_LOG, MIN_COLS_LOG, NARROW_FIRST).  Standard
// C++ only, so that the host checker tests/c/schedule_check.cpp pins every schedule without a GPU.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdlib>

#include "plan_knobs.hpp"

namespace {

// radices for log_n: near-equal split with each radix <= tile_log - min_cols_log so that every
// global access is a contiguous run of T = TILE / R >= 2^min_cols_log elements (>= 128 B).
// The pass kernels also need every column pass's block to span a whole tile (N_i = R_i ... R_p >=
// TILE, so a workgroup's T columns lie in one block) and the final pass's T blocks to fit in R_1
// (r_1 + r_p >= tile_log).  The near-equal split violates that only for short 3-pass schedules of
// big tiles (2^19 on the 8192-element P tiles: 7+6+6); ascending order fixes every such case.
static bool schedule_ok(const unsigned* r, unsigned p, unsigned tile_log) {
  if (p < 2) return true;
  if (r[0] + r[p - 1] < tile_log) return false;
  unsigned tail = r[p - 1];
  for (int i = (int)p - 2; i >= 0; --i) {
    tail += r[i];
    if (tail < tile_log) return false;
  }
  return true;
}
// narrow_first (HBM-bound engines): pass 1, whose columns are n / R_1 elements apart, takes a radix
// one below the rest so that its workgroups read twice as wide runs (2^24 P: 7+8+9 instead of 8+8+8).
// NTT_SCHEDULE="r1,r2,..." (experiments only): that radix sequence for the sizes it sums to, when the
// pass kernels accept it.
static bool schedule_env(unsigned log_n, unsigned tile_log, unsigned rmax, unsigned* r, unsigned& p) {
  const char* v = knob::schedule();
  if (!v) return false;
  unsigned rr[8], pp = 0, sum = 0;
  for (const char* c = v; *c && pp < 8;) {
    const unsigned x = (unsigned)strtoul(c, const_cast<char**>(&c), 10);
    if (x < 3 || x > rmax) return false;
    rr[pp++] = x;
    sum += x;
    if (*c == ',') ++c;
    else if (*c) return false;
  }
  if (sum != log_n || pp < 2 || !schedule_ok(rr, pp, tile_log)) return false;
  for (unsigned i = 0; i < pp; ++i) r[i] = rr[i];
  p = pp;
  return true;
}
static bool schedule(unsigned log_n, unsigned tile_log, unsigned min_cols_log, bool narrow_first, unsigned* r,
                     unsigned& p) {
  if (log_n <= 2) { p = 0; return true; }
  if (log_n <= tile_log) { p = 1; r[0] = log_n; return true; }
  if (schedule_env(log_n, tile_log, tile_log - min_cols_log, r, p)) return true;
  const unsigned rmax = tile_log - min_cols_log;
  p = (log_n + rmax - 1) / rmax;
  if (p < 2) p = 2;
  const unsigned base = log_n / p, rem = log_n % p;
  for (unsigned i = 0; i < p; ++i) r[i] = base + (i < rem ? 1 : 0);
  if (narrow_first) {
    std::sort(r, r + p);
    if (r[p - 1] < rmax && r[0] > 3) {
      r[0] -= 1;
      r[p - 1] += 1;
      std::sort(r + 1, r + p);
      if (!schedule_ok(r, p, tile_log)) { r[0] += 1; r[p - 1] -= 1; std::sort(r, r + p); }
    }
  }
  if (!schedule_ok(r, p, tile_log)) std::sort(r, r + p);
  if (schedule_ok(r, p, tile_log)) return true;
  // Neither split passes (4096-element tiles with radices <= 2^8 at 2^17: 5+6+6 has r_1 + r_p = 11):
  // the ascending sequence of p radices in [3, rmax] that does, with the smallest largest radix, then
  // the largest smallest one (2^17: 5+5+7).
  unsigned best[8] = {0}, v[8] = {0}, bmax = 99, bmin = 0;
  for (unsigned i = 0; i < p; ++i) v[i] = 3;
  for (;;) {
    unsigned sum = 0;
    for (unsigned i = 0; i < p; ++i) sum += v[i];
    if (sum == log_n && schedule_ok(v, p, tile_log) && (v[p - 1] < bmax || (v[p - 1] == bmax && v[0] > bmin))) {
      bmax = v[p - 1];
      bmin = v[0];
      for (unsigned i = 0; i < p; ++i) best[i] = v[i];
    }
    int k = (int)p - 1;  // next non-decreasing sequence
    while (k >= 0 && v[k] == rmax) --k;
    if (k < 0) break;
    ++v[k];
    for (unsigned i = k + 1; i < p; ++i) v[i] = v[k];
  }
  if (bmax == 99) return false;
  for (unsigned i = 0; i < p; ++i) r[i] = best[i];
  return true;
}

// The schedule of an engine: schedule() at the engine's MIN_COLS_LOG (the narrowest column group its
// kernels are instantiated for).  An engine may name a wider group it prefers (pref_cols_log >
// min_cols_log): that schedule is taken instead wherever it exists with the same number of passes.
static bool schedule_for(unsigned log_n, unsigned tile_log, unsigned min_cols_log, unsigned pref_cols_log,
                         bool narrow_first, unsigned* r, unsigned& p) {
  if (!schedule(log_n, tile_log, min_cols_log, narrow_first, r, p)) return false;
  if (pref_cols_log > min_cols_log) {
    unsigned r2[8] = {0}, p2 = 0;
    if (p >= 2 && !knob::schedule() && schedule(log_n, tile_log, pref_cols_log, narrow_first, r2, p2) && p2 == p)
      for (unsigned i = 0; i < p; ++i) r[i] = r2[i];
  }
  return true;
}

// The schedule of the row-major matrix calls (ntt_*_matrix): the transforms run down the columns of a
// [n][width] matrix, a workgroup's tile being (TILE >> tb) transform positions by a strip of 2^tb
// adjacent columns.  Every global access is then a run of 2^tb elements per row, and the rule is that a
// run is at least 64 bytes (half a line): tb >= strip_log (2^4 columns of 4 B, 2^3 of 8 B), so a radix
// is at most tile_log - strip_log.  The batched schedule does not serve: it puts up to a whole tile of
// one transform in a workgroup, which here is one element per row.
//   * log_n <= 2: p = 0 (the naive kernel);
//   * else p = ceil(log_n / rmax) passes, the near-equal split in ascending order (each radix >= 3
//     since rmax >= 6); p = 1 is a column pass over the strip's columns alone.
// tb[i], the strip of pass i, may differ between passes (the addresses do not depend on it).  Its range:
// the tile's columns hold a strip (tb <= tile_log - r_i); a column pass's block spans a tile
// (log N_i + tb >= tile_log); the final pass's blocks fit in R_1 (r_1 + r_p + tb >= tile_log).  Within
// the range, the tb whose strips cover the row with the fewest masked columns, the smallest such.
static bool schedule_matrix(unsigned log_n, unsigned tile_log, unsigned strip_log, unsigned width, unsigned* r,
                            unsigned* tb, unsigned& p) {
  const unsigned rmax = tile_log - strip_log;
  if (rmax < 6 || width == 0) return false;
  if (log_n <= 2) { p = 0; return true; }
  p = (log_n + rmax - 1) / rmax;
  if (p > 8) return false;
  const unsigned base = log_n / p, rem = log_n % p;
  for (unsigned i = 0; i < p; ++i) r[i] = base + (i + rem >= p ? 1 : 0);
  unsigned blk = log_n;  // log N_i
  for (unsigned i = 0; i < p; ++i) {
    const bool final_pass = p >= 2 && i + 1 == p;
    const unsigned span = final_pass ? r[0] + r[p - 1] : blk;
    unsigned lo = span >= tile_log ? 0 : tile_log - span;
    if (lo < strip_log) lo = strip_log;
    const unsigned hi = tile_log - r[i];
    if (lo > hi) return false;
    unsigned best = lo;
    unsigned long long best_cols = ~0ull;
    for (unsigned t = lo; t <= hi; ++t) {
      const unsigned long long cols = (((unsigned long long)width + (1ull << t) - 1) >> t) << t;
      if (cols < best_cols) best_cols = cols, best = t;
    }
    tb[i] = best;
    blk -= r[i];
  }
  return true;
}

// NTT_PLAN_IN_PLACE: a palindromic sequence (r_i = r_{p-1-i}, 3 <= r_i <= rmax, schedule_ok) with the
// fewest passes (>= p0), then the smallest largest radix, then the largest smallest one.  The digit
// reversal of a palindromic sequence is an involution (k_digitrev_swap).
static bool schedule_palindrome(unsigned log_n, unsigned tile_log, unsigned rmax, unsigned p0, unsigned* r,
                                unsigned& p) {
  if (rmax < 3) return false;
  const unsigned span = rmax - 2;  // radices 3..rmax
  for (unsigned pp = (p0 < 2 ? 2 : p0); pp <= 8; ++pp) {
    const unsigned h = (pp + 1) / 2;
    unsigned combos = 1;
    for (unsigned i = 0; i < h; ++i) combos *= span;
    unsigned best[8] = {0}, bmax = 99, bmin = 0;
    for (unsigned code = 0; code < combos; ++code) {
      unsigned v[8], c = code, sum = 0, mx = 0, mn = 99;
      for (unsigned i = 0; i < h; ++i) {
        v[i] = 3 + c % span;
        c /= span;
      }
      for (unsigned i = 0; i < pp; ++i) {
        v[i] = v[i < h ? i : pp - 1 - i];
        sum += v[i];
        mx = v[i] > mx ? v[i] : mx;
        mn = v[i] < mn ? v[i] : mn;
      }
      if (sum != log_n || !schedule_ok(v, pp, tile_log)) continue;
      if (mx < bmax || (mx == bmax && mn > bmin)) {
        bmax = mx;
        bmin = mn;
        for (unsigned i = 0; i < pp; ++i) best[i] = v[i];
      }
    }
    if (bmax != 99) {
      p = pp;
      for (unsigned i = 0; i < pp; ++i) r[i] = best[i];
      return true;
    }
  }
  return false;
}

// The final pass's middle digits k_2 .. k_{p-1} of a schedule r[0..p), least significant (k_{p-1})
// first: bits[m] is the digit's width, off[m] its bit offset (relative to R_1) in the output position
// (PassArgs::mid_bits / mid_off).  Writes p - 2 entries; nothing for p <= 2.
template <class T>
static void mid_digits(const unsigned* r, unsigned p, T* bits, T* off) {
  for (unsigned m = 0; m + 2 < p; ++m) {
    const unsigned idx = p - 2 - m;  // pass index (0-based) of digit k_{idx+1}
    bits[m] = r[idx];
    unsigned o = 0;
    for (unsigned j = 1; j < idx; ++j) o += r[j];
    off[m] = o;
  }
}

// Two byte ranges share an address (ranges that touch do not).  The calls that read one buffer while
// other workgroups already write another refuse such arguments.
static bool overlaps(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
  const uintptr_t a0 = (uintptr_t)a, a1 = a0 + a_bytes, b0 = (uintptr_t)b, b1 = b0 + b_bytes;
  return a0 < b1 && b0 < a1;
}

// The checks of the prover-stage calls (plan_prover.hpp) that need no plan.
// An element is one of F_p (d = 1) or of F_p[X]/(X^d - W), d = 2 or 4
static bool degree_ok(unsigned d) { return d == 1 || d == 2 || d == 4; }
// Every pointer given (null: none) is 16-byte aligned: the kernels may then use 16-byte accesses
static bool aligned16(const void* a, const void* b = nullptr, const void* c = nullptr) {
  return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) == 0;
}
// A [2^log_rows][width] matrix is not empty and every index of an element of it fits 32 bits
static bool fits32(unsigned width, unsigned log_rows) {
  return width != 0 && log_rows < 32 && ((uint64_t)width << log_rows) < (1ull << 32);
}

}  // namespace
