// The host side's arithmetic of the single-launch schedules (k_fused3 / k_fused3b / k_fused3bi, k_fused2b /
// k_fused2bi in ntt_fused_impl.hpp): where a launch's sync words live, and which counters the tiles of the
// dataflow form hand off through.  Pure functions of integers, no HIP: tests/c/fused_layout_check.cpp
// prints them on the host and tests/test_fused_layout_host.py pins the table.
#pragma once
#include <stdint.h>

namespace ntt {

// Grid barriers of each barrier form (the in-place forms count the residency decision as barrier 1).
// k_fused2b shares k_fused2bi's words and uses the first go word only.
enum : uint32_t { FUSED3B_BARRIERS = 2, FUSED3BI_BARRIERS = 4, FUSED2B_BARRIERS = 1, FUSED2BI_BARRIERS = 3 };
constexpr uint32_t kSyncLine = 32;     // words of a 128-byte line: every polled word has a line of its own
constexpr uint32_t kSyncShards = 8;    // arrival shards of a grid barrier (workgroup b adds to shard b mod 8)

// Sync words of one single launch, zero before the first launch and re-zeroed by the last workgroup out:
//   [0, rbase)   counters: [0] tile ticket / top arrivals, [1] workgroups exited (the dataflow form: then
//                its hand-off counters, FusedArgs)
//   `lines` lines from rbase: the go word of barrier k = 1.. (the dataflow form: one ready word per counter)
//   the abort line (Watchdog::abort), then the eight shard lines (FusedArgs::shards)
struct FusedSync {
  uint32_t rbase, lines;
  constexpr uint32_t go(uint32_t k) const { return rbase + kSyncLine * (k - 1); }
  constexpr uint32_t abort_word() const { return rbase + kSyncLine * lines; }
  constexpr uint32_t shards() const { return abort_word() + kSyncLine; }
  constexpr uint32_t total() const { return shards() + kSyncLine * kSyncShards; }
};
// a form of `barriers` grid barriers: one counter line, a line per barrier
constexpr FusedSync fused_sync_barriers(uint32_t barriers) { return FusedSync{kSyncLine, barriers}; }

// Geometry of the three-pass single launch of n = 2^(r1 + r2 + r3) elements on 2^tile_log-element tiles
// with room for `cap` resident workgroups (FusedArgs has the members' meaning).  ok = false: the radices
// break the kernel's contract (schedule_ok guarantees it for the plans' own schedules).
struct FusedGeom {
  bool ok;
  uint32_t tiles, nwg, k1_mask, k1_shift, cg_log, k2_shift, t3_log, r2, n12, n23, need12, need23, mode, rbase;
  // the dataflow form's words: its counters, then a ready line per counter (mode 1 takes its two go
  // words from the same lines: n12 + n23 >= 2)
  constexpr FusedSync sync() const { return FusedSync{rbase, n12 + n23}; }
};
inline FusedGeom fused_geometry(unsigned tl, uint64_t n, unsigned r1, unsigned r2, unsigned r3, uint32_t cap,
                                uint32_t mode) {
  FusedGeom F{};
  const unsigned lt1 = tl - r1, lt2 = tl - r2, lt3 = tl - r3, lu = lt1 > lt2 ? lt1 : lt2;
  if (r3 < lu || r1 < lt3) return F;
  F.ok = true;
  F.tiles = (uint32_t)(n >> tl);
  F.nwg = F.tiles < cap ? F.tiles : cap;
  F.k1_mask = (1u << (r3 - lt1)) - 1;
  F.k1_shift = lu - lt1;
  F.cg_log = r3 - lt2;
  F.k2_shift = lu - lt2;
  F.t3_log = lt3;
  F.r2 = r2;
  F.n12 = 1u << (r3 - lu);
  F.n23 = 1u << (r1 - lt3);
  F.need12 = 1u << (lu - lt1 + r2);
  F.need23 = 1u << r2;
  F.mode = mode;
  F.rbase = (4 + F.n12 + F.n23 + 31) & ~31u;
  return F;
}

}  // namespace ntt
