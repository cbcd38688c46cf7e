// Host program for tests/test_fused_layout_host.py: prints what ntt_amd/csrc/plan_fused.hpp (the text the
// plans run) gives the single-launch schedules.  For every radix triple on the command line, at its
// natural size 2^(r1 + r2 + r3) on 2^TILE_LOG-element tiles, in modes 0 and 1, with room for fewer and for
// more workgroups than tiles: every field of the geometry and the sync words that follow from it.  Then the
// sync-word layout of the forms with 1 .. 4 grid barriers.  Builds with any host C++17 compiler; its own
// main, so the sanitized build preloads nothing.
//   fused_layout_check TILE_LOG R1:R2:R3 ...
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "plan_fused.hpp"

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const unsigned tl = (unsigned)atoi(argv[1]);
  for (int a = 2; a < argc; ++a) {
    unsigned r1 = 0, r2 = 0, r3 = 0;
    if (sscanf(argv[a], "%u:%u:%u", &r1, &r2, &r3) != 3 || r1 > tl || r2 > tl || r3 > tl || r1 + r2 + r3 < tl) {
      fprintf(stderr, "fused_layout_check: bad triple %s\n", argv[a]);
      return 2;
    }
    const uint64_t n = 1ull << (r1 + r2 + r3);
    const uint32_t tiles = (uint32_t)(n >> tl);
    for (uint32_t mode = 0; mode < 2; ++mode) {
      for (uint32_t cap : {tiles / 2 + 1, 2 * tiles}) {
        const ntt::FusedGeom F = ntt::fused_geometry(tl, n, r1, r2, r3, cap, mode);
        printf("geom %u %u %u mode %u cap %u:", r1, r2, r3, mode, cap);
        if (!F.ok) {
          printf(" REFUSED\n");
          continue;
        }
        printf(" tiles %u nwg %u k1_mask %u k1_shift %u cg_log %u k2_shift %u t3_log %u r2 %u n12 %u n23 %u need12 %u "
               "need23 %u mode %u rbase %u abort %u shards %u total %u\n",
               F.tiles, F.nwg, F.k1_mask, F.k1_shift, F.cg_log, F.k2_shift, F.t3_log, F.r2, F.n12, F.n23, F.need12,
               F.need23, F.mode, F.rbase, F.sync().abort_word(), F.sync().shards(), F.sync().total());
      }
    }
  }
  for (uint32_t k = 1; k <= 4; ++k) {
    const ntt::FusedSync S = ntt::fused_sync_barriers(k);
    printf("barriers %u: rbase %u go", k, S.rbase);
    for (uint32_t b = 1; b <= k; ++b) printf(" %u", S.go(b));
    printf(" abort %u shards %u total %u\n", S.abort_word(), S.shards(), S.total());
  }
  return 0;
}
