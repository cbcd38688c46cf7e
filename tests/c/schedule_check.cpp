// Host program for tests/test_schedule_host.py: prints the pass radices that ntt_amd/csrc/plan_schedule.hpp
// (the text the plans run) gives every size 2^0 .. 2^40 for each engine-parameter tuple on the command
// line, and the palindromic schedule of the in-place plans where asked for.  NTT_SCHEDULE is read by the
// header itself.  Builds with any host C++17 compiler; its own main, so the sanitized build preloads
// nothing.
//   schedule_check NAME:TILE_LOG:MIN_COLS_LOG:PREF_COLS_LOG:NARROW_FIRST:PALINDROME ...
#include <cstdio>
#include <cstdlib>

#include "plan_schedule.hpp"

int main(int argc, char** argv) {
  const char* forced = getenv("NTT_SCHEDULE");
  printf("# NTT_SCHEDULE=%s\n", forced ? forced : "");
  for (int a = 1; a < argc; ++a) {
    char name[32];
    unsigned tl = 0, mc = 0, pc = 0, nf = 0, pal = 0;
    if (sscanf(argv[a], "%31[^:]:%u:%u:%u:%u:%u", name, &tl, &mc, &pc, &nf, &pal) != 6 || mc > tl || pc > tl) {
      fprintf(stderr, "schedule_check: bad tuple %s\n", argv[a]);
      return 2;
    }
    printf("engine %s %u %u %u %u %u\n", name, tl, mc, pc, nf, pal);
    for (unsigned log_n = 0; log_n <= 40; ++log_n) {
      unsigned r[8] = {0}, p = 0;
      const bool ok = schedule_for(log_n, tl, mc, pc, nf != 0, r, p);
      printf("%s sched %u", name, log_n);
      if (!ok) printf(" FAIL");
      for (unsigned i = 0; ok && i < p; ++i) printf(" %u", r[i]);
      printf("\n");
      if (pal && ok && p >= 2) {  // as a plan's creation does for NTT_PLAN_IN_PLACE
        const bool pok = schedule_palindrome(log_n, tl, tl - mc, p, r, p);
        printf("%s pal %u", name, log_n);
        if (!pok) printf(" NONE");
        for (unsigned i = 0; pok && i < p; ++i) printf(" %u", r[i]);
        printf("\n");
      }
    }
  }
  return 0;
}
