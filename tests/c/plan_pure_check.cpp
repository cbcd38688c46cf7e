// Host program for tests/test_plan_pure_host.py: the pure helpers the plan's parts share, from
// ntt_amd/csrc/plan_schedule.hpp (the text the plans run).  Prints the final pass's middle digits
// (mid_digits) for every schedule of three or more passes in the schedule table given as argv[1], then
// overlaps() on edge values.  Builds with any host C++17 compiler; its own main, so the sanitized build
// preloads nothing.
#include <cstdio>
#include <cstring>
#include <sstream>
#include <string>

#include "plan_schedule.hpp"

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  char line[256];
  while (fgets(line, sizeof line, f)) {
    std::istringstream in(line);
    std::string name, kind;
    unsigned log_n = 0, r[8] = {0}, p = 0, x = 0;
    if (!(in >> name >> kind >> log_n) || (kind != "sched" && kind != "pal")) continue;
    while (p < 8 && in >> x) r[p++] = x;
    if (p < 3) continue;
    uint32_t bits[8] = {0}, off[8] = {0};
    mid_digits(r, p, bits, off);
    printf("%s %s %u bits", name.c_str(), kind.c_str(), log_n);
    for (unsigned m = 0; m + 2 < p; ++m) printf(" %u", bits[m]);
    printf(" off");
    for (unsigned m = 0; m + 2 < p; ++m) printf(" %u", off[m]);
    printf(" rest %u %u\n", bits[p - 2], off[p - 2]);  // nothing is written past p - 2 entries
  }
  fclose(f);
  static char buf[64];
  const struct { size_t a, an, b, bn; } cases[] = {
      {0, 16, 16, 16},  // touching: a ends where b starts
      {16, 16, 0, 16},  // touching, the other way round
      {0, 17, 16, 16},  // one shared byte
      {16, 16, 0, 17},
      {0, 64, 8, 8},    // b inside a
      {8, 8, 0, 64},    // a inside b
      {8, 8, 8, 8},     // the same range
      {0, 0, 0, 16},    // an empty range at the edge: no
      {8, 0, 0, 16},    // an empty range strictly inside counts (the comparison the calls have always made)
      {0, 8, 32, 8},    // apart
  };
  for (const auto& c : cases)
    printf("overlaps [%zu,+%zu) [%zu,+%zu) %d\n", c.a, c.an, c.b, c.bn, (int)overlaps(buf + c.a, c.an, buf + c.b, c.bn));
  return 0;
}
