// Host program for tests/test_plan_pure_host.py: the pure helpers the plan's parts share, from
// ntt_amd/csrc/plan_schedule.hpp (the text the plans run).  Prints the final pass's middle digits
// (mid_digits) for every schedule of three or more passes in the schedule table given as argv[1], then
// overlaps() on edge values, then degree_ok(), fits32() and aligned16() on theirs.  Builds with any host C++17
// compiler; its own main, so the sanitized build preloads nothing.
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
  // the prover-stage calls' checks that need no plan
  for (unsigned d : {0u, 1u, 2u, 3u, 4u, 8u}) printf("degree_ok %u %d\n", d, (int)degree_ok(d));
  const struct { unsigned width, log_rows; } shapes[] = {
      {0, 0},  {0, 10},                // no columns
      {1, 0},  {1, 31}, {1, 32},       // log_rows 31 is the last that fits, 32 is no shift of a 32-bit width
      {2, 31}, {3, 30},                // 2^32 and 3 2^30
      {0xffffffffu, 0}, {0xffffffffu, 1},  // width << log_rows = 2^32 - 1 fits, 2^33 - 2 does not
      {0x80000000u, 1}, {0x7fffffffu, 1},  // 2^32 exactly does not, 2^32 - 2 does
      {1u << 16, 16}, {(1u << 16) - 1, 16}, {5, 40},
  };
  for (const auto& c : shapes) printf("fits32 %u %u %d\n", c.width, c.log_rows, (int)fits32(c.width, c.log_rows));
  alignas(16) static char al[64];
  const struct { int a, b, c; } ptrs[] = {  // byte offsets into a 16-byte aligned buffer, -1: a null pointer
      {0, -1, -1}, {16, 32, 48}, {0, 0, 0}, {8, -1, -1}, {0, 8, -1}, {0, 16, 8}, {8, 16, 32}, {16, 32, 1}, {-1, -1, -1},
  };
  auto at = [&](int off) { return off < 0 ? nullptr : al + off; };
  for (const auto& c : ptrs) {
    const int got = c.b < 0 ? (int)aligned16(at(c.a)) : c.c < 0 ? (int)aligned16(at(c.a), at(c.b))
                                                                : (int)aligned16(at(c.a), at(c.b), at(c.c));
    printf("aligned16 %d %d %d %d\n", c.a, c.b, c.c, got);
  }
  return 0;
}
