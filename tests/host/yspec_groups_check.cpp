// The work list of the y-spectral pass A (pygpa_amd/csrc/gpa_yspec.h: yspec_groups): for live-block masks made from every band
// rotation s, NBL = 6 and 8, one to three peaks that do and do not share their planes, and caps 1, 3, 4, 6, 12 and 16, the
// groups cover every set (plane, block) bit exactly once and nothing else, none exceeds the cap, every entry of a group is
// read at the group's block, the groups come largest first, and cap 1 gives the (plane, block) pairs themselves.
//
// With arguments  <lg> <nbl> <cap> <planes per peak> <s0> [<s1> ...]  (peaks that do not share planes) it prints the groups of
// that list as "block count" lines: tests/test_yspec_groups_host.py feeds it the benchmark's band rotations.
#include <stdio.h>
#include <stdlib.h>

#include <initializer_list>
#include <set>
#include <utility>
#include <vector>

#include "gpa_yspec.h"

using namespace gpa;

static long checked = 0;

static void check(const std::vector<unsigned>& mask, int cap, const char* what) {
  const int nplanes = (int)mask.size();
  const YspecGroups yg = yspec_groups(mask.data(), nplanes, cap);
  std::set<std::pair<int, int>> want, got;
  for (int q = 0; q < nplanes; ++q)
    for (int blk = 0; blk < 16; ++blk)
      if ((mask[q] >> blk) & 1) want.insert({q, blk});
  size_t entries = 0;
  int prev = 1 << 30;
  for (const YspecGroup& g : yg.groups) {
    if (g.count < 1 || g.count > cap) { printf("%s cap %d: group of %d\n", what, cap, g.count); exit(1); }
    if (g.count > prev) { printf("%s cap %d: groups not largest first\n", what, cap); exit(1); }
    prev = g.count;
    if (g.block < 0 || g.block > 15 || g.first < 0 || (size_t)(g.first + g.count) > yg.planes.size()) { printf("%s cap %d: range\n", what, cap); exit(1); }
    for (int k = 0; k < g.count; ++k) {
      const int q = yg.planes[g.first + k];
      if (q < 0 || q >= nplanes || !((mask[q] >> g.block) & 1)) { printf("%s cap %d: plane %d does not read block %d\n", what, cap, q, g.block); exit(1); }
      if (!got.insert({q, g.block}).second) { printf("%s cap %d: (plane %d, block %d) twice\n", what, cap, q, g.block); exit(1); }
    }
    entries += g.count;
  }
  if (got != want) { printf("%s cap %d: covers %zu pairs of %zu\n", what, cap, got.size(), want.size()); exit(1); }
  if (entries != yg.planes.size()) { printf("%s cap %d: %zu entries in a list of %zu\n", what, cap, entries, yg.planes.size()); exit(1); }
  if (cap == 1) {
    // the parent's schedule: one (plane, block) pair per workgroup -- the same pairs, as a set
    std::set<std::pair<int, int>> pairs;
    for (const YspecGroup& g : yg.groups) pairs.insert({yg.planes[g.first], g.block});
    if (yg.groups.size() != want.size() || pairs != want) { printf("%s cap 1: not the pairs\n", what); exit(1); }
  }
  ++checked;
}

int main(int argc, char** argv) {
  if (argc > 5) {
    const int lg = atoi(argv[1]), nbl = atoi(argv[2]), cap = atoi(argv[3]), pp = atoi(argv[4]);
    std::vector<unsigned> mask;
    for (int a = 5; a < argc; ++a)
      for (int q = 0; q < pp; ++q) mask.push_back(yspec_blockmask(lg, atoi(argv[a]), nbl));
    const YspecGroups yg = yspec_groups(mask.data(), (int)mask.size(), cap);
    printf("entries %zu\n", yg.planes.size());
    for (const YspecGroup& g : yg.groups) printf("%d %d\n", g.block, g.count);
    return 0;
  }
  const int PP = 4;   // planes per peak (a 4 x 4 candidate grid)
  for (int lg : {11, 12})
    for (int nbl : {6, 8})
      for (int cap : {1, 3, 4, 6, 12, 16})
        for (int s0 = 0; s0 < 16; ++s0) {
          // one peak
          check(std::vector<unsigned>(PP, yspec_blockmask(lg, s0, nbl)), cap, "one peak");
          for (int s1 = 0; s1 < 16; ++s1) {
            const unsigned m0 = yspec_blockmask(lg, s0, nbl), m1 = yspec_blockmask(lg, s1, nbl);
            // two peaks on planes of their own, two peaks that share every plane (a plane's mask is a union)
            std::vector<unsigned> own(PP, m0), shared(PP, m0 | m1);
            own.insert(own.end(), PP, m1);
            check(own, cap, "two peaks");
            check(shared, cap, "two peaks, shared planes");
            // three peaks: own planes; the first two sharing theirs; rotations s0, s1 and one between them
            const unsigned m2 = yspec_blockmask(lg, (s0 + 2 * s1 + 5) & 15, nbl);
            std::vector<unsigned> three(own), mixed(shared);
            three.insert(three.end(), PP, m2);
            mixed.insert(mixed.end(), PP, m2);
            check(three, cap, "three peaks");
            check(mixed, cap, "three peaks, two sharing planes");
          }
        }
  // a plane no peak reads, and no plane at all
  check({0u, 0x00ffu, 0u}, 4, "idle plane");
  check({}, 4, "empty");
  printf("%ld lists\nOK\n", checked);
  return 0;
}
