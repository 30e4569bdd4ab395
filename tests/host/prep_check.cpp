// Host check of pygpa_amd/csrc/gpa_prep.h (no GPU, no HIP): the disk chords against the (2r+1)^2 array, the reflect coverage
// interval against a walked extension, and the trim loop against the reference's rule applied to whole windows.
// Built and run by tests/test_prep_host.py, plain and under -fsanitize=address,undefined.  Prints "OK <checks>".
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "gpa_prep.h"

using namespace gpa;

static long checks = 0;
#define CHECK(cond, ...)                                   \
  do {                                                     \
    ++checks;                                              \
    if (!(cond)) {                                         \
      printf("FAIL %s:%d: ", __FILE__, __LINE__);          \
      printf(__VA_ARGS__);                                 \
      printf("\n");                                        \
      exit(1);                                             \
    }                                                      \
  } while (0)

static void check_fold() {
  for (int n = 1; n <= 9; ++n) {
    // walk the extension a b c d | d c b a | a b c d upwards from index 0: at an edge the sample repeats and the walk turns.
    // Index -1 - k holds what index k holds (the mirror sits half a sample before index 0).
    std::vector<int> up;
    int pos = 0, dir = 1;
    for (int k = 0; k < 6 * n; ++k) {
      up.push_back(pos);
      const int nx = pos + dir;
      if (nx < 0 || nx >= n) dir = -dir;
      else pos = nx;
    }
    for (int i = -5 * n; i < 6 * n; ++i) {
      const int want = i >= 0 ? up[i] : up[-1 - i];
      CHECK(prep_fold(i, n) == want, "fold(%d, %d) = %d, walked %d", i, n, prep_fold(i, n), want);
    }
  }
}

static void check_interval() {
  for (int n = 1; n <= 23; ++n)
    for (int R = 0; R <= 3 * n + 2; ++R)
      for (int i = 0; i < n; ++i) {
        std::vector<char> seen(n, 0);
        for (int d = -R; d <= R; ++d) seen[prep_fold(i + d, n)] = 1;
        int lo = n, hi = -1, count = 0;
        for (int k = 0; k < n; ++k)
          if (seen[k]) { lo = k < lo ? k : lo; hi = k; ++count; }
        CHECK(count == hi - lo + 1, "n %d R %d i %d: the folded run is not an interval", n, R, i);
        int l2, h2;
        prep_reflect_interval(i, R, n, &l2, &h2);
        CHECK(l2 == lo && h2 == hi, "n %d R %d i %d: [%d, %d], walked [%d, %d]", n, R, i, l2, h2, lo, hi);
        if (i + 1 < n) {   // the ends move by at most one sample per step: what the sliding count of the column pass needs
          int l3, h3;
          prep_reflect_interval(i + 1, R, n, &l3, &h3);
          CHECK(abs(l3 - l2) <= 1 && abs(h3 - h2) <= 1, "n %d R %d i %d: an end jumps", n, R, i);
        }
      }
  // a radius and a length of the size the kernels see: no overflow
  int lo, hi;
  prep_reflect_interval(5, 16384, 65536, &lo, &hi);
  CHECK(lo == 0 && hi == 16389, "large interval [%d, %d]", lo, hi);
  prep_reflect_interval(65530, 70000, 65536, &lo, &hi);
  CHECK(lo == 0 && hi == 65535, "large interval [%d, %d]", lo, hi);
}

static void check_chords() {
  for (int v = 0; v < 70000; ++v) {
    const int s = prep_isqrt(v);
    CHECK((long long)s * s <= v && (long long)(s + 1) * (s + 1) > v, "isqrt(%d) = %d", v, s);
  }
  CHECK(prep_isqrt(2147395600) == 46340 && prep_isqrt(2147483647) == 46340, "isqrt near 2^31");
  const int radii[] = {0, 1, 2, 3, 5, 20, 21, 100, PREP_MAX_R};
  for (int r : radii)
    for (int dy = -r; dy <= r; ++dy) {
      // row dy of the (2r+1)^2 array X^2 + Y^2 <= r^2
      int lo = r + 1, hi = -r - 1, count = 0;
      for (int dx = -r; dx <= r; ++dx)
        if (dx * dx + dy * dy <= r * r) { lo = dx < lo ? dx : lo; hi = dx; ++count; }
      const int c = prep_disk_chord(r, dy);
      CHECK(lo == -c && hi == c && count == 2 * c + 1, "disk(%d) row %d: chord %d, array [%d, %d]", r, dy, c, lo, hi);
      CHECK(c <= 254 + (r > 254), "a chord that does not fit the byte comparison");
    }
}

// the trim loop against the rule applied to the whole window each round (what the reference does)
struct HostCounter {
  const std::vector<char>& nan;
  int n1;
  long lines = 0;
  int row(int x, int y0, int y1) { ++lines; int v = 0; for (int y = y0; y < y1; ++y) v += nan[(size_t)x * n1 + y]; return v; }
  int col(int y, int x0, int x1) { ++lines; int v = 0; for (int x = x0; x < x1; ++x) v += nan[(size_t)x * n1 + y]; return v; }
  int at(int x, int y) const { return nan[(size_t)x * n1 + y]; }
};

static void reference_trim(const std::vector<char>& nan, int n0, int n1, int lims[4]) {
  int x0 = 0, x1 = n0, y0 = 0, y1 = n1;
  while (x1 > x0 && y1 > y0) {
    int r[2] = {0, 0}, c[2] = {0, 0};
    for (int y = y0; y < y1; ++y) { r[0] += nan[(size_t)x0 * n1 + y]; r[1] += nan[(size_t)(x1 - 1) * n1 + y]; }
    for (int x = x0; x < x1; ++x) { c[0] += nan[(size_t)x * n1 + y0]; c[1] += nan[(size_t)x * n1 + y1 - 1]; }
    if (r[0] + r[1] == 0 && c[0] + c[1] == 0) break;
    if (r[0] + r[1] > c[0] + c[1]) { x0 += r[0] > 0; x1 -= r[1] > 0; }
    else { y0 += c[0] > 0; y1 -= c[1] > 0; }
  }
  lims[0] = x0; lims[1] = x1; lims[2] = y0; lims[3] = y1;
}

static void check_trim() {
  unsigned long long state = 12345;
  auto rnd = [&state]() { state = state * 6364136223846793005ull + 1442695040888963407ull; return (unsigned)(state >> 33); };
  for (int trial = 0; trial < 4000; ++trial) {
    const int n0 = 1 + rnd() % 9, n1 = 1 + rnd() % 9;
    std::vector<char> nan((size_t)n0 * n1, 0);
    const int kind = trial % 4;
    for (int x = 0; x < n0; ++x)
      for (int y = 0; y < n1; ++y) {
        const int edge = x < (int)(rnd() % 3) || y < (int)(rnd() % 3) || n0 - 1 - x < (int)(rnd() % 3) || n1 - 1 - y < (int)(rnd() % 2);
        if (kind == 0) nan[(size_t)x * n1 + y] = edge;                       // ragged borders
        else if (kind == 1) nan[(size_t)x * n1 + y] = rnd() % 7 == 0;          // specks (ties, emptied windows)
        else if (kind == 2) nan[(size_t)x * n1 + y] = edge || rnd() % 23 == 0;
        else nan[(size_t)x * n1 + y] = trial % 8 == 3;                         // all NaN / none
      }
    int want[4], got[4];
    reference_trim(nan, n0, n1, want);
    HostCounter c{nan, n1};
    prep_trim_loop(c, n0, n1, got);
    for (int k = 0; k < 4; ++k)
      CHECK(got[k] == want[k], "trial %d (%d x %d): lims[%d] = %d, the rule gives %d", trial, n0, n1, k, got[k], want[k]);
    // never a rescan of the window: at most the four first lines, then two (new end, or both ends of a single line) per dropped line
    CHECK(c.lines <= 4 + 3L * (n0 + n1), "trial %d: %ld line counts", trial, c.lines);
  }
  // the tie goes to the columns: one NaN in the corner
  {
    std::vector<char> nan(12, 0);
    nan[0] = 1;
    HostCounter c{nan, 4};
    int l[4];
    prep_trim_loop(c, 3, 4, l);
    CHECK(l[0] == 0 && l[1] == 3 && l[2] == 1 && l[3] == 4, "tie: %d %d %d %d", l[0], l[1], l[2], l[3]);
  }
}

int main() {
  check_fold();
  check_interval();
  check_chords();
  check_trim();
  printf("OK %ld\n", checks);
  return 0;
}
