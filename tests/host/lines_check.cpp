// Host check of pygpa_amd/csrc/gpa_lines.h: the key maps, the rank rule, the fold, the LDS sizing and the transpose tiles,
// against brute force.  Built and run by tests/test_axis_host.py (plain, and under the host sanitizers).  Prints "OK <checks>".
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <limits>
#include <random>
#include <vector>

#include "gpa_lines.h"

using namespace gpa;

static long checks = 0;
#define CHECK(c)                                                        \
  do {                                                                  \
    ++checks;                                                           \
    if (!(c)) { printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); return 1; } \
  } while (0)

template <class F, class U> static U bits_of(F v) { U u; memcpy(&u, &v, sizeof u); return u; }
template <class F, class U> static F value_of(U u) { F v; memcpy(&v, &u, sizeof v); return v; }

// the median of the keys of a line as the kernel forms it: rank lo by sorting, rank hi by the rule
template <class F, class U>
static F median_by_rule(const std::vector<F>& line, U nankey) {
  std::vector<U> keys;
  for (F v : line) keys.push_back(lines_key(bits_of<F, U>(v)));
  const int n = (int)keys.size();
  int m = 0;
  for (U k : keys) m += k != nankey;
  if (m == 0) return std::numeric_limits<F>::quiet_NaN();
  std::vector<U> s = keys;
  std::sort(s.begin(), s.end());
  const U k1 = s[lines_rank_lo(m)];
  int le = 0;
  U above = nankey;
  for (int i = 0; i < n; ++i) {
    le += keys[i] <= k1;
    if (keys[i] > k1 && keys[i] < above) above = keys[i];
  }
  const F a = value_of<F, U>(lines_unkey(k1));
  if (m & 1) return a;
  const U k2 = lines_upper_is_same(le, m) ? k1 : above;
  return (a + value_of<F, U>(lines_unkey(k2))) * (F)0.5;
}

template <class F>
static F median_by_sort(std::vector<F> line) {
  std::vector<F> v;
  for (F x : line)
    if (x == x) v.push_back(x);
  const int m = (int)v.size();
  if (!m) return std::numeric_limits<F>::quiet_NaN();
  std::sort(v.begin(), v.end());
  return (m & 1) ? v[m / 2] : (v[m / 2 - 1] + v[m / 2]) / (F)2;
}

template <class F> static bool same(F a, F b) { return (a != a && b != b) || a == b; }

template <class F, class U>
static int check_keys(U nankey, std::mt19937_64& rng) {
  const F inf = std::numeric_limits<F>::infinity(), tiny = std::numeric_limits<F>::denorm_min(),
          small = std::numeric_limits<F>::min(), big = std::numeric_limits<F>::max();
  // in ascending order; -0 and +0 are distinct keys in this order
  const F ordered[] = {-inf, -big, (F)-2000.001, (F)-2000, (F)-1, -small, -small / 2, -tiny, (F)-0.0, (F)0.0, tiny, small / 2, small, (F)1,
                       (F)2000, (F)2000.001, big, inf};
  const int no = (int)(sizeof ordered / sizeof ordered[0]);
  for (int i = 0; i < no; ++i) {
    const U b = bits_of<F, U>(ordered[i]), k = lines_key(b);
    CHECK(!lines_is_nan(b) && k != nankey);
    CHECK(lines_unkey(k) == b);                       // invertible, the sign of zero included
    if (i) CHECK(lines_key(bits_of<F, U>(ordered[i - 1])) < k);
  }
  // every NaN pattern, either sign, quiet or signalling, is classified and gets the one key above +inf
  const F nan = std::numeric_limits<F>::quiet_NaN();
  U nb = bits_of<F, U>(nan);
  const U sign = (U)1 << (8 * sizeof(U) - 1);
  const U nans[] = {nb, (U)(nb | sign), (U)(bits_of<F, U>(inf) | 1), (U)(bits_of<F, U>(inf) | 1 | sign), (U)~(U)0, (U)(~(U)0 >> 1)};
  for (U b : nans) {
    CHECK(lines_is_nan(b) && lines_key(b) == nankey);
  }
  CHECK(lines_key(bits_of<F, U>(inf)) < nankey);
  const F back = value_of<F, U>(lines_unkey(nankey));
  CHECK(back != back);
  // random bit patterns over all exponents: monotone and invertible
  for (int t = 0; t < 200000; ++t) {
    const U a = (U)rng(), b = (U)rng();
    if (lines_is_nan(a) || lines_is_nan(b)) continue;
    const F fa = value_of<F, U>(a), fb = value_of<F, U>(b);
    const U ka = lines_key(a), kb = lines_key(b);
    CHECK(lines_unkey(ka) == a && lines_unkey(kb) == b);
    if (fa < fb) CHECK(ka < kb);
    if (fa > fb) CHECK(ka > kb);
    if (ka == kb) CHECK(a == b);
  }
  return 0;
}

template <class F, class U>
static int check_ranks(U nankey, std::mt19937_64& rng) {
  const F nan = std::numeric_limits<F>::quiet_NaN(), inf = std::numeric_limits<F>::infinity();
  const F pool[] = {(F)1, (F)1, (F)2, (F)3, (F)-1, (F)0.0, (F)-0.0, (F)2000.001, (F)2000, inf, -inf, std::numeric_limits<F>::denorm_min()};
  const int np = (int)(sizeof pool / sizeof pool[0]);
  // m = 0 .. 9 valid samples among up to 3 NaNs, many draws with ties straddling the middle
  for (int m = 0; m <= 9; ++m)
    for (int extra = 0; extra <= 3; ++extra)
      for (int t = 0; t < 300; ++t) {
        std::vector<F> line;
        for (int i = 0; i < m; ++i) line.push_back(pool[rng() % np]);
        for (int i = 0; i < extra; ++i) line.push_back(nan);
        if (line.empty()) continue;
        std::shuffle(line.begin(), line.end(), rng);
        CHECK(same(median_by_rule<F, U>(line, nankey), median_by_sort<F>(line)));
      }
  for (int m = 1; m <= 9; ++m) {
    CHECK(lines_rank_lo(m) == (m - 1) / 2 && lines_rank_hi(m) == m / 2);
    CHECK((lines_rank_lo(m) == lines_rank_hi(m)) == (m % 2 == 1));
  }
  // all equal: the upper rank is the same key; distinct: it is the next one
  CHECK(lines_upper_is_same(4, 4) && !lines_upper_is_same(2, 4) && lines_upper_is_same(3, 4));
  return 0;
}

// sample k >= 0 of the walk 0 1 .. n-1 | n-1 .. 1 0 | 0 1 ..: a step that would leave the line repeats the sample and turns round
static int ref_walk(long long k, int n) {
  int at = 0, dir = 1;
  for (long long s = 0; s < k; ++s) {
    int next = at + dir;
    if (next >= n || next < 0) { dir = -dir; next = at; }
    at = next;
  }
  return at;
}

int main() {
  std::mt19937_64 rng(12345);
  if (check_keys<float, uint32_t>(LINES_NAN_KEY32, rng)) return 1;
  if (check_keys<double, uint64_t>(LINES_NAN_KEY64, rng)) return 1;
  if (check_ranks<float, uint32_t>(LINES_NAN_KEY32, rng)) return 1;
  if (check_ranks<double, uint64_t>(LINES_NAN_KEY64, rng)) return 1;

  // the fold: against a walk of the extension, for radii many times the line (R = 800 on 5 samples)
  for (int n : {1, 2, 3, 5, 33, 64})
    for (int i = -2 * 800 - n; i <= 2 * 800 + n; ++i) {
      const int f = lines_fold(i, n);
      CHECK(f >= 0 && f < n);
      // to the left the extension mirrors the line: index -1 is sample 0 again
      const int want = i >= 0 ? ref_walk(i, n) : ref_walk(-(long long)i - 1, n);
      CHECK(f == want);
    }
  CHECK(lines_radius(200.0) == 800 && lines_radius(3.0) == 12 && lines_radius(1.0) == 4 && lines_radius(2.5) == 10);

  // LDS: the longest line fits one workgroup in both precisions, shorter ones take what they need
  CHECK(lines_length_ok(1) && lines_length_ok(LINES_MAX_N) && !lines_length_ok(LINES_MAX_N + 1) && !lines_length_ok(0));
  CHECK(LINES_MAX_N == 16384);
  CHECK(lines_lds_bytes(LINES_MAX_N, 8) == 128 * 1024 && lines_lds_bytes(LINES_MAX_N, 4) == 64 * 1024);
  CHECK(lines_lds_bytes(LINES_MAX_N, 8) + LINES_STATIC_LDS <= LINES_LDS_LIMIT);
  for (int n = 1; n <= LINES_MAX_N; n += 37)
    for (int kb : {4, 8}) {
      const size_t b = lines_lds_bytes(n, kb);
      CHECK(b >= (size_t)n * kb && b < (size_t)n * kb + 16 && b % 16 == 0);
      CHECK(lines_rounds(n) * LINES_BATCH * LINES_THREADS >= n && (lines_rounds(n) - 1) * LINES_BATCH * LINES_THREADS < n);
    }
  // the route: only f64 lines above 8192 samples need the raised limit
  CHECK(!lines_long_route(LINES_MAX_N, 4) && !lines_long_route(8192, 8) && lines_long_route(8193, 8) && lines_long_route(LINES_MAX_N, 8));
  // a 4096-point f32 line leaves room for 7 workgroups on a CU
  CHECK(7 * (lines_lds_bytes(4096, 4) + LINES_STATIC_LDS) <= LINES_LDS_LIMIT);

  // transpose tiles cover every sample once, ragged edges included
  for (int n : {1, 5, 31, 32, 33, 64, 150, 300, 16384}) {
    int covered = 0;
    for (int t = 0; t < lines_tiles(n); ++t) {
      const int e = lines_tile_extent(t, n);
      CHECK(e >= 1 && e <= LINES_TILE);
      covered += e;
    }
    CHECK(covered == n && lines_tile_extent(lines_tiles(n), n) == 0);
  }
  CHECK(LINES_TILE_PITCH == LINES_TILE + 1);
  printf("OK %ld\n", checks);
  return 0;
}
