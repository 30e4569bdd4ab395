// Host check of pygpa_amd/csrc/gpa_wff.h (tests/test_wff_host.py compiles and runs it): the reflect fold against a
// brute-force extension, s = round(2 sigma) with Python's rounding, the LDS budget of every tile inside the limits, refusal
// just outside them, and the window -> sf-row map of the column kernel (every window position lands inside the hull).
// Prints "OK <checks>" and, for the GPU test of the tile seams, "TILE <dtype> <s> <cols> <R>" lines.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "gpa_wff.h"

using namespace gpa;

static long checks = 0;
#define CHECK(cond)                                                      \
  do {                                                                   \
    ++checks;                                                            \
    if (!(cond)) {                                                       \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);           \
      return 1;                                                          \
    }                                                                    \
  } while (0)

// d c b a | a b c d | d c b a, built by walking: one step right of the last sample the walk turns round
static int brute_fold(int i, int n) {
  int pos = 0, dir = i < 0 ? -1 : 1;   // extension index 0 is sample 0
  const int steps = i >= 0 ? i : -i;
  for (int k = 0; k < steps; ++k) {
    const int nxt = pos + dir;
    if (nxt < 0 || nxt >= n) dir = -dir;   // the half-sample symmetry repeats the edge sample: this step stays
    else pos = nxt;
  }
  return pos;
}

int main() {
  // the walk itself, on the textbook example: a b c d extended is ... c d | d c b a | a b c d | d c b a ...
  {
    const int want[] = {3, 2, 1, 0, 0, 1, 2, 3, 3, 2, 1, 0, 0};
    for (int i = -4; i <= 8; ++i) CHECK(brute_fold(i, 4) == want[i + 4]);
  }
  for (int n = 1; n <= 9; ++n)
    for (int i = -40; i <= 40; ++i) {
      CHECK(wff_fold(i, n) == brute_fold(i, n));
      CHECK(wff_fold32(i, n) == brute_fold(i, n));
    }
  // Python rounds halves to even: round(2.5) = 2, round(4.5) = 4 (C's lround gives 3 and 5), round(3.5) = 4, round(1.5) = 2
  CHECK(wff_half_window(1.25) == 2);
  CHECK(wff_half_window(2.25) == 4);
  CHECK(wff_half_window(2.5) == 5);
  CHECK(wff_half_window(3.0) == 6);
  CHECK(wff_half_window(10.0) == 20);
  CHECK(wff_half_window(1.75) == 4);
  CHECK(wff_half_window(0.75) == 2);
  CHECK(wff_half_window(0.2) == 0);
  CHECK(wff_half_window(-1.0) == -1);
  CHECK(wff_half_window(nan("")) == -1);
  CHECK(wff_half_window(1e300) == -1);
  // every (s, T, dtype) inside the limits has a tile within 160 KiB and 512 threads; just outside there is none
  for (int f64 = 0; f64 < 2; ++f64) {
    for (int s = 1; s <= WFF_MAX_S; ++s)
      for (int T = 1; T <= WFF_MAX_T; ++T) {
        const WffTile t = wff_tile(s, T, f64 != 0);
        CHECK(t.ok);
        CHECK(t.lds_bytes <= 160 * 1024);
        CHECK(t.threads <= WFF_THREADS_MAX && t.threads % 64 == 0);
        CHECK(t.cols * (f64 ? 16 : 8) == WFF_ROW_BYTES);
        CHECK(t.R % t.P == 0 && t.wpad % t.P == 0 && t.wpad >= 2 * s && t.rows_sf % t.P == 0);
        CHECK(t.rows_sf >= t.R + 2 * s - 1);
        // the last block of sf rows reads rows_sf - P + wpad + P - 1 at most; the second convolution map[R - P + wpad + P - 1]
        CHECK(t.rows_a >= t.rows_sf + t.wpad);
        CHECK(t.nmap >= t.R + t.wpad);
        CHECK(t.lds_bytes >= (t.rows_a + t.rows_sf) * WFF_ROW_BYTES + t.nmap * 4 + 4);
        CHECK(t.threads >= 1 && wff_tslots(T) >= T && wff_tslots(T) <= WFF_MAX_T);
      }
    CHECK(!wff_tile(WFF_MAX_S + 1, 1, f64 != 0).ok);
    CHECK(!wff_tile(1, WFF_MAX_T + 1, f64 != 0).ok);
    CHECK(!wff_tile(0, 1, f64 != 0).ok);
    CHECK(!wff_tile(1, 0, f64 != 0).ok);
  }
  // the hull of a tile: an interval of at most R + 2 s - 1 rows that holds the fold of every window position
  for (int n = 4; n <= 200; n += (n < 40 ? 1 : 23))
    for (int s = 1; s <= WFF_MAX_S; s += 3)
      for (int R = 16; R <= 64; R *= 2)
        for (int r0 = 0; r0 < n; r0 += R) {
          int h0, h1;
          wff_hull(r0, R, s, n, &h0, &h1);
          CHECK(h0 >= 0 && h1 < n && h1 - h0 + 1 <= R + 2 * s - 1);
          std::vector<char> hit(n, 0);
          for (int u = 0; u < R + 2 * s - 1; ++u) {
            const int f = wff_fold(r0 - s + 1 + u, n);
            CHECK(f >= h0 && f <= h1);
            hit[f] = 1;
          }
          for (int f = h0; f <= h1; ++f) CHECK(hit[f]);
        }
  printf("OK %ld\n", checks);
  for (int f64 = 0; f64 < 2; ++f64) {
    const int ss[] = {5, 6, 20, 40};
    for (int s : ss) {
      const WffTile t = wff_tile(s, 1, f64 != 0);
      printf("TILE %s %d %d %d\n", f64 ? "f64" : "f32", s, t.cols, t.R);
    }
  }
  return 0;
}
