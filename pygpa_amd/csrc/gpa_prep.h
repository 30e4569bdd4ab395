// Image preparation (pyGPA/imagetools.py: gauss_homogenize2/3, generate_mask, cull_by_mask, trim_nans, trim_nans2): the
// integer geometry the kernels of gpa_prep.hip and the entry points of gpa_api_prep.hip share.  No HIP code:
// tests/host/prep_check.cpp includes it with a host compiler.
//
// Boundary of the Gaussian filter: scipy.ndimage's 'reflect', d c b a | a b c d | d c b a, period 2 n.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PREP_HD __host__ __device__ inline
#else
#define PREP_HD inline
#endif

namespace gpa {

// Largest erosion radius served.  The erosion stores, per sample, the distance to the nearest false sample of its row as ONE
// BYTE, saturated at r + 1; a chord of disk(r) is at most r, so the comparison `distance > chord` is exact, and r + 1 fits the
// byte while r <= 254.
// (Larger radii would need two bytes per sample and twice the traffic of the 2 r + 1 reads per pixel; the reference's default
// is r = 20.)  An r beyond the image is served -- the result is all false -- as long as it is within the limit.
constexpr int PREP_MAX_R = 254;
// The row pass of the coverage (below) keeps the prefix counts of one row in LDS, 4 (n1 + 1) bytes of the 160 KiB.
constexpr int PREP_MAX_N1 = 32768;
// Radius of the direct-sum route: 2 R + 1 taps sit in a table of 3072 doubles, as in the plain gaussian_filter.
constexpr int PREP_MAX_DIRECT_TAPS = 3072;
// rows a thread of the column pass of the coverage walks
constexpr int PREP_COV_CHUNK = 128;

// index i folded into [0, n) under the period-2n reflect rule, any integer i whose magnitude stays below 2^30
PREP_HD int prep_fold(int i, int n) {
  const int p = 2 * n;
  int m = i % p;
  if (m < 0) m += p;
  return m < n ? m : p - 1 - m;
}

// { prep_fold(i + d, n) : |d| <= R } for 0 <= i < n is the interval [lo, hi]: folding maps neighbours to neighbours or to the
// same sample, so the image of the run i - R .. i + R is connected, and it contains i.  Its lower end is 0 once the run
// passes -1 / 0 on the left; otherwise it is i - R, or the point 2 n - 1 - (i + R) the right fold reaches (0 once that fold
// passes the left end too: the extension then repeats).  The upper end mirrors this.
PREP_HD void prep_reflect_interval(int i, int R, int n, int* lo, int* hi) {
  const long long a = (long long)i - R, b = (long long)i + R;
  long long l, h;
  if (a < 0) l = 0;
  else {
    const long long f = 2LL * n - 1 - b;   // deepest point of the right fold
    l = b > n - 1 ? (f < 0 ? 0 : (f < a ? f : a)) : a;
  }
  if (b > n - 1) h = n - 1;
  else {
    const long long f = -1 - a;            // deepest point of the left fold
    h = a < 0 ? (f > n - 1 ? n - 1 : (f > b ? f : b)) : b;
  }
  *lo = (int)l;
  *hi = (int)h;
}

// floor(sqrt(v)) for 0 <= v < 2^31, in integers
PREP_HD int prep_isqrt(int v) {
  int s = 0;
  for (int bit = 1 << 15; bit; bit >>= 1) {
    const long long t = (long long)(s + bit) * (s + bit);
    if (t <= v) s += bit;
  }
  return s;
}

// half-width of row dy of skimage.morphology.disk(r), the (2 r + 1)^2 array X^2 + Y^2 <= r^2: the row holds |dx| <= chord
PREP_HD int prep_disk_chord(int r, int dy) { return prep_isqrt(r * r - dy * dy); }

// The loop of trim_nans2 (imagetools.py:145-175) on the window [x0, x1) x [y0, y1), rule for rule: with r / c the NaN counts
// of the first and last row / column of the window, stop when both sums are 0; drop every end row that holds a NaN when
// sum(r) > sum(c), otherwise every end column that holds one (a tie goes to the columns).  The window is never rescanned:
// a dropped row changes the column counts by its two corner samples, and only the line that becomes an end is counted anew.
// A window of one row is its own first and last row (the reference indexes [0, -1]) and loses both ends at once; the loop
// ends where the window is empty (x1 <= x0 or y1 <= y0), which the callers report as an error.
// C: int row(x, y0, y1), int col(y, x0, x1): NaNs of a line within the window; int at(x, y): 1 where the sample is NaN.
// On the device every thread of the workgroup runs the loop with the same values (the counts are workgroup reductions).
template <class C>
PREP_HD void prep_trim_loop(C& c, int n0, int n1, int lims[4]) {
  int x0 = 0, x1 = n0, y0 = 0, y1 = n1;
  if (n0 > 0 && n1 > 0) {
    int r0 = c.row(x0, y0, y1), r1 = c.row(x1 - 1, y0, y1), c0 = c.col(y0, x0, x1), c1 = c.col(y1 - 1, x0, x1);
    for (;;) {
      const int rs = r0 + r1, cs = c0 + c1;
      if (rs == 0 && cs == 0) break;
      if (rs > cs) {
        const int d0 = r0 > 0, d1 = r1 > 0;
        if (d0) { c0 -= c.at(x0, y0); c1 -= c.at(x0, y1 - 1); ++x0; }
        if (d1) { c0 -= c.at(x1 - 1, y0); c1 -= c.at(x1 - 1, y1 - 1); --x1; }
        if (x1 <= x0) break;
        if (d0) r0 = c.row(x0, y0, y1);
        if (d1) r1 = c.row(x1 - 1, y0, y1);
        if (x1 - x0 == 1) { r0 = r1 = c.row(x0, y0, y1); }
      } else {
        const int d0 = c0 > 0, d1 = c1 > 0;
        if (d0) { r0 -= c.at(x0, y0); r1 -= c.at(x1 - 1, y0); ++y0; }
        if (d1) { r0 -= c.at(x0, y1 - 1); r1 -= c.at(x1 - 1, y1 - 1); --y1; }
        if (y1 <= y0) break;
        if (d0) c0 = c.col(y0, x0, x1);
        if (d1) c1 = c.col(y1 - 1, x0, x1);
        if (y1 - y0 == 1) { c0 = c1 = c.col(y0, x0, x1); }
      }
    }
  }
  lims[0] = x0; lims[1] = x1; lims[2] = y0; lims[3] = y1;
}

}  // namespace gpa
