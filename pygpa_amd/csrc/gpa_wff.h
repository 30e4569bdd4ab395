// Windowed Fourier filtering (geometric_phase_analysis.py:551-580): the geometry the kernels of gpa_wff.hip and the entry
// points of gpa_api_wff.hip share.  No HIP code: tests/host/wff_geom_check.cpp includes it with a host compiler.
//
// Window: s = round(2 sigma) (Python's round: halves go to the even integer), offsets j = -s .. s - 1, 2 s taps.
// Boundary: scipy.ndimage's 'reflect', the half-sample symmetric extension d c b a | a b c d | d c b a of period 2 n.
#pragma once
#include <math.h>
#include <stddef.h>

namespace gpa {

// Limits of one call, from the budget of one workgroup of the column kernel (wff_cols_kernel):
//  - WFF_MAX_T thresholds: a thread keeps T x WFF_P complex sums in registers across the whole wy loop -- 8 x 8 x 2 = 128
//    VGPRs in f32 (WFF_P = 8), 8 x 4 x 4 = 128 in f64 (WFF_P = 4) -- beside two windows of WFF_P samples, which stays below the
//    256 VGPRs at which a 512-thread workgroup still runs two waves per SIMD;
//  - WFF_MAX_S half-window: the workgroup stages R + 4 s - 2 rows of A and R + 2 s - 1 rows of sf, 512 bytes each, in LDS;
//    at the smallest tile height (R = 16) and s = 40 that is 280 rows with the slack of the register blocks, 140 KiB of
//    the 160 KiB (tests/host/wff_geom_check.cpp walks every (s, T, dtype) inside the limits).
constexpr int WFF_MAX_T = 8;
constexpr int WFF_MAX_S = 40;
constexpr int WFF_LDS_BUDGET = 160 * 1024;
constexpr int WFF_ROW_BYTES = 512;     // one staged row of a tile: 64 complex64 or 32 complex128 columns
constexpr int WFF_THREADS_MAX = 512;
constexpr int WFF_ROWS_TILE = 256;     // outputs of one workgroup of the row kernels

// index i folded into [0, n) under the period-2n reflect rule, for any integer i (any number of reflections)
inline
#if defined(__HIPCC__)
    __host__ __device__
#endif
    int wff_fold(long long i, int n) {
  const long long p = 2LL * n;
  long long m = i % p;
  if (m < 0) m += p;
  return (int)(m < n ? m : p - 1 - m);
}

// the same in 32-bit arithmetic, for the kernels: |i| stays far below 2^31 (an index of the image plus or minus a window)
inline
#if defined(__HIPCC__)
    __host__ __device__
#endif
    int wff_fold32(int i, int n) {
  const int p = 2 * n;
  int m = i % p;
  if (m < 0) m += p;
  return m < n ? m : p - 1 - m;
}

// s = round(2 sigma) with Python's rule (round half to even); -1 where 2 sigma is not a finite number below 2^30
inline int wff_half_window(double sigma) {
  const double x = 2.0 * sigma;
  if (!(x >= 0.0) || !(x < 1073741824.0)) return -1;
  const double f = floor(x), d = x - f;
  long long r = (long long)f;
  if (d > 0.5 || (d == 0.5 && (r & 1))) ++r;
  return (int)r;
}

// outputs a thread of the column kernel keeps per threshold (the sliding-window register block)
inline constexpr int wff_block(bool f64) { return f64 ? 4 : 8; }
// the instantiation a call with T thresholds runs: the next of 1, 2, 4, 8
inline constexpr int wff_tslots(int T) { return T <= 1 ? 1 : T <= 2 ? 2 : T <= 4 ? 4 : 8; }

struct WffTile {
  int cols;        // columns per workgroup (lanes run along a row: 512-byte rows, conflict-free without padding)
  int R;           // output rows per workgroup
  int P;           // consecutive outputs of a column per thread
  int threads;     // cols * R / P
  int wpad;        // 2 s rounded up to a multiple of P: taps are consumed P at a time
  int rows_a;      // staged rows of A: the hull of the sf rows, s - 1 above and s below, and slack for the last block
  int rows_sf;     // rows of sf: R + 2 s - 1 rounded up to P
  int nmap;        // entries of the window -> sf-row map (R + wpad + P)
  int lds_bytes;
  bool ok;         // s, T inside the limits and lds_bytes inside the budget
};

inline constexpr int wff_round_up(int a, int b) { return (a + b - 1) / b * b; }

// LDS of a tile of height R: rows of A, rows of sf, the map, 16 bytes for the tile's first sf row
inline constexpr int wff_lds_bytes(int s, int R, int P) {
  const int wpad = wff_round_up(2 * s, P), rows_sf = wff_round_up(R + 2 * s - 1, P);
  return (rows_sf + wpad + P + rows_sf) * WFF_ROW_BYTES + (R + wpad + P) * (int)sizeof(int) + 16;
}

// The tile of a call: the tallest R of 64, 32, 16 whose rows fit the LDS budget (a taller tile computes fewer sf rows twice:
// R + 2 s - 1 per R outputs).  T does not enter the LDS (the sums live in registers), only the limit.
inline WffTile wff_tile(int s, int T, bool f64) {
  WffTile t{};
  t.P = wff_block(f64);
  t.cols = WFF_ROW_BYTES / (f64 ? 16 : 8);
  t.ok = s >= 1 && s <= WFF_MAX_S && T >= 1 && T <= WFF_MAX_T;
  if (s < 1) s = 1;
  t.R = 16;
  for (int R = 64; R >= 16; R /= 2)
    if (t.cols * R / t.P <= WFF_THREADS_MAX && wff_lds_bytes(s, R, t.P) <= WFF_LDS_BUDGET) { t.R = R; break; }
  t.threads = t.cols * t.R / t.P;
  t.wpad = wff_round_up(2 * s, t.P);
  t.rows_sf = wff_round_up(t.R + 2 * s - 1, t.P);
  t.rows_a = t.rows_sf + t.wpad + t.P;
  t.nmap = t.R + t.wpad + t.P;
  t.lds_bytes = wff_lds_bytes(s, t.R, t.P);
  if (t.lds_bytes > WFF_LDS_BUDGET) t.ok = false;
  return t;
}

// the sf rows a tile of output rows [r0, r0 + R) needs: the image of the window r0 - s + 1 .. r0 + R + s - 1 under the
// fold, which is an interval [h0, h1] of at most R + 2 s - 1 rows
inline void wff_hull(int r0, int R, int s, int n, int* h0, int* h1) {
  int lo = n, hi = -1;
  const long long w0 = (long long)r0 - s + 1, w1 = (long long)r0 + R + s - 1;
  if (w1 - w0 + 1 >= 2LL * n) { *h0 = 0; *h1 = n - 1; return; }
  for (long long m = w0; m <= w1; ++m) {
    const int f = wff_fold(m, n);
    lo = f < lo ? f : lo;
    hi = f > hi ? f : hi;
  }
  *h0 = lo;
  *h1 = hi;
}

}  // namespace gpa
