// Order-3 B-spline sampling as scipy.ndimage.map_coordinates evaluates it: the prefilter's tap count, the boundary
// extensions, the coordinate folds, the spline weights and the 4 x 4 tap sums (mode 'nearest', mode 'constant' and the
// folded modes 'reflect' / 'mirror' / 'grid-wrap').  Shared by the Lawler-Fujita kernels (gpa_warp.hip, which also holds
// the prefilter itself) and the unit-cell expansion (gpa_ucell.hip), so that both sample with the same arithmetic.
// The index, fold and weight functions are GPA_HD (as the per-thread steps of gpa_fft.h), so that
// tests/host/spline_modes_emulator.cpp runs the very same arithmetic on the CPU; the gathers and the samplers built on them
// exist under hipcc only.
#ifndef GPA_SPLINE_H
#define GPA_SPLINE_H
#include <math.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#ifndef GPA_HD
#if defined(__HIPCC__)
#define GPA_HD __host__ __device__ __forceinline__
#else
#define GPA_HD inline
#endif
#endif

namespace gpa {

namespace {

// taps on each side of the prefilter: the pole is z = sqrt(3) - 2, |z|^k falls below the precision's rounding of the
// centre tap at k = 16 in f32 (|z|^16 = 7e-10 against 2^-24 = 6e-8) and at k = 28 in f64 (1e-16; 32 kept: |z|^32 = 5e-19)
template <class T> struct TapHalf { static constexpr int value = sizeof(T) == 4 ? 16 : 32; };

enum Ext { EXT_REFLECT = 0, EXT_MIRROR = 1, EXT_WRAP = 2 };

GPA_HD int ext_index(int i, int n, int ext) {
  if (n == 1) return 0;
  // one remainder by the extension's period: half-sample symmetric 2 n (-1 -> 0, n -> n-1), whole-sample symmetric 2 n - 2
  // (-1 -> 1, n -> n-2), periodic n (-1 -> n-1, n -> 0); the upper half of a symmetric period reads mirrored
  const int p = ext == EXT_REFLECT ? 2 * n : (ext == EXT_MIRROR ? 2 * n - 2 : n);
  i %= p;
  if (i < 0) i += p;
  return i >= n ? p - i - (ext == EXT_REFLECT ? 1 : 0) : i;      // (periodic: i < n already)
}

// The coordinate fold of scipy's modes 'reflect' (= 'grid-mirror'), 'mirror' and 'grid-wrap', applied before floor():
// the coordinate is brought into one period of the extension -- [-0.5, n - 0.5], [0, n - 1], [0, n) -- and the taps that
// still leave [0, n - 1] there go through tap_index below.  A coordinate inside the period (all but a frame of the pixels
// of a fixed point) is returned as it is.  Outside, with y = x + 0.5 ('reflect') or x and the period p = 2 n / 2 n - 2 / n:
// y - p floor(y / p) by ONE fused multiply-add, which is exact (p and the quotient are integers below 2^22 / 2^51 and the
// result is a multiple of y's last bit no larger than y); a quotient that the division rounded across an integer leaves
// y one period off, which the two comparisons put right.  No loop, no library remainder: the long remainder code of fmod
// in a path a wavefront hardly ever takes cost the fixed-point kernel 40 VGPRs and three of its eight wavefronts per SIMD.
// NaN, infinite and |x| > 2^22 (f32; f64: 2^51, where neighbouring numbers are a whole sample or more apart) coordinates fold
// to 0 -- a defined sample, never an index out of range; so does everything on an axis of one sample.
template <class T>
GPA_HD T fold_coord(T x, int n, int ext) {
  const T xmax = sizeof(T) == 4 ? T(4194304.0) : T(2251799813685248.0);
  if (n == 1 || !(fabs(x) <= xmax)) return T(0);
  const T h = ext == EXT_REFLECT ? T(0.5) : T(0);                                        // the period starts at -h
  const T p = T(ext == EXT_REFLECT ? 2 * n : (ext == EXT_MIRROR ? 2 * n - 2 : n));
  const T top = T(ext == EXT_REFLECT ? n : (ext == EXT_MIRROR ? n - 1 : n));             // y beyond it reads mirrored
  if (x >= -h && (ext == EXT_WRAP ? x < top : x <= top - h)) return x;
  T y = x + h;
  y = fma(-floor(y / p), p, y);
  if (y < T(0)) y += p;
  if (y >= p) y -= p;                                          // (-tiny + p rounds to p: the same point of the period as 0)
  if (ext != EXT_WRAP && y > top) y = p - y;
  return y - h;
}
// a tap i0 - 1 .. i0 + 2 of a FOLDED coordinate lies in [-2, n + 1]: one step of the extension brings it home without a
// remainder where the axis has four samples or more (an axis of two or three: ext_index, the step may leave it again)
GPA_HD int tap_index(int i, int n, int ext) {
  if (n < 4) return ext_index(i, n, ext);
  if (i < 0) return ext == EXT_REFLECT ? -1 - i : (ext == EXT_MIRROR ? -i : i + n);
  if (i >= n) return ext == EXT_REFLECT ? 2 * n - 1 - i : (ext == EXT_MIRROR ? 2 * n - 2 - i : i - n);
  return i;
}

// cubic B-spline weights as scipy.ndimage evaluates them (ni_splines.c: get_spline_interpolation_weights, order 3).
// f64: the divisions by 6 as written (pinned to SciPy at 4e-15); f32: times 1/6 -- one instruction where an IEEE
// division takes ten, six times per round of the fixed point, and 0.5 ulp of f32 either way
template <class T>
GPA_HD T sixth(T v) {
  if constexpr (sizeof(T) == 4) return v * T(0.16666666666666666);
  else return v / T(6);
}
template <class T>
GPA_HD void bspline_weights(T t, T (&w)[4]) {
#pragma clang fp contract(off)   // (the same bits at every call site; SciPy's C evaluates these without fused operations too)
  const T z = T(1) - t;
  w[1] = sixth(t * t * (t - T(2)) * T(3) + T(4));
  w[2] = sixth(z * z * (z - T(2)) * T(3) + T(4));
  w[0] = sixth(z * z * z);
  w[3] = T(1) - w[0] - w[1] - w[2];
}
// one row of the 4 x 4 tap sum, and its accumulation: explicit fused multiply-adds in ONE fixed order, so that the same taps
// give the same bits whichever kernel or code path gathers them (from L1 / L2, or from the LDS window of invert_tile_kernel)
template <class T>
GPA_HD T tap_row(const T (&wy)[4], T t0, T t1, T t2, T t3) {
#pragma clang fp contract(off)
  T r = wy[0] * t0;
  r = fma(wy[1], t1, r);
  r = fma(wy[2], t2, r);
  r = fma(wy[3], t3, r);
  return r;
}
#if defined(__HIPCC__)
// index type of the coefficient gathers: 32-bit element offsets from a uniform base (one address instruction per tap,
// shared by the two components) while the field is below 2^32 bytes, 64-bit beyond
template <bool WIDE> struct GatherIdx { typedef unsigned type; };
template <> struct GatherIdx<true> { typedef size_t type; };
// element `o` of a field: as base + 32-bit BYTE offset (the form the scalar-base global loads take) or a 64-bit index
template <class T> __device__ __forceinline__ T gather(const T* __restrict__ base, unsigned o) {
  return *reinterpret_cast<const T*>(reinterpret_cast<const char*>(base) + (unsigned)(o * (unsigned)sizeof(T)));
}
template <class T> __device__ __forceinline__ T gather(const T* __restrict__ base, size_t o) { return base[o]; }
// four ADJACENT elements from element `o` on: one 16-byte (f64: 32-byte) load -- global memory takes it at 4-byte alignment --
// where four scalar gathers cost the texture-address unit four wave-instructions (the gathers of a round are bound by that
// unit, not by bytes)
template <class T> struct Tap4 { T v[4]; };
template <class T> __device__ __forceinline__ Tap4<T> gather4(const T* __restrict__ base, unsigned o) {
  return *reinterpret_cast<const Tap4<T>*>(reinterpret_cast<const char*>(base) + (unsigned)(o * (unsigned)sizeof(T)));
}
template <class T> __device__ __forceinline__ Tap4<T> gather4(const T* __restrict__ base, size_t o) {
  return *reinterpret_cast<const Tap4<T>*>(base + o);
}

// mode='nearest': coordinate (already shifted by npad) unclamped, tap indices clamped
template <class T, int NC, bool WIDE = false>
__device__ __forceinline__ void interp_nearest(const T* const (&coef)[NC], int m0, int m1, T x, T y, T (&out)[NC]) {
  typedef typename GatherIdx<WIDE>::type I;
  // keep floor() finite for wild coordinates: everything beyond one sample outside reads the edge
  x = x < T(-2) ? T(-2) : (x > T(m0 + 1) ? T(m0 + 1) : x);
  y = y < T(-2) ? T(-2) : (y > T(m1 + 1) ? T(m1 + 1) : y);
  const T fx = floor(x), fy = floor(y);
  T wx[4], wy[4];
  bspline_weights(x - fx, wx);
  bspline_weights(y - fy, wy);
  const int ix = (int)fx - 1, iy = (int)fy - 1;
  int cy[4];
#pragma unroll
  for (int b = 0; b < 4; ++b) { const int j = iy + b; cy[b] = j < 0 ? 0 : (j >= m1 ? m1 - 1 : j); }
#pragma unroll
  for (int n = 0; n < NC; ++n) out[n] = T(0);
  // (four scalar gathers per tap row, not one 16-byte load as interp_constant's interior path: measured, the fixed point
  //  got slower with it -- 13.3 -> 14.5 ms at 16384^2 -- its rounds are bound by instruction issue, not by the gathers)
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    int i = ix + a;
    i = i < 0 ? 0 : (i >= m0 ? m0 - 1 : i);
    const I row = (I)i * (I)m1;
    const I o0 = row + (I)cy[0], o1 = row + (I)cy[1], o2 = row + (I)cy[2], o3 = row + (I)cy[3];
#pragma unroll
    for (int n = 0; n < NC; ++n) {
      const T* cr = coef[n];
      out[n] = fma(wx[a], tap_row(wy, gather(cr, o0), gather(cr, o1), gather(cr, o2), gather(cr, o3)), out[n]);
    }
  }
}

// mode='constant': whole-sample mirrored taps, `cval` where the coordinate leaves [0, n-1] (NaN coordinates too)
template <class T, int NC, bool WIDE = false>
__device__ __forceinline__ void interp_constant(const T* const (&coef)[NC], int n0, int n1, T x, T y, T cval, T (&out)[NC]) {
  typedef typename GatherIdx<WIDE>::type I;
  if (!(x >= T(0) && x <= T(n0 - 1) && y >= T(0) && y <= T(n1 - 1))) {
#pragma unroll
    for (int n = 0; n < NC; ++n) out[n] = cval;
    return;
  }
  const T fx = floor(x), fy = floor(y);
  T wx[4], wy[4];
  bspline_weights(x - fx, wx);
  bspline_weights(y - fy, wy);
  const int ix = (int)fx - 1, iy = (int)fy - 1;
#pragma unroll
  for (int n = 0; n < NC; ++n) out[n] = T(0);
  if (ix >= 0 && iy >= 0 && ix + 3 < n0 && iy + 3 < n1) {
    // the 4 x 4 footprint inside the field -- all but a frame of pixels: no mirror arithmetic (eight integer remainders), the
    // four taps of a row in one load
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const I o = (I)(ix + a) * (I)n1 + (I)iy;
#pragma unroll
      for (int n = 0; n < NC; ++n) {
        const Tap4<T> q = gather4(coef[n], o);
        out[n] = fma(wx[a], tap_row(wy, q.v[0], q.v[1], q.v[2], q.v[3]), out[n]);
      }
    }
    return;
  }
  int cy[4];
#pragma unroll
  for (int b = 0; b < 4; ++b) cy[b] = ext_index(iy + b, n1, EXT_MIRROR);
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const I row = (I)ext_index(ix + a, n0, EXT_MIRROR) * (I)n1;
    const I o0 = row + (I)cy[0], o1 = row + (I)cy[1], o2 = row + (I)cy[2], o3 = row + (I)cy[3];
#pragma unroll
    for (int n = 0; n < NC; ++n) {
      const T* cr = coef[n];
      out[n] = fma(wx[a], tap_row(wy, gather(cr, o0), gather(cr, o1), gather(cr, o2), gather(cr, o3)), out[n]);
    }
  }
}

// modes 'reflect' / 'grid-mirror' (ext = EXT_REFLECT), 'mirror' (EXT_MIRROR) and 'grid-wrap' (EXT_WRAP): the coordinate folded
// into one period of the extension, the taps extended the same way -- no cval, every coordinate has a value.  Tap sums in the
// order of the two samplers above; a folded footprint inside the field (all but a frame of pixels) takes interp_constant's
// interior path: no index remainders, the four taps of a row in one load.
template <class T, int NC, bool WIDE = false>
__device__ __forceinline__ void interp_folded(const T* const (&coef)[NC], int n0, int n1, T x, T y, int ext, T (&out)[NC]) {
  typedef typename GatherIdx<WIDE>::type I;
  x = fold_coord(x, n0, ext);
  y = fold_coord(y, n1, ext);
  const T fx = floor(x), fy = floor(y);
  T wx[4], wy[4];
  bspline_weights(x - fx, wx);
  bspline_weights(y - fy, wy);
  const int ix = (int)fx - 1, iy = (int)fy - 1;
#pragma unroll
  for (int n = 0; n < NC; ++n) out[n] = T(0);
  if (ix >= 0 && iy >= 0 && ix + 3 < n0 && iy + 3 < n1) {
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const I o = (I)(ix + a) * (I)n1 + (I)iy;
#pragma unroll
      for (int n = 0; n < NC; ++n) {
        const Tap4<T> q = gather4(coef[n], o);
        out[n] = fma(wx[a], tap_row(wy, q.v[0], q.v[1], q.v[2], q.v[3]), out[n]);
      }
    }
    return;
  }
  int cy[4];
#pragma unroll
  for (int b = 0; b < 4; ++b) cy[b] = tap_index(iy + b, n1, ext);
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const I row = (I)tap_index(ix + a, n0, ext) * (I)n1;
    const I o0 = row + (I)cy[0], o1 = row + (I)cy[1], o2 = row + (I)cy[2], o3 = row + (I)cy[3];
#pragma unroll
    for (int n = 0; n < NC; ++n) {
      const T* cr = coef[n];
      out[n] = fma(wx[a], tap_row(wy, gather(cr, o0), gather(cr, o1), gather(cr, o2), gather(cr, o3)), out[n]);
    }
  }
}
#endif  // __HIPCC__

}  // namespace

}  // namespace gpa
#endif  // GPA_SPLINE_H
