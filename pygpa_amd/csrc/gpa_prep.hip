// Image preparation on the device (pyGPA/imagetools.py): masked Gaussian homogenisation, the mask of a stack, disk erosion,
// mask bounds and the NaN trims.  Geometry and limits: gpa_prep.h; entry points: gpa_api_prep.hip.
//
// gauss_homogenize2 (imagetools.py:92-105):  VV = G(where(mask, image, 0)) / G(mask),  out = image / VV,  G = scipy's
// gaussian_filter (axis 0, then axis 1; radius R = int(4 sigma + 0.5); 'reflect').  Both fields go through the SAME two passes:
//   column pass  reads image and mask once, masks in its prologue, filters num and den along axis 0, writes two planes;
//   row pass     filters the two planes along axis 1 and writes out (and VV) from its epilogue.
// On the FFT route (the overlap-save scheme of gpa_gaussfft.hip, same WgFFT engine, tables and segment lengths) a complex
// transform carries two real lines, and its rounding error scales with the magnitude of the PAIR: num lines are paired with
// num lines and den lines with den lines (adjacent columns / adjacent rows), never num + i den -- camera counts beside a field
// <= 1 would bury den in f32.
// Where VV is NaN in the reference -- no true mask sample in the (2R+1)^2 box of the reflect-extended mask -- is decided in
// integers (cov_cols_kernel, cov_rows_kernel: any-true over the reflected interval of gpa_prep.h along one axis, then the
// other), never by den == 0: the FFT leaves rounding noise there.  At covered pixels VV is held inside [min, max] of the
// masked samples, where a mean with non-negative weights lies: far from the mask den falls below the transforms' noise and
// the quotient would be arbitrary.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "gpa_dct.h"
#include "gpa_gaussfft.h"
#include "gpa_internal.h"
#include "gpa_prep.h"

namespace gpa {
namespace {

// ---- order-preserving keys of doubles for atomicMin / atomicMax ----------------------------------------------------------
__device__ __forceinline__ unsigned long long key_of(double v) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double of_key(unsigned long long k) {
  const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  return __longlong_as_double((long long)b);
}

__global__ void minmax_init_kernel(unsigned long long* mm) {
  mm[0] = ~0ull;   // min key
  mm[1] = 0ull;    // max key
}

// min / max of the calling wave's values (NaNs do not take part) into mm; T is exactly representable as a double
template <class T>
__device__ __forceinline__ void wave_minmax(T lo, T hi, unsigned long long* mm) {
  // (the smallest column tile is half a wave: lanes beyond the workgroup hold nothing)
  const int lane = threadIdx.x & 63, live = min(64, (int)blockDim.x - (int)(threadIdx.x & ~63u));
#pragma unroll
  for (int o = 32; o; o >>= 1) {
    const T l2 = __shfl_xor(lo, o), h2 = __shfl_xor(hi, o);
    if ((lane ^ o) < live) {
      lo = l2 < lo ? l2 : lo;
      hi = h2 > hi ? h2 : hi;
    }
  }
  if (lane == 0 && lo <= hi) {
    atomicMin(&mm[0], key_of((double)lo));
    atomicMax(&mm[1], key_of((double)hi));
  }
}

// VV and out of one pixel.  covered: the box holds a true sample (integers); fill: VV of an uncovered pixel (NaN or nan_scale)
template <class T>
__device__ __forceinline__ void finish_pixel(T num, T den, bool covered, T img, T fill, T lo, T hi, T* out, T* vv, size_t o) {
  T v = fill;
  if (covered) {
    // den <= 0 is rounding noise around a den below it: any value of the masked range is within the error of the quotient
    v = den > T(0) ? num / den : (den != den ? den : T(0.5) * (lo + hi));
    if (v < lo) v = lo;   // (comparisons, not fmin / fmax: a NaN stays a NaN)
    if (v > hi) v = hi;
  }
  out[o] = img / v;
  if (vv) vv[o] = v;
}

// ---- FFT route -----------------------------------------------------------------------------------------------------------
// column tiles: GfColGeom of gpa_gaussfft.h, the geometry gaussfft_choose_lg prices -- C complex transforms = 2C adjacent real
// columns per workgroup.
// One field of the column pass: forward transform, transfer function, inverse transform, the kept rows stored.  Called once
// per field, not looped over: a loop would keep the sixteen store addresses and table values of both fields live in registers.
template <class T, int LG, int NT, class TW>
__device__ __forceinline__ void cols_field(cpx<T> (&x)[NT][16], cpx<T>* lds, int t, const TW& tw, const T* __restrict__ H,
                                           T* __restrict__ dst, int base, int R, int n0, int n1, int y0, bool vec) {
  using F = WgFFT<T, LG>;
  using G = GfColGeom<T, LG>;
  static_assert(NT == G::NT, "the caller's transforms per thread are the tile's");
  constexpr int CT = G::CT, TPF = F::TPF, L = F::L, W = 2 * NT;
  struct alignas(W * sizeof(T)) Vec { T v[W]; };
  F::template forward_multi<NT, CT>(x, lds, G::REGION, t, tw);
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const T h = H[i * TPF + t];
#pragma unroll
    for (int n = 0; n < NT; ++n) x[n][i] = {x[n][i].x * h, x[n][i].y * h};
  }
  F::template inverse_multi<NT, CT>(x, lds, G::REGION, t, tw);
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int slot = t + TPF * i, row = base + slot;
    if (slot >= R && slot < L - R && row < n0) {
      Vec v;
#pragma unroll
      for (int n = 0; n < NT; ++n) { v.v[2 * n] = x[n][i].x; v.v[2 * n + 1] = x[n][i].y; }
      if (vec) *reinterpret_cast<Vec*>(dst + (size_t)row * n1 + y0) = v;
      else {
#pragma unroll
        for (int k = 0; k < W; ++k)
          if (y0 + k < n1) dst[(size_t)row * n1 + y0 + k] = v.v[k];
      }
    }
  }
}

// MODE 0: both fields in one launch.  The longest transforms (16384 points in f32, 8192 in f64: prep_split) leave a thread too
// few registers to carry anything of one field through the other, so there the two fields are two launches: MODE 1 reads image
// and mask and writes num, MODE 2 reads the mask alone and writes den (the row pass: prep_finish_kernel).
template <class T, int LG>
constexpr bool prep_split() { return sizeof(T) * WgFFT<T, LG>::TPF >= 4096; }

template <class T, int LG, int MODE>
__global__ __launch_bounds__((GfColGeom<T, LG>::THREADS)) void prep_cols_kernel(
    const T* __restrict__ image, const uint8_t* __restrict__ mask, T* __restrict__ num, T* __restrict__ den, int n0, int n1, int R,
    const T* __restrict__ H, const cpx<T>* __restrict__ twtab, unsigned long long* mm) {
  using F = WgFFT<T, LG>;
  using G = GfColGeom<T, LG>;
  constexpr int CT = G::CT, NT = G::NT, TPF = F::TPF, L = F::L, W = 2 * NT;   // W real columns per thread
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int c = threadIdx.x % CT, t = threadIdx.x / CT;
  cpx<T>* lds = reinterpret_cast<cpx<T>*>(smem) + c;
  const int tile = xcd_tile(blockIdx.x, gridDim.x), seg = blockIdx.y;
  const int y0 = tile * G::RC + c * W;
  const int S = L - 2 * R, base = seg * S - R;
  struct alignas(W * sizeof(T)) Vec { T v[W]; };
  struct alignas(W) MVec { uint8_t v[W]; };
  const bool vec = y0 + W <= n1 && (n1 % W) == 0 && (reinterpret_cast<size_t>(image) & (W * sizeof(T) - 1)) == 0 &&
                   (reinterpret_cast<size_t>(num) & (W * sizeof(T) - 1)) == 0 &&
                   (reinterpret_cast<size_t>(den) & (W * sizeof(T) - 1)) == 0 && (reinterpret_cast<size_t>(mask) & (W - 1)) == 0;
  cpx<T> x[NT][16];
  unsigned long long bits = 0;   // the mask of the thread's 16 x W samples: what the second transform is built from
  T lo = INFINITY, hi = -INFINITY;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int row = prep_fold(base + t + TPF * i, n0);
    const size_t o = (size_t)row * n1 + y0;
    Vec v;
    MVec m;
    if (vec) {
      if constexpr (MODE != 2) v = *reinterpret_cast<const Vec*>(image + o);
      m = *reinterpret_cast<const MVec*>(mask + o);
    } else {
#pragma unroll
      for (int k = 0; k < W; ++k) {
        if constexpr (MODE != 2) v.v[k] = y0 + k < n1 ? image[o + k] : T(0);
        m.v[k] = y0 + k < n1 ? mask[o + k] : uint8_t(0);
      }
    }
#pragma unroll
    for (int k = 0; k < W; ++k) {
      const bool on = m.v[k] != 0;
      if constexpr (MODE == 2) {
        v.v[k] = on ? T(1) : T(0);
      } else if (on) {
        if constexpr (MODE == 0) bits |= 1ull << (i * W + k);
        lo = v.v[k] < lo ? v.v[k] : lo;
        hi = v.v[k] > hi ? v.v[k] : hi;
      } else {
        v.v[k] = T(0);
      }
    }
#pragma unroll
    for (int n = 0; n < NT; ++n) x[n][i] = {v.v[2 * n], v.v[2 * n + 1]};
  }
  if constexpr (MODE != 2) wave_minmax(lo, hi, mm);
  typename F::Twiddles tw;
  F::load_twiddles(tw, twtab, t);
  if constexpr (MODE != 0) {
    cols_field<T, LG, NT>(x, lds, t, tw, H, MODE == 1 ? num : den, base, R, n0, n1, y0, vec);
  } else {
    cols_field<T, LG, NT>(x, lds, t, tw, H, num, base, R, n0, n1, y0, vec);
    __syncthreads();   // the first field's last LDS reads are done before the second field's first writes
#pragma unroll
    for (int i = 0; i < 16; ++i)
#pragma unroll
      for (int n = 0; n < NT; ++n)
        x[n][i] = {T((bits >> (i * W + 2 * n)) & 1ull), T((bits >> (i * W + 2 * n + 1)) & 1ull)};
    cols_field<T, LG, NT>(x, lds, t, tw, H, den, base, R, n0, n1, y0, vec);
  }
}

// rows: two adjacent rows per transform, num first (kept in registers), then den; the epilogue divides
template <class T, int LG>
__global__ __launch_bounds__((GenGeom<T, LG>::THREADS)) void prep_rows_kernel(
    const T* __restrict__ num, const T* __restrict__ den, const uint8_t* __restrict__ cov, const T* __restrict__ image, T* out, T* vv,
    int n0, int n1, int R, int nseg, const T* __restrict__ H, const cpx<T>* __restrict__ twtab, T fill,
    const unsigned long long* __restrict__ mm) {
  using F = WgFFT<T, LG>;
  using G = GenGeom<T, LG>;
  constexpr int TPF = F::TPF, L = F::L;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x % TPF, f = threadIdx.x / TPF;
  cpx<T>* lds = reinterpret_cast<cpx<T>*>(smem) + f * G::RS;
  const int g = blockIdx.x * G::NF + f;
  const int pair = g / nseg, seg = g - pair * nseg;
  const int ra = 2 * pair, rb = ra + 1;
  const bool va = ra < n0, vb = rb < n0;
  const int S = L - 2 * R, base = seg * S - R;
  const size_t oa = (size_t)(va ? ra : 0) * n1, ob = (size_t)(vb ? rb : 0) * n1;
  typename F::Twiddles tw;
  F::load_twiddles(tw, twtab, tid);
  const bool inside = base >= 0 && base + L <= n1;
  cpx<T> x[16], q[16];
  // one field: load (reflected), forward, transfer function, inverse.  Called once per field rather than looped over, so that
  // nothing of one field stays in registers for the other.
  auto filter = [&](const T* __restrict__ src) {
    const T* pa = src + oa;
    const T* pb = src + ob;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int slot = tid + TPF * i;
      const int j = inside ? base + slot : prep_fold(base + slot, n1);
      x[i] = {va ? pa[j] : T(0), vb ? pb[j] : T(0)};
    }
    F::forward(x, lds, tid, tw);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const T h = H[i * TPF + tid];
      x[i] = {x[i].x * h, x[i].y * h};
    }
    F::inverse(x, lds, tid, tw);
  };
  filter(num);
#pragma unroll
  for (int i = 0; i < 16; ++i) q[i] = x[i];
  __syncthreads();   // the first field's last LDS reads are done before the second field's first writes
  filter(den);
  if (!va) return;
  const T lo = (T)of_key(mm[0]), hi = (T)of_key(mm[1]);
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int slot = tid + TPF * i, n = base + slot;
    if (slot >= R && slot < L - R && n < n1) {
      finish_pixel<T>(q[i].x, x[i].x, cov[oa + n] != 0, image[oa + n], fill, lo, hi, out, vv, oa + n);
      if (vb) finish_pixel<T>(q[i].y, x[i].y, cov[ob + n] != 0, image[ob + n], fill, lo, hi, out, vv, ob + n);
    }
  }
}

// the row pass of the longest transforms (prep_split): the plain row filter of gpa_gaussfft.hip runs twice -- num into `out`,
// den into the num plane, which the first has consumed -- and this kernel divides
template <class T>
__global__ __launch_bounds__(256) void prep_finish_kernel(const T* __restrict__ den, const uint8_t* __restrict__ cov,
                                                         const T* __restrict__ image, T* out, T* vv, size_t npx, T fill,
                                                         const unsigned long long* __restrict__ mm) {
  const size_t o = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= npx) return;
  finish_pixel<T>(out[o], den[o], cov[o] != 0, image[o], fill, (T)of_key(mm[0]), (T)of_key(mm[1]), out, vv, o);
}

// ---- direct route (radii below GAUSS_FFT_MINR, or where no segment length fits): sums in double ----------------------------
template <class T>
__global__ __launch_bounds__(256) void prep_cols_direct_kernel(const T* __restrict__ image, const uint8_t* __restrict__ mask,
                                                              T* __restrict__ num, T* __restrict__ den, int n0, int n1, int R,
                                                              const double* __restrict__ w, unsigned long long* mm) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
  double lo = INFINITY, hi = -INFINITY;
  if (j < n1) {
    double a = 0.0, b = 0.0;
    for (int k = -R; k <= R; ++k) {
      const size_t o = (size_t)prep_fold(i + k, n0) * n1 + j;
      if (mask[o]) {
        const double v = (double)image[o];
        a += w[k + R] * v;
        b += w[k + R];
        lo = v < lo ? v : lo;
        hi = v > hi ? v : hi;
      }
    }
    num[(size_t)i * n1 + j] = (T)a;
    den[(size_t)i * n1 + j] = (T)b;
  }
  wave_minmax(lo, hi, mm);
}

template <class T>
__global__ __launch_bounds__(256) void prep_rows_direct_kernel(const T* __restrict__ num, const T* __restrict__ den,
                                                              const uint8_t* __restrict__ cov, const T* __restrict__ image, T* out,
                                                              T* vv, int n0, int n1, int R, const double* __restrict__ w, T fill,
                                                              const unsigned long long* __restrict__ mm) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
  if (j >= n1) return;
  const size_t r = (size_t)i * n1;
  double a = 0.0, b = 0.0;
  for (int k = -R; k <= R; ++k) {
    const int jj = prep_fold(j + k, n1);
    a += w[k + R] * (double)num[r + jj];
    b += w[k + R] * (double)den[r + jj];
  }
  finish_pixel<T>((T)a, (T)b, cov[r + j] != 0, image[r + j], fill, (T)of_key(mm[0]), (T)of_key(mm[1]), out, vv, r + j);
}

// ---- coverage, in integers -------------------------------------------------------------------------------------------------
// c0[i][j] = any mask[prep_fold(i + d, n0)][j], |d| <= R: a thread walks PREP_COV_CHUNK rows of one column with a running
// count over the interval of prep_reflect_interval, whose ends move by at most one sample per row
__global__ __launch_bounds__(256) void cov_cols_kernel(const uint8_t* __restrict__ mask, uint8_t* __restrict__ c0, int n0, int n1,
                                                      int R) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n1) return;
  const int i0 = blockIdx.y * PREP_COV_CHUNK, i1 = min(i0 + PREP_COV_CHUNK, n0);
  const uint8_t* m = mask + j;
  uint8_t* dst = c0 + j;
  int lo, hi, count = 0;
  prep_reflect_interval(i0, R, n0, &lo, &hi);
#pragma unroll 8
  for (int r = lo; r <= hi; ++r) count += m[(size_t)r * n1] != 0;
  dst[(size_t)i0 * n1] = count > 0;
  // rows whose run i - R .. i + R and whose predecessor's lie inside the image: one sample enters, one leaves, and the loads
  // of several rows are in flight at once
  const int ia = min(max(i0 + 1, R + 1), i1), ib = max(min(i1, n0 - R), ia);
  auto step = [&](int i) {
    int l2, h2;
    prep_reflect_interval(i, R, n0, &l2, &h2);
    while (lo > l2) { --lo; count += m[(size_t)lo * n1] != 0; }
    while (hi < h2) { ++hi; count += m[(size_t)hi * n1] != 0; }
    while (lo < l2) { count -= m[(size_t)lo * n1] != 0; ++lo; }
    while (hi > h2) { count -= m[(size_t)hi * n1] != 0; --hi; }
    dst[(size_t)i * n1] = count > 0;
  };
  for (int i = i0 + 1; i < ia; ++i) step(i);
  if (ib > ia) {
#pragma unroll 8
    for (int i = ia; i < ib; ++i) {
      count += (m[(size_t)(i + R) * n1] != 0) - (m[(size_t)(i - 1 - R) * n1] != 0);
      dst[(size_t)i * n1] = count > 0;
    }
    lo = ib - 1 - R;
    hi = ib - 1 + R;
  }
  for (int i = ib; i < i1; ++i) step(i);
}

// cov[i][j] = any c0[i][prep_fold(j + d, n1)], |d| <= R: a workgroup per row, prefix counts of the row in LDS (n1 + 1 ints)
__global__ __launch_bounds__(256) void cov_rows_kernel(const uint8_t* __restrict__ c0, uint8_t* __restrict__ cov, int n1, int R) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int* pre = reinterpret_cast<int*>(smem);   // pre[j] = true samples in [0, j)
  __shared__ int part[256];
  const int t = threadIdx.x, chunk = (n1 + 255) / 256, a = min(t * chunk, n1), b = min(a + chunk, n1);
  const uint8_t* row = c0 + (size_t)blockIdx.x * n1;
  int s = 0;
  for (int j = a; j < b; ++j) s += row[j] != 0;
  part[t] = s;
  __syncthreads();
  if (t == 0) {
    int acc = 0;
    for (int k = 0; k < 256; ++k) { const int v = part[k]; part[k] = acc; acc += v; }
    pre[n1] = acc;
  }
  __syncthreads();
  s = part[t];
  for (int j = a; j < b; ++j) { pre[j] = s; s += row[j] != 0; }
  __syncthreads();
  uint8_t* dst = cov + (size_t)blockIdx.x * n1;
  for (int j = t; j < n1; j += 256) {
    int lo, hi;
    prep_reflect_interval(j, R, n1, &lo, &hi);
    dst[j] = pre[hi + 1] - pre[lo] > 0;
  }
}

// ---- mask of a stack -------------------------------------------------------------------------------------------------------
template <class T>
__global__ __launch_bounds__(256) void any_equal_kernel(const T* __restrict__ frames, int B, size_t npx, T value, int accumulate,
                                                       uint8_t* hit) {
  const size_t o = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= npx) return;
  bool h = accumulate && hit[o] != 0;
  for (int b = 0; b < B; ++b) h = h || frames[(size_t)b * npx + o] == value;   // (a NaN never compares equal)
  hit[o] = h;
}

// ---- erosion with disk(r) --------------------------------------------------------------------------------------------------
// hd[i][j] = distance to the nearest false sample of row i, the positions -1 and n1 counting as false, saturated at r + 1
__global__ __launch_bounds__(256) void erode_dist_kernel(const uint8_t* __restrict__ in, int invert, uint8_t* __restrict__ hd, int n1,
                                                        int r) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n1) return;
  const uint8_t* row = in + (size_t)blockIdx.y * n1;
  const bool inv = invert != 0;
  int d = 0;
  for (; d <= r; ++d) {
    const int a = j - d, b = j + d;
    if (a < 0 || b >= n1) break;
    const bool ta = (row[a] != 0) != inv, tb = (row[b] != 0) != inv;
    if (!ta || !tb) break;
  }
  hd[(size_t)blockIdx.y * n1 + j] = (uint8_t)d;
}

// out[i][j] = AND over |dy| <= r of hd[i + dy][j] > chord(dy), rows outside the image counting as hd = 0
__global__ __launch_bounds__(256) void erode_disk_kernel(const uint8_t* __restrict__ hd, const uint8_t* __restrict__ chord,
                                                        uint8_t* __restrict__ out, int n0, int n1, int r) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
  if (j >= n1) return;
  bool keep = i - r >= 0 && i + r < n0;
  for (int dy = -r; keep && dy <= r; ++dy) keep = hd[(size_t)(i + dy) * n1 + j] > chord[dy + r];
  out[(size_t)i * n1 + j] = keep;
}

// ---- bounds of a mask ------------------------------------------------------------------------------------------------------
__global__ void bounds_init_kernel(int* lims, int n0, int n1) {
  lims[0] = n0; lims[1] = 0; lims[2] = n1; lims[3] = 0;
}
__global__ __launch_bounds__(256) void mask_bounds_kernel(const uint8_t* __restrict__ mask, int n0, int n1, int* lims) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
  const bool on = j < n1 && mask[(size_t)i * n1 + j] != 0;
  int jl = on ? j : n1, jh = on ? j + 1 : 0;
#pragma unroll
  for (int o = 32; o; o >>= 1) {
    jl = min(jl, __shfl_xor(jl, o));
    jh = max(jh, __shfl_xor(jh, o));
  }
  if ((threadIdx.x & 63) == 0 && jh > 0) {
    atomicMin(&lims[0], i);
    atomicMax(&lims[1], i + 1);
    atomicMin(&lims[2], jl);
    atomicMax(&lims[3], jh);
  }
}

// ---- NaN lines and the trim loop ---------------------------------------------------------------------------------------------
template <class T>
__global__ __launch_bounds__(256) void nan_rows_kernel(const T* __restrict__ image, int n1, uint8_t* rows) {
  __shared__ int seen;
  if (threadIdx.x == 0) seen = 0;
  __syncthreads();
  const T* row = image + (size_t)blockIdx.x * n1;
  int finite = 0;
  for (int j = threadIdx.x; j < n1; j += 256) finite |= !(row[j] != row[j]);
  if (finite) seen = 1;
  __syncthreads();
  if (threadIdx.x == 0) rows[blockIdx.x] = !seen;
}
template <class T>
__global__ __launch_bounds__(256) void nan_cols_kernel(const T* __restrict__ image, int n0, int n1, uint8_t* cols) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n1) return;
  int finite = 0;
  for (int i = 0; i < n0 && !finite; ++i) { const T v = image[(size_t)i * n1 + j]; finite = !(v != v); }
  cols[j] = !finite;
}

constexpr int TRIM_THREADS = 1024;
template <class T>
struct TrimCounter {
  const T* image;
  int n1;
  int* red;   // LDS: one slot per wave, then the total
  __device__ int total(int v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();   // the previous total has been read by everyone
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    int s = 0;
#pragma unroll
    for (int k = 0; k < TRIM_THREADS / 64; ++k) s += red[k];
    return s;
  }
  __device__ int row(int x, int y0, int y1) {
    int v = 0;
    for (int y = y0 + (int)threadIdx.x; y < y1; y += TRIM_THREADS) { const T s = image[(size_t)x * n1 + y]; v += s != s; }
    return total(v);
  }
  __device__ int col(int y, int x0, int x1) {
    int v = 0;
    for (int x = x0 + (int)threadIdx.x; x < x1; x += TRIM_THREADS) { const T s = image[(size_t)x * n1 + y]; v += s != s; }
    return total(v);
  }
  __device__ int at(int x, int y) const { const T s = image[(size_t)x * n1 + y]; return s != s; }
};
template <class T>
__global__ __launch_bounds__(TRIM_THREADS) void trim_kernel(const T* __restrict__ image, int n0, int n1, int* lims) {
  __shared__ int red[TRIM_THREADS / 64];
  TrimCounter<T> c{image, n1, red};
  int l[4];
  prep_trim_loop(c, n0, n1, l);
  if (threadIdx.x < 4) lims[threadIdx.x] = l[threadIdx.x];
}

template <class T, int LG>
hipError_t run_fft(const T* image, const uint8_t* mask, T* num, T* den, const uint8_t* cov, T* out, T* vv, int n0, int n1, int R,
                   int axis, const void* H, const void* tw, T fill, unsigned long long* mm, hipStream_t s) {
  if (axis == 0) {
    using G = GfColGeom<T, LG>;
    if constexpr (!G::FITS) return hipErrorInvalidValue;
    else {
      constexpr bool SPLIT = prep_split<T, LG>();
      auto kern = prep_cols_kernel<T, LG, SPLIT ? 1 : 0>;
      auto kern2 = prep_cols_kernel<T, LG, SPLIT ? 2 : 0>;
      static unsigned lds_set = 0, lds_set2 = 0;
      hipError_t e = set_dynamic_lds_once(reinterpret_cast<const void*>(kern), (int)G::LDS_BYTES, lds_set);
      if (e == hipSuccess && SPLIT) e = set_dynamic_lds_once(reinterpret_cast<const void*>(kern2), (int)G::LDS_BYTES, lds_set2);
      if (e != hipSuccess) return e;
      const int S = (1 << LG) - 2 * R, nseg = (n0 + S - 1) / S;
      const dim3 grid((n1 + G::RC - 1) / G::RC, nseg);
      GPA_PROF("prep_cols_kernel", s);
      kern<<<grid, G::THREADS, G::LDS_BYTES, s>>>(image, mask, num, den, n0, n1, R, (const T*)H, (const cpx<T>*)tw, mm);
      if constexpr (SPLIT) kern2<<<grid, G::THREADS, G::LDS_BYTES, s>>>(image, mask, num, den, n0, n1, R, (const T*)H, (const cpx<T>*)tw, mm);
      return hipGetLastError();
    }
  } else {
    using G = GenGeom<T, LG>;
    if constexpr (!G::FITS) return hipErrorInvalidValue;
    else {
      if constexpr (prep_split<T, LG>()) {
        const int dtype = sizeof(T) == 4 ? 0 : 1;
        hipError_t e = launch_gaussfft(dtype, LG, 1, num, out, n0, n1, R, H, tw, nullptr, s);
        if (e == hipSuccess) e = launch_gaussfft(dtype, LG, 1, den, num, n0, n1, R, H, tw, nullptr, s);
        if (e != hipSuccess) return e;
        const size_t npx = (size_t)n0 * n1;
        GPA_PROF("prep_finish_kernel", s);
        prep_finish_kernel<T><<<(unsigned)((npx + 255) / 256), 256, 0, s>>>(num, cov, image, out, vv, npx, fill, mm);
      } else {
        auto kern = prep_rows_kernel<T, LG>;
        static unsigned lds_set = 0;
        hipError_t e = set_dynamic_lds_once(reinterpret_cast<const void*>(kern), (int)G::LDS_BYTES, lds_set);
        if (e != hipSuccess) return e;
        const int S = (1 << LG) - 2 * R, nseg = (n1 + S - 1) / S;
        const size_t ntr = (size_t)((n0 + 1) / 2) * nseg;
        GPA_PROF("prep_rows_kernel", s);
        kern<<<(unsigned)((ntr + G::NF - 1) / G::NF), G::THREADS, G::LDS_BYTES, s>>>(num, den, cov, image, out, vv, n0, n1, R, nseg,
                                                                                     (const T*)H, (const cpx<T>*)tw, fill, mm);
      }
      return hipGetLastError();
    }
  }
}

template <class T>
hipError_t homogenize_t(const PrepHomogenize& a, hipStream_t s) {
  const int n0 = a.n0, n1 = a.n1, R = a.R;
  const T* image = (const T*)a.image;
  T *num = (T*)a.num, *den = (T*)a.den, *out = (T*)a.out, *vv = (T*)a.vv;
  const T fill = a.use_nan_scale ? (T)a.nan_scale : (T)NAN;
  hipError_t e;
  minmax_init_kernel<<<1, 1, 0, s>>>(a.mm);
  {
    GPA_PROF("prep_cov_cols_kernel", s);
    cov_cols_kernel<<<dim3((n1 + 255) / 256, (n0 + PREP_COV_CHUNK - 1) / PREP_COV_CHUNK), 256, 0, s>>>(a.mask, a.cov0, n0, n1, R);
  }
  {
    static unsigned lds_set = 0;
    e = set_dynamic_lds_once(reinterpret_cast<const void*>(cov_rows_kernel), 4 * (PREP_MAX_N1 + 1), lds_set);
    if (e != hipSuccess) return e;
    GPA_PROF("prep_cov_rows_kernel", s);
    cov_rows_kernel<<<n0, 256, 4 * ((size_t)n1 + 1), s>>>(a.cov0, a.cov, n1, R);
  }
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if (a.lg0 && a.lg1) {
#define CASE(LG) case LG: e = run_fft<T, LG>(image, a.mask, num, den, a.cov, out, vv, n0, n1, R, 0, a.H0, a.tw0, fill, a.mm, s); break;
    switch (a.lg0) { GPA_FOR_LG(CASE) default: e = hipErrorInvalidValue; }
#undef CASE
    if (e != hipSuccess) return e;
#define CASE(LG) case LG: e = run_fft<T, LG>(image, a.mask, num, den, a.cov, out, vv, n0, n1, R, 1, a.H1, a.tw1, fill, a.mm, s); break;
    switch (a.lg1) { GPA_FOR_LG(CASE) default: e = hipErrorInvalidValue; }
#undef CASE
    return e;
  }
  {
    GPA_PROF("prep_cols_direct_kernel", s);
    prep_cols_direct_kernel<T><<<dim3((n1 + 255) / 256, n0), 256, 0, s>>>(image, a.mask, num, den, n0, n1, R, a.w, a.mm);
  }
  {
    GPA_PROF("prep_rows_direct_kernel", s);
    prep_rows_direct_kernel<T><<<dim3((n1 + 255) / 256, n0), 256, 0, s>>>(num, den, a.cov, image, out, vv, n0, n1, R, a.w, fill, a.mm);
  }
  return hipGetLastError();
}

}  // namespace

hipError_t prep_homogenize(int dtype, const PrepHomogenize& a, hipStream_t s) {
  return dtype == 0 ? homogenize_t<float>(a, s) : homogenize_t<double>(a, s);
}

hipError_t prep_any_equal(int dtype, const void* frames, int B, int n0, int n1, double value, int accumulate, uint8_t* hit,
                          hipStream_t s) {
  const size_t npx = (size_t)n0 * n1;
  const unsigned grid = (unsigned)((npx + 255) / 256);
  GPA_PROF("prep_any_equal_kernel", s);
  if (dtype == 0) any_equal_kernel<float><<<grid, 256, 0, s>>>((const float*)frames, B, npx, (float)value, accumulate, hit);
  else any_equal_kernel<double><<<grid, 256, 0, s>>>((const double*)frames, B, npx, value, accumulate, hit);
  return hipGetLastError();
}

hipError_t prep_erode_disk(const uint8_t* in, int invert, int r, int n0, int n1, uint8_t* hd, const uint8_t* chord, uint8_t* out,
                           hipStream_t s) {
  const dim3 grid((n1 + 255) / 256, n0);
  {
    GPA_PROF("prep_erode_dist_kernel", s);
    erode_dist_kernel<<<grid, 256, 0, s>>>(in, invert, hd, n1, r);
  }
  {
    GPA_PROF("prep_erode_disk_kernel", s);
    erode_disk_kernel<<<grid, 256, 0, s>>>(hd, chord, out, n0, n1, r);
  }
  return hipGetLastError();
}

hipError_t prep_mask_bounds(const uint8_t* mask, int n0, int n1, int* lims, hipStream_t s) {
  bounds_init_kernel<<<1, 1, 0, s>>>(lims, n0, n1);
  GPA_PROF("prep_mask_bounds_kernel", s);
  mask_bounds_kernel<<<dim3((n1 + 255) / 256, n0), 256, 0, s>>>(mask, n0, n1, lims);
  return hipGetLastError();
}

hipError_t prep_nan_lines(int dtype, const void* image, int n0, int n1, uint8_t* rows, uint8_t* cols, hipStream_t s) {
  GPA_PROF("prep_nan_lines_kernels", s);
  if (dtype == 0) {
    nan_rows_kernel<float><<<n0, 256, 0, s>>>((const float*)image, n1, rows);
    nan_cols_kernel<float><<<(n1 + 255) / 256, 256, 0, s>>>((const float*)image, n0, n1, cols);
  } else {
    nan_rows_kernel<double><<<n0, 256, 0, s>>>((const double*)image, n1, rows);
    nan_cols_kernel<double><<<(n1 + 255) / 256, 256, 0, s>>>((const double*)image, n0, n1, cols);
  }
  return hipGetLastError();
}

hipError_t prep_trim_lims(int dtype, const void* image, int n0, int n1, int* lims, hipStream_t s) {
  GPA_PROF("prep_trim_kernel", s);
  if (dtype == 0) trim_kernel<float><<<1, TRIM_THREADS, 0, s>>>((const float*)image, n0, n1, lims);
  else trim_kernel<double><<<1, TRIM_THREADS, 0, s>>>((const double*)image, n0, n1, lims);
  return hipGetLastError();
}

}  // namespace gpa
