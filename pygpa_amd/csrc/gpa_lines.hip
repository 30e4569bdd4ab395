// Per-line medians and the passes of homogenize_per_axis (pyGPA/imagetools.py:112-125).  Geometry, keys and ranks: gpa_lines.h.
//
//   lines_transpose_kernel   image (+ mask: a masked sample becomes NaN) -> its transpose, through a padded 32 x 32 LDS tile,
//                            so that the column medians are row medians of the transposed plane
//   lines_median_kernel      one workgroup per line: the line is loaded ONCE (mask and per-column divisor applied on the way),
//                            its keys stay in LDS, a radix selection of 8 bits per pass finds the key of rank (m - 1) / 2, and
//                            rank m / 2 follows from the counts the selection leaves behind
//   lines_profile_kernel     gaussian_filter of a line of medians: one wave per output sample, a direct f64 sum over the
//                            reflect fold, rounded once
//   lines_scale_kernel       q = profile / max(profile), the maximum propagating NaN as np.max does
//   lines_apply_kernel       out = (image / q0[column]) / q1[row]: the two divisions of the reference, in its order
//
// Histogram of a pass.  Real images are smooth: nearly all keys of a line share their upper bytes, and 64 lanes adding to ONE
// LDS bin serialise.  Every wave therefore has a private histogram, and the lanes that share the bin of the wave's first pending
// lane are counted by a ballot and added by that lane alone, as one number.  A uniform wave -- the smooth image's upper bytes --
// costs one LDS add; the lanes of other bins add for themselves, and among them collisions are rare (white noise: 64 distinct
// bins) or at worst half as deep as before.  More such rounds were measured and cost more than they saved: a round is a dozen
// instructions for every key, a collision only LDS cycles.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "gpa_internal.h"
#include "gpa_lines.h"

namespace gpa {
namespace {

template <class T> struct LineKey;
template <> struct LineKey<float> {
  typedef unsigned int K;
  static constexpr K NANKEY = LINES_NAN_KEY32;
  __device__ static K key(float v) { return lines_key((uint32_t)__float_as_uint(v)); }
  __device__ static float value(K k) { return __uint_as_float(lines_unkey((uint32_t)k)); }
};
template <> struct LineKey<double> {
  typedef unsigned long long K;
  static constexpr K NANKEY = LINES_NAN_KEY64;
  __device__ static K key(double v) { return (K)lines_key((uint64_t)__double_as_longlong(v)); }
  __device__ static double value(K k) { return __longlong_as_double((long long)lines_unkey((uint64_t)k)); }
};

template <class T>
__global__ __launch_bounds__(256) void lines_transpose_kernel(const T* __restrict__ in, const uint8_t* __restrict__ mask,
                                                              T* __restrict__ out, int n0, int n1) {
  __shared__ T tile[LINES_TILE][LINES_TILE_PITCH];
  const size_t npx = (size_t)n0 * n1, f = blockIdx.z;
  const int tx = threadIdx.x, ty = threadIdx.y;
  const int x = blockIdx.x * LINES_TILE + tx;
  for (int j = ty; j < LINES_TILE; j += 8) {
    const int y = blockIdx.y * LINES_TILE + j;
    if (x < n1 && y < n0) {
      const size_t at = (size_t)y * n1 + x;
      T v = in[f * npx + at];
      if (mask && !mask[at]) v = (T)NAN;
      tile[j][tx] = v;
    }
  }
  __syncthreads();
  const int x2 = blockIdx.y * LINES_TILE + tx;        // along n0: the fast axis of the transposed plane
  for (int j = ty; j < LINES_TILE; j += 8) {
    const int y2 = blockIdx.x * LINES_TILE + j;       // along n1
    if (x2 < n0 && y2 < n1) out[f * npx + (size_t)y2 * n0 + x2] = tile[tx][j];
  }
}

// src: [frames][nlines][n]; mask (nullable): [nlines][n] bytes, shared by the frames; q (nullable): [frames] lines of n
// divisors, q_stride apart; med: [frames] lines of nlines medians, med_stride apart.  propagate: a NaN or masked sample makes
// the median NaN (np.median); otherwise such samples are left out (np.nanmedian) and a line without any sample gives NaN.
// LONG: the instantiation for lines whose keys need more than the 64 KiB of dynamic LDS a kernel gets without asking; only it
// has its limit raised (set_dynamic_lds_once), the other one is launched as it is.
template <class T, bool LONG>
__global__ __launch_bounds__(LINES_THREADS) void lines_median_kernel(const T* __restrict__ src, const uint8_t* __restrict__ mask,
                                                                     const T* __restrict__ q, size_t q_stride, int n, int nlines,
                                                                     int propagate, T* __restrict__ med, size_t med_stride) {
  typedef typename LineKey<T>::K K;
  constexpr K NANKEY = LineKey<T>::NANKEY;
  extern __shared__ __align__(16) unsigned char lines_lds[];
  K* keys = reinterpret_cast<K*>(lines_lds);
  __shared__ unsigned hist[LINES_WAVES * 256];
  __shared__ unsigned wsum[LINES_WAVES];
  __shared__ unsigned sel[3];
  __shared__ unsigned s_nan;
  __shared__ K s_above;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int line = blockIdx.x;
  const size_t f = blockIdx.y;
  const T* row = src + (f * nlines + line) * (size_t)n;
  const uint8_t* mrow = mask ? mask + (size_t)line * n : nullptr;
  const T* qf = q ? q + f * q_stride : nullptr;
  if (tid == 0) { s_nan = 0; s_above = NANKEY; }
  __syncthreads();

  // the one load of the line, four samples of a thread in flight at a time
  unsigned nans = 0;
  for (int base = tid; base < n; base += LINES_BATCH * LINES_THREADS) {
    T v[LINES_BATCH];
    uint8_t ok[LINES_BATCH];
#pragma unroll
    for (int u = 0; u < LINES_BATCH; ++u) {
      const int i = base + u * LINES_THREADS;
      v[u] = i < n ? row[i] : (T)0;
      ok[u] = (mrow && i < n) ? mrow[i] : (uint8_t)1;
    }
    if (qf) {
      T d[LINES_BATCH];
#pragma unroll
      for (int u = 0; u < LINES_BATCH; ++u) {
        const int i = base + u * LINES_THREADS;
        d[u] = i < n ? qf[i] : (T)1;
      }
#pragma unroll
      for (int u = 0; u < LINES_BATCH; ++u) v[u] = v[u] / d[u];
    }
#pragma unroll
    for (int u = 0; u < LINES_BATCH; ++u) {
      const int i = base + u * LINES_THREADS;
      if (i < n) {
        const K k = ok[u] ? LineKey<T>::key(v[u]) : NANKEY;
        keys[i] = k;
        nans += k == NANKEY;
      }
    }
  }
  for (int d = 32; d >= 1; d >>= 1) nans += (unsigned)__shfl_xor((int)nans, d);
  if (lane == 0 && nans) atomicAdd(&s_nan, nans);
  __syncthreads();
  const int m = n - (int)s_nan;

  // radix selection of rank (m - 1) / 2 among all n keys (the NaN keys are the largest, so the valid ranks are unchanged)
  unsigned r = m > 0 ? (unsigned)lines_rank_lo(m) : 0u;
  unsigned less = 0, ceq = 0;
  K prefix = 0, pmask = 0;
  unsigned* myhist = hist + wave * 256;
  for (int shift = 8 * (int)sizeof(K) - 8; shift >= 0; shift -= 8) {
    for (int j = tid; j < LINES_WAVES * 256; j += LINES_THREADS) hist[j] = 0;
    __syncthreads();
    for (int base = tid; base < n; base += LINES_BATCH * LINES_THREADS) {
      K kk[LINES_BATCH];
      bool in[LINES_BATCH];
      bool any = false;
#pragma unroll
      for (int u = 0; u < LINES_BATCH; ++u) {
        const int i = base + u * LINES_THREADS;
        kk[u] = i < n ? keys[i] : (K)0;
      }
#pragma unroll
      for (int u = 0; u < LINES_BATCH; ++u) {
        in[u] = base + u * LINES_THREADS < n && (kk[u] & pmask) == prefix;
        any = any || in[u];
      }
      if (!__ballot(any)) continue;      // no key of this batch is still in the running: the usual case of the later passes
#pragma unroll
      for (int u = 0; u < LINES_BATCH; ++u) {
        bool todo = in[u];
        const unsigned bin = (unsigned)(kk[u] >> shift) & 255u;
        const unsigned long long pending = __ballot(todo);
        if (pending) {
          const int leader = __ffsll((long long)pending) - 1;
          const unsigned b = (unsigned)__builtin_amdgcn_readlane((int)bin, leader);
          const bool same = todo && bin == b;
          const unsigned long long group = __ballot(same);
          if (lane == leader) atomicAdd(&myhist[b], (unsigned)__popcll(group));   // no return value: the wave does not wait
          todo = todo && !same;
        }
        if (todo) atomicAdd(&myhist[bin], 1u);
      }
    }
    __syncthreads();
    unsigned c = 0;
    for (int w = 0; w < LINES_WAVES; ++w) c += hist[w * 256 + tid];
    unsigned incl = c;
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned up = (unsigned)__shfl_up((int)incl, d);
      if (lane >= d) incl += up;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    for (int w = 0; w < wave; ++w) incl += wsum[w];
    const unsigned excl = incl - c;
    if (excl <= r && r < incl) { sel[0] = (unsigned)tid; sel[1] = excl; sel[2] = c; }
    __syncthreads();
    prefix |= (K)sel[0] << shift;
    pmask |= (K)255 << shift;
    less += sel[1];
    r -= sel[1];
    ceq = sel[2];
  }
  const K k1 = prefix;

  // the smallest key above k1: rank m / 2 where the keys <= k1 do not reach it
  K above = NANKEY;
  for (int base = tid; base < n; base += LINES_BATCH * LINES_THREADS) {
    K kk[LINES_BATCH];
#pragma unroll
    for (int u = 0; u < LINES_BATCH; ++u) {
      const int i = base + u * LINES_THREADS;
      kk[u] = i < n ? keys[i] : NANKEY;
    }
#pragma unroll
    for (int u = 0; u < LINES_BATCH; ++u)
      if (kk[u] > k1 && kk[u] < above) above = kk[u];
  }
  if (above != NANKEY) atomicMin(&s_above, above);
  __syncthreads();
  if (tid == 0) {
    T res;
    if (m <= 0 || (propagate && m < n)) res = (T)NAN;
    else {
      const T a = LineKey<T>::value(k1);
      if (m & 1) res = a;
      else {
        const K k2 = lines_upper_is_same((int)(less + ceq), m) ? k1 : s_above;
        res = (a + LineKey<T>::value(k2)) * (T)0.5;
      }
    }
    med[f * med_stride + line] = res;
  }
}

// prof[i] = sum_k w[k + R] line[fold(i + k)], k = -R .. R: one wave per sample, lanes stride the taps, f64 throughout
template <class T>
__global__ __launch_bounds__(256) void lines_profile_kernel(const T* __restrict__ line, size_t line_stride, const double* __restrict__ w,
                                                            int R, int n, T* __restrict__ prof, size_t prof_stride) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = blockIdx.x * 4 + wave;
  if (i >= n) return;
  const T* src = line + (size_t)blockIdx.y * line_stride;
  double acc = 0.0;
  for (int t = lane; t < 2 * R + 1; t += 64) acc = fma(w[t], (double)src[lines_fold(i + t - R, n)], acc);
  for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d);
  if (lane == 0) prof[(size_t)blockIdx.y * prof_stride + i] = (T)acc;
}

// q = prof / max(prof); one workgroup per frame
template <class T>
__global__ __launch_bounds__(256) void lines_scale_kernel(const T* __restrict__ prof, size_t stride, int n, T* __restrict__ q) {
  __shared__ T smax[256];
  __shared__ int snan;
  const int tid = threadIdx.x;
  const T* p = prof + (size_t)blockIdx.x * stride;
  T* qo = q + (size_t)blockIdx.x * stride;
  if (tid == 0) snan = 0;
  __syncthreads();
  T mx = (T)-INFINITY;
  bool nan = false;
  for (int i = tid; i < n; i += 256) {
    const T v = p[i];
    if (v != v) nan = true;
    else if (v > mx) mx = v;
  }
  smax[tid] = mx;
  if (nan) snan = 1;
  __syncthreads();
  for (int d = 128; d >= 1; d >>= 1) {
    if (tid < d && smax[tid + d] > smax[tid]) smax[tid] = smax[tid + d];
    __syncthreads();
  }
  const T top = snan ? (T)NAN : smax[0];
  for (int i = tid; i < n; i += 256) qo[i] = p[i] / top;
}

template <class T>
__global__ __launch_bounds__(256) void lines_apply_kernel(const T* __restrict__ image, const T* __restrict__ q0, size_t q0_stride,
                                                          const T* __restrict__ q1, size_t q1_stride, T* __restrict__ out, int n0, int n1) {
  const int col = blockIdx.x * 256 + threadIdx.x, row = blockIdx.y;
  const size_t f = blockIdx.z;
  if (col >= n1) return;
  const size_t at = (f * n0 + row) * (size_t)n1 + col;
  T v = image[at] / q0[f * q0_stride + col];
  if (q1) v = v / q1[f * q1_stride + row];
  out[at] = v;
}

template <class T>
hipError_t median_rows_t(const T* src, const uint8_t* mask, const T* q, size_t q_stride, int n, int nlines, int nb, int propagate,
                         T* med, size_t med_stride, hipStream_t s) {
  typedef typename LineKey<T>::K K;
  const size_t lds = lines_lds_bytes(n, sizeof(K));
  const dim3 grid((unsigned)nlines, (unsigned)nb);
  GPA_PROF("lines_median_kernel", s);
  if (lines_long_route(n, sizeof(K))) {
    static unsigned attr_done = 0;
    auto kern = lines_median_kernel<T, true>;
    const hipError_t e = set_dynamic_lds_once(reinterpret_cast<const void*>(kern), (int)lines_lds_bytes(LINES_MAX_N, sizeof(K)), attr_done);
    if (e != hipSuccess) return e;
    kern<<<grid, LINES_THREADS, lds, s>>>(src, mask, q, q_stride, n, nlines, propagate, med, med_stride);
  } else {
    lines_median_kernel<T, false><<<grid, LINES_THREADS, lds, s>>>(src, mask, q, q_stride, n, nlines, propagate, med, med_stride);
  }
  return hipGetLastError();
}

template <class T>
hipError_t median_t(const T* image, const uint8_t* mask, int n0, int n1, int nb, int axis, int propagate, const T* q, size_t q_stride,
                    T* tws, T* med, size_t med_stride, hipStream_t s) {
  if (axis == 1) return median_rows_t<T>(image, mask, q, q_stride, n1, n0, nb, propagate, med, med_stride, s);
  {
    GPA_PROF("lines_transpose_kernel", s);
    lines_transpose_kernel<T><<<dim3((unsigned)lines_tiles(n1), (unsigned)lines_tiles(n0), (unsigned)nb), dim3(LINES_TILE, 8), 0, s>>>(
        image, mask, tws, n0, n1);
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return median_rows_t<T>(tws, nullptr, nullptr, 0, n0, n1, nb, propagate, med, med_stride, s);
}

template <class T>
hipError_t profile_t(const T* line, size_t stride, int n, int nb, const double* w, int R, T* prof, T* q, hipStream_t s) {
  {
    GPA_PROF("lines_profile_kernel", s);
    lines_profile_kernel<T><<<dim3((unsigned)((n + 3) / 4), (unsigned)nb), 256, 0, s>>>(line, stride, w, R, n, prof, stride);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  GPA_PROF("lines_scale_kernel", s);
  lines_scale_kernel<T><<<(unsigned)nb, 256, 0, s>>>(prof, stride, n, q);
  return hipGetLastError();
}

template <class T>
hipError_t apply_t(const T* image, const T* q0, size_t q0_stride, const T* q1, size_t q1_stride, T* out, int n0, int n1, int nb,
                   hipStream_t s) {
  GPA_PROF("lines_apply_kernel", s);
  lines_apply_kernel<T><<<dim3((unsigned)((n1 + 255) / 256), (unsigned)n0, (unsigned)nb), 256, 0, s>>>(image, q0, q0_stride, q1, q1_stride,
                                                                                                     out, n0, n1);
  return hipGetLastError();
}

}  // namespace

hipError_t lines_median(int dtype, const void* image, const uint8_t* mask, int n0, int n1, int nb, int axis, int propagate,
                        const void* q, size_t q_stride, void* tws, void* med, size_t med_stride, hipStream_t s) {
  const int n = axis == 0 ? n0 : n1;
  if (!lines_length_ok(n) || nb < 1 || nb > LINES_MAX_FRAMES || (axis != 0 && axis != 1)) return hipErrorInvalidValue;
  if (dtype == 0)
    return median_t<float>((const float*)image, mask, n0, n1, nb, axis, propagate, (const float*)q, q_stride, (float*)tws, (float*)med,
                           med_stride, s);
  return median_t<double>((const double*)image, mask, n0, n1, nb, axis, propagate, (const double*)q, q_stride, (double*)tws, (double*)med,
                          med_stride, s);
}

hipError_t lines_profile(int dtype, const void* line, size_t stride, int n, int nb, const double* w, int R, void* prof, void* q,
                         hipStream_t s) {
  if (n < 1 || nb < 1 || nb > LINES_MAX_FRAMES || R < 0) return hipErrorInvalidValue;
  if (dtype == 0) return profile_t<float>((const float*)line, stride, n, nb, w, R, (float*)prof, (float*)q, s);
  return profile_t<double>((const double*)line, stride, n, nb, w, R, (double*)prof, (double*)q, s);
}

hipError_t lines_apply(int dtype, const void* image, const void* q0, size_t q0_stride, const void* q1, size_t q1_stride, void* out,
                       int n0, int n1, int nb, hipStream_t s) {
  if (n0 < 1 || n0 > 65535 || n1 < 1 || nb < 1 || nb > LINES_MAX_FRAMES) return hipErrorInvalidValue;
  if (dtype == 0)
    return apply_t<float>((const float*)image, (const float*)q0, q0_stride, (const float*)q1, q1_stride, (float*)out, n0, n1, nb, s);
  return apply_t<double>((const double*)image, (const double*)q0, q0_stride, (const double*)q1, q1_stride, (double*)out, n0, n1, nb, s);
}

}  // namespace gpa
