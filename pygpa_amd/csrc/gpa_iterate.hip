// a8: the kernels between the pieces of iterate_GPA (geometric_phase_analysis.py:116-154) -- polar form and crop of the
// lock-ins with the per-peak maximum of the cropped amplitude, the unwrap weight sqrt(amp / max), and the Huber moments
// (gpa_reconstruct.hip) of several planes per launch.
#include <stdint.h>

#include "gpa_internal.h"

namespace gpa {

template <class T> struct MaxBits;
template <> struct MaxBits<float> { using type = unsigned int; };
template <> struct MaxBits<double> { using type = unsigned long long; };

template <class T>
__device__ __forceinline__ void polar_store(cpx<T> v, size_t o, T* __restrict__ psi, T* __restrict__ amp, T& best) {
  // the angle in double in both precisions (np.angle(0) = atan2(0, 0) = 0): the kernel is bound by memory
  psi[o] = (T)atan2((double)v.y, (double)v.x);
  const T a = (T)hypot(v.x, v.y);
  amp[o] = a;
  best = a > best ? a : best;
}

// P lock-ins on the n0 x n1 grid -> psi = angle, amp = |.| of the window [edge : n0 - edge, edge : n1 - edge] as compact
// m0 x m1 planes; amax[p] = max of amp[p] (the bit pattern of a non-negative IEEE value orders as an unsigned integer, so
// an integer atomic max gives the same bits whatever the order of the workgroups; the caller zeroes amax first).
// grid: (column chunks, row bands, P).  f32: a thread takes the two elements of one 16-byte slot of the source row; a row
// that starts on an odd element (odd edge, or odd n1 and an odd row) leaves the first thread a lone element.
template <class T>
__global__ __launch_bounds__(256) void lockin_polar_crop_kernel(const cpx<T>* __restrict__ lock, int n0, int n1, int edge,
                                                               int m0, int m1, int vec_ok, T* __restrict__ psi,
                                                               T* __restrict__ amp,
                                                               typename MaxBits<T>::type* __restrict__ amax) {
  const int p = blockIdx.z;
  T best = (T)0;
  for (int i = blockIdx.y; i < m0; i += gridDim.y) {
    const size_t src = ((size_t)p * n0 + edge + i) * n1 + edge;   // first element of the window's row
    const size_t dst = ((size_t)p * m0 + i) * m1;
    if constexpr (sizeof(T) == 4) {
      const int lead = vec_ok ? (int)(src & 1) : 0;
      for (int t = blockIdx.x * 256 + threadIdx.x; 2 * t - lead < m1; t += gridDim.x * 256) {
        const int j = 2 * t - lead;   // -1 for the first thread of a row with an odd start
        const bool ha = j >= 0, hb = j + 1 < m1;
        if (vec_ok && ha && hb) {
          struct alignas(16) Two { cpx<T> a, b; };
          const Two v = *reinterpret_cast<const Two*>(lock + src + j);
          polar_store(v.a, dst + j, psi, amp, best);
          polar_store(v.b, dst + j + 1, psi, amp, best);
        } else {
          if (ha) polar_store(lock[src + j], dst + j, psi, amp, best);
          if (hb) polar_store(lock[src + j + 1], dst + j + 1, psi, amp, best);
        }
      }
    } else {
      for (int j = blockIdx.x * 256 + threadIdx.x; j < m1; j += gridDim.x * 256)
        polar_store(lock[src + j], dst + j, psi, amp, best);
    }
  }
  __shared__ T sh[256];
  sh[threadIdx.x] = best;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) sh[threadIdx.x] = sh[threadIdx.x + s] > sh[threadIdx.x] ? sh[threadIdx.x + s] : sh[threadIdx.x];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    using U = typename MaxBits<T>::type;
    const T m = sh[0];
    U bits;
    __builtin_memcpy(&bits, &m, sizeof(U));
    atomicMax(amax + p, bits);
  }
}

// weight = sqrt(amp / amax[p]), the division first as in the reference (:141); grid: (chunks, P)
template <class T>
__global__ __launch_bounds__(256) void sqrt_norm_kernel(const T* __restrict__ amp, size_t npx, const T* __restrict__ amax,
                                                       T* __restrict__ weight) {
  const int p = blockIdx.y;
  const T top = amax[p];
  const T* a = amp + (size_t)p * npx;
  T* w = weight + (size_t)p * npx;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < npx; i += (size_t)gridDim.x * 256) w[i] = sqrt(a[i] / top);
}

hipError_t launch_polar_crop(int dtype, const void* lockins, int P, int n0, int n1, int edge, void* psi, void* amp,
                             void* amax, hipStream_t s) {
  const int m0 = n0 - 2 * edge, m1 = n1 - 2 * edge;
  if (P < 1 || P > 65535 || edge < 0 || m0 < 1 || m1 < 1) return hipErrorInvalidValue;
  const int per = dtype == 0 ? 512 : 256;   // columns a workgroup covers per step
  dim3 grid((unsigned)((m1 + 1 + per - 1) / per), (unsigned)(m0 < 1024 ? m0 : 1024), (unsigned)P);
  if (grid.x > 8) grid.x = 8;
  GPA_PROF("lockin_polar_crop_kernel", s);
  if (dtype == 0)
    lockin_polar_crop_kernel<float><<<grid, 256, 0, s>>>((const cpx<float>*)lockins, n0, n1, edge, m0, m1,
                                                         ((uintptr_t)lockins & 15) == 0 ? 1 : 0, (float*)psi, (float*)amp,
                                                         (unsigned int*)amax);
  else
    lockin_polar_crop_kernel<double><<<grid, 256, 0, s>>>((const cpx<double>*)lockins, n0, n1, edge, m0, m1, 1, (double*)psi,
                                                          (double*)amp, (unsigned long long*)amax);
  return hipGetLastError();
}

hipError_t launch_sqrt_norm(int dtype, const void* amp, int P, size_t npx, const void* amax, void* weight, hipStream_t s) {
  if (P < 1 || P > 65535) return hipErrorInvalidValue;
  const size_t chunks = (npx + 255) / 256;
  dim3 grid((unsigned)(chunks < 4096 ? chunks : 4096), (unsigned)P);
  GPA_PROF("sqrt_norm_kernel", s);
  if (dtype == 0) sqrt_norm_kernel<float><<<grid, 256, 0, s>>>((const float*)amp, npx, (const float*)amax, (float*)weight);
  else sqrt_norm_kernel<double><<<grid, 256, 0, s>>>((const double*)amp, npx, (const double*)amax, (double*)weight);
  return hipGetLastError();
}

// ---- Huber moments of P planes per launch ----------------------------------------------------------------------------------
// The arithmetic, the workgroup geometry and the order of every sum are those of huber_moments_kernel / huber_final_kernel
// (gpa_reconstruct.hip), so a plane's ten sums are the bits the single-plane launch gives.  blockIdx.y is the plane; state:
// 4 doubles per plane -- the coefficient triple and a flag, 0 for a plane whose fit has converged (its workgroups return, its
// sums are not written); work: huber_batch_stride() doubles of partial sums per plane; sums: the ten sums of every plane.
template <class T>
__global__ __launch_bounds__(256) void huber_moments_batch_kernel(const T* __restrict__ imgs, int n0, int n1,
                                                                 const double* __restrict__ state, double cx, double cy,
                                                                 double isx, double isy, double* __restrict__ work,
                                                                 size_t stride) {
  const int plane = blockIdx.y;
  if (state[4 * plane + 3] == 0.0) return;
  const double a0 = state[4 * plane], a1 = state[4 * plane + 1], a2 = state[4 * plane + 2];
  const T* img = imgs + (size_t)plane * n0 * n1;
  double* part = work + (size_t)plane * stride;
  double acc[10];
#pragma unroll
  for (int k = 0; k < 10; ++k) acc[k] = 0.0;
  for (int x = blockIdx.x; x < n0; x += gridDim.x) {
    const double u = (x - cx) * isx, pu = a0 * u + a2;
    const T* row = img + (size_t)x * n1;
    double su = 0.0, sw = 0.0, suz = 0.0;
    for (int y = threadIdx.x; y < n1; y += 256) {
      const double v = (y - cy) * isy, z = (double)row[y];
      const double r = z - (a1 * v + pu), ar = fabs(r);
      const double w = ar <= 1.0 ? 1.0 : 1.0 / ar;
      sw += w; su += w * v; suz += w * z;
      acc[3] += w * v * v; acc[7] += w * v * z;
      acc[9] += ar <= 1.0 ? 0.5 * r * r : ar - 0.5;
    }
    acc[0] += sw * u * u; acc[1] += su * u; acc[2] += sw * u; acc[4] += su; acc[5] += sw;
    acc[6] += suz * u; acc[8] += suz;
  }
  __shared__ double sh[256];
  for (int k = 0; k < 10; ++k) {
    sh[threadIdx.x] = acc[k];
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if (threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
      __syncthreads();
    }
    if (threadIdx.x == 0) part[(size_t)k * gridDim.x + blockIdx.x] = sh[0];
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void huber_final_batch_kernel(const double* __restrict__ state, int nparts,
                                                               const double* __restrict__ work, size_t stride,
                                                               double* __restrict__ sums) {
  const int plane = blockIdx.x;
  if (state[4 * plane + 3] == 0.0) return;
  const double* part = work + (size_t)plane * stride;
  double* out = sums + (size_t)10 * plane;
  __shared__ double sh[256];
  for (int k = 0; k < 10; ++k) {
    double a = 0.0;
    for (int i = threadIdx.x; i < nparts; i += 256) a += part[(size_t)k * nparts + i];
    sh[threadIdx.x] = a;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if (threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
      __syncthreads();
    }
    if (threadIdx.x == 0) out[k] = sh[0];
    __syncthreads();
  }
}

size_t huber_batch_stride() { return (size_t)huber_sums_offset(); }

hipError_t launch_huber_moments_batch(int dtype, const void* imgs, int P, int n0, int n1, const double* state, double cx,
                                      double cy, double sx, double sy, double* work, double* sums, hipStream_t s) {
  if (P < 1 || P > 65535) return hipErrorInvalidValue;
  const int parts = huber_sums_offset() / 10;
  const int nparts = n0 < parts ? n0 : parts;
  const size_t stride = huber_batch_stride();
  dim3 grid((unsigned)nparts, (unsigned)P);
  GPA_PROF("huber_moments_batch_kernels", s);
  if (dtype == 0)
    huber_moments_batch_kernel<float><<<grid, 256, 0, s>>>((const float*)imgs, n0, n1, state, cx, cy, 1.0 / sx, 1.0 / sy, work,
                                                           stride);
  else
    huber_moments_batch_kernel<double><<<grid, 256, 0, s>>>((const double*)imgs, n0, n1, state, cx, cy, 1.0 / sx, 1.0 / sy,
                                                            work, stride);
  huber_final_batch_kernel<<<P, 256, 0, s>>>(state, nparts, work, stride, sums);
  return hipGetLastError();
}

}  // namespace gpa
