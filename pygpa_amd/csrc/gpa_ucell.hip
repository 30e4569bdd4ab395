// Unit-cell averaging and expansion -- unit_cell_average / expand_unitcell (unit_cell_averaging.py:132-217, :236-251).
//
// Average.  A pixel r = (i, j) lands at R = z (cart_in_uc(r + u(r)) - rmin) in the upscaled cell and adds value * w and w
// to the 2 x 2 bins at floor(R) + {0,1}^2, w the overlap of float_overlap; the cell is res / weights.  The reference adds
// pixel by pixel; here the scatter is a store-and-sum (no float atomics, the same bits on every run):
//   key pass   the BASE bin floor(R) of every pixel as an int32 key on the (rs0 + 1) x (rs1 + 1) grid of base bins -1 ...
//              rs - 1 (a NaN u or a base outside that range: the sentinel key, dropped)
//   sort       a stable LSD radix sort of (key, pixel index), 4 bits a pass: every base bin's list holds its pixels in
//              raster order -- the reference's own order -- whatever the hardware's scheduling
//   lists      the first position of every key in the sorted array; the two fractions R - floor(R) per list entry
//   sum pass   one wavefront per base bin sums value * w and w for its four corners in f64 (lane-strided in list order, then
//              a fixed butterfly); NaN image pixels are skipped here, so the lists serve any number of frames
//   finish     every bin adds the corner sums of the (up to 3 x 3 with wrap-around) base bins that reach it, in a fixed
//              order, and writes res / weights (NaN where nothing landed: 0 / 0) and the weights.
// Edges, as the reference indexes: a base bin of -1 (R rounding below 0) puts its lower corner in the LAST row / column
// (NumPy's negative index); a corner at index rs is dropped (NumPy raises IndexError there, numba writes out of bounds).
//
// Expand.  out(r) = map_coordinates(nan_to_num(cell), z cart_in_uc(r / z2 + u(r))), order 3, mode 'constant', cval 0:
// the prefilter and the tap sums of gpa_warp.hip / gpa_spline.h, in f64 on the f64 cell in both builds.
//
// Coordinates are computed in f64 in both builds and without contraction (build.py compiles this file with
// -ffp-contract=off): the dot products as the reference writes them, a * b + c * d, `% 1` as NumPy's remainder.
#include <math.h>
#include <float.h>

#include "gpa_internal.h"
#include "gpa_spline.h"

namespace gpa {

namespace {

constexpr int RBITS = 4, RADIX = 1 << RBITS;             // radix sort: 4 bits a pass
constexpr int SORT_T = 256, SORT_ITEMS = 16;             // a thread ranks 16 CONSECUTIVE items
constexpr int SORT_TILE = SORT_T * SORT_ITEMS;
constexpr int SCAN_TILE = 256 * 16;

// NumPy's remainder(x, 1) -- fmod, then + 1 for a negative result (a tiny negative x gives exactly 1.0), +0 for 0 -- as
// x - floor(x): fmod(x, 1) = x - trunc(x) is exact, so both forms round the same real number once (and the subtraction
// is a few instructions where the f64 fmod is a loop).  NaN stays NaN.
__device__ __forceinline__ double mod1(double x) {
  const double m = x - floor(x);
  return m == 0.0 ? 0.0 : m;
}

// cart_in_uc(v, ks, rmin): ((v @ ks.T) % 1) @ inv(ks).T - rmin
__device__ __forceinline__ void cell_coords(const UcellGeom& g, double v0, double v1, double& c0, double& c1) {
  const double a0 = mod1(v0 * g.ks[0] + v1 * g.ks[1]);
  const double a1 = mod1(v0 * g.ks[2] + v1 * g.ks[3]);
  c0 = (a0 * g.kinv[0] + a1 * g.kinv[1]) - g.rmin[0];
  c1 = (a0 * g.kinv[2] + a1 * g.kinv[3]) - g.rmin[1];
}

// base-bin key of pixel p (and the fractions of R): base bins -1 ... rs - 1 per axis, shifted by one; else the sentinel
template <class T>
__device__ __forceinline__ int pixel_key(const UcellGeom& g, const T* __restrict__ u, size_t npx, int n1, size_t p, double& f0,
                                         double& f1) {
  const int i = (int)(p / (size_t)n1), j = (int)(p - (size_t)i * n1);
  double v0 = (double)i, v1 = (double)j;
  if (u) {
    v0 = v0 + (double)u[p];
    v1 = v1 + (double)u[npx + p];
  }
  double c0, c1;
  cell_coords(g, v0, v1, c0, c1);
  const double R0 = c0 * g.z, R1 = c1 * g.z;
  const double b0 = floor(R0), b1 = floor(R1);
  f0 = R0 - b0;
  f1 = R1 - b1;
  if (!(b0 >= -1.0 && b0 <= (double)(g.rs0 - 1) && b1 >= -1.0 && b1 <= (double)(g.rs1 - 1)))   // (NaN: false)
    return (g.rs0 + 1) * (g.rs1 + 1);
  return ((int)b0 + 1) * (g.rs1 + 1) + ((int)b1 + 1);
}

template <class T>
__global__ __launch_bounds__(256) void ucell_key_kernel(const T* __restrict__ u, int n0, int n1, UcellGeom g, int* __restrict__ keys) {
  const size_t npx = (size_t)n0 * n1, p = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= npx) return;
  double f0, f1;
  keys[p] = pixel_key<T>(g, u, npx, n1, p, f0, f1);
}

// ---- stable LSD radix sort of (key, index) -------------------------------------------------------------------------
// per block of SORT_TILE items: how many carry each digit -> hist[digit * nblk + block] (digit-major: the exclusive scan of
// hist is every (digit, block)'s first output position)
__global__ __launch_bounds__(256) void radix_hist_kernel(const int* __restrict__ kin, size_t n, int shift, int nblk,
                                                         int* __restrict__ hist) {
  __shared__ int cnt[RADIX * SORT_T];
  const int t = threadIdx.x;
#pragma unroll
  for (int d = 0; d < RADIX; ++d) cnt[d * SORT_T + t] = 0;
  const size_t q0 = (size_t)blockIdx.x * SORT_TILE + (size_t)t * SORT_ITEMS;
  for (int k = 0; k < SORT_ITEMS; ++k)
    if (q0 + k < n) ++cnt[((kin[q0 + k] >> shift) & (RADIX - 1)) * SORT_T + t];
  __syncthreads();
  // digit d = t / 16 summed by 16 lanes, 16 columns each
  const int d = t >> 4, part = t & 15;
  int s = 0;
#pragma unroll
  for (int x = 0; x < 16; ++x) s += cnt[d * SORT_T + part * 16 + x];
#pragma unroll
  for (int m = 8; m > 0; m >>= 1) s += __shfl_xor(s, m);
  if (part == 0) hist[(size_t)d * nblk + blockIdx.x] = s;
}

// exclusive scan of SORT_T partial counts held one per thread (Hillis-Steele in LDS); returns the thread's offset
__device__ __forceinline__ int block_exclusive(int s, int* ts) {
  const int t = threadIdx.x;
  ts[t] = s;
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) {
    const int a = t >= off ? ts[t - off] : 0;
    __syncthreads();
    ts[t] += a;
    __syncthreads();
  }
  const int r = ts[t] - s;
  __syncthreads();
  return r;
}

// exclusive scan of SCAN_TILE ints per block; the tile's total to sums[block] (sums may be null)
__global__ __launch_bounds__(256) void scan_tile_kernel(const int* in, int* out, size_t n, int* sums) {
  __shared__ int ts[256];
  const size_t q0 = (size_t)blockIdx.x * SCAN_TILE + (size_t)threadIdx.x * 16;
  int v[16], s = 0;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int x = q0 + k < n ? in[q0 + k] : 0;
    v[k] = s;
    s += x;
  }
  const int excl = block_exclusive(s, ts);
#pragma unroll
  for (int k = 0; k < 16; ++k)
    if (q0 + k < n) out[q0 + k] = v[k] + excl;
  if (threadIdx.x == 255 && sums) sums[blockIdx.x] = excl + s;
}

__global__ __launch_bounds__(256) void scan_add_kernel(int* out, size_t n, const int* __restrict__ ofs) {
  const size_t q0 = (size_t)blockIdx.x * SCAN_TILE + (size_t)threadIdx.x * 16;
  const int a = ofs[blockIdx.x];
#pragma unroll
  for (int k = 0; k < 16; ++k)
    if (q0 + k < n) out[q0 + k] += a;
}

// one pass: every item to its stable position by digit.  iin == null: the first pass, the index is the position itself
__global__ __launch_bounds__(256) void radix_scatter_kernel(const int* __restrict__ kin, const int* __restrict__ iin, size_t n,
                                                            int shift, int nblk, const int* __restrict__ gofs,
                                                            int* __restrict__ kout, int* __restrict__ iout) {
  __shared__ int cnt[RADIX * SORT_T];   // [digit][thread]: items of this digit in the thread's run, then their positions
  __shared__ int ts[256];
  __shared__ int first[RADIX], gbase[RADIX];
  const int t = threadIdx.x;
#pragma unroll
  for (int d = 0; d < RADIX; ++d) cnt[d * SORT_T + t] = 0;
  if (t < RADIX) gbase[t] = gofs[(size_t)t * nblk + blockIdx.x];
  const size_t q0 = (size_t)blockIdx.x * SORT_TILE + (size_t)t * SORT_ITEMS;
  int kk[SORT_ITEMS], ii[SORT_ITEMS];
#pragma unroll
  for (int k = 0; k < SORT_ITEMS; ++k) {
    const size_t q = q0 + k;
    kk[k] = q < n ? kin[q] : 0;
    ii[k] = q < n ? (iin ? iin[q] : (int)q) : 0;
  }
#pragma unroll
  for (int k = 0; k < SORT_ITEMS; ++k)
    if (q0 + k < n) ++cnt[((kk[k] >> shift) & (RADIX - 1)) * SORT_T + t];
  __syncthreads();
  // exclusive scan of cnt in its flat (digit-major) order: thread t owns the 16 entries from 16 t
  int v[16], s = 0;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int x = cnt[16 * t + k];
    v[k] = s;
    s += x;
  }
  const int excl = block_exclusive(s, ts);
#pragma unroll
  for (int k = 0; k < 16; ++k) cnt[16 * t + k] = v[k] + excl;
  __syncthreads();
  if (t < RADIX) first[t] = cnt[t * SORT_T];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < SORT_ITEMS; ++k) {
    if (q0 + k >= n) continue;
    const int d = (kk[k] >> shift) & (RADIX - 1);
    const int pos = gbase[d] + cnt[d * SORT_T + t] - first[d];
    ++cnt[d * SORT_T + t];
    kout[pos] = kk[k];
    iout[pos] = ii[k];
  }
}

// start[k] = first position of key k in the sorted keys (k = 0 ... nkeys; keys run up to the sentinel nkeys)
__global__ __launch_bounds__(256) void list_start_kernel(const int* __restrict__ keys, size_t n, int nkeys, int* __restrict__ start) {
  const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  const int k = keys[p], kp = p ? keys[p - 1] : -1;
  for (int x = kp + 1; x <= k; ++x) start[x] = (int)p;
  if (p == n - 1)
    for (int x = k + 1; x <= nkeys; ++x) start[x] = (int)n;
}

// the fractions of every listed pixel, in list order
template <class T>
__global__ __launch_bounds__(256) void ucell_frac_kernel(const int* __restrict__ idx, const int* __restrict__ start, int nkeys,
                                                         const T* __restrict__ u, int n0, int n1, UcellGeom g,
                                                         double* __restrict__ F0, double* __restrict__ F1) {
  const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= (size_t)start[nkeys]) return;
  double f0, f1;
  (void)pixel_key<T>(g, u, (size_t)n0 * n1, n1, (size_t)idx[p], f0, f1);
  F0[p] = f0;
  F1[p] = f1;
}

// one wavefront per base bin (blockIdx.y: frame): sum value * w and w of its four corners over its list, NaN pixels
// skipped; corner c = 2 li + lj.  part: B x nkeys x 8 doubles (4 value sums, 4 weight sums)
template <class T>
__global__ __launch_bounds__(256) void ucell_sum_kernel(const T* __restrict__ images, size_t npx, const int* __restrict__ idx,
                                                        const int* __restrict__ start, int nkeys, const double* __restrict__ F0,
                                                        const double* __restrict__ F1, double* __restrict__ part) {
  const int lane = threadIdx.x & 63, key = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (key >= nkeys) return;
  const T* img = images + (size_t)blockIdx.y * npx;
  const int s = start[key], e = start[key + 1];
  double a[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) a[c] = 0.0;
  for (int p = s + lane; p < e; p += 64) {
    const double v = (double)img[idx[p]];
    if (isnan(v)) continue;
    const double f0 = F0[p], f1 = F1[p];
    const double w0[2] = {1.0 - f0, f0}, w1[2] = {1.0 - f1, f1};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      // float_overlap's layout: the ROW offset li takes the weight of the second fraction, the column offset lj the first
      const double w = w0[c & 1] * w1[c >> 1];
      a[c] += v * w;
      a[4 + c] += w;
    }
  }
#pragma unroll
  for (int m = 32; m > 0; m >>= 1)
#pragma unroll
    for (int c = 0; c < 8; ++c) a[c] += __shfl_xor(a[c], m);
  if (lane < 8) {
    double r = a[0];
#pragma unroll
    for (int c = 1; c < 8; ++c) r = lane == c ? a[c] : r;
    part[((size_t)blockIdx.y * nkeys + key) * 8 + lane] = r;
  }
}

// every bin of the cell (blockIdx.y: frame): the corner sums of the base bins reaching it, in a fixed order
__global__ __launch_bounds__(256) void ucell_finish_kernel(const double* __restrict__ part, int nkeys, int rs0, int rs1,
                                                           double* __restrict__ res, double* __restrict__ weights) {
  const size_t ncell = (size_t)rs0 * rs1, q = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= ncell) return;
  const int a = (int)(q / rs1), b = (int)(q - (size_t)a * rs1), E1 = rs1 + 1;
  // (base row + 1, corner) pairs that land on row a: base a with corner 0, base a - 1 with corner 1, and for the last row
  // base -1 with corner 0 (index -1 wraps)
  int er[3] = {a + 1, a, 0}, cr[3] = {0, 1, 0}, ec[3] = {b + 1, b, 0}, cc[3] = {0, 1, 0};
  const int nr = a == rs0 - 1 ? 3 : 2, nc = b == rs1 - 1 ? 3 : 2;
  const double* fp = part + (size_t)blockIdx.y * nkeys * 8;
  double R = 0.0, W = 0.0;
  for (int x = 0; x < nr; ++x)
    for (int y = 0; y < nc; ++y) {
      const double* src = fp + ((size_t)er[x] * E1 + ec[y]) * 8;
      const int c = 2 * cr[x] + cc[y];
      R += src[c];
      W += src[4 + c];
    }
  const size_t o = (size_t)blockIdx.y * ncell + q;
  res[o] = R / W;
  if (weights) weights[o] = W;
}

__global__ __launch_bounds__(256) void nan_to_num_kernel(const double* __restrict__ in, size_t n, double* __restrict__ out) {
  const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= n) return;
  const double v = in[q];
  out[q] = isnan(v) ? 0.0 : (isinf(v) ? (v > 0 ? DBL_MAX : -DBL_MAX) : v);
}

template <class T>
__global__ __launch_bounds__(256) void ucell_expand_kernel(const double* __restrict__ coef, UcellGeom g, double z2,
                                                           const T* __restrict__ u, int n0, int n1, T* __restrict__ out) {
  const size_t npx = (size_t)n0 * n1, p = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= npx) return;
  const int i = (int)(p / (size_t)n1), j = (int)(p - (size_t)i * n1);
  double v0 = (double)i / z2, v1 = (double)j / z2;
  if (u) {
    v0 = v0 + (double)u[p];
    v1 = v1 + (double)u[npx + p];
  }
  double c0, c1;
  cell_coords(g, v0, v1, c0, c1);
  const double* const cf[1] = {coef};
  double r[1];
  interp_constant<double, 1, false>(cf, g.rs0, g.rs1, c0 * g.z, c1 * g.z, 0.0, r);
  out[p] = (T)r[0];
}

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }


// exclusive scan of n ints (n <= SCAN_TILE^2); sums: ceil(n / SCAN_TILE) ints of scratch
hipError_t exclusive_scan(const int* in, int* out, size_t n, int* sums, hipStream_t s) {
  const int nb = (int)((n + SCAN_TILE - 1) / SCAN_TILE);
  {
    GPA_PROF("ucell_scan_tile_kernel", s);
    scan_tile_kernel<<<nb, 256, 0, s>>>(in, out, n, nb > 1 ? sums : nullptr);
  }
  if (nb > 1) {
    {
      GPA_PROF("ucell_scan_tile_kernel", s);
      scan_tile_kernel<<<1, 256, 0, s>>>(sums, sums, (size_t)nb, nullptr);
    }
    GPA_PROF("ucell_scan_add_kernel", s);
    scan_add_kernel<<<nb, 256, 0, s>>>(out, n, sums);
  }
  return hipGetLastError();
}

template <class T>
hipError_t average_t(const T* d_images, int B, const T* d_u, int n0, int n1, const UcellGeom& g, double* d_res, double* d_weights,
                     hipStream_t s, UcellWs* ws) {
  const size_t n = (size_t)n0 * n1;
  const int nkeys = (g.rs0 + 1) * (g.rs1 + 1);
  const int nblk = (int)((n + SORT_TILE - 1) / SORT_TILE);
  const size_t nhist = (size_t)RADIX * nblk;
  // scratch: keys and indices twice (the sort's ping-pong), histogram and its scan, list starts, fractions, corner sums
  const size_t b_int = align256(n * sizeof(int)), b_hist = align256(nhist * sizeof(int));
  const size_t b_sums = align256(((nhist + SCAN_TILE - 1) / SCAN_TILE) * sizeof(int));
  const size_t b_start = align256(((size_t)nkeys + 1) * sizeof(int)), b_frac = align256(n * sizeof(double));
  const size_t b_part = align256((size_t)B * nkeys * 8 * sizeof(double));
  hipError_t e = ws->buf.reserve(4 * b_int + 2 * b_hist + b_sums + b_start + 2 * b_frac + b_part, s);
  if (e != hipSuccess) return e;
  char* c = (char*)ws->buf.ptr;
  int* kA = (int*)c;
  int* kB = (int*)(c += b_int);
  int* iA = (int*)(c += b_int);
  int* iB = (int*)(c += b_int);
  int* hist = (int*)(c += b_int);
  int* hscan = (int*)(c += b_hist);
  int* sums = (int*)(c += b_hist);
  int* start = (int*)(c += b_sums);
  double* F0 = (double*)(c += b_start);     // (f64 in both builds: the overlaps are the reference's to the last bit)
  double* F1 = (double*)(c += b_frac);
  double* part = (double*)(c += b_frac);

  const unsigned gpx = (unsigned)((n + 255) / 256);
  {
    GPA_PROF("ucell_key_kernel", s);
    ucell_key_kernel<T><<<gpx, 256, 0, s>>>(d_u, n0, n1, g, kA);
  }
  int bits = 0;
  while ((nkeys >> bits) > 0) ++bits;        // keys run 0 ... nkeys (the sentinel)
  const int passes = (bits + RBITS - 1) / RBITS;
  const int* kin = kA;
  const int* iin = nullptr;
  int *kout = kB, *iout = iB;
  for (int ps = 0; ps < passes; ++ps) {
    {
      GPA_PROF("ucell_radix_hist_kernel", s);
      radix_hist_kernel<<<nblk, 256, 0, s>>>(kin, n, ps * RBITS, nblk, hist);
    }
    e = exclusive_scan(hist, hscan, nhist, sums, s);
    if (e != hipSuccess) return e;
    {
      GPA_PROF("ucell_radix_scatter_kernel", s);
      radix_scatter_kernel<<<nblk, 256, 0, s>>>(kin, iin, n, ps * RBITS, nblk, hscan, kout, iout);
    }
    kin = kout;
    iin = iout;
    kout = kout == kB ? kA : kB;
    iout = iout == iB ? iA : iB;
  }
  {
    GPA_PROF("ucell_list_start_kernel", s);
    list_start_kernel<<<gpx, 256, 0, s>>>(kin, n, nkeys, start);
  }
  {
    GPA_PROF("ucell_frac_kernel", s);
    ucell_frac_kernel<T><<<gpx, 256, 0, s>>>(iin, start, nkeys, d_u, n0, n1, g, F0, F1);
  }
  {
    GPA_PROF("ucell_sum_kernel", s);
    ucell_sum_kernel<T><<<dim3((nkeys + 3) / 4, B), 256, 0, s>>>(d_images, n, iin, start, nkeys, F0, F1, part);
  }
  {
    GPA_PROF("ucell_finish_kernel", s);
    const size_t ncell = (size_t)g.rs0 * g.rs1;
    ucell_finish_kernel<<<dim3((unsigned)((ncell + 255) / 256), B), 256, 0, s>>>(part, nkeys, g.rs0, g.rs1, d_res, d_weights);
  }
  return hipGetLastError();
}

template <class T>
hipError_t expand_t(const double* d_cell, const UcellGeom& g, double z2, const T* d_u, int n0, int n1, T* d_out, hipStream_t s,
                    UcellWs* ws) {
  const size_t ncell = (size_t)g.rs0 * g.rs1, b = align256(ncell * sizeof(double));
  hipError_t e = ws->buf.reserve(3 * b, s);
  if (e != hipSuccess) return e;
  double* clean = (double*)ws->buf.ptr;
  double* tmp = (double*)((char*)ws->buf.ptr + b);
  double* coef = (double*)((char*)ws->buf.ptr + 2 * b);
  {
    GPA_PROF("ucell_nan_to_num_kernel", s);
    nan_to_num_kernel<<<(unsigned)((ncell + 255) / 256), 256, 0, s>>>(d_cell, ncell, clean);
  }
  e = spline_coef_constant_f64(clean, g.rs0, g.rs1, tmp, coef, s, &ws->spline);
  if (e != hipSuccess) return e;
  {
    GPA_PROF("ucell_expand_kernel", s);
    const size_t npx = (size_t)n0 * n1;
    ucell_expand_kernel<T><<<(unsigned)((npx + 255) / 256), 256, 0, s>>>(coef, g, z2, d_u, n0, n1, d_out);
  }
  return hipGetLastError();
}

}  // namespace

hipError_t ucell_average(int dtype, const void* d_images, int B, const void* d_u, int n0, int n1, const UcellGeom& g,
                         double* d_res, double* d_weights, hipStream_t s, UcellWs* ws) {
  return dtype == 0 ? average_t<float>((const float*)d_images, B, (const float*)d_u, n0, n1, g, d_res, d_weights, s, ws)
                    : average_t<double>((const double*)d_images, B, (const double*)d_u, n0, n1, g, d_res, d_weights, s, ws);
}

hipError_t ucell_expand(int dtype, const double* d_cell, const UcellGeom& g, double z2, const void* d_u, int n0, int n1,
                        void* d_out, hipStream_t s, UcellWs* ws) {
  return dtype == 0 ? expand_t<float>(d_cell, g, z2, (const float*)d_u, n0, n1, (float*)d_out, s, ws)
                    : expand_t<double>(d_cell, g, z2, (const double*)d_u, n0, n1, (double*)d_out, s, ws);
}

}  // namespace gpa
