// Windowed Fourier filtering (geometric_phase_analysis.py:551-580) in its separable shared-sum form:
//
//   g_t = scale * sum_wx Cx[kx] ( sum_wy Cy[ky] ( T_t ( Cy[ky] ( Cx[kx] f ) ) ) )
//
// Cx / Cy: 1-D 'reflect' convolutions along axis 1 / axis 0 with the 2 s taps kx(j) = g(j) e^(i wx j), ky(j) = g(j) e^(i wy j)
// / nrm; T_t keeps the samples with |sf| >= threshold_t.  Per wx: wff_rows_kernel makes A = Cx[kx] f, wff_cols_kernel runs
// every wy on a tile of A held in LDS and leaves the T planes B_t = sum_wy ..., wff_rows_acc_kernel adds Cx[kx] B_t to g_t.
// The taps come from the host (f64, rounded once to the plan's precision), stored REVERSED: tab[t] = k(s - 1 - t), so that
// out[i] = sum_t in[i - s + 1 + t] tab[t].  Every product-sum is written with fma(): the template instantiations (T = 1, 2,
// 4, 8 threshold slots) round alike, and a call with two thresholds gives the bits of two calls with one.
#include "gpa_internal.h"
#include "gpa_wff.h"

namespace gpa {

template <class T> struct WffC;
template <> struct WffC<float> { using type = float2; };
template <> struct WffC<double> { using type = double2; };

// acc += x * k (complex), four fused operations in a fixed order
template <class T, class C>
__device__ __forceinline__ void wff_mac(C& acc, const C& x, const C& k) {
  acc.x = fma(x.x, k.x, acc.x);
  acc.x = fma(-x.y, k.y, acc.x);
  acc.y = fma(x.x, k.y, acc.y);
  acc.y = fma(x.y, k.x, acc.y);
}

// one output of a row convolution: the workgroup stages its WFF_ROWS_TILE + 2 s - 1 folded samples of the row in `e`
template <class T, class C>
__device__ __forceinline__ C wff_row_conv(const C* __restrict__ row, int n1, int c0, int s, const C* __restrict__ tab, C* e) {
  const int W = 2 * s, ne = WFF_ROWS_TILE + W - 1;
  for (int v = threadIdx.x; v < ne; v += WFF_ROWS_TILE) e[v] = row[wff_fold32(c0 - s + 1 + v, n1)];
  __syncthreads();
  C acc{T(0), T(0)};
  const C* w = e + threadIdx.x;
  for (int t = 0; t < W; ++t) wff_mac<T>(acc, w[t], tab[t]);
  return acc;
}

// A = Cx[kx] f: grid.x = n0 * ceil(n1 / WFF_ROWS_TILE)
template <class T>
__global__ __launch_bounds__(WFF_ROWS_TILE) void wff_rows_kernel(const typename WffC<T>::type* __restrict__ in, int n0, int n1,
                                                                 int s, const typename WffC<T>::type* __restrict__ tab,
                                                                 typename WffC<T>::type* __restrict__ out) {
  using C = typename WffC<T>::type;
  __shared__ C e[WFF_ROWS_TILE + 2 * WFF_MAX_S];
  const int nseg = (n1 + WFF_ROWS_TILE - 1) / WFF_ROWS_TILE;
  const int r = blockIdx.x / nseg, c0 = (blockIdx.x % nseg) * WFF_ROWS_TILE;
  const C v = wff_row_conv<T, C>(in + (size_t)r * n1, n1, c0, s, tab, e);
  const int c = c0 + threadIdx.x;
  if (c < n1) out[(size_t)r * n1 + c] = v;
}

// g_t (+)= scale * Cx[kx] B_t for the planes t = blockIdx.y; the first wx writes, the later ones add
template <class T>
__global__ __launch_bounds__(WFF_ROWS_TILE) void wff_rows_acc_kernel(const typename WffC<T>::type* __restrict__ B, int n0, int n1,
                                                                     int s, const typename WffC<T>::type* __restrict__ tab,
                                                                     T scale, int first, typename WffC<T>::type* __restrict__ g) {
  using C = typename WffC<T>::type;
  __shared__ C e[WFF_ROWS_TILE + 2 * WFF_MAX_S];
  const int nseg = (n1 + WFF_ROWS_TILE - 1) / WFF_ROWS_TILE;
  const int r = blockIdx.x / nseg, c0 = (blockIdx.x % nseg) * WFF_ROWS_TILE;
  const size_t plane = (size_t)blockIdx.y * n0 * n1;
  const C v = wff_row_conv<T, C>(B + plane + (size_t)r * n1, n1, c0, s, tab, e);
  const int c = c0 + threadIdx.x;
  if (c >= n1) return;
  C* o = g + plane + (size_t)r * n1 + c;
  C prev{T(0), T(0)};
  if (!first) prev = *o;
  prev.x = fma(scale, v.x, prev.x);
  prev.y = fma(scale, v.y, prev.y);
  *o = prev;
}

// B_t = sum_wy Cy[ky] ( T_t ( Cy[ky] A ) ) on a tile of `cols` columns x R rows (gpa_wff.h: wff_tile).  Lanes run along a row,
// a thread owns P consecutive rows of one column.  LDS: a[rows_a][cols], the rows h0 - s + 1 ... of A folded at the image ends
// (h0: the first sf row the tile needs, wff_hull), sf[rows_sf][cols], and map[u] = the sf row behind window position u of the
// second convolution (the identity away from the image ends).  Per wy: every P-row block of sf from a (the blocks go round the
// row groups), barrier, then the second convolution over the thresholded sf into the sums a thread keeps in registers, barrier.
template <class T, int TT>
__global__ __launch_bounds__(WFF_THREADS_MAX) void wff_cols_kernel(const typename WffC<T>::type* __restrict__ A, int n0, int n1, int s,
                                                                   int R, int rows_a, int rows_sf, int nmap,
                                                                   const typename WffC<T>::type* __restrict__ tyr, int Ky,
                                                                   const T* __restrict__ thr2, int Tn,
                                                                   typename WffC<T>::type* __restrict__ B) {
  using C = typename WffC<T>::type;
  constexpr int P = wff_block(sizeof(T) == 8);
  constexpr int COLS = WFF_ROW_BYTES / (int)sizeof(C);
  extern __shared__ __attribute__((aligned(16))) unsigned char wff_smem[];
  C* a = reinterpret_cast<C*>(wff_smem);
  C* sf = a + (size_t)rows_a * COLS;
  int* map = reinterpret_cast<int*>(sf + (size_t)rows_sf * COLS);
  int& sh_h0 = map[nmap];   // (the 16 bytes behind the map: wff_lds_bytes)

  const int tid = threadIdx.x, nthr = blockDim.x;
  const int c = tid % COLS, g = tid / COLS, G = R / P;
  const int c0 = blockIdx.x * COLS, r0 = blockIdx.y * R;
  const int W = 2 * s, wpad = wff_round_up(W, P), nwin = R + W - 1, w0 = r0 - s + 1;

  if (tid == 0) sh_h0 = n0;
  __syncthreads();
  for (int u = tid; u < nwin; u += nthr) atomicMin(&sh_h0, wff_fold32(w0 + u, n0));
  __syncthreads();
  const int h0 = sh_h0;
  for (int u = tid; u < nmap; u += nthr) map[u] = u < nwin ? wff_fold32(w0 + u, n0) - h0 : 0;
  {
    const int gc = min(c0 + c, n1 - 1);   // a ragged last tile repeats the last column; its results are not stored
    for (int v = g; v < rows_a; v += G) a[v * COLS + c] = A[(size_t)wff_fold32(h0 - s + 1 + v, n0) * n1 + gc];
  }
  __syncthreads();

  T thr[TT];
#pragma unroll
  for (int t = 0; t < TT; ++t) thr[t] = thr2[t];
  C acc[TT][P];
#pragma unroll
  for (int t = 0; t < TT; ++t)
#pragma unroll
    for (int p = 0; p < P; ++p) acc[t][p] = C{T(0), T(0)};

  const int nblk = rows_sf / P;
  for (int iy = 0; iy < Ky; ++iy) {
    const C* __restrict__ tab = tyr + (size_t)iy * wpad;
    // sf = Cy[ky] A, P rows at a time: a sample read from LDS serves up to P taps
    for (int b = g; b < nblk; b += G) {
      const C* col = a + (size_t)(b * P) * COLS + c;
      C w[P], nx[P], r[P];
#pragma unroll
      for (int p = 0; p < P; ++p) { w[p] = col[p * COLS]; r[p] = C{T(0), T(0)}; }
      for (int t0 = 0; t0 < wpad; t0 += P) {
#pragma unroll
        for (int p = 0; p < P; ++p) nx[p] = col[(t0 + P + p) * COLS];
#pragma unroll
        for (int tt = 0; tt < P; ++tt) {
          if (t0 + tt < W) {
            const C k = tab[t0 + tt];
#pragma unroll
            for (int p = 0; p < P; ++p) wff_mac<T>(r[p], tt + p < P ? w[(tt + p) % P] : nx[(tt + p) % P], k);
          }
        }
#pragma unroll
        for (int p = 0; p < P; ++p) w[p] = nx[p];
      }
#pragma unroll
      for (int p = 0; p < P; ++p) sf[(b * P + p) * COLS + c] = r[p];
    }
    __syncthreads();
    // B_t += Cy[ky] T_t(sf) for the thread's P output rows; |sf|^2 is formed once per sample, the masks per threshold
    {
      const int* mp = map + g * P;
      C w[P], nx[P];
      T mw[P], mn[P];
#pragma unroll
      for (int p = 0; p < P; ++p) {
        w[p] = sf[mp[p] * COLS + c];
        mw[p] = fma(w[p].x, w[p].x, w[p].y * w[p].y);
      }
      for (int t0 = 0; t0 < wpad; t0 += P) {
#pragma unroll
        for (int p = 0; p < P; ++p) {
          nx[p] = sf[mp[t0 + P + p] * COLS + c];
          mn[p] = fma(nx[p].x, nx[p].x, nx[p].y * nx[p].y);
        }
#pragma unroll
        for (int t = 0; t < TT; ++t) {
          C wm[P], nm[P];
#pragma unroll
          for (int p = 0; p < P; ++p) {
            const bool kw = mw[p] >= thr[t], kn = mn[p] >= thr[t];
            wm[p] = C{kw ? w[p].x : T(0), kw ? w[p].y : T(0)};
            nm[p] = C{kn ? nx[p].x : T(0), kn ? nx[p].y : T(0)};
          }
#pragma unroll
          for (int tt = 0; tt < P; ++tt) {
            if (t0 + tt < W) {
              const C k = tab[t0 + tt];
#pragma unroll
              for (int p = 0; p < P; ++p) wff_mac<T>(acc[t][p], tt + p < P ? wm[(tt + p) % P] : nm[(tt + p) % P], k);
            }
          }
        }
#pragma unroll
        for (int p = 0; p < P; ++p) { w[p] = nx[p]; mw[p] = mn[p]; }
      }
    }
    __syncthreads();
  }

  const int col_g = c0 + c;
  if (col_g >= n1) return;
#pragma unroll
  for (int t = 0; t < TT; ++t) {
    if (t >= Tn) break;
#pragma unroll
    for (int p = 0; p < P; ++p) {
      const int row = r0 + g * P + p;
      if (row < n0) B[((size_t)t * n0 + row) * n1 + col_g] = acc[t][p];
    }
  }
}

template <class T, int TT>
static hipError_t launch_cols(const void* A, int n0, int n1, int s, const WffTile& tl, const void* tyr, int Ky, const void* thr2, int nT,
                              void* B, hipStream_t st) {
  using C = typename WffC<T>::type;
  static unsigned lds_done = 0;
  hipError_t e = set_dynamic_lds_once(reinterpret_cast<const void*>(&wff_cols_kernel<T, TT>), WFF_LDS_BUDGET, lds_done);
  if (e != hipSuccess) return e;
  const dim3 grid((n1 + tl.cols - 1) / tl.cols, (n0 + tl.R - 1) / tl.R);
  GPA_PROF("wff_cols_kernel", st);
  wff_cols_kernel<T, TT><<<grid, tl.threads, tl.lds_bytes, st>>>(static_cast<const C*>(A), n0, n1, s, tl.R, tl.rows_a, tl.rows_sf, tl.nmap,
                                                                  static_cast<const C*>(tyr), Ky, static_cast<const T*>(thr2), nT,
                                                                  static_cast<C*>(B));
  return hipGetLastError();
}

template <class T>
static hipError_t wff_run_t(const void* img, int n0, int n1, int s, const void* txr, int Kx, const void* tyr, int Ky, const void* thr2,
                            int nT, double scale, void* A, void* B, void* out, hipStream_t st) {
  using C = typename WffC<T>::type;
  const WffTile tl = wff_tile(s, nT, sizeof(T) == 8);
  if (!tl.ok) return hipErrorInvalidValue;
  const int W = 2 * s, nseg = (n1 + WFF_ROWS_TILE - 1) / WFF_ROWS_TILE;
  const unsigned nrow_blocks = (unsigned)n0 * (unsigned)nseg;
  for (int ix = 0; ix < Kx; ++ix) {
    const C* tab = static_cast<const C*>(txr) + (size_t)ix * W;
    {
      GPA_PROF("wff_rows_kernel", st);
      wff_rows_kernel<T><<<nrow_blocks, WFF_ROWS_TILE, 0, st>>>(static_cast<const C*>(img), n0, n1, s, tab, static_cast<C*>(A));
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    switch (wff_tslots(nT)) {
      case 1: e = launch_cols<T, 1>(A, n0, n1, s, tl, tyr, Ky, thr2, nT, B, st); break;
      case 2: e = launch_cols<T, 2>(A, n0, n1, s, tl, tyr, Ky, thr2, nT, B, st); break;
      case 4: e = launch_cols<T, 4>(A, n0, n1, s, tl, tyr, Ky, thr2, nT, B, st); break;
      default: e = launch_cols<T, 8>(A, n0, n1, s, tl, tyr, Ky, thr2, nT, B, st); break;
    }
    if (e != hipSuccess) return e;
    {
      GPA_PROF("wff_rows_acc_kernel", st);
      wff_rows_acc_kernel<T><<<dim3(nrow_blocks, nT), WFF_ROWS_TILE, 0, st>>>(static_cast<const C*>(B), n0, n1, s, tab, (T)scale,
                                                                             ix == 0 ? 1 : 0, static_cast<C*>(out));
    }
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t wff_run(int dtype, const void* d_img, int n0, int n1, int s, const void* d_txr, int Kx, const void* d_tyr, int Ky,
                   const void* d_thr2, int T, double scale, void* d_A, void* d_B, void* d_out, hipStream_t st) {
  return dtype == 0 ? wff_run_t<float>(d_img, n0, n1, s, d_txr, Kx, d_tyr, Ky, d_thr2, T, scale, d_A, d_B, d_out, st)
                    : wff_run_t<double>(d_img, n0, n1, s, d_txr, Kx, d_tyr, Ky, d_thr2, T, scale, d_A, d_B, d_out, st);
}

}  // namespace gpa
