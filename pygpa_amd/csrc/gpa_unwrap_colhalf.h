// a7, the column solve of the unwrap's preconditioner for columns too long for a packed-pair transform (f64 columns of
// 16384 points: 256 KiB of LDS against 160): ONE column per complex transform of HALF the column length -- the column
// counterpart of the half-length row kernels, whose header (gpa_unwrap_rowhalf.hip) has the identities.
//
// With v the Makhoul-permuted column (gpa_dct.h) and t[n] = v[2n] + i v[2n+1], T = FFT_(N/2)(t):
//     Ve_k = (T_k + conj T_(N/2-k)) / 2,  Vo_k = -i (T_k - conj T_(N/2-k)) / 2,  V_k = Ve_k + E_k Vo_k,  E_k = e^(-2 pi i k / N)
//     U_k = w_k V_k,  X_k = 2 Re U_k,  X_(N-k) = -2 Im U_k  (0 < k < N/2),  X_0 = 2 (Re T_0 + Im T_0),  X_(N/2) = sqrt 2 (Re T_0 - Im T_0)
// is SciPy's unnormalised DCT-II (phase_unwrap.py:84-103); the bins are divided by the Laplacian eigenvalues
// (phase_unwrap.py:106-115) and the chain runs backwards into the DCT-III.  A thread owns the bins k = tid + TPF i and their
// partners N - k (bin 0's partner is bin N/2), so the tables are in NATURAL order over k = 0 .. N/2 - 1:
//     wspec[2k] = w_k = e^(-i pi k / 2N),  wspec[2k + 1] = E_k,   ha[k] = 1 - cos of bin k,   ham[k] = the same of bin N - k
//     (slot 0 of ham: bin N/2)
// The per-thread steps are GPA_HD, phase by phase, so that tests/host/colhalf_emulator.cpp runs them on the CPU.
#pragma once
#include <math.h>

#include <vector>

#include "gpa_dct.h"

namespace gpa {

// host: the tables above for a column of n0 points, in double (A0: the length the reference's eigenvalue table uses for
// this axis, n0 itself or -- its swapped-axis quirk -- n1; gpa_unwrap_tables.hip)
inline void colhalf_tables(int n0, double A0, std::vector<double>& wspec, std::vector<double>& ha, std::vector<double>& ham) {
  const int hn = n0 / 2;
  wspec.assign((size_t)4 * hn, 0.0);
  ha.assign((size_t)hn, 0.0);
  ham.assign((size_t)hn, 0.0);
  for (int k = 0; k < hn; ++k) {
    wspec[4 * (size_t)k] = cos(-M_PI * k / (2.0 * n0));
    wspec[4 * (size_t)k + 1] = sin(-M_PI * k / (2.0 * n0));
    wspec[4 * (size_t)k + 2] = cos(-2.0 * M_PI * k / n0);
    wspec[4 * (size_t)k + 3] = sin(-2.0 * M_PI * k / n0);
    const int km = k == 0 ? hn : n0 - k;
    const double sk = sin(M_PI * k / (2.0 * A0)), sm = sin(M_PI * km / (2.0 * A0));
    ha[k] = 2 * sk * sk;
    ham[k] = 2 * sm * sm;
  }
}

// keeps hipcc from hoisting the table and LDS reads of all 16 bins of a thread to the top of a phase (224 registers in f64)
#if defined(__HIP_DEVICE_COMPILE__)
#define GPA_COLHALF_FENCE(i) do { __builtin_amdgcn_sched_barrier(0); } while (0)
#else
#define GPA_COLHALF_FENCE(i) do { } while (0)
#endif

template <class T, int LG>
struct ColHalf {
  using F = WgFFT<T, LG - 1, 16>;
  static constexpr int N = 1 << LG, HN = N / 2, TPF = F::TPF, E = 16, THREADS = F::TPF;
  static constexpr size_t LDS_BYTES = (size_t)F::LDS_ELEMS * sizeof(cpx<T>);
  static constexpr bool FITS = LDS_BYTES + THREADS * sizeof(double) <= 160 * 1024;

  // rows of the column behind slot n of the half-length transform: (v[2n], v[2n + 1]) -- for n < N/4 rows 4n and 4n + 2,
  // else, with j = N/2 - 1 - n, rows 4j + 3 and 4j + 1
  GPA_HD static int row_re(int n) { return makhoul_src(2 * n, N); }
  GPA_HD static int row_im(int n) { return makhoul_src(2 * n + 1, N); }

  // after F::forward: the spectrum into LDS in natural order
  GPA_HD static void scatter(const cpx<T> (&x)[E], cpx<T>* lds, int tid) {
#pragma unroll
    for (int i = 0; i < E; ++i) lds[F::pad(F::spec_index(tid, i))] = x[i];
  }

  // DCT-II bins k and N - k from the half-length spectrum in LDS, divided by the eigenvalues -2 (ha + hb) (hb: 1 - cos of the
  // column's own row-frequency bin; the DC bin of column 0 -- first -- is divided by 1), and on to
  // x[i] = V'_k = conj(w_k) (Y_k - i Y_(N-k)) / 2, the first step of the DCT-III (k = 0: (V'_0, V'_(N/2)), both real).
  // *rho += sum_k c_k X_k Y_k over the thread's bins, c_0 = 1/2: 2N <r, z> of this column (Parseval)
  GPA_HD static void solve(cpx<T> (&x)[E], const cpx<T>* lds, int tid, const cpx<T>* __restrict__ wspec,
                           const T* __restrict__ ha, const T* __restrict__ ham, T hb, bool first, double* rho) {
    double acc = 0.0;
#pragma unroll
    for (int i = 0; i < E; ++i) {
      const int k = tid + TPF * i;
      const cpx<T> zk = lds[F::pad(k)], zm = lds[F::pad((HN - k) & (HN - 1))];
      const cpx<T> w = wspec[2 * k], ek = wspec[2 * k + 1];
      T xlo, xhi;
      if (k == 0) {
        xlo = T(2) * (zk.x + zk.y);
        xhi = T(1.41421356237309504880) * (zk.x - zk.y);
      } else {
        const cpx<T> ve = {T(0.5) * (zk.x + zm.x), T(0.5) * (zk.y - zm.y)};   // (T_k + conj T_m) / 2
        const cpx<T> vo = {T(0.5) * (zk.y + zm.y), T(-0.5) * (zk.x - zm.x)};  // -i (T_k - conj T_m) / 2
        const cpx<T> U = cmul(w, ve + cmul(ek, vo));
        xlo = T(2) * U.x;
        xhi = T(-2) * U.y;
      }
      T slo = T(-0.5) * fast_recip(ha[k] + hb);
      const T shi = T(-0.5) * fast_recip(ham[k] + hb);
      if (k == 0 && first) slo = T(1);
      const T ylo = xlo * slo, yhi = xhi * shi;
      acc += (k == 0 ? 0.5 : 1.0) * (double)xlo * (double)ylo + (double)xhi * (double)yhi;
      if (k == 0) x[i] = {T(0.5) * ylo, T(0.70710678118654752440) * yhi};
      else x[i] = cmulc(cpx<T>{T(0.5) * ylo, T(-0.5) * yhi}, w);
      GPA_COLHALF_FENCE(i);
    }
    *rho += acc;
  }

  // V' in LDS in natural order (slot 0 is never read: bin 0 keeps its pair in the register)
  GPA_HD static void park(const cpx<T> (&x)[E], cpx<T>* lds, int tid) {
#pragma unroll
    for (int i = 0; i < E; ++i) lds[F::pad(tid + TPF * i)] = x[i];
  }

  // T'_k = Ve + i Vo from V'_k and V'_(N/2-k), conjugated for the inverse transform (IFFT = conj FFT conj)
  GPA_HD static void merge(cpx<T> (&x)[E], const cpx<T>* lds, int tid, const cpx<T>* __restrict__ wspec) {
#pragma unroll
    for (int i = 0; i < E; ++i) {
      const int k = tid + TPF * i;
      cpx<T> Tk;
      if (k == 0) {
        Tk = {T(0.5) * (x[i].x + x[i].y), T(0.5) * (x[i].x - x[i].y)};
      } else {
        const cpx<T> vm = lds[F::pad(HN - k)];
        const cpx<T> ve = {T(0.5) * (x[i].x + vm.x), T(0.5) * (x[i].y - vm.y)};   // (V_k + conj V_m) / 2
        const cpx<T> d = {x[i].x - vm.x, x[i].y + vm.y};                          // V_k - conj V_m
        const cpx<T> vo = cscale(cmulc(d, wspec[2 * k + 1]), T(0.5));             // conj(E_k) (.) / 2
        Tk = {ve.x - vo.y, ve.y + vo.x};                                          // Ve + i Vo
      }
      x[i] = {Tk.x, -Tk.y};
      GPA_COLHALF_FENCE(i);
    }
  }

  // after the second F::forward: t[n] / (N/2), conjugated back, into LDS in natural order; slot n then holds rows
  // row_re(n) (real part) and row_im(n) (imaginary part) of the solved column
  GPA_HD static void inv_scatter(const cpx<T> (&x)[E], cpx<T>* lds, int tid) {
    const T inv = T(1) / T(HN);
#pragma unroll
    for (int i = 0; i < E; ++i) lds[F::pad(F::spec_index(tid, i))] = {x[i].x * inv, -x[i].y * inv};
  }
};

}  // namespace gpa
