// f-3: scipy.ndimage.gaussian_filter along one axis as an overlap-save FFT convolution (gpa_gaussfft.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "gpa_fft.h"

namespace gpa {

// geometry of the column kernels (gf_cols_kernel, and prep_cols_kernel of gpa_prep.hip, which must cut the same tiles: it is what
// gaussfft_choose_lg prices).  C complex transforms = 2C adjacent real columns per workgroup
template <class T, int LG>
struct GfColGeom {
  using F = WgFFT<T, LG>;
  static constexpr int cols() {
    int c = 16;
    while (c > 1 && (c * F::TPF > 1024 || (size_t)c * F::LDS_ELEMS * sizeof(cpx<T>) > 140 * 1024)) c /= 2;
    return c;
  }
  static constexpr int C = cols();
  static constexpr int NT = (sizeof(T) == 4 && C >= 2) ? 2 : 1;   // complex transforms per thread
  static constexpr int CT = C / NT;
  static constexpr int REGION = CT * F::LDS_ELEMS;
  static constexpr int THREADS = CT * F::TPF;
  static constexpr size_t LDS_BYTES = (size_t)NT * REGION * sizeof(cpx<T>);
  static constexpr bool FITS = (size_t)F::LDS_ELEMS * sizeof(cpx<T>) <= 140 * 1024;
  static constexpr int RC = 2 * C;   // real columns per workgroup
};

// log2 of the segment transform length for an axis of n samples and a kernel of radius R (0: no length fits, use the direct sum)
int gaussfft_choose_lg(int dtype, int n, int R, bool cols);
// transfer function of the 2R + 1 normalised taps w, / L, in the register engine's spectral layout (doubles)
std::vector<double> gaussfft_table(int lg, const std::vector<double>& w);
// out = [minuend -] gaussian_filter1d(in) along `axis` (0: columns, 1: rows; minuend only with axis 1); H, tw: device tables
hipError_t launch_gaussfft(int dtype, int lg, int axis, const void* in, void* out, int n0, int n1, int R, const void* H,
                           const void* tw, const void* minuend, hipStream_t s);

}  // namespace gpa
