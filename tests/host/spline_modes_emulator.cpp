// The folded boundary modes of the Lawler-Fujita sampler ('reflect' / 'mirror' / 'grid-wrap') on the CPU, through the
// very functions the kernels use (pygpa_amd/csrc/gpa_spline.h compiled by a plain C++ compiler): ext_index in the FIR
// prefilter, fold_coord, bspline_weights, tap_row and tap_index in the 4 x 4 tap sum of interp_folded.
//
//   spline_modes_emulator selfcheck
//       fold_coord / tap_index / ext_index on wild arguments (NaN, infinities, 1e30, the largest finite values; float and
//       double): every result is finite and inside the period, every tap index inside [0, n) and equal to ext_index's.  Prints OK.
//   spline_modes_emulator n0 n1 ext in.bin out.bin
//       in.bin : doubles -- the n0 x n1 field, the number of points P, P x-coordinates (axis 0), P y-coordinates (axis 1)
//       out.bin: P doubles -- the order-3 spline of the field with extension `ext` (0 reflect, 1 mirror, 2 wrap) at the points
// tests/test_warp_modes_host.py compares out.bin with scipy.ndimage.map_coordinates.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "gpa_spline.h"

using namespace gpa;

// the prefilter of gpa_warp.hip (ensure_taps, fir_rows_kernel, fir_cols_kernel) in double: rows first, then columns, each
// output the same sum of 2 KT + 1 products over the extended input
static std::vector<double> prefilter(const std::vector<double>& in, int n0, int n1, int ext) {
  constexpr int KT = TapHalf<double>::value;
  const double z = std::sqrt(3.0) - 2.0;
  double h[2 * KT + 1];
  for (int k = -KT; k <= KT; ++k) h[k + KT] = (-6.0 * z / (1.0 - z * z)) * std::pow(z, std::abs(k));
  std::vector<double> tmp((size_t)n0 * n1), out((size_t)n0 * n1);
  for (int x = 0; x < n0; ++x)
    for (int y = 0; y < n1; ++y) {
      double acc = 0;
      for (int k = 0; k <= 2 * KT; ++k) acc += h[k] * in[(size_t)x * n1 + ext_index(y - KT + k, n1, ext)];
      tmp[(size_t)x * n1 + y] = acc;
    }
  for (int x = 0; x < n0; ++x)
    for (int y = 0; y < n1; ++y) {
      double acc = 0;
      for (int k = 0; k <= 2 * KT; ++k) acc += h[k] * tmp[(size_t)ext_index(x - KT + k, n0, ext) * n1 + y];
      out[(size_t)x * n1 + y] = acc;
    }
  return out;
}

// interp_folded's arithmetic with every tap through tap_index (its interior path reads the same taps without it)
template <class T>
static T sample(const std::vector<T>& coef, int n0, int n1, T x, T y, int ext) {
  x = fold_coord(x, n0, ext);
  y = fold_coord(y, n1, ext);
  const T fx = std::floor(x), fy = std::floor(y);
  T wx[4], wy[4];
  bspline_weights(x - fx, wx);
  bspline_weights(y - fy, wy);
  const int ix = (int)fx - 1, iy = (int)fy - 1;
  int cy[4];
  for (int b = 0; b < 4; ++b) cy[b] = tap_index(iy + b, n1, ext);
  T out = 0;
  for (int a = 0; a < 4; ++a) {
    const T* row = coef.data() + (size_t)tap_index(ix + a, n0, ext) * n1;
    out = std::fma(wx[a], tap_row(wy, row[cy[0]], row[cy[1]], row[cy[2]], row[cy[3]]), out);
  }
  return out;
}

template <class T>
static int selfcheck_t(const char* name) {
  const T inf = std::numeric_limits<T>::infinity(), big = std::numeric_limits<T>::max();
  const T wild[] = {std::numeric_limits<T>::quiet_NaN(), inf, -inf, big, -big, T(1e30), T(-1e30), T(123456789.25), T(-987654.5),
                    T(-0.5), T(-0.50001), T(0), T(-0.0), T(1e-30), T(-1e-30)};
  int bad = 0;
  for (int n : {1, 2, 3, 4, 5, 7, 40, 4100})
    for (int ext : {(int)EXT_REFLECT, (int)EXT_MIRROR, (int)EXT_WRAP}) {
      const T lo = ext == EXT_REFLECT && n > 1 ? T(-0.5) : T(0);
      const T hi = n == 1 ? T(0) : (ext == EXT_REFLECT ? T(n) - T(0.5) : (ext == EXT_MIRROR ? T(n - 1) : T(n)));
      std::vector<T> pts(wild, wild + sizeof(wild) / sizeof(wild[0]));
      for (int k = -6 * n; k <= 6 * n; ++k) pts.push_back(T(0.5) * T(k));     // every half-integer in +-3 n
      for (T x : pts) {
        const T f = fold_coord(x, n, ext);
        const bool in_period = f >= lo && f <= hi && !(ext == EXT_WRAP && n > 1 && f >= hi);
        if (!in_period) { std::printf("%s: fold_coord(%g, %d, %d) = %g leaves the period\n", name, (double)x, n, ext, (double)f); ++bad; continue; }
        const int i0 = (int)std::floor(f) - 1;
        for (int a = 0; a < 4; ++a) {
          const int i = tap_index(i0 + a, n, ext);
          if (i < 0 || i >= n || i != ext_index(i0 + a, n, ext)) { std::printf("%s: tap_index(%d, %d, %d) = %d\n", name, i0 + a, n, ext, i); ++bad; }
        }
      }
      // ext_index against one period of the extension written out: 0 .. n-1, then n-1 .. 0 (reflect), n-2 .. 1 (mirror), nothing (wrap)
      std::vector<int> period;
      for (int i = 0; i < n; ++i) period.push_back(i);
      if (ext == EXT_REFLECT) for (int i = n - 1; i >= 0; --i) period.push_back(i);
      if (ext == EXT_MIRROR) for (int i = n - 2; i >= 1; --i) period.push_back(i);
      const int p = (int)period.size();
      for (int i = -5 * n - 3; i <= 5 * n + 3; ++i) {
        const int e = ext_index(i, n, ext);
        if (e != period[((i % p) + p) % p]) { std::printf("%s: ext_index(%d, %d, %d) = %d\n", name, i, n, ext, e); ++bad; }
      }
    }
  return bad;
}

int main(int argc, char** argv) {
  if (argc == 2 && !std::strcmp(argv[1], "selfcheck")) {
    const int bad = selfcheck_t<float>("float") + selfcheck_t<double>("double");
    // the float instantiation of the whole sampler on a constant field: the weights sum to one
    std::vector<float> ones(4 * 5, 1.0f);
    int off = 0;
    for (int ext = 0; ext < 3; ++ext)
      for (float x = -9.75f; x < 9.f; x += 0.25f)
        if (std::fabs(sample<float>(ones, 4, 5, x, 1.5f * x, ext) - 1.0f) > 4e-7f) ++off;
    if (bad || off) { std::printf("FAILED: %d fold / index results, %d partition-of-unity sums\n", bad, off); return 1; }
    std::printf("OK\n");
    return 0;
  }
  if (argc != 6) { std::fprintf(stderr, "usage: %s selfcheck | n0 n1 ext in.bin out.bin\n", argv[0]); return 2; }
  const int n0 = std::atoi(argv[1]), n1 = std::atoi(argv[2]), ext = std::atoi(argv[3]);
  if (n0 < 1 || n1 < 1 || ext < 0 || ext > 2) { std::fprintf(stderr, "bad arguments\n"); return 2; }
  std::FILE* f = std::fopen(argv[4], "rb");
  if (!f) { std::perror(argv[4]); return 2; }
  std::vector<double> field((size_t)n0 * n1);
  double np = 0;
  if (std::fread(field.data(), sizeof(double), field.size(), f) != field.size() || std::fread(&np, sizeof(double), 1, f) != 1 || np < 0 || np > 1e8) {
    std::fprintf(stderr, "short or malformed input\n");
    return 2;
  }
  const size_t P = (size_t)np;
  std::vector<double> xs(P), ys(P), out(P);
  if (std::fread(xs.data(), sizeof(double), P, f) != P || std::fread(ys.data(), sizeof(double), P, f) != P) {
    std::fprintf(stderr, "short input\n");
    return 2;
  }
  std::fclose(f);
  const std::vector<double> coef = prefilter(field, n0, n1, ext);
  for (size_t p = 0; p < P; ++p) out[p] = sample<double>(coef, n0, n1, xs[p], ys[p], ext);
  f = std::fopen(argv[5], "wb");
  if (!f) { std::perror(argv[5]); return 2; }
  if (std::fwrite(out.data(), sizeof(double), P, f) != P) { std::fprintf(stderr, "short write\n"); return 2; }
  std::fclose(f);
  std::printf("OK\n");
  return 0;
}
