// Host emulator for pygpa_amd/csrc/gpa_unwrap_colhalf.h (see fft_emulator.cpp): the half-length column solve of the
// unwrap, thread by thread and phase by phase on the CPU, with the tables colhalf_tables() builds for the device.
// Build: g++ -O2 -std=c++17 -I pygpa_amd/csrc tests/host/colhalf_emulator.cpp -o /tmp/colhalf_emu
//
// Checked per length N = 2^LG (LG = 7, 10: every bin against the defining sums; LG = 14, the length the kernel runs):
//   * the rows behind the transform's slots are a permutation of 0 .. N-1 (row_re / row_im),
//   * the DCT-II bins X_k the solve phase forms from the half-length spectrum (all of them, or 64 of them at LG = 14),
//   * the solved column z against the system it solves: (T + mu) z = r with T the second-difference matrix with
//     reflecting ends and mu = -2 hb (the DCT-II basis diagonalises T: eigenvalues -2 ha_k), which needs no transform,
//   * column 0 (hb = 0, DC bin divided by 1): T z = r - mean(r) and mean(z) = mean(r),
//   * rho against 2N <r, z>.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gpa_unwrap_colhalf.h"

using namespace gpa;

static int fails = 0;
static void check(bool ok, const char* what, int lg, double v) {
  if (!ok) { printf("FAIL %s LG=%d (%.3e)\n", what, lg, v); ++fails; }
}

template <int LG>
void test_one(bool first) {
  using T = double;
  using G = ColHalf<T, LG>;
  using F = typename G::F;
  constexpr int N = G::N, HN = G::HN, TPF = G::TPF, E = G::E;
  std::vector<double> wsp, ha, ham;
  colhalf_tables(N, (double)N, wsp, ha, ham);
  const cpx<T>* wspec = reinterpret_cast<const cpx<T>*>(wsp.data());
  // the tables' own contents: bin k and its partner
  for (int k = 0; k < HN; k += (LG > 10 ? 97 : 1)) {
    const int km = k == 0 ? HN : N - k;
    check(std::fabs(ha[k] - (1 - std::cos(M_PI * k / N))) < 1e-15 && std::fabs(ham[k] - (1 - std::cos(M_PI * km / N))) < 1e-15, "eigenvalue tables", LG, (double)k);
    check(std::fabs(wspec[2 * k].x - std::cos(M_PI * k / (2.0 * N))) < 1e-15 && std::fabs(wspec[2 * k + 1].y + std::sin(2 * M_PI * k / N)) < 1e-15, "phase tables", LG, (double)k);
  }
  std::vector<cpx<T>> twh(HN);
  for (int k = 0; k < HN; ++k) twh[k] = {std::cos(-2 * M_PI * k / HN), std::sin(-2 * M_PI * k / HN)};
  std::vector<typename F::Twiddles> tw(TPF);
  for (int t = 0; t < TPF; ++t) F::load_twiddles(tw[t], twh.data(), t);
  std::vector<cpx<T>> regs((size_t)E * TPF), lds(F::LDS_ELEMS);
  auto R = [&](int t) -> cpx<T>(&)[E] { return *reinterpret_cast<cpx<T>(*)[E]>(&regs[(size_t)E * t]); };
  auto forward = [&]() {
    for (int t = 0; t < TPF; ++t) F::template fwd_phase<0>(R(t), lds.data(), t, tw[t]);
    if constexpr (F::P > 1) for (int t = 0; t < TPF; ++t) F::template fwd_phase<1>(R(t), lds.data(), t, tw[t]);
    if constexpr (F::P > 2) for (int t = 0; t < TPF; ++t) F::template fwd_phase<2>(R(t), lds.data(), t, tw[t]);
    if constexpr (F::P > 3) for (int t = 0; t < TPF; ++t) F::template fwd_phase<3>(R(t), lds.data(), t, tw[t]);
  };
  std::vector<double> r(N), z(N);
  srand(LG + (first ? 100 : 0));
  for (int n = 0; n < N; ++n) r[n] = rand() / (double)RAND_MAX - 0.4 + std::sin(0.01 * n);
  const double hb = first ? 0.0 : 1 - std::cos(M_PI * 3 / 64.0);   // the column's own row-frequency term
  // ---- load: every row exactly once
  std::vector<int> seen(N, 0);
  for (int t = 0; t < TPF; ++t)
    for (int i = 0; i < E; ++i) {
      const int n = t + TPF * i, a = G::row_re(n), b = G::row_im(n);
      check(a >= 0 && a < N && b >= 0 && b < N, "row index range", LG, (double)n);
      ++seen[a];
      ++seen[b];
      R(t)[i] = {r[a], r[b]};
    }
  for (int n = 0; n < N; ++n) check(seen[n] == 1, "rows form a permutation", LG, (double)n);
  forward();
  for (int t = 0; t < TPF; ++t) G::scatter(R(t), lds.data(), t);
  // ---- the DCT-II bins, recovered from what the solve phase leaves: x = conj(w_k) (Y_k - i Y_(N-k)) / 2
  std::vector<double> rho_t(TPF, 0.0);
  for (int t = 0; t < TPF; ++t) G::solve(R(t), lds.data(), t, wspec, ha.data(), ham.data(), hb, first, &rho_t[t]);
  std::vector<double> Y(N);
  for (int t = 0; t < TPF; ++t)
    for (int i = 0; i < E; ++i) {
      const int k = t + TPF * i;
      if (k == 0) { Y[0] = 2 * R(t)[i].x; Y[HN] = R(t)[i].y * 1.41421356237309504880; continue; }
      const cpx<T> u = cmul(R(t)[i], wspec[2 * k]);   // (Y_k - i Y_(N-k)) / 2
      Y[k] = 2 * u.x;
      Y[N - k] = -2 * u.y;
    }
  double scale = 0;
  for (int n = 0; n < N; ++n) scale += std::fabs(r[n]);
  const int step = LG > 10 ? N / 64 + 1 : 1;
  for (int k = 0; k < N; k += step) {
    double s = 0;
    for (int n = 0; n < N; ++n) s += r[n] * std::cos(M_PI * k * (2 * n + 1) / (2.0 * N));
    const double sk = std::sin(M_PI * k / (2.0 * N));   // (1 - cos = 2 sin^2 of the half angle: no cancellation near k = 0)
    const double eig = (k == 0 && first) ? 1.0 : -2.0 * (2 * sk * sk + hb);
    check(std::fabs(Y[k] * eig - 2 * s) < 1e-12 * scale, "DCT-II bin", LG, (double)k);
  }
  // ---- DCT-III
  for (int t = 0; t < TPF; ++t) G::park(R(t), lds.data(), t);
  for (int t = 0; t < TPF; ++t) G::merge(R(t), lds.data(), t, wspec);
  forward();
  for (int t = 0; t < TPF; ++t) G::inv_scatter(R(t), lds.data(), t);
  for (int t = 0; t < TPF; ++t)
    for (int i = 0; i < E; ++i) {
      const int n = t + TPF * i;
      const cpx<T> v = lds[F::pad(n)];
      z[G::row_re(n)] = v.x;
      z[G::row_im(n)] = v.y;
    }
  // ---- (T + mu) z = r, reflecting ends
  double mean_r = 0, mean_z = 0, zmax = 0, rz = 0;
  for (int n = 0; n < N; ++n) { mean_r += r[n] / N; mean_z += z[n] / N; zmax = std::fmax(zmax, std::fabs(z[n])); rz += r[n] * z[n]; }
  double worst = 0;
  for (int n = 0; n < N; ++n) {
    const double zl = z[n > 0 ? n - 1 : 0], zr = z[n < N - 1 ? n + 1 : N - 1];
    const double lhs = zl - 2 * z[n] + zr - 2 * hb * z[n];
    worst = std::fmax(worst, std::fabs(lhs - (r[n] - (first ? mean_r : 0.0))));
  }
  // (the solve amplifies rounding by up to 1 / smallest eigenvalue: z itself is that much larger than r)
  check(worst < 1e-13 * (zmax + 1) * 4, "tridiagonal system", LG, worst);
  if (first) check(std::fabs(mean_z - mean_r) < 1e-12 * (zmax + 1), "column 0 keeps the mean", LG, mean_z - mean_r);
  double rho = 0;
  for (int t = 0; t < TPF; ++t) rho += rho_t[t];
  check(std::fabs(rho - 2.0 * N * rz) < 1e-10 * std::fabs(2.0 * N * rz) + 1e-9, "rho", LG, rho - 2.0 * N * rz);
}

int main() {
  for (int first = 0; first < 2; ++first) {
    test_one<7>(first != 0);
    test_one<10>(first != 0);
    test_one<14>(first != 0);
  }
  if (fails) return 1;
  printf("OK\n");
  return 0;
}
