// Host check of pygpa_amd/csrc/gpa_kerelsky.h, an ordinary executable (built plain and under the host sanitizers by
// tests/test_kerelsky_host.py).
//
//   kerelsky_check                  self-checks: the analytic Jacobian against central differences, the closed-form root, the
//                                   bounds, NaN pixels, psi on eps = 0; prints "OK <checks>"
//   kerelsky_check IN OUT           solves the pixels of IN with the very code the kernel runs and writes OUT.
//       IN : doubles  n, max_nfev, retry_cost, has_a0, x0[4], a0[4], then n x 4 (A, or J when has_a0)
//       OUT: n x 6 doubles  theta, psi, eps, xi, cost, trial evaluations
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gpa_kerelsky.h"

namespace k = kerelsky;

static long checks = 0;
#define CHECK(cond)                                                      \
  do {                                                                   \
    ++checks;                                                            \
    if (!(cond)) {                                                       \
      std::printf("FAILED line %d: %s\n", __LINE__, #cond);              \
      return 1;                                                          \
    }                                                                    \
  } while (0)

static double rnd(unsigned long long& s) {     // in [0, 1)
  s = s * 6364136223846793005ull + 1442695040888963407ull;
  return (double)(s >> 11) / 9007199254740992.0;
}

// the model as it is stated, V^T D V W(theta + xi) - W(xi), for a root to aim at
static void model(const double* x, double* M) {
  const double c = cos(x[1] * k::DEG), s = sin(x[1] * k::DEG), p = 1.0 / (1.0 + x[2]), q = 1.0 / (1.0 - k::DELTA * x[2]);
  const double S00 = p * c * c + q * s * s, S01 = (q - p) * c * s, S11 = p * s * s + q * c * c;
  const double cp = cos((x[0] + x[3]) * k::DEG), sp = sin((x[0] + x[3]) * k::DEG), cx = cos(x[3] * k::DEG), sx = sin(x[3] * k::DEG);
  M[0] = S00 * cp + S01 * sp - cx;
  M[1] = -S00 * sp + S01 * cp + sx;
  M[2] = S01 * cp + S11 * sp - sx;
  M[3] = -S01 * sp + S11 * cp - cx;
}

static int self_check() {
  unsigned long long seed = 12345;
  for (int it = 0; it < 2000; ++it) {
    const double x[4] = {3.0 * rnd(seed), 360.0 * rnd(seed) - 180.0, it % 7 == 0 ? 0.0 : 0.05 * rnd(seed), 360.0 * rnd(seed)};
    double A[4], r[4], J[4][4], M[4];
    for (double& a : A) a = 0.1 * (rnd(seed) - 0.5);
    const double c = k::eval(x, A, r, J);
    model(x, M);
    for (int i = 0; i < 4; ++i) CHECK(fabs(r[i] - 1000.0 * (M[i] - A[i])) <= 1e-9);
    CHECK(fabs(c - 0.5 * (r[0] * r[0] + r[1] * r[1] + r[2] * r[2] + r[3] * r[3])) <= 1e-12 * c);
    for (int j = 0; j < 4; ++j) {
      const double h = j == 2 ? 1e-6 : 1e-4;
      double xp[4] = {x[0], x[1], x[2], x[3]}, xm[4] = {x[0], x[1], x[2], x[3]}, rp[4], rm[4], Jt[4][4];
      xp[j] += h;
      xm[j] -= h;
      k::eval(xp, A, rp, Jt);
      k::eval(xm, A, rm, Jt);
      for (int i = 0; i < 4; ++i) CHECK(fabs(J[i][j] - (rp[i] - rm[i]) / (2 * h)) <= 1e-5 * (1.0 + fabs(J[i][j])));
    }
    // a root: the closed form finds it, and so does the solver from a start that is degrees away
    double xr[4], xs[4];
    model(x, A);
    if (x[2] > 1e-4) {
      const double x0[4] = {1.0, x[1] + 30.0, 0.0, x[3] + 20.0};
      CHECK(k::closed_form_root(A, x0, xr));
      CHECK(fabs(xr[0] - x[0]) <= 1e-9 && fabs(xr[2] - x[2]) <= 1e-12 && fabs(remainder(xr[1] - x[1], 180.0)) <= 1e-7 &&
            fabs(remainder(xr[3] - x[3], 360.0)) <= 1e-9);
      int nfev = 0;
      const double cs = k::solve(A, x0, 50, 1e-5, xs, &nfev);
      CHECK(cs <= 1e-20 && xs[0] >= 0.0 && xs[2] >= 0.0 && nfev >= 1 && nfev <= 150);
      CHECK(fabs(xs[1] - x0[1]) <= 90.0 && fabs(xs[3] - x0[3]) <= 180.0);
      CHECK(fabs(xs[0] - x[0]) <= 1e-8 && fabs(xs[2] - x[2]) <= 1e-11 && fabs(remainder(xs[3] - x[3], 360.0)) <= 1e-8);
    }
  }
  // no root with theta >= 0: the result sits on the bound, exactly, and the cost is that of the point returned
  for (int it = 0; it < 500; ++it) {
    const double xneg[4] = {-1.0 - rnd(seed), 180.0 * rnd(seed), 0.01 * rnd(seed), 30.0 * rnd(seed)}, x0[4] = {1.0, 0.0, 0.001, 15.0};
    double A[4], xs[4], r[4], J[4][4];
    model(xneg, A);
    int nfev = 0;
    const double cs = k::solve(A, x0, 50, 1e-5, xs, &nfev);
    CHECK(isfinite(cs) && xs[0] >= 0.0 && xs[2] >= 0.0 && nfev <= 150);
    CHECK(fabs(k::eval(xs, A, r, J) - cs) <= 1e-9 * (1.0 + cs));
  }
  // eps = 0 with the worst psi: the solver must leave the bound (the start has no psi derivative at all)
  {
    const double x[4] = {1.0, 35.0, 0.01, 10.0}, x0[4] = {1.0, 125.0, 0.0, 10.0};
    double A[4], xs[4];
    model(x, A);
    CHECK(k::solve(A, x0, 50, 1e30, xs, nullptr) <= 1e-20);     // retry_cost 1e30: the first start alone
    CHECK(fabs(xs[2] - 0.01) <= 1e-11 && fabs(remainder(xs[1] - 35.0, 180.0)) <= 1e-6);
  }
  // max_nfev is per start and is honoured
  {
    const double x[4] = {1.5, 35.0, 0.01, 40.0}, x0[4] = {0.01, 0.0, 0.0, 100.0};
    double A[4], xs[4];
    model(x, A);
    for (int m = 1; m <= 6; ++m) {
      int nfev = 0;
      const double cs = k::solve(A, x0, m, 0.0, xs, &nfev);
      CHECK(nfev <= k::N_STARTS * m && isfinite(cs));
    }
  }
  // a non-finite A: four NaNs and a NaN cost, no evaluation
  for (int i = 0; i < 4; ++i) {
    double A[4] = {0.01, 0.02, -0.02, 0.01}, xs[4];
    const double x0[4] = {1.0, 0.0, 0.0, 15.0};
    A[i] = i % 2 ? NAN : INFINITY;
    int nfev = -1;
    const double cs = k::solve(A, x0, 50, 1e-5, xs, &nfev);
    CHECK(isnan(cs) && isnan(xs[0]) && isnan(xs[1]) && isnan(xs[2]) && isnan(xs[3]) && nfev == 0);
  }
  std::printf("OK %ld\n", checks);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 1) return self_check();
  if (argc != 3) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 3;
  double head[12];
  if (std::fread(head, sizeof(double), 12, f) != 12) return 4;
  const size_t n = (size_t)head[0];
  std::vector<double> in(4 * n), out(6 * n);
  if (std::fread(in.data(), sizeof(double), 4 * n, f) != 4 * n) return 4;
  std::fclose(f);
  for (size_t i = 0; i < n; ++i) {
    double A[4];
    if (head[3] != 0.0) k::form_A(head + 8, &in[4 * i], A);
    else for (int j = 0; j < 4; ++j) A[j] = in[4 * i + j];
    int nfev = 0;
    out[6 * i + 4] = k::solve(A, head + 4, (int)head[1], head[2], &out[6 * i], &nfev);
    out[6 * i + 5] = nfev;
  }
  f = std::fopen(argv[2], "wb");
  if (!f) return 3;
  const bool ok = std::fwrite(out.data(), sizeof(double), 6 * n, f) == 6 * n;
  std::fclose(f);
  return ok ? 0 : 5;
}
