// Per-pixel Kerelsky fit (pyGPA/property_extract.py:696-704, :780-883): the single copy of the arithmetic, for the kernel of
// gpa_kerelsky.hip and for the host check tests/host/kerelsky_check.cpp.  f64 throughout in both builds.
//
// Model (a declared restatement): W(a) = [[cos a, -sin a], [sin a, cos a]], D(e) = diag(1/(1+e), 1/(1-DELTA e)),
// V = W(psi), angles in degrees,
//     F(x; A) = 1000 vec(V^T D V W(theta + xi) - W(xi) - A),   x = (theta, psi, eps, xi),   theta >= 0, eps >= 0,   cost = |F|^2 / 2.
// Evaluated without cancellation as (S - I) W(theta + xi) + W(xi) (W(theta) - I) - A, S - I from -e/(1+e) and DELTA e/(1-DELTA e),
// W(theta) - I from sin^2 of the half angle.
//
// One start is a bounded Levenberg-Marquardt iteration with the analytic Jacobian: active set (a variable on its bound whose
// gradient points outward is held), Marquardt scaling with a floor (psi has no derivative at eps = 0), steps clipped to 60 degrees
// and 0.5 in eps, trial points projected on the bounds.  On eps = 0 the cost does not depend on psi and a solver that keeps psi can
// rest on a point that is no minimum: there psi is set to the direction along which the cost falls fastest as eps leaves 0, which
// is closed form (zero_strain_psi).  A start ends after max_nfev trial evaluations, at cost <= COST_FLOOR, or when the model
// predicts a reduction below PRED_TOL of the cost.
//
// Starts, in order, each tried only while the best cost exceeds retry_cost:  x0;  x0 with psi + 90 (the reference's two);  the
// root in closed form when one with theta >= 0 exists.  (A + W(xi) = S W(theta + xi) is a polar decomposition: the difference of
// the singular values of A + W(xi) does not depend on xi, which gives eps from a quadratic, their product fixes
// t = (a + d) cos xi + (c - b) sin xi, which gives xi up to a sign, and the polar factors give theta and psi.)
//
// The whole solve is a state machine advanced by step(), one trial evaluation per call, so that the lanes of a wave share one
// instruction stream whichever start each of them is in.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define KRL_HD __host__ __device__ inline
#define KRL_UNROLL _Pragma("unroll")
#else
#define KRL_HD inline
#define KRL_UNROLL
#endif

namespace kerelsky {

constexpr double DELTA = 0.16, SCALE = 1000.0, DEG = 0.017453292519943295769, RAD = 57.295779513082320877;
constexpr double COST_FLOOR = 1e-24;     // |F| ~ 1.4e-12: 1e-15 of the matrix elements, 1e-13 degrees
constexpr double PRED_TOL = 1e-13;
constexpr double EPS_POLE = 0.98 / DELTA;     // D has a pole at eps = 1 / DELTA: a trial beyond this is refused
constexpr int N_STARTS = 3;

// residual r (row-major 2 x 2) and Jacobian J[i][j] = d r_i / d x_j at x; returns the cost
KRL_HD double eval(const double* x, const double* A, double* r, double (*J)[4]) {
  double sp, cp, sx, cx, s2, c2, sh, ch;
  sincos((x[0] + x[3]) * DEG, &sp, &cp);
  sincos(x[3] * DEG, &sx, &cx);
  sincos(2.0 * x[1] * DEG, &s2, &c2);
  sincos(0.5 * x[0] * DEG, &sh, &ch);
  const double e = x[2], ip = 1.0 / (1.0 + e), iq = 1.0 / (1.0 - DELTA * e);
  const double pm1 = -e * ip, qm1 = DELTA * e * iq;            // p - 1, q - 1
  const double m1 = 0.5 * (pm1 + qm1), h = 0.5 * (pm1 - qm1);   // S - I = m1 I + h Q,  Q = [[c2, -s2], [-s2, -c2]]
  const double dp = -ip * ip, dq = DELTA * iq * iq, dm = 0.5 * (dp + dq), dh = 0.5 * (dp - dq);
  const double t00 = m1 + h * c2, t01 = -h * s2, t11 = m1 - h * c2;
  const double u = -2.0 * sh * sh, v = 2.0 * sh * ch;           // W(theta) - I = [[u, -v], [v, u]]
  const double g00 = cx * u - sx * v, g10 = sx * u + cx * v;    // W(xi) (W(theta) - I) = [[g00, -g10], [g10, g00]]
  r[0] = SCALE * ((t00 * cp + t01 * sp) + g00 - A[0]);
  r[1] = SCALE * ((t01 * cp - t00 * sp) - g10 - A[1]);
  r[2] = SCALE * ((t01 * cp + t11 * sp) + g10 - A[2]);
  r[3] = SCALE * ((t11 * cp - t01 * sp) + g00 - A[3]);
  const double s00 = 1.0 + t00, s11 = 1.0 + t11, k = SCALE * DEG;
  // d / d theta = S W'(phi),  W' = [[-sin, -cos], [cos, -sin]];  d / d xi = the same - W'(xi)
  J[0][0] = k * (t01 * cp - s00 * sp);
  J[1][0] = k * (-s00 * cp - t01 * sp);
  J[2][0] = k * (s11 * cp - t01 * sp);
  J[3][0] = k * (-t01 * cp - s11 * sp);
  J[0][3] = J[0][0] + k * sx;
  J[1][3] = J[1][0] + k * cx;
  J[2][3] = J[2][0] - k * cx;
  J[3][3] = J[3][0] + k * sx;
  // Q W(phi) = [[qa, -qb], [-qb, -qa]],  qa = cos(2 psi + phi), qb = sin(2 psi + phi);  dQ / dpsi W = 2 [[-qb, -qa], [-qa, qb]]
  const double qa = c2 * cp - s2 * sp, qb = s2 * cp + c2 * sp, kh = 2.0 * k * h;
  J[0][1] = -kh * qb;
  J[1][1] = -kh * qa;
  J[2][1] = -kh * qa;
  J[3][1] = kh * qb;
  J[0][2] = SCALE * (dm * cp + dh * qa);
  J[1][2] = SCALE * (-dm * sp - dh * qb);
  J[2][2] = SCALE * (dm * sp - dh * qb);
  J[3][2] = SCALE * (dm * cp - dh * qa);
  return 0.5 * (r[0] * r[0] + r[1] * r[1] + r[2] * r[2] + r[3] * r[3]);
}

// On eps = 0: d cost / d eps = <R, dm I + dh Q(psi)> with R = r W(phi)^T and dh < 0; the psi (degrees, nearest to psi_now mod 180)
// that makes it smallest.  Leaves psi_now when R gives no direction.
KRL_HD double zero_strain_psi(const double* x, const double* r) {
  double sp, cp;
  sincos((x[0] + x[3]) * DEG, &sp, &cp);
  const double R00 = r[0] * cp - r[1] * sp, R01 = r[0] * sp + r[1] * cp, R10 = r[2] * cp - r[3] * sp, R11 = r[2] * sp + r[3] * cp;
  const double a = R00 - R11, b = R01 + R10;     // maximise a cos(2 psi) - b sin(2 psi)
  if (a == 0.0 && b == 0.0) return x[1];
  const double psi = -0.5 * RAD * atan2(b, a);
  return x[1] + remainder(psi - x[1], 180.0);
}

// The root of F in closed form, as the start nearest to x0; false when none exists with theta >= 0.
KRL_HD bool closed_form_root(const double* A, const double* x0, double* x) {
  const double a = A[0], b = A[1], c = A[2], d = A[3];
  const double s = sqrt((a - d) * (a - d) + (b + c) * (b + c));     // sigma_2 - sigma_1 of A + W(xi), whatever xi
  const double bq = (1.0 + DELTA) - s * (1.0 - DELTA);
  const double e = 2.0 * s / (bq + sqrt(bq * bq + 4.0 * DELTA * s * s));
  if (!(e >= 0.0) || !(e < EPS_POLE)) return false;
  const double pq1 = (DELTA * e * e - (1.0 - DELTA) * e) / ((1.0 + e) * (1.0 - DELTA * e));     // sigma_1 sigma_2 - 1
  const double t = pq1 - (a * d - b * c), rho = hypot(a + d, c - b);
  if (!(fabs(t) <= rho) || !(rho > 0.0)) return false;
  const double xi_mid = RAD * atan2(c - b, a + d), dxi = RAD * acos(t / rho);
  bool found = false;
  double dist = 0.0;
  for (int sgn = -1; sgn <= 1; sgn += 2) {
    const double xi = xi_mid + sgn * dxi;
    double sx, cx;
    sincos(xi * DEG, &sx, &cx);
    const double B00 = a + cx, B01 = b - sx, B10 = c + sx, B11 = d + cx;
    const double phi = atan2(B10 - B01, B00 + B11);
    const double theta = remainder(RAD * phi - xi, 360.0);
    if (!(theta >= 0.0)) continue;
    double sp, cp;
    sincos(phi, &sp, &cp);
    const double S00 = B00 * cp - B01 * sp, S01 = B00 * sp + B01 * cp, S11 = B10 * sp + B11 * cp;     // S = B W(phi)^T
    const double psi = 0.5 * RAD * atan2(2.0 * S01, S11 - S00);
    const double far = fabs(remainder(xi - x0[3], 360.0));
    if (found && !(far < dist)) continue;
    found = true;
    dist = far;
    x[0] = theta;
    x[1] = psi;
    x[2] = e;
    x[3] = xi;
  }
  return found;
}

struct State {
  double A[4], x0[4];
  double x[4], r[4], J[4][4], cost, mu;     // the running start
  double best[4], best_cost;
  double retry_cost;
  int max_nfev, nfev, start, total;         // nfev: of the running start; start: the running one, N_STARTS: finished; total: all evaluations
  bool fresh;                               // the next step() evaluates the start point itself
};

KRL_HD bool finished(const State& st) { return st.start >= N_STARTS; }

// the point the next start begins from; false when this start has none
KRL_HD bool start_point(const State& st, int start, double* x) {
  if (start == 2) {
    if (!closed_form_root(st.A, st.x0, x)) return false;
  } else {
    for (int i = 0; i < 4; ++i) x[i] = st.x0[i];
    if (start == 1) x[1] += 90.0;
  }
  x[0] = fmax(x[0], 0.0);
  x[2] = fmax(x[2], 0.0);
  return true;
}

KRL_HD void init(State& st, const double* A, const double* x0, int max_nfev, double retry_cost) {
  bool ok = true;
  for (int i = 0; i < 4; ++i) {
    st.A[i] = A[i];
    st.x0[i] = x0[i];
    st.best[i] = NAN;
    ok = ok && isfinite(A[i]);
  }
  st.best_cost = NAN;
  st.retry_cost = retry_cost;
  st.max_nfev = max_nfev;
  st.nfev = st.total = 0;
  st.cost = st.mu = 0.0;
  st.fresh = true;
  st.start = ok ? 0 : N_STARTS;     // a non-finite A: four NaNs and a NaN cost
  if (ok) start_point(st, 0, st.x);
}

// the running start is over: keep the better result, move to the next start that exists, or finish
KRL_HD void end_start(State& st) {
  if (!(st.best_cost <= st.cost)) {     // also the first result, over the NaN
    st.best_cost = st.cost;
    for (int i = 0; i < 4; ++i) st.best[i] = st.x[i];
  }
  st.fresh = true;
  st.nfev = 0;
  for (;;) {
    ++st.start;
    if (st.start >= N_STARTS || !(st.best_cost > st.retry_cost)) {
      st.start = N_STARTS;
      return;
    }
    if (start_point(st, st.start, st.x)) return;
  }
}

// psi has no say on eps = 0: give it the value along which eps can leave the bound (r is unchanged, J is not)
KRL_HD void settle(State& st) {
  if (st.x[2] == 0.0) {
    st.x[1] = zero_strain_psi(st.x, st.r);
    st.cost = eval(st.x, st.A, st.r, st.J);
  }
}

// one trial evaluation of an unfinished solve
KRL_HD void step(State& st) {
  if (st.fresh) {
    st.fresh = false;
    st.cost = eval(st.x, st.A, st.r, st.J);
    st.nfev = 1;
    ++st.total;
    st.mu = 1e-3;
    if (!isfinite(st.cost)) { st.cost = INFINITY; end_start(st); return; }
    settle(st);
    if (st.cost <= COST_FLOOR || st.nfev >= st.max_nfev) end_start(st);
    return;
  }
  // gradient and Gauss-Newton matrix; a variable on its bound with the gradient pointing outward is held
  double g[4], H[4][4];
KRL_UNROLL
  for (int i = 0; i < 4; ++i) {
    g[i] = st.J[0][i] * st.r[0] + st.J[1][i] * st.r[1] + st.J[2][i] * st.r[2] + st.J[3][i] * st.r[3];
KRL_UNROLL
    for (int j = 0; j <= i; ++j) H[i][j] = H[j][i] = st.J[0][i] * st.J[0][j] + st.J[1][i] * st.J[1][j] + st.J[2][i] * st.J[2][j] + st.J[3][i] * st.J[3][j];
  }
  const bool held0 = st.x[0] <= 0.0 && g[0] > 0.0, held2 = st.x[2] <= 0.0 && g[2] > 0.0;
  const double dmax = fmax(fmax(H[0][0], H[1][1]), fmax(H[2][2], H[3][3]));
  double M[4][4], dx[4];
KRL_UNROLL
  for (int i = 0; i < 4; ++i) {
    const bool hi = (i == 0 && held0) || (i == 2 && held2);
KRL_UNROLL
    for (int j = 0; j < 4; ++j) {
      const bool hj = (j == 0 && held0) || (j == 2 && held2);
      M[i][j] = (hi || hj) ? 0.0 : H[i][j];
    }
    M[i][i] = hi ? 1.0 : H[i][i] + st.mu * fmax(H[i][i], 1e-10 * dmax) + 1e-300;
    dx[i] = hi ? 0.0 : -g[i];
  }
  // Cholesky M = L L^T in place (lower), then the two triangular solves
  bool spd = true;
KRL_UNROLL
  for (int j = 0; j < 4; ++j) {
    double djj = M[j][j];
KRL_UNROLL
    for (int k = 0; k < j; ++k) djj -= M[j][k] * M[j][k];
    spd = spd && djj > 0.0;
    const double l = sqrt(djj), il = 1.0 / l;
    M[j][j] = l;
KRL_UNROLL
    for (int i = j + 1; i < 4; ++i) {
      double v = M[i][j];
KRL_UNROLL
      for (int k = 0; k < j; ++k) v -= M[i][k] * M[j][k];
      M[i][j] = v * il;
    }
  }
KRL_UNROLL
  for (int i = 0; i < 4; ++i) {
KRL_UNROLL
    for (int k = 0; k < i; ++k) dx[i] -= M[i][k] * dx[k];
    dx[i] /= M[i][i];
  }
KRL_UNROLL
  for (int i = 3; i >= 0; --i) {
KRL_UNROLL
    for (int k = i + 1; k < 4; ++k) dx[i] -= M[k][i] * dx[k];
    dx[i] /= M[i][i];
  }
  const double amax = fmax(fmax(fabs(dx[0]), fabs(dx[1])), fabs(dx[3]));
  double scale = 1.0;
  if (amax > 60.0) scale = 60.0 / amax;
  if (fabs(dx[2]) * scale > 0.5) scale = 0.5 / fabs(dx[2]);
  double xn[4], d[4];
KRL_UNROLL
  for (int i = 0; i < 4; ++i) xn[i] = st.x[i] + scale * dx[i];
  xn[0] = fmax(xn[0], 0.0);
  xn[2] = fmax(xn[2], 0.0);
  double pred = 0.0;     // what the quadratic model promises for the step actually taken
KRL_UNROLL
  for (int i = 0; i < 4; ++i) d[i] = xn[i] - st.x[i];
KRL_UNROLL
  for (int i = 0; i < 4; ++i) pred -= d[i] * (g[i] + 0.5 * (H[i][0] * d[0] + H[i][1] * d[1] + H[i][2] * d[2] + H[i][3] * d[3]));
  if (!spd || !isfinite(pred) || !(pred > PRED_TOL * st.cost)) {
    // a step that the projection bent uphill says nothing about the point: damp more, which turns it towards the projected
    // gradient.  Otherwise there is nothing left to gain from here.
    const bool bent = xn[0] != st.x[0] + scale * dx[0] || xn[2] != st.x[2] + scale * dx[2];
    st.mu *= 5.0;
    if (!spd || !isfinite(pred) || !bent || st.mu > 1e15) end_start(st);
    return;
  }
  double rn[4], Jn[4][4];
  const double cn = xn[2] < EPS_POLE ? eval(xn, st.A, rn, Jn) : INFINITY;
  ++st.nfev;
  ++st.total;
  if (cn < st.cost) {
    const double gain = (st.cost - cn) / pred;
    st.mu = gain > 0.75 ? fmax(st.mu * 0.2, 1e-15) : gain < 0.25 ? st.mu * 2.0 : st.mu;
KRL_UNROLL
    for (int i = 0; i < 4; ++i) {
      st.x[i] = xn[i];
      st.r[i] = rn[i];
KRL_UNROLL
      for (int j = 0; j < 4; ++j) st.J[i][j] = Jn[i][j];
    }
    st.cost = cn;
    settle(st);
  } else {
    st.mu *= 5.0;
  }
  if (st.cost <= COST_FLOOR || st.nfev >= st.max_nfev || st.mu > 1e15) end_start(st);
}

// theta, psi (within 90 degrees of the start's), eps, xi (within 180 degrees of the start's) and the cost
KRL_HD double result(const State& st, double* x) {
  x[0] = st.best[0];
  x[1] = st.x0[1] + remainder(st.best[1] - st.x0[1], 180.0);
  x[2] = st.best[2];
  x[3] = st.x0[3] + remainder(st.best[3] - st.x0[3], 360.0);
  return st.best_cost;
}

// A = A0 + A0 J, each element a0_ij + (a0_i0 J_0j + a0_i1 J_1j) in this order, unfused
KRL_HD void form_A(const double* a0, const double* Jm, double* A) {
  A[0] = a0[0] + (a0[0] * Jm[0] + a0[1] * Jm[2]);
  A[1] = a0[1] + (a0[0] * Jm[1] + a0[1] * Jm[3]);
  A[2] = a0[2] + (a0[2] * Jm[0] + a0[3] * Jm[2]);
  A[3] = a0[3] + (a0[2] * Jm[1] + a0[3] * Jm[3]);
}

// one pixel on the calling thread (the host check; the kernel interleaves step() across the lanes itself)
KRL_HD double solve(const double* A, const double* x0, int max_nfev, double retry_cost, double* x, int* nfev) {
  State st;
  init(st, A, x0, max_nfev, retry_cost);
  while (!finished(st)) step(st);
  if (nfev) *nfev = st.total;
  return result(st, x);
}

}  // namespace kerelsky
