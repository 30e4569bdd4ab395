// Per-pixel device arithmetic the Jacobian and property kernels share (gpa_reconstruct.hip, gpa_fieldjac.hip): phase wraps, the
// 2 x 2 normal-equation solve, and the closed-form singular value decomposition of a 2 x 2 matrix with the lattice properties
// read off it.  One copy, so that a fused kernel and the stand-alone props_kernel compute the same bits from the same J.
#pragma once
#include <hip/hip_runtime.h>

namespace gpa {

template <class T> struct Consts;
template <> struct Consts<float> {
  static constexpr float pi = 3.14159265358979323846f, two_pi = 6.28318530717958647692f;
};
template <> struct Consts<double> {
  static constexpr double pi = 3.14159265358979323846, two_pi = 6.28318530717958647692;
};

// (x + pi) mod 2 pi - pi with floored mod: [-pi, pi), +pi -> -pi (mathtools.py:72-75)
template <class T>
__device__ __forceinline__ T wrap_to_pi(T x) {
  const T t = x + Consts<T>::pi;
  return t - Consts<T>::two_pi * floor(t / Consts<T>::two_pi) - Consts<T>::pi;
}

// the same for the difference of two phases, |x| < 2 pi: floor((x + pi) / 2 pi) is -1, 0 or 1 and follows from
// two comparisons -- no division, and (like NumPy's exact float modulo) no quotient rounding at the seams
template <class T>
__device__ __forceinline__ T wrap_phase_diff(T x) {
  const T t = x + Consts<T>::pi;
  const T r = t >= Consts<T>::two_pi ? t - Consts<T>::two_pi : (t < T(0) ? t + Consts<T>::two_pi : t);
  return r - Consts<T>::pi;
}

// general argument, fast path for the usual |x| < 2 pi (same arithmetic as wrap_to_pi there)
template <class T>
__device__ __forceinline__ T wrap_to_pi_fast(T x) {
  return fabs(x) < Consts<T>::two_pi ? wrap_phase_diff(x) : wrap_to_pi(x);
}

// The symmetric 2 x 2 normal system A x = r of a per-pixel weighted least-squares problem (A = M^T M, M = diag(w) K).
// det / tr^2 is about 1 / kappa(M)^2, and the computed det carries rounding noise of up to (2 P + 11) / 4 unit round-offs of
// tr^2 (P terms per sum; 3.4 eps at P = 8).  A determinant at that level says nothing: dividing by it returned answers of
// any size.  Such a pixel is rank 1 to working precision and gets the minimum-norm answer along its dominant direction,
// r / tr, which is what LAPACK's lstsq returns for an exactly rank-deficient pixel; tr = 0 (every weight 0) gives 0.
// The test is det > 4 eps tr^2 in both precisions: 4 is the smallest power of two above the noise bound.  Measured with the
// NumPy emulation of tools/lstsq_threshold.py (8 k-vector sets, P = 2 ... 8, 200 000 pixels each): with weights (1, r, r),
// r = 1e-4 ... 1e-7, in f32 the answer stays within 1.000 of max(|x_lapack|, |x_rank1|) for every multiple from 2 eps on (1.2
// at 1 eps); exactly rank-1 pixels are within 0.07 of their rounding bound from 1 eps on in both precisions.  The constants
// used before, 1e-12 (f32) and 1e-28 (f64), lie below the noise: 13.9 times LAPACK's size at r = 1e-4 in f32, and answers
// unrelated to LAPACK's on exactly rank-1 pixels in both precisions.  An f32 solve therefore keeps only the dominant direction
// from kappa = 1 / sqrt(4 eps) = 1450 on, an f64 solve from 3.4e7 on ("Conditioning").
template <class T>
__device__ __forceinline__ void solve2(T a00, T a01, T a11, T r0, T r1, T& x0, T& x1) {
  const T det = a00 * a11 - a01 * a01, tr = a00 + a11;
  const T tiny = sizeof(T) == 4 ? T(4.76837158203125e-7) : T(8.8817841970012523e-16);   // 4 eps: 2^-21, 2^-50
  if (det > tiny * tr * tr) {
    const T inv = T(1) / det;
    x0 = (a11 * r0 - a01 * r1) * inv;
    x1 = (a00 * r1 - a01 * r0) * inv;
  } else if (tr > T(0)) {
    x0 = r0 / tr;
    x1 = r1 / tr;
  } else {
    x0 = T(0);
    x1 = T(0);
  }
}

// one pixel's 2 x 2 matrix, row-major: J[., ., 0, 0], [0, 1], [1, 0], [1, 1]
template <class T> struct alignas(4 * sizeof(T)) Quad { T a, b, c, d; };

// Closed-form SVD of the 2 x 2 matrix j + ident I.  The reference takes a LAPACK SVD and normalises the signs of U
// (property_extract.py:163-169); for a 2 x 2 matrix the same quantities follow from
//   E,H = (a+d)/2, (c-b)/2   (rotation part),   F,G = (a-d)/2, (c+b)/2   (shear part):
//   s0,s1 = Q+R, |Q-R| with Q=|(E,H)|, R=|(F,G)|; U = rot((atan2(H,E)+atan2(G,F))/2);
//   U V^T = rot(atan2(H,E)) for det>0 and the reflection of angle -atan2(G,F) for det<0.
// s0 and s1 are those of the matrix divided by m, its largest entry: the squares must not leave the range of T.
template <class T> struct Svd2 { T m, s0, s1, angle, ani; };   // angles in degrees, ani before the diffraction turn and the mod

template <class T>
__device__ __forceinline__ Svd2<T> svd2_closed(const Quad<T>& j, T ident) {
  T a = j.a + ident, b = j.b, c = j.c, d = j.d + ident;
  const T m = fmax(fmax(fabs(a), fabs(b)), fmax(fabs(c), fabs(d)));
  const T im = m > T(0) ? T(1) / m : T(0);
  a *= im; b *= im; c *= im; d *= im;
  const T E = T(0.5) * (a + d), F = T(0.5) * (a - d), G = T(0.5) * (c + b), H = T(0.5) * (c - b);
  const T Q = sqrt(E * E + H * H), R = sqrt(F * F + G * G);
  const T a1 = atan2(G, F), a2 = atan2(H, E);
  const T deg = T(180) / Consts<T>::pi;
  Svd2<T> s;
  s.m = m;
  s.s0 = Q + R;
  s.s1 = fabs(Q - R);
  s.angle = (Q >= R ? a2 : -a1) * deg;
  s.ani = T(-0.5) * (a1 + a2) * deg;
  return s;
}

// (angle + refangle, aniangle, alpha refscale, kappa): props_from_Jac (property_extract.py:137-178)
template <class T>
__device__ __forceinline__ void lattice_props(const Quad<T>& j, T ident, T refangle, T refscale, int diff, T out[4]) {
  const Svd2<T> s = svd2_closed(j, ident);
  T ani = s.ani + (diff ? T(90) : T(0));
  ani -= T(180) * floor(ani / T(180));
  out[0] = s.angle + refangle;
  out[1] = ani;
  out[2] = (diff ? s.s0 : s.s1) * s.m * refscale;
  out[3] = s.s0 / s.s1;
}

// (angle + refangle, aniangle, alpha refscale, epsilon): phys_props_from_Jac (property_extract.py:181-217), delta the Poisson ratio
template <class T>
__device__ __forceinline__ void lattice_phys_props(const Quad<T>& j, T ident, T refangle, T refscale, int diff, T delta, T out[4]) {
  const Svd2<T> s = svd2_closed(j, ident);
  T ani = s.ani + (diff ? T(90) : T(0));
  ani -= T(180) * floor(ani / T(180));
  const T eps = (s.s0 - s.s1) / (s.s0 + delta * s.s1);   // a ratio of singular values: the scale m cancels
  const T alpha = diff ? s.s0 / (T(1) + eps) : s.s1 * (T(1) + eps);
  out[0] = s.angle + refangle;
  out[1] = ani;
  out[2] = alpha * s.m * refscale;
  out[3] = eps;
}

// Hands a value on unchanged but opaque to the optimiser: what is computed from the result cannot be contracted (fused
// multiply-add) with the operation that produced the argument.  The fused kernels pass J through it between its solve and
// the properties, so that these start from the rounded J that is stored, as props_kernel does when it loads it.
template <class T>
__device__ __forceinline__ T rounded(T x) {
  asm volatile("" : "+v"(x));
  return x;
}

}  // namespace gpa
