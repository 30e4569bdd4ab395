// Per-pixel Kerelsky fits on the device: one pixel per lane, the solver of gpa_kerelsky.h in registers, no LDS.
//
// The solve is the state machine of gpa_kerelsky.h advanced one trial evaluation per trip of a single loop.  The loop runs while
// any lane of the wave is unfinished and finished lanes are masked; a lane in its second start executes the same instructions
// as a lane in its first, so the trips of a wave are those of its slowest pixel and not the sum over the starts in use.
// A workgroup is ONE wave: a wave that is done gives its registers back without waiting for three others, which matters because
// the trip count varies between waves (rough fields) and the register budget, not the memory system, bounds this kernel.
//
// This file is compiled with -ffp-contract=off (build.py): the host check of gpa_kerelsky.h is compiled the same way, so both
// perform one sequence of rounded operations and differ only in the sincos / atan2 of their maths libraries, and
// A = A0 + A0 J is formed with the roundings of the element-wise NumPy expression the callers and tests use.
#include "gpa_internal.h"
#include "gpa_kerelsky.h"

namespace gpa {

namespace {

template <class T>
struct alignas(4 * sizeof(T)) Quad4 { T v[4]; };

template <class T>
__global__ __launch_bounds__(64) void kerelsky_kernel(const Quad4<T>* __restrict__ jac, size_t npx, KerelskyArgs p,
                                                      Quad4<T>* __restrict__ out, double* __restrict__ cost) {
  const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= npx) return;
  const Quad4<T> q = jac[i];
  const double Jm[4] = {(double)q.v[0], (double)q.v[1], (double)q.v[2], (double)q.v[3]};
  double A[4];
  if (p.has_a0) kerelsky::form_A(p.a0, Jm, A);
  else
    for (int j = 0; j < 4; ++j) A[j] = Jm[j];
  kerelsky::State st;
  kerelsky::init(st, A, p.x0, p.max_nfev, p.retry_cost);
  while (!kerelsky::finished(st)) kerelsky::step(st);
  double x[4];
  const double c = kerelsky::result(st, x);
  Quad4<T> o;
  for (int j = 0; j < 4; ++j) o.v[j] = (T)x[j];
  out[i] = o;
  if (cost) cost[i] = c;
}

}  // namespace

hipError_t launch_kerelsky(int dtype, const void* jac, size_t npx, const KerelskyArgs& p, void* out, double* cost, hipStream_t s) {
  const unsigned grid = (unsigned)((npx + 63) / 64);
  GPA_PROF("kerelsky_kernel", s);
  if (dtype == 0) kerelsky_kernel<float><<<grid, 64, 0, s>>>((const Quad4<float>*)jac, npx, p, (Quad4<float>*)out, cost);
  else kerelsky_kernel<double><<<grid, 64, 0, s>>>((const Quad4<double>*)jac, npx, p, (Quad4<double>*)out, cost);
  return hipGetLastError();
}

}  // namespace gpa
