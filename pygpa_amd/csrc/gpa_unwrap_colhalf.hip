// a7, column half of the preconditioner z = idctn(dctn(r) / eig) (phase_unwrap.py:95-115) for columns whose packed-pair
// transform does not fit LDS (f64 columns of 16384 points beside a shorter row axis; square images take the transform-free
// solves): one column per workgroup through one complex transform of half the column length (gpa_unwrap_colhalf.h).
// A workgroup touches 8 bytes of every row: the kernel is there so that the shape limit is one line, not for its speed.
#include "gpa_unwrap_colhalf.h"
#include "gpa_unwrap_impl.h"

namespace gpa {
namespace {

// same contract as colsolve_kernel (gpa_unwrap_cols.hip): arguments, flags / scal protocol and stopping test, partial sums,
// Zin, blockIdx.z = problem.  twtab: twiddles of length N/2; wspec / ha / ham: the natural-order tables of gpa_unwrap_colhalf.h
template <class T, int LG>
__global__ __launch_bounds__((ColHalf<T, LG>::THREADS)) void colsolve_half_kernel(T* __restrict__ Z, int n1,
                                                                               const cpx<T>* __restrict__ twtab,
                                                                               const cpx<T>* __restrict__ wspec,
                                                                               const T* __restrict__ ha,
                                                                               const T* __restrict__ ham,
                                                                               const T* __restrict__ hb, int* flags,
                                                                               const double* part_norm, int nnorm, int it,
                                                                               double eps, double* scal, double* part_rho,
                                                                               const T* __restrict__ Zin, size_t pimg) {
  {
    const size_t pb = blockIdx.z;
    Z += pb * pimg;
    if (Zin) Zin += pb * pimg;
    flags += pb * FLAGS_N;
    scal += pb * SCAL_N;
    part_norm += pb * PART_N;
    part_rho += pb * PART_N;
  }
  using G = ColHalf<T, LG>;
  using F = typename G::F;
  constexpr int E = G::E, TPF = G::TPF, N = G::N;
  if (flags[1]) return;
  const T* Zsrc = Zin ? Zin : Z;   // fused path: reads the kept row spectrum of r, writes the solve to Z
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ double shn[ColHalf<T, LG>::THREADS];
  cpx<T>* lds = reinterpret_cast<cpx<T>*>(smem);
  const int tid = threadIdx.x;
  // XCD-aware order (see passA_kernel): neighbouring columns, which share their cache lines, meet in one L2
  const int y = xcd_tile(blockIdx.x, gridDim.x);   // gridDim.x == n1
  // (the base twiddles are fetched from the table where a butterfly needs them: kept in registers, the three twiddled passes'
  //  36 complex doubles cost another 190 bytes of scratch per lane)
  typename F::TwiddlesMem tw;
  F::load_twiddles(tw, twtab, tid);
  cpx<T> x[E];
#pragma unroll
  for (int i = 0; i < E; ++i) {
    const int n = tid + TPF * i;
    x[i] = {Zsrc[(size_t)G::row_re(n) * n1 + y], Zsrc[(size_t)G::row_im(n) * n1 + y]};
  }
  if (it > 0) {
    // fused path: the update of iteration it-1 was applied by this iteration's row kernel; every workgroup evaluates the
    // reference's stopping test (phase_unwrap.py:348) on it
    const double tot = reduce_partials(part_norm, nnorm, shn);
    const double best = scal[10 + ((it - 1) & 1)], norm0 = scal[5];
    double stall;
    const bool stop = sqrt(tot) < eps * sqrt(norm0) || tot == 0.0 || pcg_breakdown(tot, best, norm0, sizeof(T) == 4, scal[SC_STALL + ((it - 1) & 1)], &stall, scal[SC_STALL_LIMIT]);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      flags[0] = it;                                   // updates completed
      scal[6] = tot;
      scal[10 + (it & 1)] = tot < best ? tot : best;
      scal[SC_STALL + (it & 1)] = stall;
      if (stop) flags[1] = 1;
    }
    if (stop) return;
  }
  F::forward(x, lds, tid, tw);
  __syncthreads();
  G::scatter(x, lds, tid);
  __syncthreads();
  // (each phase works from its own opaque copy of the thread index: hipcc otherwise computes the table and LDS addresses of
  //  every later phase ahead of the first transform and spills them)
  auto fresh = [](int t) { asm volatile("" : "+v"(t)); return t; };
  double rho = 0.0;
  G::solve(x, lds, fresh(tid), wspec, ha, ham, hb[y], y == 0, &rho);
  __syncthreads();
  G::park(x, lds, tid);
  __syncthreads();
  G::merge(x, lds, fresh(tid), wspec);
  __syncthreads();
  F::forward(x, lds, fresh(tid), tw);
  __syncthreads();
  G::inv_scatter(x, lds, fresh(tid));
  __syncthreads();
  // the store addresses equal the load addresses: recomputed from an opaque copy of the thread index so that the compiler
  // does not keep 32 64-bit addresses alive (or spilled) across the transforms
  int ts = tid;
  asm volatile("" : "+v"(ts));
#pragma unroll
  for (int i = 0; i < E; ++i) {
    const int n = ts + TPF * i;
    const cpx<T> v = lds[F::pad(n)];
    Z[(size_t)G::row_re(n) * n1 + y] = v.x;
    Z[(size_t)G::row_im(n) * n1 + y] = v.y;
  }
  // <r, z> = sum_j c_j / (2 n1) * (1 / 2N) sum_k c_k X_k Y_k, c_0 = 1/2 (SciPy's unnormalised DCT-II on both axes)
  const double tot = block_sum(rho, shn);
  if (threadIdx.x == 0) part_rho[blockIdx.x] = (y == 0 ? 0.5 : 1.0) * tot / (2.0 * (double)N) / (2.0 * (double)n1);
}

template <class T, int LG>
hipError_t run_colsolve_half(const Impl* w, int compat, hipStream_t s, const double* part_norm, int nnorm, int it, double eps,
                             double* part_rho, int* nrho, const void* zin) {
  using G = ColHalf<T, LG>;
  static_assert(G::FITS, "the half-length column transform must fit LDS");
  if (!part_rho) return hipErrorInvalidValue;   // (the only caller is the fused iteration)
  if (w->n1 > MAXPART) return hipErrorInvalidValue;
  auto kern = colsolve_half_kernel<T, LG>;
  static unsigned lds_set = 0;
  hipError_t e = set_dynamic_lds_once(reinterpret_cast<const void*>(kern), (int)G::LDS_BYTES, lds_set);
  if (e != hipSuccess) return e;
  if (nrho) *nrho = w->n1;
  GPA_PROF("colsolve_half_kernel", s);
  kern<<<dim3(w->n1, 1, w->nprob), G::THREADS, G::LDS_BYTES, s>>>((T*)w->z, w->n1, (const cpx<T>*)w->tw0h, (const cpx<T>*)w->wk0h,
                                                                (const T*)w->ha0h[compat], (const T*)w->ham0h[compat],
                                                                (const T*)w->hb1[compat], w->flags, part_norm, nnorm, it, eps,
                                                                w->scal, part_rho, (const T*)zin, (size_t)w->n0 * w->n1);
  return hipGetLastError();
}

}  // namespace

// f64 columns of 16384 points: the one length whose packed-pair transform (colsolve_kernel) does not fit LDS
hipError_t colhalf_colsolve(const Impl* w, int compat, hipStream_t s, const double* part_norm, int nnorm, int it, double eps,
                            double* part_rho, int* nrho, const void* zin) {
  if (w->dtype != 1 || w->lg0 != 14 || !w->wk0h) return hipErrorInvalidValue;
  return run_colsolve_half<double, 14>(w, compat, s, part_norm, nnorm, it, eps, part_rho, nrho, zin);
}

}  // namespace gpa
