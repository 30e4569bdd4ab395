// C ABI, a5-a7: phases / weights / per-pixel least squares and the weighted unwrap
// (geometric_phase_analysis.py:97-113, :196-245, :922-926; phase_unwrap.py:141-350).
#include "gpa_plan.h"
#include "gpa_unwrap_batch.h"

// ---- a5/a6 -------------------------------------------------------------------
int gpa_reconstruct_grad_dev(gpa_plan* p, const void* lockin, const double* kvecs, int P, int mask_border,
                             void* dudx, void* dudy, void* wnorm) {
  if (!p || !lockin || !kvecs || !dudx || !dudy) return fail(GPA_ERR_ARG, "gpa_reconstruct_grad: null argument");
  if (P < 2 || P > p->max_peaks) return fail(GPA_ERR_STATE, "gpa_reconstruct_grad: need 2 <= P <= 8");
  HIP_TRY(hipSetDevice(p->device));
  TRY(stage_kmat(p, kvecs, P));
  HIP_TRY(launch_reconstruct(p->dtype, lockin, p->d_kmat, P, p->n0, p->n1, mask_border, dudx, dudy, wnorm,
                             p->stream));
  return GPA_OK;
}

int gpa_reconstruct_grad(gpa_plan* p, const void* lockin, const double* kvecs, int P, int mask_border,
                         void* dudx, void* dudy, void* wnorm) {
  if (!p || !lockin || !kvecs || !dudx || !dudy) return fail(GPA_ERR_ARG, "gpa_reconstruct_grad: null argument");
  if (P < 2 || P > p->max_peaks) return fail(GPA_ERR_STATE, "gpa_reconstruct_grad: need 2 <= P <= 8");
  HIP_TRY(hipSetDevice(p->device));
  const size_t npx = (size_t)p->n0 * p->n1;
  HIP_TRY(hipMemcpyAsync(p->d_lockin, lockin, (size_t)P * npx * p->csz, hipMemcpyHostToDevice, p->stream));
  TRY(gpa_reconstruct_grad_dev(p, p->d_lockin, kvecs, P, mask_border, p->d_dudx, p->d_dudy, p->d_wnorm));
  HIP_TRY(hipMemcpyAsync(dudx, p->d_dudx, (size_t)2 * p->n0 * (p->n1 - 1) * p->rsz, hipMemcpyDeviceToHost, p->stream));
  HIP_TRY(hipMemcpyAsync(dudy, p->d_dudy, (size_t)2 * (p->n0 - 1) * p->n1 * p->rsz, hipMemcpyDeviceToHost, p->stream));
  if (wnorm) HIP_TRY(hipMemcpyAsync(wnorm, p->d_wnorm, npx * p->rsz, hipMemcpyDeviceToHost, p->stream));
  HIP_TRY(hipStreamSynchronize(p->stream));
  return GPA_OK;
}

// reconstruct_u_inv_from_phases(pre_diff=True) (geometric_phase_analysis.py:228-237): the phase gradients are given
int gpa_reconstruct_prediff(gpa_plan* p, const void* grads, const void* weights, const double* kvecs, int P, void* dudx,
                            void* dudy, void* wnorm) {
  if (!p || !grads || !weights || !kvecs || !dudx || !dudy) return fail(GPA_ERR_ARG, "gpa_reconstruct_prediff: null argument");
  if (P < 2 || P > p->max_peaks) return fail(GPA_ERR_STATE, "gpa_reconstruct_prediff: need 2 <= P <= 8 (and P <= max_batch)");
  HIP_TRY(hipSetDevice(p->device));
  const size_t npx = (size_t)p->n0 * p->n1;
  TRY(ensure_tbuf(p, (P + 1) / 2));
  // staging: grads (P x npx x 2 reals = P complex planes) in d_lockin, weights in Tbuf
  HIP_TRY(hipMemcpyAsync(p->d_lockin, grads, (size_t)P * npx * 2 * p->rsz, hipMemcpyHostToDevice, p->stream));
  HIP_TRY(hipMemcpyAsync(p->Tbuf.ptr, weights, (size_t)P * npx * p->rsz, hipMemcpyHostToDevice, p->stream));
  TRY(stage_kmat(p, kvecs, P));
  HIP_TRY(launch_prediff(p->dtype, p->d_lockin, p->Tbuf.ptr, p->d_kmat, P, p->n0, p->n1, p->d_dudx, p->d_dudy, p->d_wnorm,
                         p->stream));
  HIP_TRY(hipMemcpyAsync(dudx, p->d_dudx, (size_t)2 * p->n0 * (p->n1 - 1) * p->rsz, hipMemcpyDeviceToHost, p->stream));
  HIP_TRY(hipMemcpyAsync(dudy, p->d_dudy, (size_t)2 * (p->n0 - 1) * p->n1 * p->rsz, hipMemcpyDeviceToHost, p->stream));
  if (wnorm) HIP_TRY(hipMemcpyAsync(wnorm, p->d_wnorm, npx * p->rsz, hipMemcpyDeviceToHost, p->stream));
  HIP_TRY(hipStreamSynchronize(p->stream));
  return GPA_OK;
}

int gpa_weighted_lstsq(gpa_plan* p, const void* b, const void* weights, const double* kvecs, int P, void* out) {
  if (!p || !b || !weights || !kvecs || !out) return fail(GPA_ERR_ARG, "gpa_weighted_lstsq: null argument");
  if (P < 2 || P > p->max_peaks) return fail(GPA_ERR_STATE, "gpa_weighted_lstsq: need 2 <= P <= 8 (and P <= max_batch)");
  HIP_TRY(hipSetDevice(p->device));
  const size_t npx = (size_t)p->n0 * p->n1;
  // staging: b in d_lockin (P complex planes hold 2P real ones), weights in Tbuf
  TRY(ensure_tbuf(p, (P + 1) / 2));
  HIP_TRY(hipMemcpyAsync(p->d_lockin, b, (size_t)P * npx * p->rsz, hipMemcpyHostToDevice, p->stream));
  HIP_TRY(hipMemcpyAsync(p->Tbuf.ptr, weights, (size_t)P * npx * p->rsz, hipMemcpyHostToDevice, p->stream));
  TRY(stage_kmat(p, kvecs, P));
  HIP_TRY(launch_wlstsq(p->dtype, p->d_lockin, p->Tbuf.ptr, p->d_kmat, P, npx, p->d_u, p->stream));
  HIP_TRY(hipMemcpyAsync(out, p->d_u, 2 * npx * p->rsz, hipMemcpyDeviceToHost, p->stream));
  HIP_TRY(hipStreamSynchronize(p->stream));
  return GPA_OK;
}

// ---- a7 ----------------------------------------------------------------------
int gpa_unwrap_prediff_dev(gpa_plan* p, const void* dx, const void* dy, const void* weight, int kmax,
                           double eps, int compat, void* phi, int* iters_out) {
  if (!p || !dx || !dy || !phi) return fail(GPA_ERR_ARG, "gpa_unwrap_prediff: null argument");
  if (kmax < 1) return fail(GPA_ERR_ARG, "gpa_unwrap_prediff: kmax must be >= 1");
  NEED_UNWRAP(p, "gpa_unwrap_prediff");
  HIP_TRY(hipSetDevice(p->device));
  int iters = 0;
  ProfInstall prof(p);   // (gpa_set_profiling: per-kernel times of this solve through gpa_last_kernel_profile)
  hipError_t e = unwrap_run(&p->uw, dx, dy, weight, false, kmax, eps, compat != 0, phi, &iters, p->stream);
  if (e != hipSuccess) return unwrap_fail(e);
  if (p->profiling) collect_kernel_profile(p);
  if (iters_out) *iters_out = iters;
  return GPA_OK;
}

int gpa_unwrap_prediff_enqueue_dev(gpa_plan* p, const void* dx, const void* dy, const void* weight, int kmax, double eps,
                                   int compat, void* phi) {
  if (!p || !dx || !dy || !phi) return fail(GPA_ERR_ARG, "gpa_unwrap_prediff_enqueue: null argument");
  if (kmax < 1) return fail(GPA_ERR_ARG, "gpa_unwrap_prediff_enqueue: kmax must be >= 1");
  NEED_UNWRAP(p, "gpa_unwrap_prediff_enqueue");
  HIP_TRY(hipSetDevice(p->device));
  hipError_t e = unwrap_enqueue(&p->uw, dx, dy, weight, false, kmax, eps, compat != 0, phi, p->stream);
  if (e != hipSuccess) return unwrap_fail(e);
  return GPA_OK;
}

int gpa_unwrap_finish(gpa_plan* p, int* iters_out) {
  if (!p) return fail(GPA_ERR_ARG, "gpa_unwrap_finish: null plan");
  NEED_UNWRAP(p, "gpa_unwrap_finish");
  HIP_TRY(hipSetDevice(p->device));
  int iters = 0;
  hipError_t e = unwrap_finish(&p->uw, &iters, p->stream);
  if (e != hipSuccess) return unwrap_fail(e);
  if (iters_out) *iters_out = iters;
  return GPA_OK;
}

int gpa_unwrap_prediff(gpa_plan* p, const void* dx, const void* dy, const void* weight, int kmax, double eps,
                       int compat, void* phi, int* iters_out) {
  if (!p || !dx || !dy || !phi) return fail(GPA_ERR_ARG, "gpa_unwrap_prediff: null argument");
  HIP_TRY(hipSetDevice(p->device));
  const size_t npx = (size_t)p->n0 * p->n1;
  const size_t nx = (size_t)p->n0 * (p->n1 - 1), ny = (size_t)(p->n0 - 1) * p->n1;
  HIP_TRY(hipMemcpyAsync(p->d_dudx, dx, nx * p->rsz, hipMemcpyHostToDevice, p->stream));
  HIP_TRY(hipMemcpyAsync(p->d_dudy, dy, ny * p->rsz, hipMemcpyHostToDevice, p->stream));
  if (weight) HIP_TRY(hipMemcpyAsync(p->d_wnorm, weight, npx * p->rsz, hipMemcpyHostToDevice, p->stream));
  TRY(gpa_unwrap_prediff_dev(p, p->d_dudx, p->d_dudy, weight ? p->d_wnorm : nullptr, kmax, eps, compat, p->d_u,
                             iters_out));
  HIP_TRY(hipMemcpyAsync(phi, p->d_u, npx * p->rsz, hipMemcpyDeviceToHost, p->stream));
  HIP_TRY(hipStreamSynchronize(p->stream));
  return GPA_OK;
}

int gpa_unwrap_dev(gpa_plan* p, const void* psi, const void* weight, int kmax, double eps, int compat, void* phi,
                   int* iters_out) {
  if (!p || !psi || !phi) return fail(GPA_ERR_ARG, "gpa_unwrap: null argument");
  if (kmax < 1) return fail(GPA_ERR_ARG, "gpa_unwrap: kmax must be >= 1");
  NEED_UNWRAP(p, "gpa_unwrap");
  HIP_TRY(hipSetDevice(p->device));
  int iters = 0;
  ProfInstall prof(p);   // (as gpa_unwrap_prediff_dev)
  hipError_t e = unwrap_run(&p->uw, psi, nullptr, weight, true, kmax, eps, compat != 0, phi, &iters, p->stream);
  if (e != hipSuccess) return unwrap_fail(e);
  if (p->profiling) collect_kernel_profile(p);
  if (iters_out) *iters_out = iters;
  return GPA_OK;
}

int gpa_unwrap(gpa_plan* p, const void* psi, const void* weight, int kmax, double eps, int compat, void* phi,
               int* iters_out) {
  if (!p || !psi || !phi) return fail(GPA_ERR_ARG, "gpa_unwrap: null argument");
  if (kmax < 1) return fail(GPA_ERR_ARG, "gpa_unwrap: kmax must be >= 1");
  NEED_UNWRAP(p, "gpa_unwrap");
  HIP_TRY(hipSetDevice(p->device));
  const size_t npx = (size_t)p->n0 * p->n1;
  HIP_TRY(hipMemcpyAsync(p->d_image, psi, npx * p->rsz, hipMemcpyHostToDevice, p->stream));
  if (weight) HIP_TRY(hipMemcpyAsync(p->d_wnorm, weight, npx * p->rsz, hipMemcpyHostToDevice, p->stream));
  TRY(gpa_unwrap_dev(p, p->d_image, weight ? p->d_wnorm : nullptr, kmax, eps, compat, p->d_u, iters_out));
  HIP_TRY(hipMemcpyAsync(phi, p->d_u, npx * p->rsz, hipMemcpyDeviceToHost, p->stream));
  HIP_TRY(hipStreamSynchronize(p->stream));
  return GPA_OK;
}

// ---- a7, a stack of phase maps in one call -----------------------------------------
// nb weighted unwraps of one shape as ONE set of launches per chunk (blockIdx.z = problem) on the plan's batched workspace
// (gpa_plan::uwb, shared with the batched driver).  A small frame is bound by its chain of 4 - 5 dependent launches per PCG
// iteration, not by their work; the stack shares the chain.  Problem b's phi and count are those of the
// single call on its planes under the same kernels, bit for bit.
namespace {

size_t unwrap_stack_budget() {
  size_t budget = (size_t)2 << 30;   // UNWRAP_STACK_BYTES: another bound, for tests
  if (opt_set(OPT_UNWRAP_STACK_BYTES) && opt(OPT_UNWRAP_STACK_BYTES).num >= 1.0) budget = (size_t)opt(OPT_UNWRAP_STACK_BYTES).num;
  return budget;
}

bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const char *a0 = (const char*)a, *b0 = (const char*)b;
  return a && b && a0 < b0 + nb && b0 < a0 + na;
}

struct StackShape { size_t npx, astride, bstride; };   // samples per plane of phi / weight, of a (psi or dx), of b (dy)
StackShape stack_shape(const gpa_plan* p, bool from_psi) {
  const size_t n0 = p->n0, n1 = p->n1;
  return {n0 * n1, from_psi ? n0 * n1 : n0 * (n1 - 1), (n0 - 1) * n1};
}

// every argument error, before anything is launched; then the plan's ability
int stack_check(gpa_plan* p, const std::string& fn, const void* a, const void* b, bool from_psi, int nb, const void* weight,
                int weight_planes, int kmax, const void* phi) {
  if (!p) return fail(GPA_ERR_ARG, fn + ": plan is null");
  if (nb < 1 || nb > GPA_UNWRAP_BATCH_MAX)
    return fail(GPA_ERR_ARG, fn + ": nb must be 1 ... " + std::to_string(GPA_UNWRAP_BATCH_MAX) + " (got " + std::to_string(nb) + ")");
  if (!a) return fail(GPA_ERR_ARG, fn + (from_psi ? ": psi is null" : ": dx is null"));
  if (!from_psi && !b) return fail(GPA_ERR_ARG, fn + ": dy is null");
  if (!phi) return fail(GPA_ERR_ARG, fn + ": phi is null");
  if (weight_planes != 0 && weight_planes != 1 && weight_planes != nb)
    return fail(GPA_ERR_ARG, fn + ": weight_planes must be 0, 1 or nb (got " + std::to_string(weight_planes) + ")");
  if (weight && weight_planes == 0) return fail(GPA_ERR_ARG, fn + ": weight must be null when weight_planes is 0");
  if (!weight && weight_planes != 0) return fail(GPA_ERR_ARG, fn + ": weight is null but weight_planes is not 0");
  if (kmax < 1) return fail(GPA_ERR_ARG, fn + ": kmax must be >= 1");
  const StackShape sh = stack_shape(p, from_psi);
  const size_t rsz = p->rsz, phib = (size_t)nb * sh.npx * rsz;
  if (ranges_overlap(phi, phib, a, (size_t)nb * sh.astride * rsz))
    return fail(GPA_ERR_ARG, fn + (from_psi ? ": phi overlaps psi" : ": phi overlaps dx"));
  if (!from_psi && ranges_overlap(phi, phib, b, (size_t)nb * sh.bstride * rsz)) return fail(GPA_ERR_ARG, fn + ": phi overlaps dy");
  if (ranges_overlap(phi, phib, weight, (size_t)weight_planes * sh.npx * rsz)) return fail(GPA_ERR_ARG, fn + ": phi overlaps weight");
  NEED_UNWRAP(p, fn);
  if (!unwrap_supports_batch(&p->uw))
    return fail(GPA_ERR_STATE, fn + ": this image shape has no batched unwrap (its solve runs the plain Bluestein scheme, not the "
                                    "fused iteration, the only one that takes several problems per launch); loop over the single call");
  return GPA_OK;
}

// problems per set of launches of a call of nb
int stack_chunk(const gpa_plan* p, int nb, int kmax) {
  const int fit = unwrap_batch_chunk((size_t)p->n0 * p->n1, p->rsz, unwrap_ring_for(kmax), unwrap_problem_fixed_bytes(&p->uw),
                                     unwrap_stack_budget());
  return std::min(nb, fit);
}

// problems c0 .. c0 + n - 1 of a call of nb_call: one set of launches, their flag words to the plan's pinned counts.
// a, b, weight, phi: the device planes of problem c0.
int stack_enqueue(gpa_plan* p, const std::string& fn, const void* a, const void* b, const void* weight, bool own_weights,
                  bool from_psi, int c0, int n, int nb_call, int kmax, double eps, int compat, void* phi) {
  TRY(ensure_unwrap_problems(p, n, fn.c_str()));
  HIP_TRY(p->h_iters_b.reserve((size_t)4 * nb_call * sizeof(int), p->stream));
  hipError_t e = unwrap_enqueue_stack(&p->uwb, a, b, weight, own_weights, from_psi, nb_call, kmax, eps, compat != 0, phi, p->stream);
  if (e == hipSuccess) e = unwrap_fetch_flags(&p->uwb, p->h_iters_b.as<int>() + (size_t)4 * c0, p->stream);
  p->uwb_bytes = p->uwb_base_bytes + unwrap_ring_bytes(&p->uwb);
  if (e != hipSuccess) return unwrap_fail(e);
  return GPA_OK;
}

int stack_counts(gpa_plan* p, int nb, int* iters_out) {
  HIP_TRY(hipStreamSynchronize(p->stream));
  const int slot = unwrap_iters_slot(&p->uwb);
  for (int j = 0; j < nb; ++j) iters_out[j] = p->h_iters_b.as<int>()[4 * j + slot];
  return GPA_OK;
}

int stack_dev(gpa_plan* p, const char* fn, const void* a, const void* b, bool from_psi, int nb, const void* weight,
              int weight_planes, int kmax, double eps, int compat, void* phi, int* iters_out) {
  TRY(stack_check(p, fn, a, b, from_psi, nb, weight, weight_planes, kmax, phi));
  HIP_TRY(hipSetDevice(p->device));
  const StackShape sh = stack_shape(p, from_psi);
  const size_t rsz = p->rsz;
  const bool own = weight && weight_planes == nb && nb > 1;
  const int chunk = stack_chunk(p, nb, kmax);
  ProfInstallIf prof(p, iters_out != nullptr);   // (per-kernel times need the wait at the end)
  p->uwb_last_nb = 0;
  for (int c0 = 0; c0 < nb; c0 += chunk) {
    const int n = std::min(chunk, nb - c0);
    TRY(stack_enqueue(p, fn, (const char*)a + (size_t)c0 * sh.astride * rsz, b ? (const char*)b + (size_t)c0 * sh.bstride * rsz : nullptr,
                      own ? (const char*)weight + (size_t)c0 * sh.npx * rsz : (const char*)weight, own, from_psi, c0, n, nb, kmax, eps,
                      compat, (char*)phi + (size_t)c0 * sh.npx * rsz));
  }
  p->uwb_last_nb = nb;
  if (!iters_out) return GPA_OK;
  TRY(stack_counts(p, nb, iters_out));
  if (prof.own) collect_kernel_profile(p);
  return GPA_OK;
}

// host pointers: one chunk at a time through the plan's shared staging buffer (psi or dx | dy | weights | phi)
int stack_host(gpa_plan* p, const char* fn, const void* a, const void* b, bool from_psi, int nb, const void* weight,
               int weight_planes, int kmax, double eps, int compat, void* phi, int* iters_out) {
  TRY(stack_check(p, fn, a, b, from_psi, nb, weight, weight_planes, kmax, phi));
  HIP_TRY(hipSetDevice(p->device));
  const StackShape sh = stack_shape(p, from_psi);
  const size_t rsz = p->rsz;
  const bool own = weight && weight_planes == nb && nb > 1;
  const int chunk = stack_chunk(p, nb, kmax);
  p->uwb_last_nb = 0;
  for (int c0 = 0; c0 < nb; c0 += chunk) {
    const int n = std::min(chunk, nb - c0);
    HostStage st(p->host_stage, p->stream);
    const int ia = st.in((const char*)a + (size_t)c0 * sh.astride * rsz, (size_t)n * sh.astride * rsz);
    const int ib = st.in(b ? (const char*)b + (size_t)c0 * sh.bstride * rsz : nullptr, (size_t)n * sh.bstride * rsz);
    const int iw = st.in(own ? (const char*)weight + (size_t)c0 * sh.npx * rsz : (const char*)weight, (size_t)(own ? n : 1) * sh.npx * rsz);
    const int io = st.out((char*)phi + (size_t)c0 * sh.npx * rsz, (size_t)n * sh.npx * rsz);
    HIP_TRY(st.upload());
    TRY(stack_enqueue(p, fn, st.dev(ia), st.dev(ib), st.dev(iw), own, from_psi, c0, n, nb, kmax, eps, compat, st.dev(io)));
    HIP_TRY(st.download());   // (drains the stream: the next chunk may overwrite the staging buffer)
  }
  p->uwb_last_nb = nb;
  return iters_out ? stack_counts(p, nb, iters_out) : GPA_OK;
}

}  // namespace

int gpa_unwrap_batch_dev(gpa_plan* p, const void* psi, int nb, const void* weight, int weight_planes, int kmax, double eps,
                         int compat, void* phi, int* iters_out) {
  return stack_dev(p, "gpa_unwrap_batch_dev", psi, nullptr, true, nb, weight, weight_planes, kmax, eps, compat, phi, iters_out);
}

int gpa_unwrap_prediff_batch_dev(gpa_plan* p, const void* dx, const void* dy, int nb, const void* weight, int weight_planes,
                                 int kmax, double eps, int compat, void* phi, int* iters_out) {
  return stack_dev(p, "gpa_unwrap_prediff_batch_dev", dx, dy, false, nb, weight, weight_planes, kmax, eps, compat, phi, iters_out);
}

int gpa_unwrap_batch(gpa_plan* p, const void* psi, int nb, const void* weight, int weight_planes, int kmax, double eps,
                     int compat, void* phi, int* iters_out) {
  return stack_host(p, "gpa_unwrap_batch", psi, nullptr, true, nb, weight, weight_planes, kmax, eps, compat, phi, iters_out);
}

int gpa_unwrap_prediff_batch(gpa_plan* p, const void* dx, const void* dy, int nb, const void* weight, int weight_planes, int kmax,
                             double eps, int compat, void* phi, int* iters_out) {
  return stack_host(p, "gpa_unwrap_prediff_batch", dx, dy, false, nb, weight, weight_planes, kmax, eps, compat, phi, iters_out);
}

int gpa_unwrap_batch_finish(gpa_plan* p, int nb, int* iters_out) {
  if (!p) return fail(GPA_ERR_ARG, "gpa_unwrap_batch_finish: plan is null");
  if (!iters_out) return fail(GPA_ERR_ARG, "gpa_unwrap_batch_finish: iters_out is null");
  if (nb < 1 || nb > p->uwb_last_nb)
    return fail(GPA_ERR_ARG, "gpa_unwrap_batch_finish: nb must be 1 ... the problems of the last batch call (" +
                                 std::to_string(p->uwb_last_nb) + ")");
  HIP_TRY(hipSetDevice(p->device));
  return stack_counts(p, nb, iters_out);
}

size_t gpa_unwrap_batch_problem_bytes(gpa_plan* p, int kmax) {
  if (!p || !p->uw.impl) return 0;
  return unwrap_problem_bytes((size_t)p->n0 * p->n1, p->rsz, unwrap_ring_for(kmax), unwrap_problem_fixed_bytes(&p->uw));
}
