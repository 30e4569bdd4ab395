// C ABI, a8: iterate_GPA (geometric_phase_analysis.py:116-154) as one call -- lock-ins, polar crop, weighted unwraps and
// Huber plane fits on device memory; the host keeps the k-vector correction (P x 2 doubles) and the stopping tests.
#include <chrono>

#include "gpa_plan.h"

// the plan's a8 scratch, at least `bytes` (grown with a stream synchronisation; counted in gpa_plan_workspace_bytes)
static int ensure_iter(gpa_plan* p, size_t bytes) { return plan_reserve(p, p->d_iter, bytes, "hipMalloc"); }

// the head of the scratch: Huber work of P planes, then their 4-double states and 10-double sums; a multiple of 256 bytes
static size_t fit_bytes(int P) {
  const size_t b = (size_t)P * (huber_batch_stride() + 14) * sizeof(double);
  return (b + 255) & ~(size_t)255;
}

// gpa_fit_plane_dev of P contiguous planes: every round is one launch pair and one readback for all planes that still move.
// p->d_iter holds at least fit_bytes(P).
static int fit_planes_run(gpa_plan* p, const void* images, int P, int max_iter, double tol, double* coef, int* iters_out) {
  TRY(plan_reserve(p, p->h_iter, (size_t)P * 14 * sizeof(double), "hipHostMalloc"));
  const int n0 = p->n0, n1 = p->n1;
  const double cx = 0.5 * (n0 - 1), cy = 0.5 * (n1 - 1), sx = 0.5 * n0, sy = 0.5 * n1;
  const size_t stride = huber_batch_stride();
  double* work = p->d_iter.as<double>();
  double* d_state = work + (size_t)P * stride;
  double* d_sums = d_state + (size_t)4 * P;
  double* h_state = p->h_iter.as<double>();
  double* h_sums = h_state + (size_t)4 * P;
  std::vector<double> c((size_t)3 * P, 0.0);   // every plane starts at the zero plane
  std::vector<int> its((size_t)P, 0);
  std::vector<char> live((size_t)P, 1);
  int nlive = P;
  for (int it = 0; it < max_iter && nlive > 0; ++it) {
    for (int q = 0; q < P; ++q) {
      h_state[4 * q] = c[3 * q];
      h_state[4 * q + 1] = c[3 * q + 1];
      h_state[4 * q + 2] = c[3 * q + 2];
      h_state[4 * q + 3] = live[q] ? 1.0 : 0.0;
    }
    HIP_TRY(hipMemcpyAsync(d_state, h_state, (size_t)4 * P * sizeof(double), hipMemcpyHostToDevice, p->stream));
    HIP_TRY(launch_huber_moments_batch(p->dtype, images, P, n0, n1, d_state, cx, cy, sx, sy, work, d_sums, p->stream));
    HIP_TRY(hipMemcpyAsync(h_sums, d_sums, (size_t)10 * P * sizeof(double), hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    for (int q = 0; q < P; ++q) {
      if (!live[q]) continue;   // a converged plane keeps its coefficients
      const double* sums = h_sums + (size_t)10 * q;
      double nc[3];
      if (!solve3(sums, sums + 6, nc))
        return fail(GPA_ERR_STATE, "gpa_fit_planes: singular normal equations (plane " + std::to_string(q) + ")");
      double* cq = &c[3 * q];
      const double step = fabs(nc[0] - cq[0]) + fabs(nc[1] - cq[1]) + fabs(nc[2] - cq[2]);
      cq[0] = nc[0]; cq[1] = nc[1]; cq[2] = nc[2];
      its[q] = it + 1;
      if (step <= tol) { live[q] = 0; --nlive; }
    }
  }
  for (int q = 0; q < P; ++q) {
    const double* cq = &c[3 * q];
    coef[3 * q] = cq[0] / sx;
    coef[3 * q + 1] = cq[1] / sy;
    coef[3 * q + 2] = cq[2] - cq[0] * cx / sx - cq[1] * cy / sy;
    if (iters_out) iters_out[q] = its[q];
  }
  return GPA_OK;
}

int gpa_fit_planes_dev(gpa_plan* p, const void* images, int P, int max_iter, double tol, double* coef, int* iters_out) {
  if (!p || !images || !coef) return fail(GPA_ERR_ARG, "gpa_fit_planes: null argument");
  if (P < 1 || P > 65535) return fail(GPA_ERR_ARG, "gpa_fit_planes: need 1 <= P <= 65535");
  if (max_iter < 1 || !(tol >= 0.0)) return fail(GPA_ERR_ARG, "gpa_fit_planes: need max_iter >= 1, tol >= 0");
  HIP_TRY(hipSetDevice(p->device));
  TRY(ensure_iter(p, fit_bytes(P)));
  ProfInstall prof(p);
  TRY(fit_planes_run(p, images, P, max_iter, tol, coef, iters_out));
  if (p->profiling) collect_kernel_profile(p);
  return GPA_OK;
}

int gpa_lockin_polar_crop_dev(gpa_plan* p, const void* lockins, int P, int edge, void* psi, void* amp, void* weight,
                              void* amax) {
  if (!p || !lockins || !psi || !amp || !amax) return fail(GPA_ERR_ARG, "gpa_lockin_polar_crop: null argument");
  if (P < 1 || P > 65535) return fail(GPA_ERR_ARG, "gpa_lockin_polar_crop: need 1 <= P <= 65535");
  if (edge < 0 || 2 * edge >= std::min(p->n0, p->n1) - 1)
    return fail(GPA_ERR_ARG, "gpa_lockin_polar_crop: edge must leave a window of at least 2 x 2");
  HIP_TRY(hipSetDevice(p->device));
  const size_t m = (size_t)(p->n0 - 2 * edge) * (p->n1 - 2 * edge);
  HIP_TRY(hipMemsetAsync(amax, 0, (size_t)P * p->rsz, p->stream));
  HIP_TRY(launch_polar_crop(p->dtype, lockins, P, p->n0, p->n1, edge, psi, amp, amax, p->stream));
  if (weight) HIP_TRY(launch_sqrt_norm(p->dtype, amp, P, m, amax, weight, p->stream));
  return GPA_OK;
}

// what both forms of the driver check before anything is launched; *cp_out: the plan of the window
static int iterate_check(gpa_plan* p, gpa_plan* crop, const void* image, const double* kvecs, int P, double sigma, int edge,
                         int iters, int kmax_iter, int kmax, const void* prs, const void* w, const double* corr,
                         gpa_plan** cp_out) {
  if (!p) return fail(GPA_ERR_ARG, "gpa_iterate_gpa: plan is null");
  if (!image) return fail(GPA_ERR_ARG, "gpa_iterate_gpa: image is null");
  if (!kvecs) return fail(GPA_ERR_ARG, "gpa_iterate_gpa: kvecs is null");
  if (!prs) return fail(GPA_ERR_ARG, "gpa_iterate_gpa: prs is null");
  if (!w) return fail(GPA_ERR_ARG, "gpa_iterate_gpa: w is null");
  if (!corr) return fail(GPA_ERR_ARG, "gpa_iterate_gpa: corr is null");
  if (P < 1) return fail(GPA_ERR_ARG, "gpa_iterate_gpa: P must be >= 1");
  if (P > p->max_batch) return fail(GPA_ERR_ARG, "gpa_iterate_gpa: P exceeds the plan's max_batch");
  if (!(sigma > 0)) return fail(GPA_ERR_ARG, "gpa_iterate_gpa: sigma must be positive");
  if (iters < 0) return fail(GPA_ERR_ARG, "gpa_iterate_gpa: iters must be >= 0");
  if (edge < 0) return fail(GPA_ERR_ARG, "gpa_iterate_gpa: edge must be >= 0");
  if (2 * edge >= std::min(p->n0, p->n1) - 1)
    return fail(GPA_ERR_ARG, "gpa_iterate_gpa: edge must leave a window of at least 2 x 2 (2 edge < min(n0, n1) - 1)");
  if (kmax_iter < 1) return fail(GPA_ERR_ARG, "gpa_iterate_gpa: kmax_iter must be >= 1");
  if (kmax < 1) return fail(GPA_ERR_ARG, "gpa_iterate_gpa: kmax must be >= 1");
  gpa_plan* cp = crop ? crop : p;
  const int m0 = p->n0 - 2 * edge, m1 = p->n1 - 2 * edge;
  if (!crop && edge > 0) return fail(GPA_ERR_ARG, "gpa_iterate_gpa: crop_plan is null (only edge = 0 does without one)");
  if (cp->n0 != m0 || cp->n1 != m1)
    return fail(GPA_ERR_ARG, "gpa_iterate_gpa: crop_plan has shape " + std::to_string(cp->n0) + " x " + std::to_string(cp->n1) +
                                 ", the window is " + std::to_string(m0) + " x " + std::to_string(m1));
  if (cp->dtype != p->dtype) return fail(GPA_ERR_ARG, "gpa_iterate_gpa: crop_plan has another dtype than plan");
  if (cp->device != p->device) return fail(GPA_ERR_ARG, "gpa_iterate_gpa: crop_plan is on another device than plan");
  if (p->spectral_only)
    return fail(GPA_ERR_STATE, "gpa_iterate_gpa: plan (the frame) is too large for the sweep kernels (an axis above 16384 pow2 / "
                               "8192 other in f32, 8192 / 4096 in f64)");
  if (!unwrap_has_kernels(&cp->uw))
    return fail(GPA_ERR_STATE, std::string("gpa_iterate_gpa: ") + (crop ? "crop_plan (the window)" : "plan (as the window's plan)") +
                                   " has no unwrap kernels for its shape -- an axis that is not a power of two needs both axes "
                                   "<= 8192 (f32) / 4096 (f64); powers of two go to 16384 (INTEGRATION.md, size limits)");
  *cp_out = cp;
  return GPA_OK;
}

// layout of the window plan's scratch behind the fit's head: amax (256 bytes per 32 planes), then planes of m reals
static size_t iterate_planes_at(int P) { return fit_bytes(P) + (((size_t)P * 8 + 255) & ~(size_t)255); }

static int iterate_run(gpa_plan* p, gpa_plan* cp, const void* image, const double* kvecs, int P, double sigma, int edge,
                       int iters, int kmax_iter, int kmax, void* prs, void* w, double* corr, double* delta_ks,
                       int* unwrap_iters) {
  const size_t npx = (size_t)p->n0 * p->n1, m = (size_t)cp->n0 * cp->n1;
  char* base = cp->d_iter.as<char>();
  void* amax = base + fit_bytes(P);
  char* psi = base + iterate_planes_at(P);
  char* weight = psi + (size_t)P * m * p->rsz;
  TRY(ensure_sf(p, (size_t)P * npx * p->csz));
  if (cp != p) TRY(plan_event(p));
  const bool prof = p->profiling;
  for (float& v : p->stage_ms) v = 0.f;
  auto t_last = std::chrono::steady_clock::now();
  // profiling: the stage that just ended is waited for and its wall time added to stage_ms[idx]
  auto mark = [&](int idx) -> int {
    if (!prof) return GPA_OK;
    HIP_TRY(hipStreamSynchronize(p->stream));
    HIP_TRY(hipStreamSynchronize(cp->stream));
    const auto now = std::chrono::steady_clock::now();
    p->stage_ms[idx] += std::chrono::duration<float, std::milli>(now - t_last).count();
    t_last = now;
    return GPA_OK;
  };
  std::vector<double> ks((size_t)2 * P), coef((size_t)3 * P);
  for (int i = 0; i < 2 * P; ++i) corr[i] = 0.0;
  for (int pass = 0; pass <= iters; ++pass) {
    const bool last = pass == iters;
    for (int i = 0; i < 2 * P; ++i) ks[i] = kvecs[i] + corr[i];
    TRY(gpa_lockin_batch_dev(p, image, ks.data(), P, sigma, p->d_sf.ptr));
    TRY(mark(0));
    TRY(gpa_lockin_polar_crop_dev(p, p->d_sf.ptr, P, edge, psi, w, weight, amax));
    if (cp != p) {
      HIP_TRY(hipEventRecord(p->ev_x, p->stream));
      HIP_TRY(hipStreamWaitEvent(cp->stream, p->ev_x, 0));
    }
    TRY(mark(1));
    for (int q = 0; q < P; ++q) {
      int it = 0;
      hipError_t e = unwrap_run(&cp->uw, psi + (size_t)q * m * p->rsz, nullptr, weight + (size_t)q * m * p->rsz, true,
                                last ? kmax : kmax_iter, 1e-9, true, (char*)prs + (size_t)q * m * p->rsz, &it, cp->stream);
      if (e != hipSuccess) return unwrap_fail(e);
      if (unwrap_iters) unwrap_iters[(size_t)pass * P + q] = it;
    }
    TRY(mark(2));
    if (last) break;
    TRY(fit_planes_run(cp, prs, P, 200, 1e-12, coef.data(), nullptr));
    for (int q = 0; q < P; ++q)
      for (int a = 0; a < 2; ++a) {
        const double dk = coef[3 * q + a] / (2 * M_PI);
        if (delta_ks) delta_ks[((size_t)pass * P + q) * 2 + a] = dk;
        corr[2 * q + a] -= dk;
      }
    TRY(mark(3));
  }
  return GPA_OK;
}

int gpa_iterate_gpa_dev(gpa_plan* p, gpa_plan* crop, const void* image, const double* kvecs, int P, double sigma, int edge,
                        int iters, int kmax_iter, int kmax, void* prs, void* w, double* corr, double* delta_ks,
                        int* unwrap_iters) {
  gpa_plan* cp = nullptr;
  TRY(iterate_check(p, crop, image, kvecs, P, sigma, edge, iters, kmax_iter, kmax, prs, w, corr, &cp));
  HIP_TRY(hipSetDevice(p->device));
  const size_t m = (size_t)cp->n0 * cp->n1;
  TRY(ensure_iter(cp, iterate_planes_at(P) + 2 * (size_t)P * m * p->rsz));
  return iterate_run(p, cp, image, kvecs, P, sigma, edge, iters, kmax_iter, kmax, prs, w, corr, delta_ks, unwrap_iters);
}

int gpa_iterate_gpa(gpa_plan* p, gpa_plan* crop, const void* image, const double* kvecs, int P, double sigma, int edge,
                    int iters, int kmax_iter, int kmax, void* prs, void* w, double* corr, double* delta_ks,
                    int* unwrap_iters) {
  gpa_plan* cp = nullptr;
  TRY(iterate_check(p, crop, image, kvecs, P, sigma, edge, iters, kmax_iter, kmax, prs, w, corr, &cp));
  HIP_TRY(hipSetDevice(p->device));
  const size_t npx = (size_t)p->n0 * p->n1, m = (size_t)cp->n0 * cp->n1, planes = (size_t)P * m * p->rsz;
  // the scratch's last two plane sets stage prs and w
  TRY(ensure_iter(cp, iterate_planes_at(P) + 4 * planes));
  char* d_prs = cp->d_iter.as<char>() + iterate_planes_at(P) + 2 * planes;
  char* d_w = d_prs + planes;
  HIP_TRY(hipMemcpyAsync(p->d_image, image, npx * p->rsz, hipMemcpyHostToDevice, p->stream));
  TRY(iterate_run(p, cp, p->d_image, kvecs, P, sigma, edge, iters, kmax_iter, kmax, d_prs, d_w, corr, delta_ks, unwrap_iters));
  // (every solve has been waited for on the window plan's stream, which had waited for the crop on the frame's)
  HIP_TRY(hipMemcpyAsync(prs, d_prs, planes, hipMemcpyDeviceToHost, cp->stream));
  HIP_TRY(hipMemcpyAsync(w, d_w, planes, hipMemcpyDeviceToHost, cp->stream));
  HIP_TRY(hipStreamSynchronize(cp->stream));
  return GPA_OK;
}
