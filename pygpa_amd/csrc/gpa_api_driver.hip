// C ABI, the fused driver: extract_displacement_field in one call (geometric_phase_analysis.py:907-932), its asynchronous
// and batched forms.
#include "gpa_plan.h"

// ---- fused driver --------------------------------------------------------------
// the optional outputs of a driver call (each may be NULL; grad_mode: the stencil of grads).  grads (P x n0 x n1 x 2) / absw
// (P x n0 x n1) != NULL is the one-sweep form, see extract_launch
struct ExtractOut {
  void* lockins;
  int32_t* kidx;
  void* grads;
  void* absw;
  int grad_mode;
};

// the ranges every driver accepts, in the words of entry point `fn`
static int check_ranges(gpa_plan* p, const std::string& fn, int P, int K, int kmax) {
  if (P < 2 || P > p->max_peaks) return fail(GPA_ERR_STATE, fn + ": need 2 <= P <= 8");
  if (K < 1 || P * K > p->max_batch) return fail(GPA_ERR_STATE, fn + ": P*K exceeds max_batch");
  if (kmax < 1) return fail(GPA_ERR_ARG, "kmax must be >= 1");
  return GPA_OK;
}

// host-side preparation: filter / carrier / k-matrix tables (re-staged only when they change; these upload
// synchronously), the x-plane buffer, and the second unwrap workspace + stream
static int extract_stage(gpa_plan* p, const double* kvecs, int P, const double* klists, int K, double sigma, int* Bx, int passb) {
  TRY(stage_sweep(p, kvecs, P, klists, K, sigma, Bx, passb));
  TRY(stage_kmat(p, kvecs, P));
  {
    // (PAIR_MAXSIDE: measurement switch for the size up to which both components share one set of launches)
    const size_t side = opt_set(OPT_PAIR_MAXSIDE) ? (size_t)opt(OPT_PAIR_MAXSIDE).num : 1024;
    p->use_pair = (size_t)p->n0 * p->n1 <= side * side && !opt_set(OPT_NO_PAIR);
  }
  if (p->use_pair && !p->have_uwp) {
    size_t bp = 0;
    hipError_t ep = unwrap_workspace_create(p->dtype, p->n0, p->n1, p->stream, &p->uwp, &bp, 2);
    if (ep != hipSuccess) {
      unwrap_workspace_destroy(&p->uwp);
      return fail(GPA_ERR_HIP, std::string("paired unwrap workspace: ") + hipGetErrorString(ep));
    }
    p->ws_bytes += bp;
    p->have_uwp = true;
  }
  if (p->use_pair && !unwrap_supports_batch(&p->uwp)) p->use_pair = false;
  if (!p->stream2) {
    // the two displacement components are independent solves: give the second one its own
    // workspace and stream so the latency-bound kernels of one fill the gaps of the other
    HIP_TRY(hipStreamCreateWithFlags(&p->stream2, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&p->ev_fork, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&p->ev_join, hipEventDisableTiming));
    size_t b2 = 0;
    hipError_t e2 = unwrap_workspace_create(p->dtype, p->n0, p->n1, p->stream2, &p->uw2, &b2);
    if (e2 != hipSuccess) return fail(GPA_ERR_HIP, std::string("second unwrap workspace: ") + hipGetErrorString(e2));
    p->ws_bytes += b2;
  }
  return GPA_OK;
}

// every launch of the driver, nothing else: this is what a hipGraph of the call holds
// o.grads / o.absw != NULL: the one-sweep form -- pass B also leaves the phase of every candidate in p->d_sf (sized by the
// caller), the multi-peak stencil turns them into the winners' phase gradients, |lock-in| goes to absw; the lock-ins are
// compensated then.  Both NULL: the launches of the plain driver, nothing else.
static int extract_launch(gpa_plan* p, const void* image, int P, int K, int Bx, int mask_border, int kmax, void* u,
                          const ExtractOut& o) {
  const size_t npx = (size_t)p->n0 * p->n1;
  void* lk = o.lockins ? o.lockins : p->d_lockin;
  if (p->profiling) HIP_TRY(hipEventRecord(p->stage_ev[0], p->stream));
  HIP_TRY(launch_mean(p->dtype, image, npx, p->d_scratch, p->d_mean, p->stream));
  if (p->profiling) HIP_TRY(hipEventRecord(p->stage_ev[1], p->stream));
  TRY(run_passA(p, image, p->d_mean, p->Tbuf.ptr, Bx, 1));
  if (p->profiling) HIP_TRY(hipEventRecord(p->stage_ev[2], p->stream));
  if (o.grads) {
    int32_t* kidx = o.kidx ? o.kidx : p->d_kidx;   // (the stencil reads the winners' indices)
    bool shared = false;
    TRY(passB_phases(p, {p->Tbuf.ptr, 1, 0}, P, K, lk, kidx, p->d_sf.ptr, &shared));
    HIP_TRY(launch_phasegrad(p->dtype, p->d_sf.ptr, K, kidx, p->n0, p->n1, p->d_kl, p->d_kr, o.grad_mode, o.grads, p->stream,
                             shared ? p->d_ystep : nullptr, P));
  } else {
    // (lock-ins nobody reads but reconstruct_setup may stay raw)
    TRY(passB_select(p, {p->Tbuf.ptr, 1, 0}, P, K, lk, o.kidx, !o.lockins && !o.absw));
  }
  if (o.absw) HIP_TRY(launch_cabs(p->dtype, lk, (size_t)P * npx, o.absw, p->stream));
  const double* ystep = p->lk_raw ? p->d_ystep : nullptr;
  if (p->profiling) HIP_TRY(hipEventRecord(p->stage_ev[3], p->stream));
  // phases / weights / per-pixel least squares fused with the unwrap's set-up: the gradient fields never
  // go to HBM, the kernel leaves r0 of both components in the two unwrap workspaces
  int nparts = 0;
  if (p->use_pair && p->have_uwp && !p->profiling && !p->serial_unwrap) {
    HIP_TRY(launch_reconstruct_setup(p->dtype, lk, p->d_kmat, P, p->n0, p->n1, mask_border, p->d_wnorm,
                                     unwrap_residual_buffer(&p->uwp, 0), unwrap_residual_buffer(&p->uwp, 1),
                                     unwrap_partials_buffer(&p->uwp, 0), unwrap_partials_buffer(&p->uwp, 1), &nparts,
                                     p->stream, 1, 0, 0, ystep));
    hipError_t ep = unwrap_enqueue_prepared(&p->uwp, p->d_wnorm, nparts, kmax, 1e-9, true, u, p->stream);
    if (ep == hipSuccess) ep = unwrap_fetch_iters(&p->uwp, p->h_iters.as<int>(), p->stream);
    if (ep != hipSuccess) return unwrap_fail(ep);
    p->iters_stride = 4;
    p->iters_off = unwrap_iters_slot(&p->uwp);
    return GPA_OK;
  }
  p->iters_stride = 1;
  p->iters_off = 0;
  HIP_TRY(launch_reconstruct_setup(p->dtype, lk, p->d_kmat, P, p->n0, p->n1, mask_border, p->d_wnorm,
                                   unwrap_residual_buffer(&p->uw), unwrap_residual_buffer(&p->uw2),
                                   unwrap_partials_buffer(&p->uw), unwrap_partials_buffer(&p->uw2), &nparts, p->stream, 1, 0,
                                   0, ystep));
  if (p->profiling) HIP_TRY(hipEventRecord(p->stage_ev[4], p->stream));
  HIP_TRY(hipEventRecord(p->ev_fork, p->stream));
  HIP_TRY(hipStreamWaitEvent(p->stream2, p->ev_fork, 0));
  // the second component's launches go out from the plan's helper thread while this thread enqueues the first
  // (not while profiling: the per-kernel event pairs belong to this thread)
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  (void)hipStreamIsCapturing(p->stream, &cap);
  const bool threaded = p->use_worker && !p->profiling && !p->serial_unwrap && cap == hipStreamCaptureStatusNone;
  hipError_t e2 = hipSuccess;
  void* u1 = (char*)u + npx * p->rsz;
  auto second = [&]() {
    e2 = unwrap_enqueue_prepared(&p->uw2, p->d_wnorm, nparts, kmax, 1e-9, true, u1, p->stream2);
    if (e2 == hipSuccess) e2 = unwrap_fetch_iters(&p->uw2, p->h_iters.as<int>() + 1, p->stream2);
  };
  if (threaded) {
    if (!p->worker) p->worker = new EnqueueWorker(p->device);
    p->worker->submit(second);
  }
  hipError_t e = unwrap_enqueue_prepared(&p->uw, p->d_wnorm, nparts, kmax, 1e-9, true, u, p->stream);
  if (p->profiling || p->serial_unwrap) {   // per-kernel timings: run the second component after the first
    HIP_TRY(hipEventRecord(p->ev_fork, p->stream));
    HIP_TRY(hipStreamWaitEvent(p->stream2, p->ev_fork, 0));
  }
  if (e == hipSuccess) e = unwrap_fetch_iters(&p->uw, p->h_iters.as<int>(), p->stream);
  if (threaded) p->worker->wait(); else second();
  if (e == hipSuccess) e = e2;
  if (e != hipSuccess) return unwrap_fail(e);
  HIP_TRY(hipEventRecord(p->ev_join, p->stream2));
  HIP_TRY(hipStreamWaitEvent(p->stream, p->ev_join, 0));
  if (p->profiling) HIP_TRY(hipEventRecord(p->stage_ev[5], p->stream));
  return GPA_OK;
}

// enqueue the whole driver on the plan's streams without any host synchronisation: ~110 eager kernel launches.
// (Rounds 2-4 could capture them into a hipGraph -- USE_GRAPH=1 -- and replay it: measured NOT faster than eager launches at
// any size on MI355X / ROCm 7.2, 512^2 0.65 against 0.60 ms, 4096^2 equal, and it serialised with the copy stream of
// gpa_download_async: profiles/r02_graph_vs_eager.txt.  Removed in round 5; git history has it.)
// what: the entry point's name for the messages
static int extract_enqueue(gpa_plan* p, const char* what, const void* image, const double* kvecs, int P, const double* klists,
                           int K, double sigma, int mask_border, int kmax, void* u, const ExtractOut& o) {
  const std::string fn(what);
  if (!p || !image || !kvecs || !klists || !u) return fail(GPA_ERR_ARG, fn + ": null argument");
  TRY(check_ranges(p, fn, P, K, kmax));
  if (o.grads && (o.grad_mode < 0 || o.grad_mode > 2)) return fail(GPA_ERR_ARG, fn + ": grad_mode must be 0, 1 or 2");
  HIP_TRY(hipSetDevice(p->device));
  int Bx = 0;
  TRY(extract_stage(p, kvecs, P, klists, K, sigma, &Bx, o.grads ? SWEEP_PASSB_PHASES : SWEEP_PASSB_SELECT));
  // the phases of all P K candidates (reals): allocated by the first call that asks for gradients, kept by the plan
  if (o.grads) TRY(ensure_sf(p, (size_t)P * K * p->n0 * p->n1 * p->rsz));
  // per-kernel event pairs while profiling (installed for this thread until the function returns)
  ProfInstall prof(p);
  return extract_launch(p, image, P, K, Bx, mask_border, kmax, u, o);
}

// the iteration counts of the last driver call, once its stream has been waited for
static void read_iters(const gpa_plan* p, int* iters2) {
  const int* h = p->h_iters.as<int>();
  iters2[0] = h[p->iters_off];
  iters2[1] = h[p->iters_stride + p->iters_off];
}

int gpa_last_iters(gpa_plan* p, int* iters2) {
  if (!p || !iters2) return fail(GPA_ERR_ARG, "null argument");
  HIP_TRY(hipStreamSynchronize(p->stream));
  read_iters(p, iters2);
  return GPA_OK;
}

// the synchronising end of a driver call: stage / kernel times of a profiled call, iteration counts
static int extract_finish(gpa_plan* p, int* iters_out) {
  HIP_TRY(hipStreamSynchronize(p->stream));
  if (p->profiling) {
    for (int i = 0; i < 5; ++i) hipEventElapsedTime(&p->stage_ms[i], p->stage_ev[i], p->stage_ev[i + 1]);
    collect_kernel_profile(p);
  }
  if (iters_out) read_iters(p, iters_out);
  return GPA_OK;
}

// the host-pointer form: upload, enqueue on the plan's staging buffers, finish, download what was asked for (o: host pointers)
static int extract_host(gpa_plan* p, const char* what, const void* image, const double* kvecs, int P, const double* klists,
                        int K, double sigma, int mask_border, int kmax, void* u, const ExtractOut& o, int* iters_out) {
  if (!p || !image || !u) return fail(GPA_ERR_ARG, std::string(what) + ": null argument");
  HIP_TRY(hipSetDevice(p->device));
  const size_t npx = (size_t)p->n0 * p->n1;
  // device staging of the one-sweep outputs, sized for the plan's peaks on the first call that asks for them
  if (o.grads && !p->d_grads) TRY(dmalloc(p, &p->d_grads, (size_t)p->max_peaks * 2 * npx * p->rsz));
  if (o.absw && !p->d_absw) TRY(dmalloc(p, &p->d_absw, (size_t)p->max_peaks * npx * p->rsz));
  HIP_TRY(hipMemcpyAsync(p->d_image, image, npx * p->rsz, hipMemcpyHostToDevice, p->stream));
  const ExtractOut dev{o.lockins ? p->d_lockin : nullptr, o.kidx ? p->d_kidx : nullptr, o.grads ? p->d_grads : nullptr,
                       o.absw ? p->d_absw : nullptr, o.grad_mode};
  TRY(extract_enqueue(p, what, p->d_image, kvecs, P, klists, K, sigma, mask_border, kmax, p->d_u, dev));
  TRY(extract_finish(p, iters_out));
  HIP_TRY(hipMemcpyAsync(u, p->d_u, 2 * npx * p->rsz, hipMemcpyDeviceToHost, p->stream));
  if (o.lockins) HIP_TRY(hipMemcpyAsync(o.lockins, p->d_lockin, (size_t)P * npx * p->csz, hipMemcpyDeviceToHost, p->stream));
  if (o.kidx) HIP_TRY(hipMemcpyAsync(o.kidx, p->d_kidx, (size_t)P * npx * sizeof(int32_t), hipMemcpyDeviceToHost, p->stream));
  if (o.grads) HIP_TRY(hipMemcpyAsync(o.grads, p->d_grads, (size_t)P * 2 * npx * p->rsz, hipMemcpyDeviceToHost, p->stream));
  if (o.absw) HIP_TRY(hipMemcpyAsync(o.absw, p->d_absw, (size_t)P * npx * p->rsz, hipMemcpyDeviceToHost, p->stream));
  HIP_TRY(hipStreamSynchronize(p->stream));
  return GPA_OK;
}

// ---- the entry points: host pointers / device pointers / enqueue only, each plain (messages in the name of
// gpa_extract_displacement_field) and with the one-sweep outputs (messages in the entry point's own name)
int gpa_extract_displacement_field(gpa_plan* p, const void* image, const double* kvecs, int P,
                                   const double* klists, int K, double sigma, int mask_border, int kmax,
                                   void* u, void* lockins, int32_t* kidx, int* iters_out) {
  return extract_host(p, "gpa_extract_displacement_field", image, kvecs, P, klists, K, sigma, mask_border, kmax, u,
                      {lockins, kidx, nullptr, nullptr, 0}, iters_out);
}

int gpa_extract_displacement_field_grad(gpa_plan* p, const void* image, const double* kvecs, int P,
                                        const double* klists, int K, double sigma, int mask_border, int kmax,
                                        int grad_mode, void* u, void* lockins, int32_t* kidx, void* grads, void* absw,
                                        int* iters_out) {
  return extract_host(p, "gpa_extract_displacement_field_grad", image, kvecs, P, klists, K, sigma, mask_border, kmax, u,
                      {lockins, kidx, grads, absw, grad_mode}, iters_out);
}

int gpa_extract_displacement_field_dev(gpa_plan* p, const void* image, const double* kvecs, int P,
                                       const double* klists, int K, double sigma, int mask_border, int kmax,
                                       void* u, void* lockins, int32_t* kidx, int* iters_out) {
  TRY(extract_enqueue(p, "gpa_extract_displacement_field", image, kvecs, P, klists, K, sigma, mask_border, kmax, u,
                      {lockins, kidx, nullptr, nullptr, 0}));
  return extract_finish(p, iters_out);
}

int gpa_extract_displacement_field_grad_dev(gpa_plan* p, const void* image, const double* kvecs, int P,
                                            const double* klists, int K, double sigma, int mask_border, int kmax,
                                            int grad_mode, void* u, void* lockins, int32_t* kidx, void* grads, void* absw,
                                            int* iters_out) {
  TRY(extract_enqueue(p, "gpa_extract_displacement_field_grad_dev", image, kvecs, P, klists, K, sigma, mask_border, kmax, u,
                      {lockins, kidx, grads, absw, grad_mode}));
  return extract_finish(p, iters_out);
}

int gpa_extract_displacement_field_async(gpa_plan* p, const void* image, const double* kvecs, int P,
                                         const double* klists, int K, double sigma, int mask_border, int kmax,
                                         void* u, void* lockins, int32_t* kidx) {
  return extract_enqueue(p, "gpa_extract_displacement_field", image, kvecs, P, klists, K, sigma, mask_border, kmax, u,
                         {lockins, kidx, nullptr, nullptr, 0});
}

int gpa_extract_displacement_field_grad_async(gpa_plan* p, const void* image, const double* kvecs, int P,
                                              const double* klists, int K, double sigma, int mask_border, int kmax,
                                              int grad_mode, void* u, void* lockins, int32_t* kidx, void* grads, void* absw) {
  return extract_enqueue(p, "gpa_extract_displacement_field_grad_async", image, kvecs, P, klists, K, sigma, mask_border, kmax, u,
                         {lockins, kidx, grads, absw, grad_mode});
}

// ---- batched driver ---------------------------------------------------------------
// The plan's batched unwrap workspace, shared by the batched driver (2 problems per image) and the stack unwrap
// (gpa_unwrap_batch_dev).  It is a capacity in problems: a call that needs fewer (a ragged last chunk, a shorter stack, the
// other entry point) reuses it, one that needs more rebuilds it.
int ensure_unwrap_problems(gpa_plan* p, int nprob, const char* who) {
  if (nprob > p->uwb_probs) {
    if (!unwrap_supports_batch(&p->uw))   // (asked of the plan's own workspace: nothing is built for a shape that cannot use it)
      return fail(GPA_ERR_STATE, std::string(who) + ": this image shape has no batched unwrap");
    HIP_TRY(hipStreamSynchronize(p->stream));
    if (p->uwb_probs) unwrap_workspace_destroy(&p->uwb);
    p->uwb_probs = 0;
    p->uwb_bytes = p->uwb_base_bytes = 0;
    size_t bb = 0;
    hipError_t e = unwrap_workspace_create(p->dtype, p->n0, p->n1, p->stream, &p->uwb, &bb, nprob);
    if (e != hipSuccess) {
      unwrap_workspace_destroy(&p->uwb);
      return fail(GPA_ERR_HIP, std::string("batched unwrap workspace: ") + hipGetErrorString(e));
    }
    if (!unwrap_supports_batch(&p->uwb)) {
      unwrap_workspace_destroy(&p->uwb);
      return fail(GPA_ERR_STATE, std::string(who) + ": this image shape has no batched unwrap");
    }
    p->uwb_probs = nprob;
    p->uwb_bytes = p->uwb_base_bytes = bb;
  }
  if (!unwrap_set_active(&p->uwb, nprob)) return fail(GPA_ERR_STATE, "batched unwrap workspace: bad active count");
  HIP_TRY(p->h_iters_b.reserve((size_t)4 * std::max(nprob, p->uwb_probs) * sizeof(int), p->stream));
  return GPA_OK;
}

// the unwrap workspace of the 2 B problems of B images, their weights and pinned iteration counts
static int ensure_batch_unwrap(gpa_plan* p, int B) {
  TRY(ensure_unwrap_problems(p, 2 * B, "gpa_extract_displacement_field_batch"));
  p->uwb_last_nb = 0;   // (gpa_unwrap_batch_finish: the counts in flight are no stack unwrap's)
  HIP_TRY(p->d_wnorm_b.reserve((size_t)B * p->n0 * p->n1 * p->rsz, p->stream));
  return GPA_OK;
}

// x-planes (t_img bytes per image), lock-ins (l_img), means and mean scratch of a chunk of images swept in one set of launches
static int ensure_batch_sweep(gpa_plan* p, int chunk, size_t t_img, size_t l_img) {
  TRY(plan_reserve(p, p->bT, (size_t)chunk * t_img, "batched sweep buffers"));
  TRY(plan_reserve(p, p->bL, (size_t)chunk * l_img, "batched sweep buffers"));
  TRY(plan_reserve(p, p->bMean, (size_t)chunk * 8, "batched sweep buffers"));
  return plan_reserve(p, p->bScratch, (size_t)chunk * 1024 * sizeof(double), "batched sweep buffers");
}

// the iteration counts of the last batched call (2 per image), after waiting for it
static int read_batch_iters(gpa_plan* p, int B, int* iters_out) {
  HIP_TRY(hipStreamSynchronize(p->stream));
  for (int j = 0; j < 2 * B; ++j) iters_out[j] = p->h_iters_b.as<int>()[4 * j + unwrap_iters_slot(&p->uwb)];
  return GPA_OK;
}

// A stack of images of one shape in one call: every kernel of the driver takes an image / problem index from its
// grid, so the stack is ONE set of ~50 launches instead of ~110 per image -- a small image is bound by its chain of
// dependent launches, not by their work.
// images: B x n0 x n1, u: B x 2 x n0 x n1 (device pointers), iters_out: 2 B counts (host, may be NULL: no
// synchronisation then).  The results are those of B separate gpa_extract_displacement_field_dev calls, bit for bit.
// o: the optional outputs of gpa_extract_displacement_field_grad_dev with a leading image axis; all NULL: the plain stack
// driver's launches and nothing else.  o.grads / o.absw != NULL is the one-sweep form of extract_launch, a chunk at a time.
static int extract_batch(gpa_plan* p, const char* fn, const void* images, int B, const double* kvecs, int P,
                         const double* klists, int K, double sigma, int mask_border, int kmax, void* u, const ExtractOut& o,
                         int* iters_out) {
  if (!p || !images || !kvecs || !klists || !u) return fail(GPA_ERR_ARG, std::string(fn) + ": null argument");
  if (B < 1 || B > 4096) return fail(GPA_ERR_ARG, std::string(fn) + ": need 1 <= images <= 4096");
  TRY(check_ranges(p, fn, P, K, kmax));
  if (o.grads && (o.grad_mode < 0 || o.grad_mode > 2)) return fail(GPA_ERR_ARG, std::string(fn) + ": grad_mode must be 0, 1 or 2");
  HIP_TRY(hipSetDevice(p->device));
  int Bx = 0;
  TRY(extract_stage(p, kvecs, P, klists, K, sigma, &Bx, o.grads ? SWEEP_PASSB_PHASES : SWEEP_PASSB_SELECT));
  TRY(ensure_batch_unwrap(p, B));
  const size_t npx = (size_t)p->n0 * p->n1;
  // the sweep and the least squares of a chunk of images are ONE set of launches too (blockIdx.z / .y = image);
  // the chunk is what fits ~3 GB of x-planes (512^2: the whole stack, 4096^2: one image at a time) and, with gradients, ~3 GB
  // of candidate phases (P K reals per pixel) as well
  const size_t t_img = (size_t)Bx * npx * p->csz, l_img = (size_t)P * npx * p->csz, s_img = (size_t)P * K * npx * p->rsz;
  const size_t k_img = (size_t)P * npx * sizeof(int32_t);
  size_t fit = ((size_t)3 << 30) / t_img;
  if (o.grads) fit = std::min(fit, ((size_t)3 << 30) / s_img);
  const int chunk = (int)std::min<size_t>((size_t)B, std::max<size_t>(1, fit));
  TRY(ensure_batch_sweep(p, chunk, t_img, o.lockins ? 0 : l_img));
  if (o.grads) TRY(ensure_sf(p, (size_t)chunk * s_img));
  if (o.grads && !o.kidx) TRY(plan_reserve(p, p->bK, (size_t)chunk * k_img, "batched sweep buffers"));   // (the stencil reads the winners' indices)
  int nparts = 0;
  const size_t rstride = 2 * npx;                                                     // residual slices per image
  const size_t pstride = (size_t)(unwrap_partials_buffer(&p->uwb, 2) - unwrap_partials_buffer(&p->uwb, 0));
  for (int c0 = 0; c0 < B; c0 += chunk) {
    const int nimg = std::min(chunk, B - c0);
    const void* image = (const char*)images + (size_t)c0 * npx * p->rsz;
    // this chunk's slices of the outputs that were asked for; lock-ins nobody asked for stay in the chunk's own buffer
    void* lk = o.lockins ? (char*)o.lockins + (size_t)c0 * l_img : p->bL.ptr;
    int32_t* kidx = o.kidx ? o.kidx + (size_t)c0 * P * npx : nullptr;
    HIP_TRY(launch_mean(p->dtype, image, npx, p->bScratch.as<double>(), p->bMean.ptr, p->stream, nimg));
    TRY(run_passA(p, image, p->bMean.ptr, p->bT.ptr, Bx, nimg));
    if (o.grads) {
      if (!kidx) kidx = p->bK.as<int32_t>();
      bool shared = false;
      TRY(passB_phases(p, {p->bT.ptr, nimg, Bx}, P, K, lk, kidx, p->d_sf.ptr, &shared));
      HIP_TRY(launch_phasegrad(p->dtype, p->d_sf.ptr, K, kidx, p->n0, p->n1, p->d_kl, p->d_kr, o.grad_mode,
                               (char*)o.grads + (size_t)c0 * 2 * P * npx * p->rsz, p->stream, shared ? p->d_ystep : nullptr, P, nimg));
    } else {
      // (lock-ins nobody reads but reconstruct_setup may stay raw)
      TRY(passB_select(p, {p->bT.ptr, nimg, Bx}, P, K, lk, kidx, !o.lockins && !o.absw));
    }
    if (o.absw)
      HIP_TRY(launch_cabs(p->dtype, lk, (size_t)nimg * P * npx, (char*)o.absw + (size_t)c0 * P * npx * p->rsz, p->stream));
    HIP_TRY(launch_reconstruct_setup(p->dtype, lk, p->d_kmat, P, p->n0, p->n1, mask_border,
                                     p->d_wnorm_b.as<char>() + (size_t)c0 * npx * p->rsz,
                                     unwrap_residual_buffer(&p->uwb, 2 * c0), unwrap_residual_buffer(&p->uwb, 2 * c0 + 1),
                                     unwrap_partials_buffer(&p->uwb, 2 * c0), unwrap_partials_buffer(&p->uwb, 2 * c0 + 1),
                                     &nparts, p->stream, nimg, rstride, pstride, p->lk_raw ? p->d_ystep : nullptr));
  }
  hipError_t e = unwrap_enqueue_prepared(&p->uwb, p->d_wnorm_b.ptr, nparts, kmax, 1e-9, true, u, p->stream);
  if (e == hipSuccess) e = unwrap_fetch_iters(&p->uwb, p->h_iters_b.as<int>(), p->stream);
  p->uwb_bytes = p->uwb_base_bytes + unwrap_ring_bytes(&p->uwb);   // (the solve allocates the search directions it keeps)
  if (e != hipSuccess) return fail(GPA_ERR_HIP, std::string("batched unwrap: ") + hipGetErrorString(e));
  return iters_out ? read_batch_iters(p, B, iters_out) : GPA_OK;
}

int gpa_extract_displacement_field_batch_dev(gpa_plan* p, const void* images, int B, const double* kvecs, int P,
                                             const double* klists, int K, double sigma, int mask_border, int kmax,
                                             void* u, int* iters_out) {
  return extract_batch(p, "gpa_extract_displacement_field_batch", images, B, kvecs, P, klists, K, sigma, mask_border, kmax, u,
                       {nullptr, nullptr, nullptr, nullptr, 0}, iters_out);
}

int gpa_extract_displacement_field_grad_batch_dev(gpa_plan* p, const void* images, int B, const double* kvecs, int P,
                                                  const double* klists, int K, double sigma, int mask_border, int kmax,
                                                  int grad_mode, void* u, void* lockins, int32_t* kidx, void* grads, void* absw,
                                                  int* iters_out) {
  // (without an optional output the messages are the plain stack driver's, like everything else about the call)
  const bool plain = !lockins && !kidx && !grads && !absw;
  return extract_batch(p, plain ? "gpa_extract_displacement_field_batch" : "gpa_extract_displacement_field_grad_batch", images, B,
                       kvecs, P, klists, K, sigma, mask_border, kmax, u, {lockins, kidx, grads, absw, grad_mode}, iters_out);
}

// whether gpa_extract_displacement_field_batch_dev can take this plan's image shape (the fused iteration covers it);
// callers with other shapes loop over gpa_extract_displacement_field_dev instead
int gpa_supports_batch(gpa_plan* p) {
  if (!p) return 0;
  return unwrap_supports_batch(&p->uw) ? 1 : 0;
}

int gpa_last_batch_iters(gpa_plan* p, int B, int* iters_out) {
  if (!p || !iters_out || B < 1 || 2 * B > p->uwb_probs) return fail(GPA_ERR_ARG, "gpa_last_batch_iters: bad argument");
  return read_batch_iters(p, B, iters_out);
}

int gpa_extract_gradients(gpa_plan* p, const void* image, const double* kvecs, int P, const double* klists, int K,
                          double sigma, int mask_border, void* dudx, void* dudy, void* wnorm) {
  if (!p || !image || !kvecs || !klists || !dudx || !dudy || !wnorm)
    return fail(GPA_ERR_ARG, "gpa_extract_gradients: null argument");
  TRY(check_ranges(p, "gpa_extract_gradients", P, K, 1));   // (no unwrap here: no kmax)
  HIP_TRY(hipSetDevice(p->device));
  const size_t npx = (size_t)p->n0 * p->n1;
  HIP_TRY(hipMemcpyAsync(p->d_image, image, npx * p->rsz, hipMemcpyHostToDevice, p->stream));
  // no mean subtraction here: a tile must be offset by the mean of the WHOLE image
  // (geometric_phase_analysis.py:919), which only the caller knows
  TRY(sweep_peaks_dev(p, p->d_image, nullptr, kvecs, P, klists, K, sigma, p->d_lockin, nullptr, true));
  TRY(stage_kmat(p, kvecs, P));
  HIP_TRY(launch_reconstruct(p->dtype, p->d_lockin, p->d_kmat, P, p->n0, p->n1, mask_border, p->d_dudx, p->d_dudy,
                             p->d_wnorm, p->stream, p->lk_raw ? p->d_ystep : nullptr));
  HIP_TRY(hipMemcpyAsync(dudx, p->d_dudx, (size_t)2 * p->n0 * (p->n1 - 1) * p->rsz, hipMemcpyDeviceToHost, p->stream));
  HIP_TRY(hipMemcpyAsync(dudy, p->d_dudy, (size_t)2 * (p->n0 - 1) * p->n1 * p->rsz, hipMemcpyDeviceToHost, p->stream));
  HIP_TRY(hipMemcpyAsync(wnorm, p->d_wnorm, npx * p->rsz, hipMemcpyDeviceToHost, p->stream));
  HIP_TRY(hipStreamSynchronize(p->stream));
  return GPA_OK;
}

