/* gpa_hip.h -- C ABI of libgpa_hip.so, the MI355X (gfx950) implementation of the
 * pyGPA displacement-field hot path.
 *
 * The reference (TAdeJong/pyGPA) is pure Python and has no FFI layer; its GPU
 * path is the CuPy module pyGPA/cuGPA.py.  Each entry point below names the
 * reference function(s) whose arithmetic it replaces (file:line in the reference
 * checkout); the Python host mirror in pygpa_amd/ binds them with ctypes (see
 * INTEGRATION.md for the stub a pyGPA maintainer would add).
 *
 * Conventions
 *   - return 0 on success, < 0 on error; gpa_last_error() gives the message of
 *     the last failing call on the calling thread.
 *   - images are C-contiguous (n0, n1): axis 0 <-> "x" <-> kvec[0], axis 1 <->
 *     "y" <-> kvec[1] (geometric_phase_analysis.py:72-73).
 *   - `dtype` of a plan fixes the element type of EVERY real/complex buffer
 *     passed to it: GPA_F32 -> float / interleaved float2, GPA_F64 -> double /
 *     interleaved double2.  k-vectors and sigma are always double.
 *   - functions without suffix take HOST pointers (copies in/out are part of the
 *     call); `_dev` variants take DEVICE pointers valid on the plan's device
 *     (e.g. torch.Tensor.data_ptr()) and are asynchronous on the plan's stream
 *     until gpa_plan_sync().
 *   - the caller owns every buffer; nothing passed in is modified unless
 *     documented as an output.  A plan is bound to one device and one stream and
 *     is not re-entrant: serialise calls per plan.
 */
#ifndef GPA_HIP_H
#define GPA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* the library is built with -fvisibility=hidden: these declarations are its whole dynamic symbol table (tests/test_abi.py) */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define GPA_F32 0
#define GPA_F64 1

#define GPA_OK 0
#define GPA_ERR_ARG (-1)      /* bad argument (shape, NULL, unsupported size)   */
#define GPA_ERR_HIP (-2)      /* a HIP runtime call failed                       */
#define GPA_ERR_NODEV (-3)    /* no usable GPU                                   */
#define GPA_ERR_STATE (-4)    /* plan too small for the request (max_batch, ...) */

typedef struct gpa_plan gpa_plan;

int gpa_version(void);
const char* gpa_last_error(void);
int gpa_device_count(void);
/* Diagnostic / test switches of the library (no counterpart in the reference).  `name` is one of
 * the switches documented in INTEGRATION.md ("NO_LAT", "COLSOLVE", "F32_EPS_FLOOR", ..., with or
 * without the GPA_ prefix), `value` its text value or NULL to clear it.  The switches start from
 * the environment variables GPA_<NAME> as they were when the library was first used; after that
 * only this call changes them (the library never reads the environment on a call path).
 * Switches read at plan creation (NO_SHARED, NO_COMPACT, NO_KSPLIT, NO_MR, MR_FORCE_BLUESTEIN,
 * SERIAL_UNWRAP, NO_WORKER, DFT_ENGINE) apply to plans created afterwards.  Process-wide.        */
int gpa_set_option(const char* name, const char* value);

/* One plan = one device + one stream + workspace for images of shape (n0, n1)
 * and up to max_batch simultaneous lock-ins (peaks x k-vectors).              */
gpa_plan* gpa_plan_create(int device, int n0, int n1, int max_batch, int dtype);
void gpa_plan_destroy(gpa_plan* plan);
int gpa_plan_sync(gpa_plan* plan);
size_t gpa_plan_workspace_bytes(const gpa_plan* plan);
/* the hipStream_t of the plan, as an opaque pointer */
void* gpa_plan_stream(const gpa_plan* plan);
/* FFT lengths used along each axis (== n for powers of two, else the next power
 * of two >= 2n-1; the circular Gaussian convolution is evaluated exactly either way) */
int gpa_plan_fft_len(const gpa_plan* plan, int axis);

/* a1/a2 -- batched spatial lock-in
 *   out[b] = ifft2( fft2(image * exp(2 pi i (x kx_b + y ky_b))) * G_sigma )
 * replaces GPA (geometric_phase_analysis.py:20-45), optGPA (:48-76), vecGPA
 * (:79-89) and cuGPA.cuGPA (cuGPA.py:11-38).  kvecs: B x 2 doubles, out: B x n0 x n1
 * complex.  B <= max_batch.                                                    */
int gpa_lockin_batch(gpa_plan* plan, const void* image, const double* kvecs, int B,
                     double sigma, void* out);
int gpa_lockin_batch_dev(gpa_plan* plan, const void* image, const double* kvecs, int B,
                         double sigma, void* out);

/* a3 -- reference-vector sweep over an explicit, host-built k-list (K x 2,
 * candidate order = list order).  Per pixel the candidate with the strictly
 * largest |lock-in| wins (first maximum wins ties); the stored value is
 * re-referenced to kref: sf * exp(-2 pi i ((wx-kx) x + (wy-ky) y)).
 * replaces optwfr2 (geometric_phase_analysis.py:669-686), wfr2 (:615-644), wfr3
 * (:647-666), wfr2_only_lockin (:689-702) and cuGPA.wfr2_only_lockin
 * (cuGPA.py:136-158).
 *   lockin : n0 x n1 complex (output)
 *   kidx   : n0 x n1 int32 index of the winner in klist, -1 where nothing won
 *            (nullable)
 *   grad   : n0 x n1 x 2 real, a4 -- gradient of the winner's -angle(sf) by
 *            np.gradient stencils + 2 pi (w - kref), wrapped as wrapToPi(2g)/2
 *            (nullable); replaces wfr2_grad_opt (:763-813) and
 *            cuGPA.wfr2_grad_opt / wfr2_grad_single / wfr2_only_grad
 *            (cuGPA.py:41-133, :161-202).                                     */
int gpa_sweep(gpa_plan* plan, const void* image, const double* kref, const double* klist,
              int K, double sigma, void* lockin, int32_t* kidx, void* grad);
int gpa_sweep_dev(gpa_plan* plan, const void* image, const double* kref, const double* klist,
                  int K, double sigma, void* lockin, int32_t* kidx, void* grad);

/* a4 with the other gradient stencils of the reference, and a3's gated form:
 * gpa_sweep_grad: gpa_sweep with grad != NULL and a selectable stencil.  grad_mode 0 = np.gradient (= gpa_sweep);
 *   1 = forward differences along axis 0, axis 1 with NaN at the last index -- grad='diff' of cuGPA.wfr2_grad_opt /
 *   wfr2_grad_single / wfr2_only_grad (cuGPA.py:58-62); 2 = the same with the two components exchanged -- grad='diff'
 *   of wfr2_grad (geometric_phase_analysis.py:738-742).  wfr2_grad (:722-760) differentiates the compensated
 *   lock-in and wraps per candidate, which is the same number up to rounding.
 * gpa_sweep_gated: wfr4 (geometric_phase_analysis.py:839-862): candidate k replaces the kept candidate j (klist[0]
 *   until something is accepted) only where |sf_k| is strictly larger AND gate[j * K + k] != 0; the caller builds
 *   gate (K x K bytes, host) as || klist[j] - klist[k] || < 2 sqrt(2) dk in double.  kidx = -1 where nothing was
 *   accepted (the reference reports klist[0] as 'w' there).                                                   */
int gpa_sweep_grad(gpa_plan* plan, const void* image, const double* kref, const double* klist, int K,
                   double sigma, int grad_mode, void* lockin, int32_t* kidx, void* grad);
int gpa_sweep_grad_dev(gpa_plan* plan, const void* image, const double* kref, const double* klist, int K,
                       double sigma, int grad_mode, void* lockin, int32_t* kidx, void* grad);
int gpa_sweep_gated(gpa_plan* plan, const void* image, const double* kref, const double* klist, int K,
                    double sigma, const uint8_t* gate, void* lockin, int32_t* kidx);

/* a5+a6 -- phases/weights glue and per-pixel weighted least squares.
 *   phases = angle(lockin), weights = |lockin| * (mask + 1e-6), mask = 1 on
 *   [mask_border:-mask_border]^2 (extract_displacement_field,
 *   geometric_phase_analysis.py:922-926); dbdx = wrapToPi(diff along axis 1),
 *   dbdy = wrapToPi(diff along axis 0) (:234-235); per pixel solve
 *   min || w (2 pi kvecs x - b) || (myweighed_lstsq :97-113).
 * lockin: P x n0 x n1 complex; kvecs: P x 2; dudx: 2 x n0 x (n1-1); dudy:
 * 2 x (n0-1) x n1; wnorm: n0 x n1 = || weights ||_2 over peaks (:240), nullable. */
int gpa_reconstruct_grad(gpa_plan* plan, const void* lockin, const double* kvecs, int P,
                         int mask_border, void* dudx, void* dudy, void* wnorm);
int gpa_reconstruct_grad_dev(gpa_plan* plan, const void* lockin, const double* kvecs, int P,
                             int mask_border, void* dudx, void* dudy, void* wnorm);

/* a6 with pre_diff=True (reconstruct_u_inv_from_phases, geometric_phase_analysis.py:228-237): grads
 * (P x n0 x n1 x 2, host) already hold the phase gradients along axis 1 ([..., 0]) and axis 0 ([..., 1]) -- e.g.
 * the `grad` outputs of gpa_sweep; they are wrapped, solved per pixel against 2 pi kvecs with `weights`
 * (P x n0 x n1) and cropped to the difference grids: dudx 2 x n0 x (n1-1), dudy 2 x (n0-1) x n1, wnorm as above. */
int gpa_reconstruct_prediff(gpa_plan* plan, const void* grads, const void* weights, const double* kvecs, int P,
                            void* dudx, void* dudy, void* wnorm);

/* a8 helper -- per-pixel weighted least squares on given right-hand sides:
 * minimise || w (2 pi kvecs x - b) || per pixel; the weighted branch of reconstruct_u_inv
 * (geometric_phase_analysis.py:188 -> myweighed_lstsq :97-113).  b, weights: P x n0 x n1
 * (host), out: 2 x n0 x n1.                                                    */
int gpa_weighted_lstsq(gpa_plan* plan, const void* b, const void* weights, const double* kvecs, int P,
                       void* out);

/* a7 -- DCT-Laplacian weighted least-squares phase unwrap (Ghiglia-Romero PCG)
 * from pre-differenced gradients: replaces phase_unwrap_prediff
 * (phase_unwrap.py:282-350) with helpers :95-132.
 *   dx: n0 x (n1-1), dy: (n0-1) x n1, weight: n0 x n1 or NULL (unweighted),
 *   phi: n0 x n1 output.  Stops after kmax iterations or when
 *   ||r|| < eps ||r0|| (eps = 1e-9 in the reference).  poisson_axes_compat != 0
 *   replicates the reference's swapped-axis eigenvalues (phase_unwrap.py:107-109;
 *   identical for square images; where one side is at least twice the other that
 *   table is singular and the reference returns NaN -- the true eigenvalues are used
 *   there).  The f32 build floors eps at 4e-6 (what an f32 recurrence can reach).
 *   *iters_out receives the iteration count.                                    */
int gpa_unwrap_prediff(gpa_plan* plan, const void* dx, const void* dy, const void* weight,
                       int kmax, double eps, int poisson_axes_compat, void* phi, int* iters_out);
int gpa_unwrap_prediff_dev(gpa_plan* plan, const void* dx, const void* dy, const void* weight,
                           int kmax, double eps, int poisson_axes_compat, void* phi,
                           int* iters_out);
/* the two halves of gpa_unwrap_prediff_dev for callers that overlap a global unwrap with other work on the same GPU
 * (the image-pipelined multi-GPU schedule, pygpa_amd/distributed.py): `_enqueue_dev` puts the whole solve on the
 * plan's stream and returns at once; gpa_unwrap_finish waits for it and hands back the iteration count.  One solve
 * in flight per plan.                                                                                        */
int gpa_unwrap_prediff_enqueue_dev(gpa_plan* plan, const void* dx, const void* dy, const void* weight,
                                   int kmax, double eps, int poisson_axes_compat, void* phi);
int gpa_unwrap_finish(gpa_plan* plan, int* iters_out);
/* same from a wrapped phase image psi (phase_unwrap.py:141-208) */
int gpa_unwrap(gpa_plan* plan, const void* psi, const void* weight, int kmax, double eps,
               int poisson_axes_compat, void* phi, int* iters_out);
/* ... on device pointers (psi, weight, phi: n0 x n1 of the plan's dtype; phi must not overlap psi or weight).  Waits for
 * the solve (the iteration count is its last word); gpa_unwrap is upload + this + download.                              */
int gpa_unwrap_dev(gpa_plan* plan, const void* psi, const void* weight, int kmax, double eps,
                   int poisson_axes_compat, void* phi, int* iters_out);

/* A stack of nb phase maps of the plan's shape, unwrapped as ONE set of kernel launches (problem = blockIdx.z): a small
 * frame is bound by the chain of 4 - 5 dependent launches per PCG iteration, which the stack shares.  No counterpart in
 * the reference, where a loop over phase_unwrap (phase_unwrap.py:141-208) or phase_unwrap_prediff (:282-350) gives the
 * same numbers.  Every problem keeps its own stopping test and guards; problem b's phi and iteration count are those of
 * gpa_unwrap_dev / gpa_unwrap_prediff_dev on its planes, bit for bit where both run the same kernels (nb <= 2, or the
 * option NO_LAT: a single frame of up to 1024 points a side otherwise takes latency-tuned kernels that agree to rounding).
 *   psi: nb x n0 x n1;  dx: nb x n0 x (n1 - 1), dy: nb x (n0 - 1) x n1;  phi: nb x n0 x n1, overlapping no input.
 *   weight_planes: 0 (weight must be NULL: unweighted), 1 (one n0 x n1 plane for all problems) or nb (one plane each).
 *   nb: 1 ... GPA_UNWRAP_BATCH_MAX.  iters_out: nb counts.
 * A call whose work space would pass 2 GiB (option UNWRAP_STACK_BYTES=<bytes>: another bound) runs in chunks of problems
 * inside the call, each chunk one set of launches with the kernels of the whole call: chunking changes no bit.  The work
 * space is the plan's ONE batched unwrap workspace, shared with gpa_extract_displacement_field_batch_dev, grown to the
 * largest need seen and counted in gpa_plan_workspace_bytes; offsets into the stack are 64-bit.
 * _dev: device pointers on the plan's stream; iters_out == NULL only enqueues, gpa_unwrap_batch_finish then waits and
 * hands over the nb counts of the last batch call.  The host-pointer forms stage one chunk at a time.
 * Errors: GPA_ERR_ARG naming the argument, before anything is launched; GPA_ERR_STATE for plans without unwrap kernels
 * and for shapes where gpa_supports_batch says 0 (loop over the single call there).
 * gpa_unwrap_batch_problem_bytes: device bytes one problem of a kmax-iteration solve takes in that workspace (what the
 * chunk size divides the bound by); 0 for a plan without unwrap kernels.                                               */
#define GPA_UNWRAP_BATCH_MAX 4096
int gpa_unwrap_batch_dev(gpa_plan* plan, const void* psi, int nb, const void* weight, int weight_planes,
                         int kmax, double eps, int poisson_axes_compat, void* phi, int* iters_out);
int gpa_unwrap_prediff_batch_dev(gpa_plan* plan, const void* dx, const void* dy, int nb, const void* weight,
                                 int weight_planes, int kmax, double eps, int poisson_axes_compat, void* phi,
                                 int* iters_out);
int gpa_unwrap_batch_finish(gpa_plan* plan, int nb, int* iters_out);
int gpa_unwrap_batch(gpa_plan* plan, const void* psi, int nb, const void* weight, int weight_planes,
                     int kmax, double eps, int poisson_axes_compat, void* phi, int* iters_out);
int gpa_unwrap_prediff_batch(gpa_plan* plan, const void* dx, const void* dy, int nb, const void* weight,
                             int weight_planes, int kmax, double eps, int poisson_axes_compat, void* phi,
                             int* iters_out);
size_t gpa_unwrap_batch_problem_bytes(gpa_plan* plan, int kmax);

/* fused driver: extract_displacement_field (geometric_phase_analysis.py:907-932,
 * deconvolve=False) with every intermediate kept in HBM.
 *   image : n0 x n1 (its mean is subtracted on the device, :919)
 *   kvecs : P x 2 peak centres; klists: P x K x 2 host-built candidate lists
 *   sigma : Gaussian width; mask_border = 2*sigma in the reference (:924)
 *   kmax  : PCG iterations of the weighted unwrap (10 in the reference, :241)
 *   u     : 2 x n0 x n1 output;  lockins (P x n0 x n1 complex) and kidx
 *           (P x n0 x n1 int32) optional outputs;  iters_out[2] optional.
 * P*K <= max_batch.                                                           */
int gpa_extract_displacement_field(gpa_plan* plan, const void* image, const double* kvecs, int P,
                                   const double* klists, int K, double sigma, int mask_border,
                                   int kmax, void* u, void* lockins, int32_t* kidx,
                                   int* iters_out);
int gpa_extract_displacement_field_dev(gpa_plan* plan, const void* image, const double* kvecs,
                                       int P, const double* klists, int K, double sigma,
                                       int mask_border, int kmax, void* u, void* lockins,
                                       int32_t* kidx, int* iters_out);

/* Asynchronous form of the fused driver (device pointers): enqueues everything on the plan's
 * streams and returns without waiting, so that several plans (one per image in flight) overlap
 * on the GPU -- the VALU-bound sweep of one image runs beside the bandwidth-bound unwrap of
 * another.  Calls on ONE plan still execute in order.  gpa_plan_sync() waits for completion,
 * gpa_last_iters() (which synchronises) returns the two PCG iteration counts of the last call. */
int gpa_extract_displacement_field_async(gpa_plan* plan, const void* image, const double* kvecs, int P,
                                         const double* klists, int K, double sigma, int mask_border,
                                         int kmax, void* u, void* lockins, int32_t* kidx);
int gpa_last_iters(gpa_plan* plan, int* iters2);

/* The fused driver that also hands out what ONE sweep knows about every peak: extract_displacement_field with
 * return_gs=True and a gradient sweep as wfr_func -- wfr2_grad_opt / wfr2_grad_vec (geometric_phase_analysis.py:763-836),
 * cuGPA.wfr2_grad_opt / wfr2_grad_single (cuGPA.py:41-133), the reference's drop-in call (tests/test_cuGPA.py:46-56,
 * geometric_phase_analysis.py:919-922) -- whose g['grad'] and |g['lockin']| feed property_extract.phasegradient2J
 * (property_extract.py:69-101).  Arguments as gpa_extract_displacement_field, and
 *   grad_mode : the stencil of gpa_sweep_grad (0 np.gradient, 1 / 2 forward differences)
 *   grads     : P x n0 x n1 x 2 phase gradients of the winners (the `grad` of gpa_sweep per peak), nullable
 *   absw      : P x n0 x n1 reals |lockins| (the weights of phasegradient2J), nullable
 * lockins and kidx are nullable as before.  With grads != NULL pass B writes the phase of all P K candidates to plan
 * scratch (P K n0 n1 reals, allocated by the first such call) and one stencil launch serves the P peaks; with grads ==
 * NULL and absw == NULL the call enqueues exactly the launches of gpa_extract_displacement_field_dev.
 * The three forms: host pointers; device pointers, synchronising; device pointers, enqueue only (gpa_last_iters). */
int gpa_extract_displacement_field_grad(gpa_plan* plan, const void* image, const double* kvecs, int P,
                                        const double* klists, int K, double sigma, int mask_border, int kmax,
                                        int grad_mode, void* u, void* lockins, int32_t* kidx, void* grads,
                                        void* absw, int* iters_out);
int gpa_extract_displacement_field_grad_dev(gpa_plan* plan, const void* image, const double* kvecs, int P,
                                            const double* klists, int K, double sigma, int mask_border, int kmax,
                                            int grad_mode, void* u, void* lockins, int32_t* kidx, void* grads,
                                            void* absw, int* iters_out);
int gpa_extract_displacement_field_grad_async(gpa_plan* plan, const void* image, const double* kvecs, int P,
                                              const double* klists, int K, double sigma, int mask_border, int kmax,
                                              int grad_mode, void* u, void* lockins, int32_t* kidx, void* grads,
                                              void* absw);

/* A STACK of images of the plan's shape in one call (device pointers; no counterpart in the reference,
 * whose extract_displacement_field (geometric_phase_analysis.py:907-932) takes one image): images
 * B x n0 x n1, u B x 2 x n0 x n1.  The sweep and the least squares run image after image; the 2 B
 * weighted unwraps (phase_unwrap.py:282-350) share one set of kernel launches, which is what bounds a
 * small image.  Results equal B separate gpa_extract_displacement_field_dev calls bit for bit.
 * iters_out: 2 B iteration counts, or NULL to return without synchronising (gpa_plan_sync).         */
int gpa_extract_displacement_field_batch_dev(gpa_plan* plan, const void* images, int B,
                                             const double* kvecs, int P, const double* klists, int K,
                                             double sigma, int mask_border, int kmax, void* u,
                                             int* iters_out);
/* The stack call that also hands out what the sweep knows, per frame: the arguments of
 * gpa_extract_displacement_field_batch_dev (the same B range) and the optional outputs of
 * gpa_extract_displacement_field_grad_dev with one leading frame axis each -- lockins B x P x n0 x n1 complex, kidx
 * B x P x n0 x n1 int32, grads B x P x n0 x n1 x 2, absw B x P x n0 x n1 -- each nullable.  Frame b's outputs are those of
 * gpa_extract_displacement_field_grad_dev on frame b, bit for bit.  With all four NULL the call enqueues exactly what
 * gpa_extract_displacement_field_batch_dev enqueues.  With grads != NULL a chunk of frames is one set of launches for pass A,
 * pass B with phases, the stencil, |lock-in| and the unwrap set-up, and the 2 B unwraps stay one chain; the candidate phases
 * of a chunk (chunk x P K n0 n1 reals of plan scratch, counted in gpa_plan_workspace_bytes) bound the chunk at ~3 GB, as
 * the x-planes do.  iters_out NULL: no synchronisation, gpa_last_batch_iters reads the counts.  Shapes for which
 * gpa_supports_batch answers 0 are refused (GPA_ERR_STATE).                                                             */
int gpa_extract_displacement_field_grad_batch_dev(gpa_plan* plan, const void* images, int B,
                                                  const double* kvecs, int P, const double* klists, int K,
                                                  double sigma, int mask_border, int kmax, int grad_mode, void* u,
                                                  void* lockins, int32_t* kidx, void* grads, void* absw,
                                                  int* iters_out);
/* waits for the plan's stream and returns the 2 B iteration counts of the last batch call (B <= its stack size) */
int gpa_last_batch_iters(gpa_plan* plan, int B, int* iters_out);
/* 1 if the batch call above covers the plan's image shape (every shape whose unwrap runs the fused
 * iteration), 0 if the caller has to loop over gpa_extract_displacement_field_dev instead            */
int gpa_supports_batch(gpa_plan* plan);

/* tile stage of the multi-GPU path: sweep + phases/weights + per-pixel least squares of
 * extract_displacement_field (:919-926, :234-237) WITHOUT the unwrap; the gradient tiles of all
 * ranks are stitched and unwrapped once globally.  The image is used
 * as given (the caller subtracts the mean of the WHOLE image from its tiles).  Host pointers;
 * dudx: 2 x n0 x (n1-1), dudy: 2 x (n0-1) x n1, wnorm: n0 x n1.                  */
int gpa_extract_gradients(gpa_plan* plan, const void* image, const double* kvecs, int P,
                          const double* klists, int K, double sigma, int mask_border, void* dudx,
                          void* dudy, void* wnorm);

/* device-resident tile stage (BASELINE configs 4-5): the window [r0, r0+n0) x [c0, c0+n1) of a
 * larger image that lives on the device (row pitch image_pitch, in elements) is analysed like
 * gpa_extract_gradients with `mean` (of the whole image, e.g. from gpa_mean_dev) subtracted, and
 * the interior rectangle [i0, i0+t0) x [j0, j0+t1) (window coordinates) of dudx / dudy / wnorm is
 * written to dx / dy / wn: 2 planes each for dx, dy (plane stride *_plane, row pitch *_pitch,
 * elements), clipped to the one-short last column / row of the window's difference fields.  The
 * destinations may be compact per-tile buffers (to be all-gathered) or the stitched fields of the
 * whole image.  Asynchronous on the plan's stream (gpa_plan_sync).                            */
int gpa_mean_dev(gpa_plan* plan, const void* data, size_t count, double* mean_out);
int gpa_tile_gradients_dev(gpa_plan* plan, const void* image, size_t image_pitch, int r0, int c0,
                           double mean, const double* kvecs, int P, const double* klists, int K,
                           double sigma, int mask_border, int i0, int j0, int t0, int t1, void* dx,
                           size_t dx_pitch, size_t dx_plane, void* dy, size_t dy_pitch,
                           size_t dy_plane, void* wn, size_t wn_pitch);

/* The tile pipeline's own data path (SURVEY.md 8(b) "gpa_extract_sharded", 8(e) option 2; no counterpart in the
 * reference, whose only batching is the dask k-batch, geometric_phase_analysis.py:705-719).  Everything below is
 * asynchronous on the plan's stream and leaves its result on the device: an image goes through
 * pygpa_amd.distributed.TiledPipeline without a host synchronisation between its stages.
 *
 * gpa_tile_sums_dev: sum over the interior rectangles of `ntiles` windows that lie win_stride elements apart (row
 *   pitch win_pitch): rects_dev = ntiles x (o0, o1, z0, z1) ints ON THE DEVICE, max_rows >= every z0, the sum as ONE
 *   double at sum_dev (fixed summation order: reruns are bit-identical).  The ranks all-reduce these sums.
 * gpa_tile_set_mean_dev: the plan's tile mean = sum_dev[0] * scale (scale = 1 / pixels of the whole image): what
 *   gpa_tile_gradients_meandev_dev subtracts (geometric_phase_analysis.py:919) instead of a host-side value.
 * gpa_tile_gradients_meandev_dev: gpa_tile_gradients_dev with that mean; a window whose pitch equals the plan's n1 is
 *   read in place; wn_plane != 0 writes a second copy of the weight wn_plane elements behind the first (each unwrap
 *   owner receives its component's two gradients AND the weight as one contiguous block).
 * gpa_stitch_tiles_dev: tiles[slot][f] (t0 x t1 elements, pitch tile_pitch; slots slot_stride and fields field_stride
 *   elements apart) -> dst[f] (host array of nf <= 6 device pointers) at (r0, c0) of table_dev = ntiles x (slot, r0, c0,
 *   z0, z1) ints on the device, clipped to dst_rows[f] x dst_cols[f] (the difference fields are one column / row
 *   short of the image).  One launch for all tiles and fields.
 * gpa_plan_wait_stream / gpa_stream_wait_plan: the plan's stream waits for the work enqueued so far on `stream` (a
 *   hipStream_t as an opaque pointer, NULL = the default stream; e.g. torch.cuda.current_stream().cuda_stream, on
 *   which the RCCL collectives are ordered) and the other way round -- events, no host synchronisation.          */
int gpa_tile_sums_dev(gpa_plan* plan, const void* wins, size_t win_stride, size_t win_pitch, const int* rects_dev,
                      int ntiles, int max_rows, double* sum_dev);
int gpa_tile_set_mean_dev(gpa_plan* plan, const double* sum_dev, double scale);
int gpa_tile_gradients_meandev_dev(gpa_plan* plan, const void* image, size_t image_pitch, int r0, int c0,
                                   const double* kvecs, int P, const double* klists, int K, double sigma,
                                   int mask_border, int i0, int j0, int t0, int t1, void* dx, size_t dx_pitch,
                                   size_t dx_plane, void* dy, size_t dy_pitch, size_t dy_plane, void* wn,
                                   size_t wn_pitch, size_t wn_plane);
int gpa_stitch_tiles_dev(gpa_plan* plan, const void* tiles, size_t slot_stride, size_t field_stride,
                         size_t tile_pitch, const int* table_dev, int ntiles, int t0, int t1, int nf,
                         void* const* dst, const size_t* dst_pitch, const int* dst_rows, const int* dst_cols);
int gpa_plan_wait_stream(gpa_plan* plan, void* stream);
int gpa_stream_wait_plan(gpa_plan* plan, void* stream);

/* f-1 -- Lawler-Fujita undistortion.
 * gpa_invert_u_overlap: fixed-point inverse of a displacement field, `iters` rounds of cubic-
 *   spline resampling with mode='nearest' on the grid extended by `edge` pixels; replaces
 *   invert_u_overlap (geometric_phase_analysis.py:262-300).  u: 2 x n0 x n1 (host),
 *   out: 2 x (n0+2 edge) x (n1+2 edge).
 * gpa_undistort_image: out = deformed resampled at r + invert_u_overlap(-u)(r) with
 *   scipy.ndimage.map_coordinates' defaults (order 3, mode='constant', cval=0); replaces
 *   undistort_image (:935-974).  deformed, out: n0 x n1.                          */
int gpa_invert_u_overlap(gpa_plan* plan, const void* u, int iters, int edge, void* out);
/* invert_u (geometric_phase_analysis.py:248-259), the variant without overlap: out is 2 x n0 x n1 and every
 * round after the first samples at r + u_it(r) - edge.                                              */
int gpa_invert_u(gpa_plan* plan, const void* u, int iters, int edge, void* out);
/* both with scipy.ndimage's boundary mode as an argument (the `mode=` keyword of the two reference functions):
 * mode 0 = 'nearest' (their default, what the two entry points above run), 1 = 'constant' (cval 0; the last round of
 * invert_u_overlap passes cval = nan, geometric_phase_analysis.py:297-299), 2 = 'reflect' / 'grid-mirror', 3 = 'mirror',
 * 4 = 'grid-wrap' (coordinate and taps folded by the mode's extension; cval is never used: no NaN).  Any other code is
 * GPA_ERR_ARG.  'reflect' is the exact half-sample symmetric spline; SciPy's own 'reflect' prefilter differs from it on
 * axes shorter than 12 samples (3.7e-6 of the field at n = 4, rounding from n = 12).  SciPy's 'wrap' (legacy: coordinates
 * of period n - 1 over coefficients of period n) and 'grid-constant' (all NaN from the reference's cval = nan round) have
 * no code.  overlap != 0: invert_u_overlap.                                                                       */
int gpa_invert_u_mode(gpa_plan* plan, const void* u, int iters, int edge, int overlap, int mode, void* out);
int gpa_undistort_image(gpa_plan* plan, const void* deformed, const void* u, void* out);
/* The same on device pointers, enqueued on the plan's stream WITHOUT a host synchronisation (gpa_plan_sync, or
 * gpa_stream_wait_plan for another stream); scratch is kept by the plan.  gpa_invert_u_mode_dev inverts scale * u
 * (undistort_image passes -u: scale = -1).  rects = nrect x {r0, c0, h, w} (host ints; nrect = 0: the whole grid) restricts
 * the fixed-point rounds and the resampling to those windows of the output grid -- the tiles a rank owns once it holds the
 * stitched field; the rest of out_dev is left untouched, the spline prefilter of the whole field runs once per call.
 * gpa_undistort_image_dev: uinv_dev (2 x n0 x n1, nullable) receives u_inv.                                           */
int gpa_invert_u_mode_dev(gpa_plan* plan, const void* u_dev, double scale, int iters, int edge, int overlap, int mode,
                          const int* rects, int nrect, void* out_dev);
int gpa_undistort_image_dev(gpa_plan* plan, const void* deformed_dev, const void* u_dev, const int* rects, int nrect,
                            void* uinv_dev, void* out_dev);
/* undistort_image(deformed, scale * u) on device pointers: scale = -1 undistorts with the field exactly as
 * extract_displacement_field returns it (the reference's tests recover the true displacement as MINUS that field,
 * tests/test_geometric_phase_analysis.py:63, and undistort with the true one, :76).                                   */
int gpa_undistort_image_scaled_dev(gpa_plan* plan, const void* deformed_dev, const void* u_dev, double scale,
                                   const int* rects, int nrect, void* uinv_dev, void* out_dev);
/* undistort_image of a STACK of B frames (B x n0 x n1, contiguous; 1 <= B <= 65535, else GPA_ERR_ARG) in one call -- no
 * counterpart in the reference, where a loop over undistort_image (geometric_phase_analysis.py:935-974) gives the same
 * numbers.  u_per_frame == 0: u is 2 x n0 x n1, one field for every frame (a static detector distortion): it is
 * prefiltered and inverted ONCE, the spline weights of a pixel are shared by the frames.  u_per_frame != 0: u is
 * B x 2 x n0 x n1 (the output of gpa_extract_displacement_field_batch_dev as it stands: scale = -1), inverted in one set
 * of launches per chunk.  uinv_dev (nullable) receives u_inv in the layout of u.  Frame b's result is bitwise what
 * gpa_undistort_image_scaled_dev gives for it alone.  The frames pass through the plan's scratch in chunks whose spline
 * planes fit 512 MiB (one frame at least; counted in gpa_plan_workspace_bytes); offsets into the stack are 64-bit.
 * _dev: device pointers, enqueued on the plan's stream without a host synchronisation.  The host-pointer form undistorts
 * with u itself (scale = 1), like gpa_undistort_image.                                                                */
#define GPA_UNDISTORT_MAX_FRAMES 65535
int gpa_undistort_image_batch_dev(gpa_plan* plan, const void* frames_dev, int B, const void* u_dev, int u_per_frame,
                                  double scale, void* uinv_dev, void* out_dev);
int gpa_undistort_image_batch(gpa_plan* plan, const void* frames, int B, const void* u, int u_per_frame, void* out);

/* f-2 -- phase gradient -> Jacobian -> lattice properties.
 * gpa_phasegradient2J: J[n,m,i,j] = (per-pixel weighted least squares of grads[:,n,m,j] against
 *   2 pi kvecs)_i / nmperpixel; replaces phasegradient2J (property_extract.py:69-101).
 *   dks == NULL is iso_ref=False; with dks (P x 2, = calc_diff_from_isotropic(kvecs)) the
 *   gradients are taken relative to the isotropic lattice: K = 2 pi (kvecs + dks) and
 *   g <- wrapToPi(g - 2 pi dk) (:87-92).  grads: P x n0 x n1 x 2 (the `grad` output of
 *   gpa_sweep per peak), weights: P x n0 x n1, J: n0 x n1 x 2 x 2.
 * gpa_props_from_jac: (angle [deg], aniangle [deg, mod 180], alpha, kappa) per pixel from the 2x2
 *   Jacobian (+ identity when add_identity != 0, i.e. phasegradient2Jac :104-111); replaces
 *   props_from_Jac (:137-178).  Needs no plan: jac is npx x 2 x 2 for any number of pixels,
 *   props 4 x npx.
 * The _dev variants take device pointers and run asynchronously (on the plan's stream, or on
 * the given hipStream_t for gpa_props_from_jac_dev).                                        */
int gpa_phasegradient2J(gpa_plan* plan, const double* kvecs, int P, const void* grads,
                        const void* weights, double nmperpixel, const double* dks, void* J);
int gpa_phasegradient2J_dev(gpa_plan* plan, const double* kvecs, int P, const void* grads,
                            const void* weights, double nmperpixel, const double* dks, void* J);
/* np.abs of P lock-ins (P x n0 x n1 complex -> P x n0 x n1 real), the `weights` the reference's callers hand to
 * phasegradient2J (property_extract.py:69); device pointers, on the plan's stream.                              */
int gpa_lockin_weights_dev(gpa_plan* plan, const void* lockins, int P, void* weights);
int gpa_props_from_jac(int device, int dtype, size_t npx, const void* jac, int add_identity,
                       double refangle, double refscale, int diff, void* props);
int gpa_props_from_jac_dev(int device, int dtype, size_t npx, const void* jac, int add_identity,
                           double refangle, double refscale, int diff, void* props,
                           void* stream);

/* Per-pixel Kerelsky fits -- twist theta, strain direction psi, heterostrain eps and lattice angle xi (degrees, eps a ratio)
 * from the displacement-gradient field; replaces Kerelsky_J's per-pixel least squares (property_extract.py:780-883) and, with
 * npx = 1, its global fit and Kerelsky_Jac's (:707-777).  Per pixel, with W(a) the rotation by a, D(e) = diag(1/(1+e),
 * 1/(1-0.16 e)) and V = W(psi), it minimises |1000 vec(V^T D V W(theta+xi) - W(xi) - A)|^2 / 2 over theta >= 0, eps >= 0 by a
 * bounded Levenberg-Marquardt iteration with the analytic Jacobian, in f64 whatever the dtype (csrc/gpa_kerelsky.h).
 *   jac   npx x 2 x 2 in the dtype: J when a0 is given, and then A = a0 + a0 J is formed per pixel; A itself when a0 is NULL
 *   a0    4 doubles (2 x 2, row-major) or NULL
 *   x0    the start (theta, psi, eps, xi), theta >= 0 and eps >= 0
 *   max_nfev    trial evaluations per start, >= 1 (the reference's default: 50)
 *   retry_cost  further starts -- psi + 90 degrees, then the closed-form root where one exists -- are tried while the best
 *               cost exceeds this (the reference: 1e-5 per pixel, 1e-20 in the global fits); the best result is kept
 *   out   npx x 4 in the dtype: theta, psi (the representative within 90 degrees of x0's), eps, xi (within 180 of x0's);
 *         theta >= 0 and eps >= 0 exactly
 *   cost  npx doubles, the cost at out before rounding to the dtype; may be NULL
 * A pixel whose A is not finite gives four NaNs and a NaN cost (the reference raises there).  Needs no plan.  Argument errors
 * (GPA_ERR_ARG) name the argument and come before any device is touched.  _dev: device pointers (a0 and x0 stay host
 * pointers), asynchronous on the given hipStream_t.                                                                       */
#define GPA_KERELSKY_MAX_NPX 0x1000000000ull
int gpa_kerelsky_fit(int device, int dtype, size_t npx, const void* jac, const double* a0,
                     const double* x0, int max_nfev, double retry_cost, void* out, double* cost);
int gpa_kerelsky_fit_dev(int device, int dtype, size_t npx, const void* jac, const double* a0,
                         const double* x0, int max_nfev, double retry_cost, void* out, double* cost,
                         void* stream);

/* Jacobian J = grad(-u) and lattice-property maps straight from a displacement field or from phases, one pass over the data;
 * replaces u2J / u2Jac (property_extract.py:13-26), phases2J / phases2Jac (:29-52), calc_props_from_phases (:258-278) and
 * phys_props_from_Jac (:181-217).  None needs a plan.
 * gpa_field_jacobian: u is nimg x 2 x n0 x n1; J[f, n, m, c, a] = np.gradient(-u[f, c], nmperpixel, axis=a), nimg x n0 x n1 x 2 x 2:
 *   central differences over 2 nmperpixel inside, one-sided ones over nmperpixel at the first and last sample of an axis, each
 *   one subtraction and one division by the divisor rounded to the dtype.  Frames are independent.
 * gpa_phases_jacobian: phases and weights are P x n0 x n1, 2 <= P <= 8, kvecs P x 2 (host).  Per peak and axis
 *   b = wrapToPi(2 np.gradient(phase)) / 2 / nmperpixel; J = -(per-pixel weighted least squares of b against 2 pi kvecs), the solve
 *   of gpa_phasegradient2J; 0 where every weight is 0.
 * Both: J and props may each be NULL, not both.  With add_identity the stored J is I + J (the ...Jac spellings).  props is
 *   nimg x 4 x n0 x n1 = gpa_props_from_jac(add_identity = 1) of the plain J, bit for bit, with the same refangle, refscale, diff.
 *   A device J must be aligned to 4 elements.  An output must not overlap an input or the other output.
 * gpa_phys_props_from_jac: jac npx x 2 x 2 -> props 4 x npx = (angle + refangle, aniangle, alpha refscale, epsilon) with
 *   epsilon = (s0 - s1) / (s0 + poisson_ratio s1) of the singular values s0 >= s1, alpha = s1 (1 + epsilon), or
 *   s0 / (1 + epsilon) with diff (which also turns aniangle by 90 degrees before the mod 180).
 * Argument errors (GPA_ERR_ARG) name the argument and come before any device is touched: an axis < 2, nimg < 1, P outside
 * 2 ... 8, nmperpixel zero or not finite, both outputs NULL, overlapping buffers.  _dev: device pointers (kvecs stays a host
 * pointer), asynchronous on the given hipStream_t, no allocation and no synchronisation.                                    */
int gpa_field_jacobian(int device, int dtype, int nimg, int n0, int n1, const void* u, double nmperpixel,
                       int add_identity, void* J, void* props, double refangle, double refscale, int diff);
int gpa_field_jacobian_dev(int device, int dtype, int nimg, int n0, int n1, const void* u, double nmperpixel,
                           int add_identity, void* J, void* props, double refangle, double refscale, int diff,
                           void* stream);
int gpa_phases_jacobian(int device, int dtype, int n0, int n1, int P, const double* kvecs, const void* phases,
                        const void* weights, double nmperpixel, int add_identity, void* J, void* props,
                        double refangle, double refscale, int diff);
int gpa_phases_jacobian_dev(int device, int dtype, int n0, int n1, int P, const double* kvecs, const void* phases,
                            const void* weights, double nmperpixel, int add_identity, void* J, void* props,
                            double refangle, double refscale, int diff, void* stream);
/* gpa_gradients_jacobian: the third source, the phase gradients and weights a one-sweep driver call hands out
 * (gpa_extract_displacement_field_grad*), for a stack of frames and without a plan.  grads is nimg x P x n0 x n1 x 2, weights
 * nimg x P x n0 x n1, 2 <= P <= 8, n0, n1 >= 1 with n0 n1 < 2^31; kvecs P x 2 (host); dks NULL or P x 2 (host) with the iso_ref
 * meaning of gpa_phasegradient2J: g <- wrapToPi(g - 2 pi dk) against 2 pi (kvecs + dks).  J (nimg x n0 x n1 x 2 x 2) is
 * gpa_phasegradient2J's of every frame, bit for bit (I + J with add_identity), 0 where every weight of a pixel is 0; props
 * (nimg x 4 x n0 x n1) is gpa_props_from_jac(add_identity = 1) of the plain J, bit for bit.  Either may be NULL, not both: with
 * props alone J never goes to memory (3 P reals in and 4 out per pixel, against 3 P + 12 of the two-kernel chain).  A device
 * J must be aligned to 4 elements, device grads to 2.  Errors as above (an axis < 1 here).                                  */
int gpa_gradients_jacobian(int device, int dtype, int nimg, int n0, int n1, int P, const double* kvecs,
                           const double* dks, const void* grads, const void* weights, double nmperpixel,
                           int add_identity, void* J, void* props, double refangle, double refscale, int diff);
int gpa_gradients_jacobian_dev(int device, int dtype, int nimg, int n0, int n1, int P, const double* kvecs,
                               const double* dks, const void* grads, const void* weights, double nmperpixel,
                               int add_identity, void* J, void* props, double refangle, double refscale, int diff,
                               void* stream);
int gpa_phys_props_from_jac(int device, int dtype, size_t npx, const void* jac, int add_identity, double refangle,
                            double refscale, int diff, double poisson_ratio, void* props);
int gpa_phys_props_from_jac_dev(int device, int dtype, size_t npx, const void* jac, int add_identity,
                                double refangle, double refscale, int diff, double poisson_ratio, void* props,
                                void* stream);

/* f-4 -- robust plane fit a0*x + a1*y + a2 (x = row, y = column index) through an n0 x n1 map:
 * the minimiser of the Huber cost that fit_plane (mathtools.py:30-47, scipy least_squares with
 * loss='huber', f_scale 1, start at 0) approaches, by iteratively reweighted least squares with the
 * per-iteration sums reduced on the device.  Stops when the plane changes by <= tol (sum of the
 * three coefficient changes in centred unit coordinates) or after max_iter passes.             */
int gpa_fit_plane(gpa_plan* plan, const void* image, int max_iter, double tol, double* coef3,
                  int* iters_out);
int gpa_fit_plane_dev(gpa_plan* plan, const void* image, int max_iter, double tol, double* coef3,
                      int* iters_out);
/* the same fit of P contiguous planes of the plan's shape (device, P x n0 x n1; 1 <= P <= 65535): every IRLS round is one
 * launch pair and one synchronisation for all planes that have not converged yet; a plane that has keeps its coefficients.
 * coef: P x 3 and iters_out (nullable): P, host.  Plane q gets the coefficients and the pass count gpa_fit_plane_dev gives
 * for it alone, bit for bit.                                                                                              */
int gpa_fit_planes_dev(gpa_plan* plan, const void* images, int P, int max_iter, double tol, double* coef,
                       int* iters_out);

/* a8 -- iterate_GPA (geometric_phase_analysis.py:116-154) on device memory.
 * gpa_lockin_polar_crop_dev: P lock-ins on the plan's n0 x n1 grid (device, complex) -> the window
 * [edge : n0 - edge, edge : n1 - edge] as compact m0 x m1 planes (m = n - 2 edge): psi = angle, amp = |lock-in|, and, where
 * weight is not NULL, weight = sqrt(amp / amax[p]).  amax (device, P reals of the plan's dtype) receives the maximum of
 * amp[p] over the WINDOW (:141), whatever the order the workgroups finish in.  Enqueued on the plan's stream.              */
int gpa_lockin_polar_crop_dev(gpa_plan* plan, const void* lockins, int P, int edge, void* psi, void* amp,
                              void* weight, void* amax);
/* The whole loop.  image: n0 x n1, its mean already subtracted by the caller as in the reference; kvecs: P x 2 (host);
 * prs, w: P x m0 x m1 -- the unwrapped phases and the un-normalised amplitudes of the final pass; corr (P x 2), delta_ks
 * (nullable, iters x P x 2: what each pass subtracted from corr) and unwrap_iters (nullable, (iters + 1) x P) are host
 * memory.  plan has the frame's shape and max_batch >= P; crop_plan has the window's shape m0 x m1, the same dtype and
 * device (edge = 0: plan itself, or NULL).  Each of the iters + 1 passes: lock-ins at kvecs + corr, polar crop, P weighted
 * unwraps (kmax_iter iterations, kmax in the last pass; eps 1e-9, the reference's swapped-axis eigenvalues) and, except in
 * the last pass, the Huber plane fits whose slopes / 2 pi are subtracted from corr -- in double on the host.  Inside a pass
 * only the unwraps' iteration counts and the fits' sums come to the host.  Both forms return when everything is done.
 * GPA_ERR_ARG names the offending argument; GPA_ERR_STATE says whether plan (a frame the sweep does not take) or crop_plan
 * (a window without unwrap kernels) refuses -- nothing has been launched then.  With gpa_set_profiling on, gpa_last_stage_ms
 * of plan gives [0] lock-ins [1] polar crop [2] unwraps [3] plane fits (wall time, every stage waited for).               */
int gpa_iterate_gpa_dev(gpa_plan* plan, gpa_plan* crop_plan, const void* image, const double* kvecs, int P,
                        double sigma, int edge, int iters, int kmax_iter, int kmax, void* prs, void* w,
                        double* corr, double* delta_ks, int* unwrap_iters);
/* image, prs, w in host memory */
int gpa_iterate_gpa(gpa_plan* plan, gpa_plan* crop_plan, const void* image, const double* kvecs, int P,
                    double sigma, int edge, int iters, int kmax_iter, int kmax, void* prs, void* w,
                    double* corr, double* delta_ks, int* unwrap_iters);

/* gaussian_deconvolve (geometric_phase_analysis.py:892-904) of ONE field: reflect-pad by 2 dr,
 * Wiener-Hunt deconvolution (skimage.restoration.wiener, Laplacian regulariser, `balance`) with the
 * Gaussian the lock-ins were smoothed by, crop.  The plan has the PADDED shape
 * (m0 + 4 dr) x (m1 + 4 dr); data, out: m0 x m1 (host).                                       */
int gpa_gaussian_deconvolve(gpa_plan* plan, const void* data, int dr, double sigma, double balance,
                            void* out);
/* the same on device pointers (d_data, d_out: m0 x m1 reals), on the plan's stream; returns after the stream has drained */
int gpa_gaussian_deconvolve_dev(gpa_plan* plan, const void* d_data, int dr, double sigma, double balance,
                                void* d_out);

/* a9 -- DFT of the periodic component of Moisan's periodic+smooth decomposition
 * (third-party moisan2011.per(image, inverse_dft=False)[0], call site
 * geometric_phase_analysis.py:429).  out: n0 x n1 complex.                    */
int gpa_per_dft(gpa_plan* plan, const void* image, void* out);
/* the same on device pointers, enqueued on the plan's stream (no host synchronisation); d_image is not modified.
 * Image sizes: every axis length 1 ... 65536 in both precisions (gpa_dft.h: a power of two up to 16384 (f32) / 8192 (f64)
 * runs the register FFT at its own length, other lengths a chirp-z transform, in one workgroup while 2n - 1 <= 16384 / 8192
 * and as a two-level transform through HBM beyond).                                                                        */
int gpa_per_dft_dev(gpa_plan* plan, const void* d_image, void* d_out);

/* a9, the whole of moisan2011.per(image, inverse_dft) (the reference imports it at
 * geometric_phase_analysis.py:9 and calls it at :429 with inverse_dft=False):
 * inverse_dft == 0: p_out, s_out = DFTs of the periodic and the smooth component (n0 x n1 complex; s_out may be NULL);
 * inverse_dft != 0: p_out, s_out = the two components themselves (n0 x n1 real), p + s = image.      */
int gpa_per(gpa_plan* plan, const void* image, int inverse_dft, void* p_out, void* s_out);

/* f-3 -- Bragg-peak candidates, the array work of extract_primary_ks
 * (geometric_phase_analysis.py:427-437): smooth = gaussian_filter(|fftshift(per_dft(image - mean))|,
 * sigma) minus, when dog_sigma > 0, the same with dog_sigma (scipy.ndimage.gaussian_filter
 * semantics: truncate 4, mode 'reflect'); peaks = skimage.feature.peak_local_max(smooth,
 * threshold_rel=threshold_rel) with its defaults (3x3 maxima above max(min, rel*max), 1-pixel
 * border excluded).  image: n0 x n1 (host).  coords: up to max_out (row, column) pairs in the
 * fftshift-ed frame, values: their smooth values (plan dtype), in no particular order (sort by
 * value, then raster index, for skimage's order); *count_out = number found (> max_out means
 * the arrays hold only a subset: call again with more room).  smooth_out: n0 x n1 or NULL.   */
int gpa_find_peaks(gpa_plan* plan, const void* image, double sigma, double dog_sigma,
                   double threshold_rel, int max_out, int32_t* coords, void* values,
                   int* count_out, void* smooth_out);
/* the same with the image (not modified) and the optional smooth_out on the device; coords, values, count_out stay host
 * arrays (a handful of entries).  Synchronises the plan's stream (the count decides what is copied).                    */
int gpa_find_peaks_dev(gpa_plan* plan, const void* d_image, double sigma, double dog_sigma,
                       double threshold_rel, int max_out, int32_t* coords, void* values,
                       int* count_out, void* d_smooth_out);
/* peak_local_max at another threshold_rel of the smoothed spectrum that the last gpa_find_peaks / gpa_find_peaks_dev call
 * of this plan computed (the plan keeps it): the re-evaluations of extract_primary_ks' parameter relaxation
 * (geometric_phase_analysis.py:447-467) while sigma and DoG stay the same cost one threshold + maxima pass instead of the
 * transforms and filters.  GPA_ERR_STATE before the first gpa_find_peaks call.                                           */
int gpa_find_peaks_again(gpa_plan* plan, double threshold_rel, int max_out, int32_t* coords, void* values,
                         int* count_out);

/* Unit-cell averaging and expansion (unit_cell_averaging.py).  The geometry is computed on the host exactly as
 * the reference computes it: ks = the first two k-vectors (cycles / pixel, row-major 2 x 2), kinv = np.linalg.inv(ks),
 * (rmin, rsize) = calc_ucell_parameters(ks, z).  rsize[0] x rsize[1] <= 2^24 bins (GPA_ERR_STATE beyond).        */
typedef struct gpa_ucell_geom {
  double ks[4];
  double kinv[4];
  double rmin[2];
  int32_t rsize[2];
  double z;
} gpa_ucell_geom;
/* unit_cell_average (unit_cell_averaging.py:132-205): every pixel of the plan-shaped image lands at
 * z (cart_in_uc(r + u(r)) - rmin) and adds value * overlap and overlap to the 2 x 2 bins around it; res = sums / weights
 * (NaN where nothing landed), weights (nullable) = the overlap sums.  NaN image pixels and NaN u are skipped.  u: 2 x n0 x
 * n1 (plan dtype) or NULL for none; res, weights: rsize[0] x rsize[1] DOUBLES in both precisions (summed in f64).
 * Edges: a corner at index rsize is dropped (the reference raises IndexError there); a corner at -1 lands in the last
 * row / column, as NumPy indexes.  The result is the same bits on every call.                                        */
int gpa_unit_cell_average(gpa_plan* plan, const void* image, const void* u, const gpa_ucell_geom* geom, double* res,
                          double* weights);
int gpa_unit_cell_average_dev(gpa_plan* plan, const void* image_dev, const void* u_dev, const gpa_ucell_geom* geom,
                              double* res_dev, double* weights_dev);
/* B frames (B x n0 x n1, contiguous; 1 <= B <= 65535, else GPA_ERR_ARG) that share u: the pixel lists are built
 * once; res, weights: B x rsize.  Frame b's result is bitwise what gpa_unit_cell_average_dev gives for it alone.  */
int gpa_unit_cell_average_batch_dev(gpa_plan* plan, const void* images_dev, int B, const void* u_dev,
                                    const gpa_ucell_geom* geom, double* res_dev, double* weights_dev);
/* expand_unitcell (unit_cell_averaging.py:236-251): out(r) = nan_to_num(cell) sampled at z cart_in_uc(r / z2 + u(r))
 * (order-3 B-spline, mode 'constant', cval 0; f64 arithmetic in both precisions).  cell: rsize[0] x rsize[1] doubles;
 * u: 2 x n0 x n1 (plan dtype) or NULL for none; out: n0 x n1 (plan dtype), the plan's shape.                          */
int gpa_expand_unitcell(gpa_plan* plan, const double* cell, const gpa_ucell_geom* geom, double z2, const void* u,
                        void* out);
int gpa_expand_unitcell_dev(gpa_plan* plan, const double* cell_dev, const gpa_ucell_geom* geom, double z2,
                            const void* u_dev, void* out_dev);

/* Windowed Fourier filtering, wff (geometric_phase_analysis.py:551-580), in its separable form: for every threshold t
 *   out_t = scale * sum_wx Cx[kx] ( sum_wy Cy[ky] ( keep_t ( Cy[ky] ( Cx[kx] image ) ) ) )
 * with the window s = round(2 sigma) (halves to even, as Python rounds), offsets j = -s .. s - 1, g(j) = exp(-j^2 / 2 sigma^2),
 * kx(j) = g(j) e^(i wx j) along axis 1, ky(j) = g(j) e^(i wy j) / sum g^2 along axis 0, scipy.ndimage's 'reflect' boundary, and
 * keep_t(sf) = sf where |sf| >= thresholds[t], else 0 -- decided as |sf|^2 >= thresholds[t]^2 in the plan's precision; a
 * negative threshold keeps every sample.  image: n0 x n1 interleaved complex of the plan's dtype; wxs[Kx], wys[Ky],
 * thresholds[T]: doubles (the reference passes np.arange(wl, wu + wi / 2, wi), wi = 1 / sigma, for both lists and
 * scale = wi^2 / 4 pi^2); out: T x n0 x n1 interleaved complex, not overlapping image.  Limits of one call, GPA_ERR_ARG
 * beyond: s <= GPA_WFF_MAX_S, T <= GPA_WFF_MAX_T (split longer threshold lists).  Null pointers, Kx / Ky / T < 1,
 * sigma <= 0 and non-finite values are GPA_ERR_ARG before a device is touched.  The sums run in a fixed order: the same
 * bits on every call, and a call with T thresholds gives the planes of T calls with one.
 * _dev: device pointers, enqueued on the plan's stream (one host synchronisation, for the tap tables).                */
#define GPA_WFF_MAX_S 40
#define GPA_WFF_MAX_T 8
int gpa_wff(gpa_plan* plan, const void* image, double sigma, const double* wxs, int Kx, const double* wys, int Ky,
            const double* thresholds, int T, double scale, void* out);
int gpa_wff_dev(gpa_plan* plan, const void* image_dev, double sigma, const double* wxs, int Kx, const double* wys, int Ky,
                const double* thresholds, int T, double scale, void* out_dev);

/* Image preparation (pyGPA/imagetools.py:92-194).  Images are n0 x n1 reals of the plan's dtype; masks are uint8_t planes of
 * n0 x n1, 0 is false and anything else is true (what is written is 0 or 1).  Each entry point has a host-pointer form and a
 * _dev form on device pointers.  The _dev forms with small host outputs (lims, rows, cols) synchronise the plan's stream, the
 * others only enqueue work on it (the first call with a new sigma or r uploads its table and synchronises once).  Null
 * pointers, sigma <= 0 or not finite, r < 0 or > GPA_PREP_MAX_R and B < 1 are GPA_ERR_ARG, with a message that names the
 * argument, before a device is touched.  Work space is the plan's and counted in the plan's workspace bytes.
 *
 * gauss_homogenize (imagetools.py:92-109):  VV = G(mask ? image : 0) / G(mask),  out = image / VV,  G = scipy.ndimage's
 * gaussian_filter(sigma): axis 0 then axis 1, radius int(4 sigma + 0.5), 'reflect'.  Where the (2R+1)^2 box of the
 * reflect-extended mask holds no true sample the reference's VV is NaN (0 / 0): that pattern is reproduced exactly (it is
 * decided in integers) and VV is NaN there, or nan_scale when use_nan_scale != 0.  Elsewhere VV is held within [min, max] of
 * the masked samples.  vv_out (nullable) receives VV.  out and vv_out may not overlap image or mask.  Samples outside the
 * mask may be anything (NaN included); a non-finite sample UNDER the mask yields NaN in VV and out on at least the
 * reference's (2R+1)^2 box around it, on the FFT route on the whole overlap-save segments that hold it.  Radii from
 * GAUSS_FFT_MINR (option, default 12) on run as overlap-save FFT convolutions, which need 4 R <= 16384 (f32) / 8192 (f64):
 * sigma <= 1024 / 512, GPA_ERR_ARG naming sigma beyond; shorter radii run as direct sums (and so does every radius with
 * 2 R + 1 <= 3072 when the option is set above it).  Rows longer than GPA_PREP_MAX_N1: GPA_ERR_STATE.                    */
#define GPA_PREP_MAX_R 254
#define GPA_PREP_MAX_N1 32768
int gpa_gauss_homogenize(gpa_plan* plan, const void* image, const uint8_t* mask, double sigma, int use_nan_scale,
                         double nan_scale, void* out, void* vv_out);
int gpa_gauss_homogenize_dev(gpa_plan* plan, const void* image_dev, const uint8_t* mask_dev, double sigma, int use_nan_scale,
                             double nan_scale, void* out_dev, void* vv_dev);
/* hit = [hit |] any over b of (frames[b] == value): frames is B x n0 x n1 of the plan's dtype and value is compared in that
 * precision (an f32 plan compares against (float)value); a NaN value hits nothing.  accumulate != 0 keeps what hit holds,
 * so a long stack can be sent in chunks.  generate_mask (imagetools.py:178-185) is the erosion of !hit.              */
int gpa_mask_any_equal(gpa_plan* plan, const void* frames, int B, double value, int accumulate, uint8_t* hit);
int gpa_mask_any_equal_dev(gpa_plan* plan, const void* frames_dev, int B, double value, int accumulate, uint8_t* hit_dev);
/* out = scipy.ndimage.binary_erosion(invert ? !in : in, structure = skimage.morphology.disk(r)), border_value 0: the mask is
 * eaten from the image edges too; r = 0 is the identity; out may be in.  0 <= r <= GPA_PREP_MAX_R.                      */
int gpa_mask_erode_disk(gpa_plan* plan, const uint8_t* in, int invert, int r, uint8_t* out);
int gpa_mask_erode_disk_dev(gpa_plan* plan, const uint8_t* in_dev, int invert, int r, uint8_t* out_dev);
/* lims = { first row, last row + 1, first column, last column + 1 } with a true sample (cull_by_mask, imagetools.py:188-194);
 * an all-false mask gives the empty { n0, 0, n1, 0 }.  lims is a host array in both forms.                               */
int gpa_mask_bounds(gpa_plan* plan, const uint8_t* mask, int32_t* lims);
int gpa_mask_bounds_dev(gpa_plan* plan, const uint8_t* mask_dev, int32_t* lims);
/* rows[n0], cols[n1] (host arrays in both forms): 1 where every sample of the line is NaN (trim_nans, imagetools.py:128-142) */
int gpa_nan_lines(gpa_plan* plan, const void* image, uint8_t* rows, uint8_t* cols);
int gpa_nan_lines_dev(gpa_plan* plan, const void* image_dev, uint8_t* rows, uint8_t* cols);
/* the loop of trim_nans2 (imagetools.py:145-175), run on the device: lims = { x0, x1, y0, y1 } (host array) of the window
 * image[x0:x1, y0:y1] it ends with.  A window that empties on the way (an all-NaN image) ends the loop with x1 <= x0 or
 * y1 <= y0, where the reference fails with an IndexError.                                                               */
int gpa_nan_trim_lims(gpa_plan* plan, const void* image, int32_t* lims);
int gpa_nan_trim_lims_dev(gpa_plan* plan, const void* image_dev, int32_t* lims);

/* ---- per-line medians and homogenize_per_axis (pyGPA/imagetools.py:112-125) ------------------------------------------------
 * out = the median of every line of the plan's n0 x n1 image along `axis`: axis 0 gives the n1 column medians, axis 1 the n0
 * row medians, in the plan's precision and with NumPy's bits (the median is selected, not approximated: the middle sample,
 * or (a + b) / 2 of the two middle ones).  mask (nullable, n0 x n1 bytes, 0 is false) leaves samples out, as NaN samples are
 * left out: np.nanmedian(where(mask, image, nan), axis); a line without any sample gives NaN.  propagate_nan != 0 gives
 * np.median instead: a NaN or masked sample makes the median of its line NaN.  A line holds at most GPA_LINES_MAX_N samples
 * (its keys stay in LDS): GPA_ERR_ARG beyond; the other axis is only bound by the plan.                                   */
#define GPA_LINES_MAX_N 16384
int gpa_line_nanmedian(gpa_plan* plan, const void* image, const uint8_t* mask, int axis, int propagate_nan, void* out);
int gpa_line_nanmedian_dev(gpa_plan* plan, const void* image_dev, const uint8_t* mask_dev, int axis, int propagate_nan, void* out_dev);
/* homogenize_per_axis of nb frames (nb x n0 x n1, one mask for all, nullable) with reducfunc = np.nanmedian (propagate_nan = 0)
 * or np.median (1):  for axis 0, then axis 1:  profile = gaussian_filter(median of where(mask, res, nan) along the axis, sigma),
 * res /= profile / max(profile).  The medians of axis 1 are those of the image after the division of axis 0, which is applied
 * as the rows are loaded; the image is written once, out = (image / q0[column]) / q1[row].  The filter runs along the line
 * only (along the unit axis the reference's second pass multiplies by the taps' sum), as a direct f64 sum over the 'reflect'
 * extension, rounded once.  max propagates NaN as np.max does: one line without a sample turns the whole frame NaN, as in the
 * reference.  profiles (nullable) receives per frame the n1 values of the axis-0 profile, then the n0 values of the axis-1
 * profile.  Both axes <= GPA_LINES_MAX_N, sigma <= 16384, 1 <= nb <= 65535: GPA_ERR_ARG otherwise.  out may be image in the
 * _dev form.                                                                                                             */
int gpa_homogenize_per_axis(gpa_plan* plan, const void* image, const uint8_t* mask, double sigma, int propagate_nan, int nb,
                            void* out, void* profiles);
int gpa_homogenize_per_axis_dev(gpa_plan* plan, const void* image_dev, const uint8_t* mask_dev, double sigma, int propagate_nan,
                                int nb, void* out_dev, void* profiles_dev);
/* The same filter and divisions for one frame whose REDUCED lines the caller computed (any reducfunc): line0 = the n1 values
 * reduced along axis 0, line1 = the n0 values reduced along axis 1 of the image after axis 0.  line1 null: out = image / q0,
 * the image after axis 0, from which the caller reduces line1.  profiles (nullable): n1 values, then n0 when line1 is given. */
int gpa_homogenize_lines(gpa_plan* plan, const void* image, double sigma, const void* line0, const void* line1, void* out,
                         void* profiles);
int gpa_homogenize_lines_dev(gpa_plan* plan, const void* image_dev, double sigma, const void* line0_dev, const void* line1_dev,
                             void* out_dev, void* profiles_dev);

/* timing hooks used by bench.py: elapsed milliseconds between two recorded
 * events on the plan's stream (HIP events, so it measures the stream the
 * kernels are launched on).                                                   */
int gpa_timer_start(gpa_plan* plan);
int gpa_timer_stop(gpa_plan* plan, float* ms_out);
/* per-stage device times (ms) of the last fused-driver call, measured with HIP
 * events when gpa_set_profiling(plan, 1) is on:
 *   [0] tables+mean  [1] sweep pass A (x-axis)  [2] sweep pass B (y-axis+select)
 *   [3] reconstruct  [4] unwrap (both components)                             */
int gpa_set_profiling(gpa_plan* plan, int on);
int gpa_last_stage_ms(gpa_plan* plan, float* ms5);
/* per-KERNEL device times of the last fused-driver call made with profiling on (every launch is
 * bracketed by HIP events on the stream it runs on; the two unwraps then run one after the other):
 * one text line "name launches total_ms" per kernel, NUL-terminated, into out[cap].              */
int gpa_last_kernel_profile(gpa_plan* plan, char* out, size_t cap);
/* The shared-forward pass B of the sweep skips a candidate on the rows where a spectral bound proves that it cannot
 * win a pixel (same winners, bit for bit; gpa_set_option("NO_PB_SKIP", "1") switches the test off -- a
 * diagnostic switch, not the kernel as it was before the test: the loop keeps its new shape and runs about 5 % longer).  Of the last such
 * launch made with profiling on: the (row, candidate) pairs it skipped and all it visited (rows x candidates x peaks x
 * images); both 0 when the last sweep of the plan was not profiled or took another kernel.  Waits for the stream.   */
int gpa_last_passb_skips(gpa_plan* plan, long long* skipped, long long* visited);
/* The order in which that kernel visits the K candidates of one peak (klist: K x 2, kref: 2): order_out[0 .. K) = list
 * positions, x-planes (distinct wx) kept together, nearest to kref first; list order under NO_REORDER or for a list with two
 * different k-vectors equal modulo whole cycles.  Host only: no plan, no device.                                       */
int gpa_passb_visiting_order(const double* klist, const double* kref, int K, int* order_out);

/* Download of a result while the GPU goes on with the next call: copies `bytes` from device memory
 * (e.g. the u of gpa_extract_displacement_field_async) to PAGE-LOCKED host memory on the plan's copy
 * stream, ordered after everything enqueued on the plan so far.  `slot` (0..3) names the completion
 * event: gpa_download_wait(plan, slot) blocks the host until that copy has landed.  The caller must not
 * let a later call overwrite dev_src before the copy is done (alternate two result buffers and wait for
 * slot i before reusing buffer i).  This is how bench.py keeps the D2H of u inside the timed step
 *  without serialising it with the kernels.                                       */
int gpa_download_async(gpa_plan* plan, void* host_dst, const void* dev_src, size_t bytes, int slot);
int gpa_download_wait(gpa_plan* plan, int slot);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* GPA_HIP_H */
