// Internal header of the C-ABI translation units (gpa_api*.hip): the plan object, error / try macros and the helpers the
// entry-point files share.  Not part of the public interface (include/gpa_hip.h is).
#pragma once
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <complex>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#include <string>
#include <limits>
#include <vector>

#include "../../include/gpa_hip.h"
#include "gpa_internal.h"
#include "gpa_passb_shared.h"
#include "gpa_yspec.h"
#include "gpa_unwrap.h"
#include "gpa_dft.h"
#include "gpa_gaussfft.h"
#include "gpa_hoststage.h"

using namespace gpa;

int gpa_fail(int code, const std::string& msg);   // sets gpa_last_error() of the calling thread, returns code
static inline int fail(int code, const std::string& msg) { return gpa_fail(code, msg); }

#define HIP_TRY(expr)                                                                         \
  do {                                                                                        \
    hipError_t _e = (expr);                                                                   \
    if (_e != hipSuccess)                                                                     \
      return fail(GPA_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));            \
  } while (0)

// the two limits are separate: the f64 unwrap reaches power-of-two axes of 16384 points, the f64 sweep stops at 8192
#define NEED_SWEEP(p, what)                                                                                         \
  do {                                                                                                             \
    if ((p)->spectral_only)                                                                                        \
      return fail(GPA_ERR_STATE, std::string(what) + ": this plan's image is too large for the sweep kernels "          \
                                 "(an axis above 16384 pow2 / 8192 other in f32, 8192 / 4096 in f64); it serves per, "  \
                                 "find_peaks, gaussian_deconvolve, the per-pixel entry points and, where the plan has " \
                                 "one (f64: power-of-two axes up to 16384), the unwrap");                               \
  } while (0)

#define NEED_UNWRAP(p, what)                                                                                     \
  do {                                                                                                             \
    if (!(p)->uw.impl)                                                                                             \
      return fail(GPA_ERR_STATE, std::string(what) + ": this plan's image is too large for the sweep / unwrap kernels " \
                                 "(an axis above 16384 pow2 / 8192 other in f32, 16384 pow2 / 4096 other in f64); it "  \
                                 "serves per, find_peaks, gaussian_deconvolve and the per-pixel entry points only");     \
  } while (0)

#define TRY(expr)            \
  do {                       \
    int _r = (expr);         \
    if (_r != GPA_OK) return _r; \
  } while (0)

// One helper thread per plan: the fused driver enqueues the second displacement component's ~45 launches from it
// while the calling thread enqueues the first component's.  A 4096^2 image does not care (the GPU is the limit), but
// a call costs ~0.4 ms of host time for its ~110 launches, which IS the limit below ~1024^2 (tools/enqueue_cost.py).
struct EnqueueWorker {
  std::thread th;
  std::mutex m;
  std::condition_variable cv;
  std::function<void()> job;
  bool has_job = false, done = true, quit = false;
  explicit EnqueueWorker(int device) {
    th = std::thread([this, device] {
      (void)hipSetDevice(device);
      std::unique_lock<std::mutex> lk(m);
      for (;;) {
        cv.wait(lk, [this] { return has_job || quit; });
        if (quit) return;
        std::function<void()> j = std::move(job);
        has_job = false;
        lk.unlock();
        j();
        lk.lock();
        done = true;
        cv.notify_all();
      }
    });
  }
  void submit(std::function<void()> j) {
    std::lock_guard<std::mutex> lk(m);
    job = std::move(j);
    has_job = true;
    done = false;
    cv.notify_all();
  }
  void wait() {
    std::unique_lock<std::mutex> lk(m);
    cv.wait(lk, [this] { return done; });
  }
  ~EnqueueWorker() {
    {
      std::lock_guard<std::mutex> lk(m);
      quit = true;
      cv.notify_all();
    }
    if (th.joinable()) th.join();
  }
};

struct gpa_plan {
  int device = 0, dtype = 0, n0 = 0, n1 = 0, max_batch = 0;
  // an axis beyond what one workgroup transforms (f32: 16384 pow2 / 8192 other; f64: 8192 pow2 / 4096 other): no sweep
  // -- the plan serves the plain-DFT rows (per, find_peaks, gaussian_deconvolve: any axis up to 65536) and
  // the per-pixel kernels (reconstruct, Lawler-Fujita, Jacobian / properties, plane fit)
  bool spectral_only = false;
  // ... and no unwrap workspace either, unless the long axes are f64 power-of-two axes of 16384 points: the unwrap's
  // half-length transforms and transform-free column solves reach those (gpa_unwrap_rowhalf.hip, gpa_unwrap_colhalf.hip)
  bool no_unwrap = false;
  Axis ax0{}, ax1{};              // the geometry in use (depends on sigma for non-power-of-two axes)
  Axis ax0_full{}, ax1_full{};    // the plan's largest geometry (L >= 2n - 1): what the tables are sized for
  hipStream_t stream = nullptr;
  size_t rsz = 4, csz = 8;        // bytes per real / complex element
  // Memory.  Every device buffer of the plan is a DevBuf (gpa_devbuf.h) that reports to ws_bytes and frees itself with the
  // plan: the fixed and allocate-once ones sit in `owned` (dmalloc hands out their pointers), the grown ones are members.
  size_t ws_bytes = 0;            // gpa_plan_workspace_bytes: device bytes of all of them and of the unwrap workspaces
  std::vector<DevBuf> owned;
  // device buffers
  void* tw0 = nullptr;            // twiddle tables exp(-2 pi i t / L)
  void* tw1 = nullptr;
  void* Hx = nullptr;             // filter tables for the current sigma
  void* Hy = nullptr;
  double sigma_cached = -1.0;
  // shared-forward pass B (gpa_passb_shared.h): per-sigma taps, per-(sigma, k-list) candidate tables
  PassBSharedTables sh{};
  double* d_taps = nullptr;       // g(0 .. sh_etab) of the y axis' circular filter, doubles
  int sh_etab = 0, sh_E = 0, sh_Epad = 0;
  int sh_nbl = 16;                // live spectral registers of the staged candidates (band rotation, passB_shared_nbl)
  double sh_sigma = 0.0;          // the sigma the taps belong to (band cut-off)
  double* d_wys = nullptr;        // [max_batch] candidate frequencies wy + rotation
  int* d_shifts = nullptr;        // [max_peaks] band rotation of every peak, in blocks of L / 16 bins
  Axis ax1s{};                    // its geometry of the y axis: periodic as ax1, or zero-padded to L >= n1 + E
  void* tw1s = nullptr;           // twiddles of ax1s.L when that differs from ax1.L
  int tw1s_L = 0;
  bool sh_ok = false;             // this sigma / axis can run it
  bool use_shared = true;         // GPA_NO_SHARED=1 keeps the per-candidate forward transforms
  int sh_epoch = 0, sh_built_epoch = -1, sh_built_K = 0, sh_built_B = 0;   // tables follow sigma and the staged k-list
  bool sh_built_reorder = true;   // ... and the NO_REORDER option they were built under
  double* d_ystep = nullptr;      // [max_peaks] 2 pi frac(ky_p + band rotation_p): phase step along y of the compensation phasor
  bool sh_one_kref = true;        // every candidate of a peak shares its reference vector (what d_ystep assumes)
  bool lk_raw = false;            // the last passB_select left the lock-ins raw (fused driver): the consumer applies d_ystep
  bool sh_built_ok = false;       // the tables of that key are complete and worth using
  bool sh_use = false;            // ... and the staged candidates form runs of >= 2 on an x-plane
  DevBuf sh_Gb{&ws_bytes}, sh_psi{&ws_bytes}, sh_pre{&ws_bytes};   // behind sh.Gb / sh.psi / sh.pre, grown on demand
  // y-spectral sweep: pass A filters columns of FFT_y(image), pass B runs no forward transform
  bool ys_ok = false;             // the staged list / rows can take it (built with the shared tables)
  bool ys_use = false;            // ... and the sweep being staged does (sweep_choose_path; NO_YSPEC=1 keeps the spatial path)
  PassAYspec ys{};                // Yhat / strips (grown on demand, ensure_yspec), the (block, planes) groups of the staged list
  int* d_ys_groups = nullptr;     // [16 max_batch][4]: the plane list (16 max_batch entries), behind it 3 ints per group
  int ys_gmax = 0;                // the cap (YSPEC_GROUP) the staged groups were cut with
  DevBuf ys_Yhat{&ws_bytes}, ys_strips{&ws_bytes};   // behind ys.Yhat / ys.strips
  std::vector<int> staged_planeof;
  DevBuf Tbuf{&ws_bytes};         // [tbuf_planes][n0][n1] complex: one plane per DISTINCT wx (x-plane), grown on demand
  int tbuf_planes = 0;
  SweepTables tb{};
  double* d_kl = nullptr;         // [max_batch][2]
  double* d_kr = nullptr;
  double* d_pw = nullptr;         // [max_batch] distinct wx values (x-planes)
  int last_planes = 0;
  std::vector<double> staged_kl, staged_kr, staged_kmat;   // what the device tables currently hold
  DevBuf h_iters{nullptr, true};  // pinned ints: iteration counts of the last (possibly asynchronous) driver call
  int iters_stride = 1;           // 1: two-stream driver (h_iters[0], [1]); 4: paired workspace (flag words of 2 problems)
  int iters_off = 0;              // paired / batched: the word of a problem's flags that holds its count
  // images of up to 1024^2: both components of u in ONE set of launches (blockIdx.z) on one stream -- measured 8 %
  // (512^2) to 14 % (256^2) faster than two streams, whose kernels are too small to overlap; from 2048^2 on the two
  // streams win by 4 % (profiles/r02_image_stacks.txt, 'stack of 1')
  UnwrapWorkspace uwp{};
  bool have_uwp = false, use_pair = false;
  DevBuf h_k{nullptr, true};      // pinned staging, 6 * max_batch + 32 doubles
  void* d_image = nullptr;        // staging for host-pointer entry points
  void* d_mean = nullptr;
  void* d_tile_mean = nullptr;    // whole-image mean of the tile path (gpa_tile_gradients_dev)
  DevBuf d_tsum_part{&ws_bytes};  // partial sums of gpa_tile_sums_dev (doubles), grown on demand
  hipEvent_t ev_x = nullptr;      // stream-to-stream ordering (gpa_plan_wait_stream / gpa_stream_wait_plan)
  double tile_mean = std::numeric_limits<double>::quiet_NaN();
  DevBuf d_sf{&ws_bytes};         // [K][n0][n1] complex, grown on demand (a4 gradient path)
  void* d_grad = nullptr;         // n0 x n1 x 2 staging for the host-pointer a4 call
  void* d_grads = nullptr;        // [max_peaks] n0 x n1 x 2 and
  void* d_absw = nullptr;         // [max_peaks] n0 x n1: staging of gpa_extract_displacement_field_grad, allocated on first use
  double* d_scratch = nullptr;    // 16384 doubles (mean partials, Gaussian weights at + 1024, Huber partials: 10 x 1024 + 10)
  void* d_aux0 = nullptr;         // n0 / n1 complex doubles: border-difference spectra (a9), Gaussian factors (f-4);
  void* d_aux1 = nullptr;         // NOT the sweep's compensation tables, which stay valid across those calls
  void* d_lockin = nullptr;       // [P<=max_peaks][n0][n1] complex (staging / fused driver)
  int32_t* d_kidx = nullptr;
  int max_peaks = 0;
  // reconstruct + unwrap workspace
  void* d_dudx = nullptr;         // 2 x n0 x (n1-1)
  void* d_dudy = nullptr;         // 2 x (n0-1) x n1
  void* d_wnorm = nullptr;        // n0 x n1
  void* d_u = nullptr;            // 2 x n0 x n1
  double* d_kmat = nullptr;       // [max_peaks][2]
  UnwrapWorkspace uw{};
  // ONE batched workspace per plan, its capacity counted in problems: the 2 x images solves of a batched driver call
  // (gpa_extract_displacement_field_batch_dev) and the problems of a stack unwrap (gpa_unwrap_batch_dev) share it.  Grown to
  // the largest need seen (ensure_unwrap_problems); smaller calls reuse it through unwrap_set_active.
  UnwrapWorkspace uwb{};
  int uwb_probs = 0;
  size_t uwb_base_bytes = 0;      // device bytes it was created with
  size_t uwb_bytes = 0;           // ... and with the search directions allocated since: the one workspace that is rebuilt, so
                                  // counted beside ws_bytes
  int uwb_last_nb = 0;            // problems of the last gpa_unwrap_batch[_dev] call (gpa_unwrap_batch_finish)
  DevBuf d_wnorm_b{&ws_bytes};    // images x n0 x n1
  DevBuf h_iters_b{nullptr, true};   // pinned: 4 ints per problem
  // sweep of a chunk of images in one set of launches: x-planes, lock-ins, means, mean scratch (doubles) per image, and the
  // winners' indices where a stack call wants gradients but not the indices
  DevBuf bT{&ws_bytes}, bL{&ws_bytes}, bMean{&ws_bytes}, bScratch{&ws_bytes}, bK{&ws_bytes};
  UnwrapWorkspace uw2{};          // second workspace + stream: the two components of u unwrap concurrently
  hipStream_t stream2 = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  DftAxis bx0{}, bx1{};           // the two axes of the plain 2-D DFT (a9, f-3, f-4: gpa_dft.h), built on first use
  DftWork dftw{};                 // scratch of its through-HBM engine, grown on demand
  void* d_pertab = nullptr;       // a9: per-axis factors 1 - e^(2 pi i j / n) and sin^2(pi j / n) (per_tables_create)
  // f-3: tables of the FFT form of gaussian_filter (gpa_gaussfft.h), two sigmas per axis (difference of Gaussians)
  struct GaussTab { double sigma = -1.0; int lg = 0; DevBuf H, tw; unsigned stamp = 0; };
  GaussTab gft[2][2];
  unsigned gft_clock = 0;
  double* d_peakws = nullptr;     // f-3: min / max partials (2 x 2048), threshold, candidate counter
  void* d_peaksmooth = nullptr;   // f-3: the smoothed spectrum of the last gpa_find_peaks call, n0 x n1 reals (gpa_find_peaks_again)
  bool peaks_smooth_valid = false;
  WarpWs warp{};                  // scratch + taps of the Lawler-Fujita kernels (gpa_warp.hip), grown on first use
  UcellWs ucell{};                // scratch of unit-cell averaging / expansion (gpa_ucell.hip), grown on first use
  // Device staging of the host-pointer forms of wff, image preparation, the per-line medians and the unit-cell calls (the
  // cell-shaped operands), laid out per call by a HostStage (gpa_hoststage.h) and grown on demand.  One buffer serves them all:
  // every one of these forms drains the stream before it returns -- itself, or through the _dev form it tail-calls
  // (gpa_mask_bounds, gpa_nan_lines, gpa_nan_trim_lims) -- and none calls another host form while its staged pointers are
  // live: between upload and download they run only their own checked device path or _dev form.
  DevBuf host_stage{&ws_bytes};
  // windowed Fourier filtering (gpa_api_wff.hip), grown on demand: tap tables, the A plane and the T planes B of a call
  DevBuf wff{&ws_bytes};
  // image preparation (gpa_api_prep.hip), grown on demand: the num / den planes, two byte planes, the chords and the small
  // words of a call; the filter tables of the last (sigma, segment lengths)
  DevBuf prep{&ws_bytes}, prep_tab{&ws_bytes};
  double prep_sigma = -1.0;       // what prep_tab holds: sigma, the two transform lengths (0, 0: the direct route's taps)
  int prep_lg0 = -1, prep_lg1 = -1;
  int prep_chord_r = -1;          // the radius whose chords sit in prep
  // per-line medians and homogenize_per_axis (gpa_api_lines.hip), grown on demand: the transposed planes and the median /
  // profile / divisor lines of a call; the taps of the last sigma
  DevBuf lines{&ws_bytes}, lines_tab{&ws_bytes};
  double lines_sigma = -1.0;      // the sigma whose taps sit in lines_tab
  // a8 iterate_GPA (gpa_api_iterate.hip), grown on demand: the Huber work of the batched plane fit, behind it the driver's
  // amax / psi / weight planes (and the prs / w planes of its host form)
  DevBuf d_iter{&ws_bytes};
  DevBuf h_iter{nullptr, true};   // pinned doubles: per plane 4 up (coefficients, flag), 10 down (sums)
  // timing
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  bool profiling = false;
  hipEvent_t stage_ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  float stage_ms[5] = {0, 0, 0, 0, 0};
  EnqueueWorker* worker = nullptr;   // second enqueueing thread of the fused driver
  bool use_worker = true, no_ksplit = false, no_compact = false;
  bool serial_unwrap = false;
  KernelProfiler* kprof = nullptr;   // per-kernel event pairs of the last profiled driver call
  std::string kprof_table;           // "name calls total_ms" lines of that call
  unsigned long long* d_pbskip = nullptr;   // two words: candidate rows the shared pass B skipped / visited in its last profiled launch
  bool pbskip_valid = false;                // ... and whether the last shared pass B was such a launch
  // downloads overlapped with the next call (gpa_download_async)
  hipStream_t copy_stream = nullptr;
  hipEvent_t ev_dl_ready = nullptr, ev_dl_done[4] = {nullptr, nullptr, nullptr, nullptr};

  // the workspaces and tables that live in structs of their own report to the plan's counter too.  (Hidden: the public header
  // declares the type inside its visibility pragma, which would export the two.)
  __attribute__((visibility("hidden"))) ~gpa_plan() = default;
  __attribute__((visibility("hidden"))) gpa_plan() {
    warp.buf.counted = ucell.buf.counted = dftw.buf.counted = &ws_bytes;
    for (auto& ax : gft)
      for (auto& g : ax) g.H.counted = g.tw.counted = &ws_bytes;
  }
};

template <class T>
static hipError_t upload_as(void* dst, const std::vector<double>& v, hipStream_t s) {
  std::vector<T> tmp(v.begin(), v.end());
  hipError_t e = hipMemcpyAsync(dst, tmp.data(), tmp.size() * sizeof(T), hipMemcpyHostToDevice, s);
  if (e != hipSuccess) return e;
  return hipStreamSynchronize(s);
}

// ---- helpers shared by the entry-point files (defined in the file named) ----
void host_fft_pow2(std::vector<std::complex<double>>& a, bool inverse);
std::vector<double> gaussian_kspace(int n, double sigma);
std::vector<double> spatial_kernel(int n, const std::vector<double>& g);
int kernel_support(const std::vector<double>& h, double tol);
std::vector<double> spatial_taps(int n, const std::vector<double>& g, int mmax);
void build_filter_table(const Axis& ax, const std::vector<double>& g, const std::vector<double>& hsp,
                               std::vector<double>& out);
int ensure_filters(gpa_plan* p, double sigma);
int shared_prepare(gpa_plan* p, int P, int K);
int stage_kvectors(gpa_plan* p, const double* kl, const double* kr_per_b, int B, int* planes_out);
int ensure_tbuf(gpa_plan* p, int planes);
int ensure_sf(gpa_plan* p, size_t bytes);
// at least `bytes` in a buffer of the plan (DevBuf::reserve on the plan's stream), failing in the words of `what`
int plan_reserve(gpa_plan* p, DevBuf& b, size_t bytes, const char* what);
int stage_kmat(gpa_plan* p, const double* kvecs, int P);
// the plan's batched unwrap workspace with room for `nprob` problems, the first nprob of them active, and pinned room for their
// flag words (gpa_api_driver.hip); GPA_ERR_STATE in the words of `who` where the shape has no batched unwrap
int ensure_unwrap_problems(gpa_plan* p, int nprob, const char* who);
// the x-planes pass B reads: those of one image in the plan's own buffer ({p->Tbuf, 1, 0}), or those of a stack of nimg images
// `stride` planes apart (stride != 0 marks a stack)
struct XPlanes { const void* T; int nimg, stride; };
// passb: the pass B the caller will run on the staged planes -- SWEEP_PASSB_OTHER (per-candidate / gated / plain lock-ins:
// spatial pass A), SWEEP_PASSB_SELECT (passB_select), SWEEP_PASSB_PHASES (passB_phases); the two shared-forward users decide
// HERE, before pass A, whether the sweep takes the y-spectral path (p->ys_use)
enum { SWEEP_PASSB_OTHER = 0, SWEEP_PASSB_SELECT = 1, SWEEP_PASSB_PHASES = 2 };
int stage_sweep(gpa_plan* p, const double* krefs, int P, const double* klists, int K, double sigma, int* Bx,
                int passb = SWEEP_PASSB_OTHER);
int ensure_yspec(gpa_plan* p, int nimg, int Bx);
int run_passA(gpa_plan* p, const void* image, const void* mean, void* Tbuf, int Bx, int nimg);
int passB_select(gpa_plan* p, const XPlanes& xp, int P, int K, void* lockin, int32_t* kidx, bool raw);
int passB_phases(gpa_plan* p, const XPlanes& xp, int P, int K, void* lockin, int32_t* kidx, void* psi, bool* shared);
void collect_kernel_profile(gpa_plan* p);
// the tail of a profiled entry point: drain the stream, read the kernel events of the call
inline int prof_finish(gpa_plan* p) {
  if (p->profiling) { HIP_TRY(hipStreamSynchronize(p->stream)); collect_kernel_profile(p); }
  return GPA_OK;
}
// what a plan-less host form needs before it touches a device: one to be there, and `device` selected
inline int need_device(const char* who, int device) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(GPA_ERR_NODEV, std::string(who) + ": no HIP device");
  HIP_TRY(hipSetDevice(device));
  return GPA_OK;
}
inline size_t dtype_size(int dtype) { return dtype == GPA_F32 ? 4 : 8; }   // bytes of a real
int sweep_peaks_dev(gpa_plan* p, const void* image, const void* mean, const double* krefs, int P,
                           const double* klists, int K, double sigma, void* lockin, int32_t* kidx, bool raw);
int tile_gradients_impl(gpa_plan* p, const void* image, size_t image_pitch, int r0, int c0, bool mean_on_device,
                               double mean, const double* kvecs, int P, const double* klists, int K, double sigma,
                               int mask_border, int i0, int j0, int t0, int t1, void* dx, size_t dx_pitch, size_t dx_plane,
                               void* dy, size_t dy_pitch, size_t dy_plane, void* wn, size_t wn_pitch, size_t wn_plane);
int plan_event(gpa_plan* p);
int dft_axes(gpa_plan* p);
int per_dft_staged(gpa_plan* p, const void* d_image, void* abs_out);
int gaussian_filter_dev(gpa_plan* p, const void* in, void* tmp, void* out, double sigma, const void* minuend);
int gaussian_weights(double sigma, std::vector<double>& w);
bool solve3(const double* m /*uu uv u vv v 1*/, const double* b, double* x);
Axis make_axis(int n);
Axis compact_axis(const Axis& full, int E);
int upload_real_table(gpa_plan* p, void* dst, const std::vector<double>& v);
int dmalloc(gpa_plan* p, void** ptr, size_t bytes);
// an unwrap that did not start: hipErrorNotSupported is the workspace's "this shape has no kernels" (gpa_unwrap_tables.hip)
inline int unwrap_fail(hipError_t e) {
  if (e == hipErrorNotSupported)
    return fail(GPA_ERR_STATE, "unwrap: no kernels for this shape -- an image with an axis that is not a power of two needs both axes <= 8192 "
                               "(f32) / 4096 (f64); powers of two go to 16384 per axis in both precisions (INTEGRATION.md, size limits)");
  return fail(GPA_ERR_HIP, std::string("unwrap: ") + hipGetErrorString(e));
}
int plan_build(gpa_plan* p);
int upload_twiddles(gpa_plan* p, void* dst, int L);

// installs the plan's profiler on the calling thread for the lifetime of the object (while gpa_set_profiling is on)
// the same, only when `own` (an entry point that may also be called from inside another profiled one)
struct ProfInstallIf {
  bool own;
  ProfInstallIf(gpa_plan* p, bool own_) : own(own_ && p->profiling) {
    if (!own) return;
    if (!p->kprof) p->kprof = new KernelProfiler();
    p->kprof->n = 0;
    g_kprof = p->kprof;
  }
  ~ProfInstallIf() { if (own) g_kprof = nullptr; }
};
struct ProfInstall {
  explicit ProfInstall(gpa_plan* p) {
    if (!p->profiling) return;
    if (!p->kprof) p->kprof = new KernelProfiler();
    p->kprof->n = 0;
    g_kprof = p->kprof;
  }
  ~ProfInstall() { g_kprof = nullptr; }
};

