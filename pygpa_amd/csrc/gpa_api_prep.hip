// C ABI: image preparation (pyGPA/imagetools.py:92-194), kernels in gpa_prep.hip, geometry and limits in gpa_prep.h.
//
// Every argument is checked before a device is touched.  All work space is the plan's (gpa_plan::prep, ::prep_tab; the
// host-pointer forms stage in gpa_plan::host_stage), so gpa_plan_workspace_bytes counts it.  The filter tables (transfer functions and twiddles of the two segment
// lengths, or the taps of the direct route) are built in f64, rounded once and kept for the last sigma: a repeated call with
// the same sigma uploads nothing and does not synchronise.
#include "gpa_plan.h"
#include "gpa_prep.h"

static_assert(GPA_PREP_MAX_R == PREP_MAX_R && GPA_PREP_MAX_N1 == PREP_MAX_N1, "the limits of gpa_hip.h are those of gpa_prep.h");

namespace {

// the plan's work buffer: [0, 16) min / max keys, [64, 80) lims, [256, 768) chords, from 1024 on two real planes and two byte planes
struct PrepWork {
  unsigned long long* mm;
  int* lims;
  uint8_t* chord;
  void *num, *den;
  uint8_t *cov0, *cov;
};
int prep_work(gpa_plan* p, PrepWork* w) {
  const size_t npx = (size_t)p->n0 * p->n1, pr = up256(npx * p->rsz), pb = up256(npx);
  const void* before = p->prep.ptr;
  TRY(plan_reserve(p, p->prep, 1024 + 2 * pr + 2 * pb, "hipMalloc"));
  if (p->prep.ptr != before) p->prep_chord_r = -1;
  unsigned char* b = p->prep.as<unsigned char>();
  w->mm = reinterpret_cast<unsigned long long*>(b);
  w->lims = reinterpret_cast<int*>(b + 64);
  w->chord = b + 256;
  w->num = b + 1024;
  w->den = b + 1024 + pr;
  w->cov0 = b + 1024 + 2 * pr;
  w->cov = w->cov0 + pb;
  return GPA_OK;
}

int check_plan(const gpa_plan* p, const std::string& w) {
  if (!p) return fail(GPA_ERR_ARG, w + "null plan");
  return GPA_OK;
}

// the route and the radius of a sigma on this plan; GPA_ERR_ARG naming sigma where neither route serves it
int homogenize_route(const gpa_plan* p, double sigma, const std::string& w, int* R_out, int* lg0, int* lg1) {
  if (!std::isfinite(sigma) || !(sigma > 0.0)) return fail(GPA_ERR_ARG, w + "need a finite sigma > 0");
  if (sigma > 16384.0) return fail(GPA_ERR_ARG, w + "sigma = " + std::to_string(sigma) + " is beyond every segment length");
  const int R = (int)(4.0 * sigma + 0.5);
  const int minr = opt_set(OPT_GAUSS_FFT_MINR) ? (int)opt(OPT_GAUSS_FFT_MINR).num : 12;
  *lg0 = *lg1 = 0;
  if (R >= minr) {
    *lg0 = gaussfft_choose_lg(p->dtype, p->n0, R, true);
    *lg1 = gaussfft_choose_lg(p->dtype, p->n1, R, false);
  }
  if (!*lg0 || !*lg1) {
    *lg0 = *lg1 = 0;
    if (2 * R + 1 > PREP_MAX_DIRECT_TAPS)
      return fail(GPA_ERR_ARG, w + "sigma = " + std::to_string(sigma) + " gives the radius " + std::to_string(R) +
                                   ": no FFT segment length fits (4 R <= 16384 in f32, 8192 in f64) and the direct sum stops at " +
                                   std::to_string(PREP_MAX_DIRECT_TAPS) + " taps");
  }
  *R_out = R;
  return GPA_OK;
}

int homogenize_check(const gpa_plan* p, const void* image, const void* mask, double sigma, const void* out, const char* who, int* R,
                     int* lg0, int* lg1) {
  const std::string w = std::string(who) + ": ";
  TRY(check_plan(p, w));
  if (!image) return fail(GPA_ERR_ARG, w + "null image");
  if (!mask) return fail(GPA_ERR_ARG, w + "null mask");
  if (!out) return fail(GPA_ERR_ARG, w + "null out");
  if (p->n1 > PREP_MAX_N1)
    return fail(GPA_ERR_STATE, w + "the plan's rows are longer than GPA_PREP_MAX_N1 = " + std::to_string(PREP_MAX_N1));
  return homogenize_route(p, sigma, w, R, lg0, lg1);
}

// device tables of (sigma, lg0, lg1) in prep_tab: H0 | tw0 | H1 | tw1 on the FFT route, the taps (doubles) on the direct one
int homogenize_tables(gpa_plan* p, double sigma, int R, int lg0, int lg1, PrepHomogenize* a) {
  const size_t L0 = lg0 ? (size_t)1 << lg0 : 0, L1 = lg1 ? (size_t)1 << lg1 : 0;
  const size_t oH0 = 0, otw0 = up256(L0 * p->rsz), oH1 = otw0 + up256(L0 * p->csz), otw1 = oH1 + up256(L1 * p->rsz);
  const size_t bytes = lg0 ? otw1 + up256(L1 * p->csz) : PREP_MAX_DIRECT_TAPS * sizeof(double);
  const void* before = p->prep_tab.ptr;
  TRY(plan_reserve(p, p->prep_tab, bytes, "hipMalloc"));
  unsigned char* b = p->prep_tab.as<unsigned char>();
  if (p->prep_tab.ptr != before || p->prep_sigma != sigma || p->prep_lg0 != lg0 || p->prep_lg1 != lg1) {
    HIP_TRY(hipStreamSynchronize(p->stream));   // an earlier call may still read the tables being replaced
    p->prep_sigma = -1.0;
    std::vector<double> w;
    gaussian_weights(sigma, w);
    if (lg0) {
      TRY(upload_real_table(p, b + oH0, gaussfft_table(lg0, w)));
      TRY(upload_twiddles(p, b + otw0, (int)L0));
      TRY(upload_real_table(p, b + oH1, gaussfft_table(lg1, w)));
      TRY(upload_twiddles(p, b + otw1, (int)L1));
    } else {
      HIP_TRY(hipMemcpyAsync(b, w.data(), w.size() * sizeof(double), hipMemcpyHostToDevice, p->stream));
      HIP_TRY(hipStreamSynchronize(p->stream));   // w is a pageable host vector
    }
    p->prep_sigma = sigma;
    p->prep_lg0 = lg0;
    p->prep_lg1 = lg1;
  }
  a->R = R;
  a->lg0 = lg0;
  a->lg1 = lg1;
  a->H0 = b + oH0; a->tw0 = b + otw0; a->H1 = b + oH1; a->tw1 = b + otw1;
  a->w = reinterpret_cast<const double*>(b);
  return GPA_OK;
}

int homogenize_checked(gpa_plan* p, const void* image, const void* mask, double sigma, int R, int lg0, int lg1, int use_nan_scale,
                       double nan_scale, void* out, void* vv) {
  HIP_TRY(hipSetDevice(p->device));
  PrepWork w;
  TRY(prep_work(p, &w));
  PrepHomogenize a{};
  TRY(homogenize_tables(p, sigma, R, lg0, lg1, &a));
  a.image = image;
  a.mask = static_cast<const uint8_t*>(mask);
  a.num = w.num; a.den = w.den; a.cov0 = w.cov0; a.cov = w.cov; a.mm = w.mm;
  a.out = out; a.vv = vv;
  a.n0 = p->n0; a.n1 = p->n1;
  a.use_nan_scale = use_nan_scale != 0;
  a.nan_scale = nan_scale;
  ProfInstall prof(p);
  const hipError_t e = prep_homogenize(p->dtype, a, p->stream);
  if (e != hipSuccess) return fail(GPA_ERR_HIP, std::string("gpa_gauss_homogenize: ") + hipGetErrorString(e));
  return prof_finish(p);
}

int erode_check(const gpa_plan* p, const void* in, int r, const void* out, const char* who) {
  const std::string w = std::string(who) + ": ";
  TRY(check_plan(p, w));
  if (!in) return fail(GPA_ERR_ARG, w + "null in");
  if (!out) return fail(GPA_ERR_ARG, w + "null out");
  if (r < 0) return fail(GPA_ERR_ARG, w + "need r >= 0 (r = " + std::to_string(r) + ")");
  if (r > PREP_MAX_R)
    return fail(GPA_ERR_ARG, w + "r = " + std::to_string(r) + " is beyond GPA_PREP_MAX_R = " + std::to_string(PREP_MAX_R) +
                                 " (row distances are kept as bytes)");
  return GPA_OK;
}

int erode_checked(gpa_plan* p, const void* in, int invert, int r, void* out) {
  HIP_TRY(hipSetDevice(p->device));
  PrepWork w;
  TRY(prep_work(p, &w));
  if (p->prep_chord_r != r) {
    HIP_TRY(hipStreamSynchronize(p->stream));   // an earlier erosion may still read the chords being replaced
    uint8_t chord[2 * PREP_MAX_R + 1];
    for (int dy = -r; dy <= r; ++dy) chord[dy + r] = (uint8_t)prep_disk_chord(r, dy);
    p->prep_chord_r = -1;
    HIP_TRY(hipMemcpyAsync(w.chord, chord, (size_t)2 * r + 1, hipMemcpyHostToDevice, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    p->prep_chord_r = r;
  }
  ProfInstall prof(p);
  const hipError_t e = prep_erode_disk(static_cast<const uint8_t*>(in), invert != 0, r, p->n0, p->n1, w.cov0, w.chord,
                                       static_cast<uint8_t*>(out), p->stream);
  if (e != hipSuccess) return fail(GPA_ERR_HIP, std::string("gpa_mask_erode_disk: ") + hipGetErrorString(e));
  return prof_finish(p);
}

int any_equal_check(const gpa_plan* p, const void* frames, int B, const void* hit, const char* who) {
  const std::string w = std::string(who) + ": ";
  TRY(check_plan(p, w));
  if (!frames) return fail(GPA_ERR_ARG, w + "null frames");
  if (!hit) return fail(GPA_ERR_ARG, w + "null hit");
  if (B < 1) return fail(GPA_ERR_ARG, w + "need B >= 1 (B = " + std::to_string(B) + ")");
  return GPA_OK;
}

}  // namespace

int gpa_gauss_homogenize_dev(gpa_plan* p, const void* image_dev, const uint8_t* mask_dev, double sigma, int use_nan_scale,
                             double nan_scale, void* out_dev, void* vv_dev) {
  int R = 0, lg0 = 0, lg1 = 0;
  TRY(homogenize_check(p, image_dev, mask_dev, sigma, out_dev, "gpa_gauss_homogenize_dev", &R, &lg0, &lg1));
  return homogenize_checked(p, image_dev, mask_dev, sigma, R, lg0, lg1, use_nan_scale, nan_scale, out_dev, vv_dev);
}

int gpa_gauss_homogenize(gpa_plan* p, const void* image, const uint8_t* mask, double sigma, int use_nan_scale, double nan_scale,
                         void* out, void* vv_out) {
  int R = 0, lg0 = 0, lg1 = 0;
  TRY(homogenize_check(p, image, mask, sigma, out, "gpa_gauss_homogenize", &R, &lg0, &lg1));
  HIP_TRY(hipSetDevice(p->device));
  const size_t npx = (size_t)p->n0 * p->n1;
  HostStage st(p->host_stage, p->stream);
  const int i_img = st.in(image, npx * p->rsz), i_out = st.out(out, npx * p->rsz), i_vv = st.out(vv_out, npx * p->rsz);
  const int i_mask = st.in(mask, npx);
  HIP_TRY(st.upload());
  TRY(homogenize_checked(p, st.dev(i_img), st.dev(i_mask), sigma, R, lg0, lg1, use_nan_scale, nan_scale, st.dev(i_out), st.dev(i_vv)));
  HIP_TRY(st.download());
  return GPA_OK;
}

int gpa_mask_any_equal_dev(gpa_plan* p, const void* frames_dev, int B, double value, int accumulate, uint8_t* hit_dev) {
  TRY(any_equal_check(p, frames_dev, B, hit_dev, "gpa_mask_any_equal_dev"));
  HIP_TRY(hipSetDevice(p->device));
  ProfInstall prof(p);
  const hipError_t e = prep_any_equal(p->dtype, frames_dev, B, p->n0, p->n1, value, accumulate != 0, hit_dev, p->stream);
  if (e != hipSuccess) return fail(GPA_ERR_HIP, std::string("gpa_mask_any_equal: ") + hipGetErrorString(e));
  return prof_finish(p);
}

int gpa_mask_any_equal(gpa_plan* p, const void* frames, int B, double value, int accumulate, uint8_t* hit) {
  TRY(any_equal_check(p, frames, B, hit, "gpa_mask_any_equal"));
  HIP_TRY(hipSetDevice(p->device));
  const size_t npx = (size_t)p->n0 * p->n1;
  HostStage st(p->host_stage, p->stream);
  const int i_hit = st.inout(hit, npx, accumulate != 0), i_frames = st.in(frames, (size_t)B * npx * p->rsz);
  HIP_TRY(st.upload());
  TRY(gpa_mask_any_equal_dev(p, st.dev(i_frames), B, value, accumulate, st.as<uint8_t>(i_hit)));
  HIP_TRY(st.download());
  return GPA_OK;
}

int gpa_mask_erode_disk_dev(gpa_plan* p, const uint8_t* in_dev, int invert, int r, uint8_t* out_dev) {
  TRY(erode_check(p, in_dev, r, out_dev, "gpa_mask_erode_disk_dev"));
  return erode_checked(p, in_dev, invert, r, out_dev);
}

int gpa_mask_erode_disk(gpa_plan* p, const uint8_t* in, int invert, int r, uint8_t* out) {
  TRY(erode_check(p, in, r, out, "gpa_mask_erode_disk"));
  HIP_TRY(hipSetDevice(p->device));
  const size_t npx = (size_t)p->n0 * p->n1;
  HostStage st(p->host_stage, p->stream);
  const int i_in = st.in(in, npx), i_out = st.out(out, npx);
  HIP_TRY(st.upload());
  TRY(erode_checked(p, st.dev(i_in), invert, r, st.dev(i_out)));
  HIP_TRY(st.download());
  return GPA_OK;
}

int gpa_mask_bounds_dev(gpa_plan* p, const uint8_t* mask_dev, int32_t* lims) {
  const std::string w = "gpa_mask_bounds_dev: ";
  TRY(check_plan(p, w));
  if (!mask_dev) return fail(GPA_ERR_ARG, w + "null mask");
  if (!lims) return fail(GPA_ERR_ARG, w + "null lims");
  HIP_TRY(hipSetDevice(p->device));
  PrepWork wk;
  TRY(prep_work(p, &wk));
  HIP_TRY(prep_mask_bounds(mask_dev, p->n0, p->n1, wk.lims, p->stream));
  HIP_TRY(hipMemcpyAsync(lims, wk.lims, 4 * sizeof(int32_t), hipMemcpyDeviceToHost, p->stream));
  HIP_TRY(hipStreamSynchronize(p->stream));
  return GPA_OK;
}

int gpa_mask_bounds(gpa_plan* p, const uint8_t* mask, int32_t* lims) {
  const std::string w = "gpa_mask_bounds: ";
  TRY(check_plan(p, w));
  if (!mask) return fail(GPA_ERR_ARG, w + "null mask");
  if (!lims) return fail(GPA_ERR_ARG, w + "null lims");
  HIP_TRY(hipSetDevice(p->device));
  HostStage st(p->host_stage, p->stream);
  const int i_mask = st.in(mask, (size_t)p->n0 * p->n1);
  HIP_TRY(st.upload());
  return gpa_mask_bounds_dev(p, st.as<uint8_t>(i_mask), lims);   // (drains the stream)
}

int gpa_nan_lines_dev(gpa_plan* p, const void* image_dev, uint8_t* rows, uint8_t* cols) {
  const std::string w = "gpa_nan_lines_dev: ";
  TRY(check_plan(p, w));
  if (!image_dev) return fail(GPA_ERR_ARG, w + "null image");
  if (!rows) return fail(GPA_ERR_ARG, w + "null rows");
  if (!cols) return fail(GPA_ERR_ARG, w + "null cols");
  HIP_TRY(hipSetDevice(p->device));
  PrepWork wk;
  TRY(prep_work(p, &wk));
  // the flags land in the first byte plane of the work buffer: n0 + n1 <= n0 n1 for the plan's shapes (both axes >= 2)
  uint8_t *d_rows = wk.cov0, *d_cols = wk.cov0 + p->n0;
  HIP_TRY(prep_nan_lines(p->dtype, image_dev, p->n0, p->n1, d_rows, d_cols, p->stream));
  HIP_TRY(hipMemcpyAsync(rows, d_rows, (size_t)p->n0, hipMemcpyDeviceToHost, p->stream));
  HIP_TRY(hipMemcpyAsync(cols, d_cols, (size_t)p->n1, hipMemcpyDeviceToHost, p->stream));
  HIP_TRY(hipStreamSynchronize(p->stream));
  return GPA_OK;
}

int gpa_nan_lines(gpa_plan* p, const void* image, uint8_t* rows, uint8_t* cols) {
  const std::string w = "gpa_nan_lines: ";
  TRY(check_plan(p, w));
  if (!image) return fail(GPA_ERR_ARG, w + "null image");
  if (!rows) return fail(GPA_ERR_ARG, w + "null rows");
  if (!cols) return fail(GPA_ERR_ARG, w + "null cols");
  HIP_TRY(hipSetDevice(p->device));
  HostStage st(p->host_stage, p->stream);
  const int i_img = st.in(image, (size_t)p->n0 * p->n1 * p->rsz);
  HIP_TRY(st.upload());
  return gpa_nan_lines_dev(p, st.dev(i_img), rows, cols);   // (drains the stream)
}

int gpa_nan_trim_lims_dev(gpa_plan* p, const void* image_dev, int32_t* lims) {
  const std::string w = "gpa_nan_trim_lims_dev: ";
  TRY(check_plan(p, w));
  if (!image_dev) return fail(GPA_ERR_ARG, w + "null image");
  if (!lims) return fail(GPA_ERR_ARG, w + "null lims");
  HIP_TRY(hipSetDevice(p->device));
  PrepWork wk;
  TRY(prep_work(p, &wk));
  HIP_TRY(prep_trim_lims(p->dtype, image_dev, p->n0, p->n1, wk.lims, p->stream));
  HIP_TRY(hipMemcpyAsync(lims, wk.lims, 4 * sizeof(int32_t), hipMemcpyDeviceToHost, p->stream));
  HIP_TRY(hipStreamSynchronize(p->stream));
  return GPA_OK;
}

int gpa_nan_trim_lims(gpa_plan* p, const void* image, int32_t* lims) {
  const std::string w = "gpa_nan_trim_lims: ";
  TRY(check_plan(p, w));
  if (!image) return fail(GPA_ERR_ARG, w + "null image");
  if (!lims) return fail(GPA_ERR_ARG, w + "null lims");
  HIP_TRY(hipSetDevice(p->device));
  HostStage st(p->host_stage, p->stream);
  const int i_img = st.in(image, (size_t)p->n0 * p->n1 * p->rsz);
  HIP_TRY(st.upload());
  return gpa_nan_trim_lims_dev(p, st.dev(i_img), lims);   // (drains the stream)
}
