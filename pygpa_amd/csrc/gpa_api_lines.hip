// C ABI: per-line medians and homogenize_per_axis (pyGPA/imagetools.py:112-125), kernels in gpa_lines.hip, keys, ranks and
// limits in gpa_lines.h.
//
// Every argument is checked before a device is touched.  All work space is the plan's (gpa_plan::lines, ::lines_tab; the
// host-pointer forms stage in gpa_plan::host_stage), so gpa_plan_workspace_bytes counts it.  The taps are built in f64 exactly as
// scipy.ndimage builds them and kept for the last sigma: a repeated call with the same sigma uploads nothing and does not synchronise.
//
// One homogenisation of nb frames:  transpose (mask applied) -> column medians -> profile 0, q0 -> row medians of image / q0
// (mask and division applied as the rows are loaded: `res` after axis 0 is never stored) -> profile 1, q1 -> out = (image / q0) / q1.
#include "gpa_plan.h"
#include "gpa_lines.h"

static_assert(GPA_LINES_MAX_N == LINES_MAX_N, "the limit of gpa_hip.h is that of gpa_lines.h");

namespace {

// the plan's work buffer for nb frames: nb transposed planes, then per frame three lines of n1 + n0 reals -- the reduced lines
// (axis 0: n1 values, then axis 1: n0 values), the filtered profiles and the divisors q
struct LinesWork {
  void* tws;
  unsigned char *med, *prof, *q;
  size_t stride;   // n1 + n0, elements between the lines of consecutive frames
};
int lines_work(gpa_plan* p, int nb, bool transpose, LinesWork* w) {
  const size_t planes = transpose ? up256((size_t)nb * p->n0 * p->n1 * p->rsz) : 0;
  const size_t stride = (size_t)p->n0 + p->n1, lines = up256((size_t)nb * stride * p->rsz);
  TRY(plan_reserve(p, p->lines, planes + 3 * lines, "hipMalloc"));
  unsigned char* b = p->lines.as<unsigned char>();
  w->tws = b;
  w->med = b + planes;
  w->prof = w->med + lines;
  w->q = w->prof + lines;
  w->stride = stride;
  return GPA_OK;
}

int lines_taps(gpa_plan* p, double sigma, const double** w_dev, int* R) {
  *R = lines_radius(sigma);
  const size_t bytes = (2 * (size_t)*R + 1) * sizeof(double);
  const void* before = p->lines_tab.ptr;
  TRY(plan_reserve(p, p->lines_tab, bytes, "hipMalloc"));
  if (p->lines_tab.ptr != before || p->lines_sigma != sigma) {
    HIP_TRY(hipStreamSynchronize(p->stream));   // an earlier call may still read the taps being replaced
    p->lines_sigma = -1.0;
    std::vector<double> w;
    gaussian_weights(sigma, w);
    HIP_TRY(hipMemcpyAsync(p->lines_tab.ptr, w.data(), bytes, hipMemcpyHostToDevice, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));   // w is a pageable host vector
    p->lines_sigma = sigma;
  }
  *w_dev = p->lines_tab.as<double>();
  return GPA_OK;
}

int check_sigma(double sigma, const std::string& w) {
  if (!std::isfinite(sigma) || !(sigma > 0.0)) return fail(GPA_ERR_ARG, w + "need a finite sigma > 0");
  if (sigma > LINES_MAX_SIGMA) return fail(GPA_ERR_ARG, w + "sigma = " + std::to_string(sigma) + " is beyond " + std::to_string((int)LINES_MAX_SIGMA));
  return GPA_OK;
}

int check_length(int n, const char* axis, const std::string& w) {
  if (!lines_length_ok(n))
    return fail(GPA_ERR_ARG, w + "a line along " + axis + " has " + std::to_string(n) + " samples, beyond GPA_LINES_MAX_N = " +
                                 std::to_string(LINES_MAX_N) + " (the keys of one line stay in LDS)");
  return GPA_OK;
}

int median_check(const gpa_plan* p, const void* image, int axis, const void* out, const char* who) {
  const std::string w = std::string(who) + ": ";
  if (!p) return fail(GPA_ERR_ARG, w + "null plan");
  if (!image) return fail(GPA_ERR_ARG, w + "null image");
  if (!out) return fail(GPA_ERR_ARG, w + "null out");
  if (axis != 0 && axis != 1) return fail(GPA_ERR_ARG, w + "axis must be 0 or 1 (axis = " + std::to_string(axis) + ")");
  return check_length(axis == 0 ? p->n0 : p->n1, axis == 0 ? "axis 0" : "axis 1", w);
}

int homogenize_check(const gpa_plan* p, const void* image, double sigma, int nb, const void* out, const char* who) {
  const std::string w = std::string(who) + ": ";
  if (!p) return fail(GPA_ERR_ARG, w + "null plan");
  if (!image) return fail(GPA_ERR_ARG, w + "null image");
  if (!out) return fail(GPA_ERR_ARG, w + "null out");
  if (nb < 1 || nb > LINES_MAX_FRAMES)
    return fail(GPA_ERR_ARG, w + "need 1 <= nb <= " + std::to_string(LINES_MAX_FRAMES) + " (nb = " + std::to_string(nb) + ")");
  TRY(check_sigma(sigma, w));
  TRY(check_length(p->n0, "axis 0", w));
  return check_length(p->n1, "axis 1", w);
}

int hip_fail(const char* who, hipError_t e) { return fail(GPA_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e)); }

#define LINES_TRY(who, expr)                          \
  do {                                                \
    const hipError_t _le = (expr);                    \
    if (_le != hipSuccess) return hip_fail(who, _le); \
  } while (0)

// all pointers on the device; profiles (nullable): nb x (n1 + n0)
int homogenize_checked(gpa_plan* p, const void* image, const uint8_t* mask, double sigma, int propagate, int nb, void* out,
                       void* profiles) {
  static const char* who = "gpa_homogenize_per_axis";
  HIP_TRY(hipSetDevice(p->device));
  LinesWork w;
  TRY(lines_work(p, nb, true, &w));
  const double* taps = nullptr;
  int R = 0;
  TRY(lines_taps(p, sigma, &taps, &R));
  const size_t rsz = p->rsz, off1 = (size_t)p->n1 * rsz;   // the axis-1 lines sit behind the n1 values of axis 0
  ProfInstall prof(p);
  LINES_TRY(who, lines_median(p->dtype, image, mask, p->n0, p->n1, nb, 0, propagate, nullptr, 0, w.tws, w.med, w.stride, p->stream));
  LINES_TRY(who, lines_profile(p->dtype, w.med, w.stride, p->n1, nb, taps, R, w.prof, w.q, p->stream));
  LINES_TRY(who, lines_median(p->dtype, image, mask, p->n0, p->n1, nb, 1, propagate, w.q, w.stride, nullptr, w.med + off1, w.stride, p->stream));
  LINES_TRY(who, lines_profile(p->dtype, w.med + off1, w.stride, p->n0, nb, taps, R, w.prof + off1, w.q + off1, p->stream));
  LINES_TRY(who, lines_apply(p->dtype, image, w.q, w.stride, w.q + off1, w.stride, out, p->n0, p->n1, nb, p->stream));
  if (profiles)
    HIP_TRY(hipMemcpyAsync(profiles, w.prof, (size_t)nb * w.stride * rsz, hipMemcpyDeviceToDevice, p->stream));
  return prof_finish(p);
}

// one frame with the reduced lines given: line0 (n1 values), line1 (n0 values, nullable: out = image / q0)
int homogenize_lines_checked(gpa_plan* p, const void* image, double sigma, const void* line0, const void* line1, void* out, void* profiles) {
  static const char* who = "gpa_homogenize_lines";
  HIP_TRY(hipSetDevice(p->device));
  LinesWork w;
  TRY(lines_work(p, 1, false, &w));
  const double* taps = nullptr;
  int R = 0;
  TRY(lines_taps(p, sigma, &taps, &R));
  const size_t rsz = p->rsz, off1 = (size_t)p->n1 * rsz;
  ProfInstall prof(p);
  LINES_TRY(who, lines_profile(p->dtype, line0, 0, p->n1, 1, taps, R, w.prof, w.q, p->stream));
  if (line1) LINES_TRY(who, lines_profile(p->dtype, line1, 0, p->n0, 1, taps, R, w.prof + off1, w.q + off1, p->stream));
  LINES_TRY(who, lines_apply(p->dtype, image, w.q, 0, line1 ? w.q + off1 : nullptr, 0, out, p->n0, p->n1, 1, p->stream));
  if (profiles)
    HIP_TRY(hipMemcpyAsync(profiles, w.prof, ((size_t)p->n1 + (line1 ? p->n0 : 0)) * rsz, hipMemcpyDeviceToDevice, p->stream));
  return prof_finish(p);
}

}  // namespace

int gpa_line_nanmedian_dev(gpa_plan* p, const void* image_dev, const uint8_t* mask_dev, int axis, int propagate_nan, void* out_dev) {
  static const char* who = "gpa_line_nanmedian_dev";
  TRY(median_check(p, image_dev, axis, out_dev, who));
  HIP_TRY(hipSetDevice(p->device));
  LinesWork w;
  TRY(lines_work(p, 1, axis == 0, &w));
  ProfInstall prof(p);
  LINES_TRY(who, lines_median(p->dtype, image_dev, mask_dev, p->n0, p->n1, 1, axis, propagate_nan != 0, nullptr, 0, w.tws, out_dev, 0, p->stream));
  return prof_finish(p);
}

int gpa_line_nanmedian(gpa_plan* p, const void* image, const uint8_t* mask, int axis, int propagate_nan, void* out) {
  TRY(median_check(p, image, axis, out, "gpa_line_nanmedian"));
  HIP_TRY(hipSetDevice(p->device));
  const size_t npx = (size_t)p->n0 * p->n1;
  HostStage st(p->host_stage, p->stream);
  const int i_img = st.in(image, npx * p->rsz), i_mask = st.in(mask, npx);
  const int i_out = st.out(out, (size_t)(axis == 0 ? p->n1 : p->n0) * p->rsz);
  HIP_TRY(st.upload());
  TRY(gpa_line_nanmedian_dev(p, st.dev(i_img), st.as<uint8_t>(i_mask), axis, propagate_nan, st.dev(i_out)));
  HIP_TRY(st.download());
  return GPA_OK;
}

int gpa_homogenize_per_axis_dev(gpa_plan* p, const void* image_dev, const uint8_t* mask_dev, double sigma, int propagate_nan, int nb,
                                void* out_dev, void* profiles_dev) {
  TRY(homogenize_check(p, image_dev, sigma, nb, out_dev, "gpa_homogenize_per_axis_dev"));
  return homogenize_checked(p, image_dev, mask_dev, sigma, propagate_nan != 0, nb, out_dev, profiles_dev);
}

int gpa_homogenize_per_axis(gpa_plan* p, const void* image, const uint8_t* mask, double sigma, int propagate_nan, int nb, void* out,
                            void* profiles) {
  TRY(homogenize_check(p, image, sigma, nb, out, "gpa_homogenize_per_axis"));
  HIP_TRY(hipSetDevice(p->device));
  const size_t npx = (size_t)p->n0 * p->n1, frames = (size_t)nb * npx * p->rsz;
  HostStage st(p->host_stage, p->stream);
  const int i_img = st.in(image, frames), i_out = st.out(out, frames), i_mask = st.in(mask, npx);
  const int i_prof = st.out(profiles, (size_t)nb * ((size_t)p->n0 + p->n1) * p->rsz);
  HIP_TRY(st.upload());
  TRY(homogenize_checked(p, st.dev(i_img), st.as<uint8_t>(i_mask), sigma, propagate_nan != 0, nb, st.dev(i_out), st.dev(i_prof)));
  HIP_TRY(st.download());
  return GPA_OK;
}

int gpa_homogenize_lines_dev(gpa_plan* p, const void* image_dev, double sigma, const void* line0_dev, const void* line1_dev, void* out_dev,
                             void* profiles_dev) {
  TRY(homogenize_check(p, image_dev, sigma, 1, out_dev, "gpa_homogenize_lines_dev"));
  if (!line0_dev) return fail(GPA_ERR_ARG, "gpa_homogenize_lines_dev: null line0");
  return homogenize_lines_checked(p, image_dev, sigma, line0_dev, line1_dev, out_dev, profiles_dev);
}

int gpa_homogenize_lines(gpa_plan* p, const void* image, double sigma, const void* line0, const void* line1, void* out, void* profiles) {
  TRY(homogenize_check(p, image, sigma, 1, out, "gpa_homogenize_lines"));
  if (!line0) return fail(GPA_ERR_ARG, "gpa_homogenize_lines: null line0");
  HIP_TRY(hipSetDevice(p->device));
  const size_t plane = (size_t)p->n0 * p->n1 * p->rsz, l0 = (size_t)p->n1 * p->rsz, l1 = (size_t)p->n0 * p->rsz;
  HostStage st(p->host_stage, p->stream);
  const int i_img = st.in(image, plane), i_out = st.out(out, plane), i_l0 = st.in(line0, l0), i_l1 = st.in(line1, l1);
  const int i_prof = st.out(profiles, l0 + (line1 ? l1 : 0));
  HIP_TRY(st.upload());
  TRY(homogenize_lines_checked(p, st.dev(i_img), sigma, st.dev(i_l0), st.dev(i_l1), st.dev(i_out), st.dev(i_prof)));
  HIP_TRY(st.download());
  return GPA_OK;
}
