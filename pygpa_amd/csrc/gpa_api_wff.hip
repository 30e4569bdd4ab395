// C ABI: windowed Fourier filtering (geometric_phase_analysis.py:551-580), kernels in gpa_wff.hip, geometry in gpa_wff.h.
//
// The taps are built here in f64 -- g(j) = exp(-j^2 / 2 sigma^2), kx(j) = g(j) e^(i wx j), ky(j) = g(j) e^(i wy j) / sum g^2,
// every phasor from its own cos / sin, none by recurrence -- rounded once to the plan's precision and uploaded once per call.
// All work space is the plan's (gpa_plan::wff; the host-pointer form stages in gpa_plan::host_stage), so
// gpa_plan_workspace_bytes counts it.
#include "gpa_plan.h"
#include "gpa_wff.h"

static_assert(GPA_WFF_MAX_S == WFF_MAX_S && GPA_WFF_MAX_T == WFF_MAX_T, "the limits of gpa_hip.h are those of gpa_wff.h");

static bool all_finite(const double* v, int n) {
  for (int i = 0; i < n; ++i)
    if (!std::isfinite(v[i])) return false;
  return true;
}

// every argument error of the two entry points, before a device is touched; *s_out: the half-window
static int wff_check(const gpa_plan* p, const void* image, double sigma, const double* wxs, int Kx, const double* wys, int Ky,
                     const double* thresholds, int T, double scale, const void* out, const char* who, int* s_out) {
  const std::string w = std::string(who) + ": ";
  if (!p) return fail(GPA_ERR_ARG, w + "null plan");
  if (!image) return fail(GPA_ERR_ARG, w + "null image");
  if (!out) return fail(GPA_ERR_ARG, w + "null out");
  if (!wxs) return fail(GPA_ERR_ARG, w + "null wxs");
  if (!wys) return fail(GPA_ERR_ARG, w + "null wys");
  if (!thresholds) return fail(GPA_ERR_ARG, w + "null thresholds");
  if (Kx < 1) return fail(GPA_ERR_ARG, w + "need Kx >= 1 (Kx = " + std::to_string(Kx) + ")");
  if (Ky < 1) return fail(GPA_ERR_ARG, w + "need Ky >= 1 (Ky = " + std::to_string(Ky) + ")");
  if (T < 1) return fail(GPA_ERR_ARG, w + "need T >= 1 (T = " + std::to_string(T) + ")");
  if (!std::isfinite(sigma) || !(sigma > 0.0)) return fail(GPA_ERR_ARG, w + "need a finite sigma > 0");
  if (!all_finite(wxs, Kx)) return fail(GPA_ERR_ARG, w + "wxs holds a value that is not finite");
  if (!all_finite(wys, Ky)) return fail(GPA_ERR_ARG, w + "wys holds a value that is not finite");
  if (!all_finite(thresholds, T)) return fail(GPA_ERR_ARG, w + "thresholds holds a value that is not finite");
  if (!std::isfinite(scale)) return fail(GPA_ERR_ARG, w + "scale is not finite");
  const int s = wff_half_window(sigma);
  if (s < 1)
    return fail(GPA_ERR_ARG, w + "sigma = " + std::to_string(sigma) + " gives an empty window (s = round(2 sigma) must be >= 1)");
  if (s > WFF_MAX_S)
    return fail(GPA_ERR_ARG, w + "sigma = " + std::to_string(sigma) + " gives the half-window s = round(2 sigma) = " + std::to_string(s) +
                                 ", beyond GPA_WFF_MAX_S = " + std::to_string(WFF_MAX_S) + " (the column tile must fit 160 KiB of LDS)");
  if (T > WFF_MAX_T)
    return fail(GPA_ERR_ARG, w + "T = " + std::to_string(T) + " thresholds are beyond GPA_WFF_MAX_T = " + std::to_string(WFF_MAX_T) +
                                 " per call (split the list)");
  if ((size_t)Kx > ((size_t)1 << 20) || (size_t)Ky > ((size_t)1 << 20))
    return fail(GPA_ERR_ARG, w + "Kx and Ky may not exceed 2^20 frequencies");
  *s_out = s;
  return GPA_OK;
}

// the tables of a call, as the bytes the kernels read: txr [Kx][2 s], tyr [Ky][wpad] (zero behind 2 s), thr2 [wff_tslots(T)]
template <class R>
static void wff_tables(double sigma, int s, int wpad, const double* wxs, int Kx, const double* wys, int Ky, const double* thr, int T,
                       std::vector<unsigned char>& bytes, size_t* off_tyr, size_t* off_thr) {
  const int W = 2 * s, TT = wff_tslots(T);
  std::vector<double> g(W);
  double nrm = 0.0;
  for (int t = 0; t < W; ++t) {   // reversed: entry t is offset j = s - 1 - t
    const double j = (double)(s - 1 - t);
    g[t] = exp(-(j * j) / (2.0 * sigma * sigma));
    nrm += g[t] * g[t];
  }
  *off_tyr = up256((size_t)Kx * W * 2 * sizeof(R));
  *off_thr = up256(*off_tyr + (size_t)Ky * wpad * 2 * sizeof(R));
  bytes.assign(*off_thr + up256(TT * sizeof(R)), 0);
  R* tx = reinterpret_cast<R*>(bytes.data());
  R* ty = reinterpret_cast<R*>(bytes.data() + *off_tyr);
  R* t2 = reinterpret_cast<R*>(bytes.data() + *off_thr);
  for (int k = 0; k < Kx; ++k)
    for (int t = 0; t < W; ++t) {
      const double ph = wxs[k] * (double)(s - 1 - t);
      tx[((size_t)k * W + t) * 2] = (R)(g[t] * cos(ph));
      tx[((size_t)k * W + t) * 2 + 1] = (R)(g[t] * sin(ph));
    }
  for (int k = 0; k < Ky; ++k)
    for (int t = 0; t < W; ++t) {
      const double ph = wys[k] * (double)(s - 1 - t);
      ty[((size_t)k * wpad + t) * 2] = (R)(g[t] * cos(ph) / nrm);
      ty[((size_t)k * wpad + t) * 2 + 1] = (R)(g[t] * sin(ph) / nrm);
    }
  // np.abs(sf) >= thr, decided as |sf|^2 >= thr^2: a negative threshold keeps everything (also a NaN-free zero), the unused
  // slots of the instantiation keep nothing
  for (int t = 0; t < TT; ++t)
    t2[t] = t >= T ? std::numeric_limits<R>::infinity() : thr[t] < 0.0 ? (R)-1 : (R)(thr[t] * thr[t]);
}

static int wff_dev_checked(gpa_plan* p, const void* image_dev, double sigma, int s, const double* wxs, int Kx, const double* wys, int Ky,
                           const double* thresholds, int T, double scale, void* out_dev) {
  const bool f64 = p->dtype == GPA_F64;
  const WffTile tl = wff_tile(s, T, f64);
  if (!tl.ok) return fail(GPA_ERR_ARG, "gpa_wff: no column tile for s = " + std::to_string(s) + ", T = " + std::to_string(T));
  HIP_TRY(hipSetDevice(p->device));
  std::vector<unsigned char> tab;
  size_t off_tyr = 0, off_thr = 0;
  if (f64) wff_tables<double>(sigma, s, tl.wpad, wxs, Kx, wys, Ky, thresholds, T, tab, &off_tyr, &off_thr);
  else wff_tables<float>(sigma, s, tl.wpad, wxs, Kx, wys, Ky, thresholds, T, tab, &off_tyr, &off_thr);
  const size_t plane = up256((size_t)p->n0 * p->n1 * p->csz);
  TRY(plan_reserve(p, p->wff, tab.size() + (size_t)(1 + T) * plane, "hipMalloc"));
  unsigned char* base = p->wff.as<unsigned char>();
  // (pageable source: the copy has left `tab` when the stream has drained)
  HIP_TRY(hipMemcpyAsync(base, tab.data(), tab.size(), hipMemcpyHostToDevice, p->stream));
  HIP_TRY(hipStreamSynchronize(p->stream));
  ProfInstall prof(p);
  const hipError_t e = wff_run(p->dtype, image_dev, p->n0, p->n1, s, base, Kx, base + off_tyr, Ky, base + off_thr, T, scale,
                               base + tab.size(), base + tab.size() + plane, out_dev, p->stream);
  if (e != hipSuccess) return fail(GPA_ERR_HIP, std::string("gpa_wff: ") + hipGetErrorString(e));
  return prof_finish(p);
}

int gpa_wff_dev(gpa_plan* p, const void* image_dev, double sigma, const double* wxs, int Kx, const double* wys, int Ky,
                const double* thresholds, int T, double scale, void* out_dev) {
  int s = 0;
  TRY(wff_check(p, image_dev, sigma, wxs, Kx, wys, Ky, thresholds, T, scale, out_dev, "gpa_wff_dev", &s));
  return wff_dev_checked(p, image_dev, sigma, s, wxs, Kx, wys, Ky, thresholds, T, scale, out_dev);
}

int gpa_wff(gpa_plan* p, const void* image, double sigma, const double* wxs, int Kx, const double* wys, int Ky,
            const double* thresholds, int T, double scale, void* out) {
  int s = 0;
  TRY(wff_check(p, image, sigma, wxs, Kx, wys, Ky, thresholds, T, scale, out, "gpa_wff", &s));
  HIP_TRY(hipSetDevice(p->device));
  const size_t plane = (size_t)p->n0 * p->n1 * p->csz;
  HostStage st(p->host_stage, p->stream);
  const int i_img = st.in(image, plane), i_out = st.out(out, (size_t)T * plane);
  HIP_TRY(st.upload());
  TRY(wff_dev_checked(p, st.dev(i_img), sigma, s, wxs, Kx, wys, Ky, thresholds, T, scale, st.dev(i_out)));
  HIP_TRY(st.download());
  return GPA_OK;
}
