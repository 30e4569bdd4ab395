// C ABI: per-pixel Kerelsky fits (pyGPA/property_extract.py:780-883), kernel in gpa_kerelsky.hip, arithmetic in gpa_kerelsky.h.
// Needs no plan: the host-pointer form stages in one DevBuf of its own (gpa_hoststage.h) that goes when the call returns.
// Every argument is checked, and named in the error, before a device is touched.
#include "gpa_plan.h"
#include "gpa_kerelsky.h"

namespace {

int kerelsky_check(const char* who, int dtype, size_t npx, const void* jac, const double* a0, const double* x0, int max_nfev,
                   double retry_cost, const void* out) {
  const std::string w = std::string(who) + ": ";
  if (dtype != GPA_F32 && dtype != GPA_F64) return fail(GPA_ERR_ARG, w + "dtype must be GPA_F32 or GPA_F64 (dtype = " + std::to_string(dtype) + ")");
  if (npx > GPA_KERELSKY_MAX_NPX) return fail(GPA_ERR_ARG, w + "npx = " + std::to_string(npx) + " is beyond GPA_KERELSKY_MAX_NPX");
  if (!jac) return fail(GPA_ERR_ARG, w + "null jac");
  if (!x0) return fail(GPA_ERR_ARG, w + "null x0");
  if (!out) return fail(GPA_ERR_ARG, w + "null out");
  for (int i = 0; i < 4; ++i) {
    if (a0 && !std::isfinite(a0[i])) return fail(GPA_ERR_ARG, w + "a0 must be finite");
    if (!std::isfinite(x0[i])) return fail(GPA_ERR_ARG, w + "x0 must be finite");
  }
  if (x0[0] < 0.0 || x0[2] < 0.0) return fail(GPA_ERR_ARG, w + "x0 must respect the bounds theta >= 0 and eps >= 0");
  if (!(x0[2] < kerelsky::EPS_POLE)) return fail(GPA_ERR_ARG, w + "x0 has eps beyond the pole of the strain matrix");
  if (max_nfev < 1) return fail(GPA_ERR_ARG, w + "max_nfev must be >= 1 (max_nfev = " + std::to_string(max_nfev) + ")");
  if (std::isnan(retry_cost)) return fail(GPA_ERR_ARG, w + "retry_cost must not be NaN");
  return GPA_OK;
}

KerelskyArgs pack(const double* a0, const double* x0, int max_nfev, double retry_cost) {
  KerelskyArgs p;
  for (int i = 0; i < 4; ++i) {
    p.a0[i] = a0 ? a0[i] : 0.0;
    p.x0[i] = x0[i];
  }
  p.retry_cost = retry_cost;
  p.max_nfev = max_nfev;
  p.has_a0 = a0 != nullptr;
  return p;
}

}  // namespace

int gpa_kerelsky_fit_dev(int device, int dtype, size_t npx, const void* jac, const double* a0, const double* x0, int max_nfev,
                         double retry_cost, void* out, double* cost, void* stream) {
  TRY(kerelsky_check("gpa_kerelsky_fit_dev", dtype, npx, jac, a0, x0, max_nfev, retry_cost, out));
  if (npx == 0) return GPA_OK;
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(launch_kerelsky(dtype, jac, npx, pack(a0, x0, max_nfev, retry_cost), out, cost, (hipStream_t)stream));
  return GPA_OK;
}

int gpa_kerelsky_fit(int device, int dtype, size_t npx, const void* jac, const double* a0, const double* x0, int max_nfev,
                     double retry_cost, void* out, double* cost) {
  TRY(kerelsky_check("gpa_kerelsky_fit", dtype, npx, jac, a0, x0, max_nfev, retry_cost, out));
  if (npx == 0) return GPA_OK;
  TRY(need_device("gpa_kerelsky_fit", device));
  const size_t bytes = 4 * npx * dtype_size(dtype);
  DevBuf tmp;   // a temporary of this call
  HostStage st(tmp, nullptr);
  const int i_jac = st.in(jac, bytes), i_out = st.out(out, bytes), i_cost = st.out(cost, npx * sizeof(double));
  HIP_TRY(st.upload());
  HIP_TRY(launch_kerelsky(dtype, st.dev(i_jac), npx, pack(a0, x0, max_nfev, retry_cost), st.dev(i_out), st.as<double>(i_cost), nullptr));
  HIP_TRY(st.download());
  return GPA_OK;
}
