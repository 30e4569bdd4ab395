// C ABI: per-pixel Kerelsky fits (pyGPA/property_extract.py:780-883), kernel in gpa_kerelsky.hip, arithmetic in gpa_kerelsky.h.
// Needs no plan.  Every argument is checked, and named in the error, before a device is touched.
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
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(GPA_ERR_NODEV, "gpa_kerelsky_fit: no HIP device");
  HIP_TRY(hipSetDevice(device));
  const size_t bytes = 4 * npx * (dtype == GPA_F32 ? 4 : 8);
  DevBuf d_j, d_x, d_c;   // temporaries of this call
  HIP_TRY(d_j.reserve(bytes, nullptr));
  HIP_TRY(d_x.reserve(bytes, nullptr));
  if (cost) HIP_TRY(d_c.reserve(npx * sizeof(double), nullptr));
  HIP_TRY(hipMemcpy(d_j.ptr, jac, bytes, hipMemcpyHostToDevice));
  HIP_TRY(launch_kerelsky(dtype, d_j.ptr, npx, pack(a0, x0, max_nfev, retry_cost), d_x.ptr, cost ? d_c.as<double>() : nullptr, nullptr));
  HIP_TRY(hipMemcpy(out, d_x.ptr, bytes, hipMemcpyDeviceToHost));
  if (cost) HIP_TRY(hipMemcpy(cost, d_c.ptr, npx * sizeof(double), hipMemcpyDeviceToHost));
  return GPA_OK;
}
