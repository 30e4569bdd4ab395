// C ABI: Jacobian and property maps from a displacement field or from phases (pyGPA/property_extract.py:13-52, :181-217,
// :258-278), kernels in gpa_fieldjac.hip, geometry in gpa_fieldjac.h.  Needs no plan.  Every argument is checked, and named in
// the error, before a device is touched.
#include "gpa_plan.h"
#include "gpa_fieldjac.h"

namespace {

size_t esize(int dtype) { return dtype == GPA_F32 ? 4 : 8; }

bool overlaps(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return a && b && x < y + nb && y < x + na;
}

// what the two Jacobian entry points share: dtype, shape, spacing, outputs
int jac_common(const std::string& w, int dtype, int nimg, int n0, int n1, double nmperpixel, const void* J, const void* props) {
  if (dtype != GPA_F32 && dtype != GPA_F64) return fail(GPA_ERR_ARG, w + "dtype must be GPA_F32 or GPA_F64 (dtype = " + std::to_string(dtype) + ")");
  if (nimg < 1) return fail(GPA_ERR_ARG, w + "nimg must be >= 1 (nimg = " + std::to_string(nimg) + ")");
  if (n0 < 2) return fail(GPA_ERR_ARG, w + "n0 must be >= 2, a difference needs two samples (n0 = " + std::to_string(n0) + ")");
  if (n1 < 2) return fail(GPA_ERR_ARG, w + "n1 must be >= 2, a difference needs two samples (n1 = " + std::to_string(n1) + ")");
  if (!std::isfinite(nmperpixel) || nmperpixel == 0.0) return fail(GPA_ERR_ARG, w + "nmperpixel must be finite and not zero");
  if (!J && !props) return fail(GPA_ERR_ARG, w + "J and props are both null: nothing to compute");
  if (gpa::fieldjac::grid_blocks(gpa::fieldjac::make_geom(nimg, n0, n1, (int)esize(dtype))) == 0)
    return fail(GPA_ERR_ARG, w + "nimg x n0 x n1 is beyond one launch");
  return GPA_OK;
}

// dev: the pointers are the kernel's own (a device J is stored as whole matrices); the host forms copy
int field_check(const char* who, bool dev, int dtype, int nimg, int n0, int n1, const void* u, double nmperpixel, const void* J,
                const void* props) {
  const std::string w = std::string(who) + ": ";
  TRY(jac_common(w, dtype, nimg, n0, n1, nmperpixel, J, props));
  if (!u) return fail(GPA_ERR_ARG, w + "null u");
  const size_t npx = (size_t)nimg * n0 * n1 * esize(dtype);
  if (overlaps(J, 4 * npx, u, 2 * npx)) return fail(GPA_ERR_ARG, w + "J overlaps u");
  if (overlaps(props, 4 * npx, u, 2 * npx)) return fail(GPA_ERR_ARG, w + "props overlaps u");
  if (overlaps(props, 4 * npx, J, 4 * npx)) return fail(GPA_ERR_ARG, w + "props overlaps J");
  if (dev && (uintptr_t)J % (4 * esize(dtype)) != 0) return fail(GPA_ERR_ARG, w + "J must be aligned to one 2 x 2 matrix of the dtype");
  return GPA_OK;
}

int phases_check(const char* who, bool dev, int dtype, int n0, int n1, int P, const double* kvecs, const void* phases, const void* weights,
                 double nmperpixel, const void* J, const void* props) {
  const std::string w = std::string(who) + ": ";
  if (P < 2 || P > 8) return fail(GPA_ERR_ARG, w + "P must be 2 ... 8 (P = " + std::to_string(P) + ")");
  TRY(jac_common(w, dtype, 1, n0, n1, nmperpixel, J, props));
  if (!kvecs) return fail(GPA_ERR_ARG, w + "null kvecs");
  if (!phases) return fail(GPA_ERR_ARG, w + "null phases");
  if (!weights) return fail(GPA_ERR_ARG, w + "null weights");
  for (int i = 0; i < 2 * P; ++i)
    if (!std::isfinite(kvecs[i])) return fail(GPA_ERR_ARG, w + "kvecs must be finite");
  const size_t npx = (size_t)n0 * n1 * esize(dtype);
  if (overlaps(J, 4 * npx, phases, P * npx)) return fail(GPA_ERR_ARG, w + "J overlaps phases");
  if (overlaps(J, 4 * npx, weights, P * npx)) return fail(GPA_ERR_ARG, w + "J overlaps weights");
  if (overlaps(props, 4 * npx, phases, P * npx)) return fail(GPA_ERR_ARG, w + "props overlaps phases");
  if (overlaps(props, 4 * npx, weights, P * npx)) return fail(GPA_ERR_ARG, w + "props overlaps weights");
  if (overlaps(props, 4 * npx, J, 4 * npx)) return fail(GPA_ERR_ARG, w + "props overlaps J");
  if (dev && (uintptr_t)J % (4 * esize(dtype)) != 0) return fail(GPA_ERR_ARG, w + "J must be aligned to one 2 x 2 matrix of the dtype");
  return GPA_OK;
}

int phys_check(const char* who, int dtype, const void* jac, double poisson_ratio, const void* props, size_t npx) {
  const std::string w = std::string(who) + ": ";
  if (dtype != GPA_F32 && dtype != GPA_F64) return fail(GPA_ERR_ARG, w + "dtype must be GPA_F32 or GPA_F64 (dtype = " + std::to_string(dtype) + ")");
  if (!jac) return fail(GPA_ERR_ARG, w + "null jac");
  if (!props) return fail(GPA_ERR_ARG, w + "null props");
  if (!std::isfinite(poisson_ratio)) return fail(GPA_ERR_ARG, w + "poisson_ratio must be finite");
  if (npx > (size_t)0x7fffffff * 256) return fail(GPA_ERR_ARG, w + "npx is beyond one launch");
  if (overlaps(props, 4 * npx * esize(dtype), jac, 4 * npx * esize(dtype))) return fail(GPA_ERR_ARG, w + "props overlaps jac");
  return GPA_OK;
}

int need_device(const char* who, int device) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(GPA_ERR_NODEV, std::string(who) + ": no HIP device");
  HIP_TRY(hipSetDevice(device));
  return GPA_OK;
}

}  // namespace

int gpa_field_jacobian_dev(int device, int dtype, int nimg, int n0, int n1, const void* u, double nmperpixel, int add_identity,
                           void* J, void* props, double refangle, double refscale, int diff, void* stream) {
  TRY(field_check("gpa_field_jacobian_dev", true, dtype, nimg, n0, n1, u, nmperpixel, J, props));
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(launch_field_jacobian(dtype, nimg, n0, n1, u, nmperpixel, add_identity, J, props, refangle, refscale, diff,
                                (hipStream_t)stream));
  return GPA_OK;
}

int gpa_field_jacobian(int device, int dtype, int nimg, int n0, int n1, const void* u, double nmperpixel, int add_identity,
                       void* J, void* props, double refangle, double refscale, int diff) {
  TRY(field_check("gpa_field_jacobian", false, dtype, nimg, n0, n1, u, nmperpixel, J, props));
  TRY(need_device("gpa_field_jacobian", device));
  const size_t plane = (size_t)nimg * n0 * n1 * esize(dtype);
  DevBuf d_u, d_j, d_p;   // temporaries of this call
  HIP_TRY(d_u.reserve(2 * plane, nullptr));
  if (J) HIP_TRY(d_j.reserve(4 * plane, nullptr));
  if (props) HIP_TRY(d_p.reserve(4 * plane, nullptr));
  HIP_TRY(hipMemcpy(d_u.ptr, u, 2 * plane, hipMemcpyHostToDevice));
  HIP_TRY(launch_field_jacobian(dtype, nimg, n0, n1, d_u.ptr, nmperpixel, add_identity, J ? d_j.ptr : nullptr,
                                props ? d_p.ptr : nullptr, refangle, refscale, diff, nullptr));
  if (J) HIP_TRY(hipMemcpy(J, d_j.ptr, 4 * plane, hipMemcpyDeviceToHost));
  if (props) HIP_TRY(hipMemcpy(props, d_p.ptr, 4 * plane, hipMemcpyDeviceToHost));
  return GPA_OK;
}

int gpa_phases_jacobian_dev(int device, int dtype, int n0, int n1, int P, const double* kvecs, const void* phases,
                            const void* weights, double nmperpixel, int add_identity, void* J, void* props, double refangle,
                            double refscale, int diff, void* stream) {
  TRY(phases_check("gpa_phases_jacobian_dev", true, dtype, n0, n1, P, kvecs, phases, weights, nmperpixel, J, props));
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(launch_phases_jacobian(dtype, n0, n1, P, kvecs, phases, weights, nmperpixel, add_identity, J, props, refangle, refscale,
                                 diff, (hipStream_t)stream));
  return GPA_OK;
}

int gpa_phases_jacobian(int device, int dtype, int n0, int n1, int P, const double* kvecs, const void* phases, const void* weights,
                        double nmperpixel, int add_identity, void* J, void* props, double refangle, double refscale, int diff) {
  TRY(phases_check("gpa_phases_jacobian", false, dtype, n0, n1, P, kvecs, phases, weights, nmperpixel, J, props));
  TRY(need_device("gpa_phases_jacobian", device));
  const size_t plane = (size_t)n0 * n1 * esize(dtype);
  DevBuf d_ph, d_w, d_j, d_p;   // temporaries of this call
  HIP_TRY(d_ph.reserve(P * plane, nullptr));
  HIP_TRY(d_w.reserve(P * plane, nullptr));
  if (J) HIP_TRY(d_j.reserve(4 * plane, nullptr));
  if (props) HIP_TRY(d_p.reserve(4 * plane, nullptr));
  HIP_TRY(hipMemcpy(d_ph.ptr, phases, P * plane, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_w.ptr, weights, P * plane, hipMemcpyHostToDevice));
  HIP_TRY(launch_phases_jacobian(dtype, n0, n1, P, kvecs, d_ph.ptr, d_w.ptr, nmperpixel, add_identity, J ? d_j.ptr : nullptr,
                                 props ? d_p.ptr : nullptr, refangle, refscale, diff, nullptr));
  if (J) HIP_TRY(hipMemcpy(J, d_j.ptr, 4 * plane, hipMemcpyDeviceToHost));
  if (props) HIP_TRY(hipMemcpy(props, d_p.ptr, 4 * plane, hipMemcpyDeviceToHost));
  return GPA_OK;
}

int gpa_phys_props_from_jac_dev(int device, int dtype, size_t npx, const void* jac, int add_identity, double refangle,
                                double refscale, int diff, double poisson_ratio, void* props, void* stream) {
  TRY(phys_check("gpa_phys_props_from_jac_dev", dtype, jac, poisson_ratio, props, npx));
  if (npx == 0) return GPA_OK;
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(launch_phys_props(dtype, jac, npx, add_identity, refangle, refscale, diff, poisson_ratio, props, (hipStream_t)stream));
  return GPA_OK;
}

int gpa_phys_props_from_jac(int device, int dtype, size_t npx, const void* jac, int add_identity, double refangle, double refscale,
                            int diff, double poisson_ratio, void* props) {
  TRY(phys_check("gpa_phys_props_from_jac", dtype, jac, poisson_ratio, props, npx));
  if (npx == 0) return GPA_OK;
  TRY(need_device("gpa_phys_props_from_jac", device));
  const size_t bytes = 4 * npx * esize(dtype);
  DevBuf d_j, d_p;   // temporaries of this call
  HIP_TRY(d_j.reserve(bytes, nullptr));
  HIP_TRY(d_p.reserve(bytes, nullptr));
  HIP_TRY(hipMemcpy(d_j.ptr, jac, bytes, hipMemcpyHostToDevice));
  HIP_TRY(launch_phys_props(dtype, d_j.ptr, npx, add_identity, refangle, refscale, diff, poisson_ratio, d_p.ptr, nullptr));
  HIP_TRY(hipMemcpy(props, d_p.ptr, bytes, hipMemcpyDeviceToHost));
  return GPA_OK;
}
