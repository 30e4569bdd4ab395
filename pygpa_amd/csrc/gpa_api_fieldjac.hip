// C ABI: Jacobian and property maps from a displacement field, from phases or from phase gradients (pyGPA/property_extract.py:13-52,
// :69-101, :181-217, :258-278), kernels in gpa_fieldjac.hip, geometry in gpa_fieldjac.h.  Needs no plan: a host-pointer form stages in one DevBuf
// of its own (gpa_hoststage.h) that goes when the call returns.  Every argument is checked, and named in the error, before a
// device is touched.
#include "gpa_plan.h"
#include "gpa_fieldjac.h"

namespace {

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
  if (gpa::fieldjac::grid_blocks(gpa::fieldjac::make_geom(nimg, n0, n1, (int)dtype_size(dtype))) == 0)
    return fail(GPA_ERR_ARG, w + "nimg x n0 x n1 is beyond one launch");
  return GPA_OK;
}

// dev: the pointers are the kernel's own (a device J is stored as whole matrices); the host forms copy
int field_check(const char* who, bool dev, int dtype, int nimg, int n0, int n1, const void* u, double nmperpixel, const void* J,
                const void* props) {
  const std::string w = std::string(who) + ": ";
  TRY(jac_common(w, dtype, nimg, n0, n1, nmperpixel, J, props));
  if (!u) return fail(GPA_ERR_ARG, w + "null u");
  const size_t npx = (size_t)nimg * n0 * n1 * dtype_size(dtype);
  if (overlaps(J, 4 * npx, u, 2 * npx)) return fail(GPA_ERR_ARG, w + "J overlaps u");
  if (overlaps(props, 4 * npx, u, 2 * npx)) return fail(GPA_ERR_ARG, w + "props overlaps u");
  if (overlaps(props, 4 * npx, J, 4 * npx)) return fail(GPA_ERR_ARG, w + "props overlaps J");
  if (dev && (uintptr_t)J % (4 * dtype_size(dtype)) != 0) return fail(GPA_ERR_ARG, w + "J must be aligned to one 2 x 2 matrix of the dtype");
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
  const size_t npx = (size_t)n0 * n1 * dtype_size(dtype);
  if (overlaps(J, 4 * npx, phases, P * npx)) return fail(GPA_ERR_ARG, w + "J overlaps phases");
  if (overlaps(J, 4 * npx, weights, P * npx)) return fail(GPA_ERR_ARG, w + "J overlaps weights");
  if (overlaps(props, 4 * npx, phases, P * npx)) return fail(GPA_ERR_ARG, w + "props overlaps phases");
  if (overlaps(props, 4 * npx, weights, P * npx)) return fail(GPA_ERR_ARG, w + "props overlaps weights");
  if (overlaps(props, 4 * npx, J, 4 * npx)) return fail(GPA_ERR_ARG, w + "props overlaps J");
  if (dev && (uintptr_t)J % (4 * dtype_size(dtype)) != 0) return fail(GPA_ERR_ARG, w + "J must be aligned to one 2 x 2 matrix of the dtype");
  return GPA_OK;
}

// the pointwise member: any frame of at least one pixel
int grads_check(const char* who, bool dev, int dtype, int nimg, int n0, int n1, int P, const double* kvecs, const double* dks,
                const void* grads, const void* weights, double nmperpixel, const void* J, const void* props) {
  const std::string w = std::string(who) + ": ";
  if (dtype != GPA_F32 && dtype != GPA_F64) return fail(GPA_ERR_ARG, w + "dtype must be GPA_F32 or GPA_F64 (dtype = " + std::to_string(dtype) + ")");
  if (nimg < 1) return fail(GPA_ERR_ARG, w + "nimg must be >= 1 (nimg = " + std::to_string(nimg) + ")");
  if (n0 < 1) return fail(GPA_ERR_ARG, w + "n0 must be >= 1 (n0 = " + std::to_string(n0) + ")");
  if (n1 < 1) return fail(GPA_ERR_ARG, w + "n1 must be >= 1 (n1 = " + std::to_string(n1) + ")");
  if (P < 2 || P > 8) return fail(GPA_ERR_ARG, w + "P must be 2 ... 8 (P = " + std::to_string(P) + ")");
  if (!std::isfinite(nmperpixel) || nmperpixel == 0.0) return fail(GPA_ERR_ARG, w + "nmperpixel must be finite and not zero");
  if (!J && !props) return fail(GPA_ERR_ARG, w + "J and props are both null: nothing to compute");
  if (!gpa::fieldjac::gradients_fits(n0, n1) ||
      gpa::fieldjac::grid_blocks(gpa::fieldjac::gradients_geom(nimg, n0, n1, (int)dtype_size(dtype))) == 0)
    return fail(GPA_ERR_ARG, w + "nimg x n0 x n1 is beyond one launch");
  if (!kvecs) return fail(GPA_ERR_ARG, w + "null kvecs");
  if (!grads) return fail(GPA_ERR_ARG, w + "null grads");
  if (!weights) return fail(GPA_ERR_ARG, w + "null weights");
  for (int i = 0; i < 2 * P; ++i) {
    if (!std::isfinite(kvecs[i])) return fail(GPA_ERR_ARG, w + "kvecs must be finite");
    if (dks && !std::isfinite(dks[i])) return fail(GPA_ERR_ARG, w + "dks must be finite");
  }
  const size_t npx = (size_t)nimg * n0 * n1 * dtype_size(dtype);
  if (overlaps(J, 4 * npx, grads, 2 * P * npx)) return fail(GPA_ERR_ARG, w + "J overlaps grads");
  if (overlaps(J, 4 * npx, weights, P * npx)) return fail(GPA_ERR_ARG, w + "J overlaps weights");
  if (overlaps(props, 4 * npx, grads, 2 * P * npx)) return fail(GPA_ERR_ARG, w + "props overlaps grads");
  if (overlaps(props, 4 * npx, weights, P * npx)) return fail(GPA_ERR_ARG, w + "props overlaps weights");
  if (overlaps(props, 4 * npx, J, 4 * npx)) return fail(GPA_ERR_ARG, w + "props overlaps J");
  if (dev && (uintptr_t)J % (4 * dtype_size(dtype)) != 0) return fail(GPA_ERR_ARG, w + "J must be aligned to one 2 x 2 matrix of the dtype");
  if (dev && (uintptr_t)grads % (2 * dtype_size(dtype)) != 0) return fail(GPA_ERR_ARG, w + "grads must be aligned to one pair of the dtype");
  return GPA_OK;
}

int phys_check(const char* who, int dtype, const void* jac, double poisson_ratio, const void* props, size_t npx) {
  const std::string w = std::string(who) + ": ";
  if (dtype != GPA_F32 && dtype != GPA_F64) return fail(GPA_ERR_ARG, w + "dtype must be GPA_F32 or GPA_F64 (dtype = " + std::to_string(dtype) + ")");
  if (!jac) return fail(GPA_ERR_ARG, w + "null jac");
  if (!props) return fail(GPA_ERR_ARG, w + "null props");
  if (!std::isfinite(poisson_ratio)) return fail(GPA_ERR_ARG, w + "poisson_ratio must be finite");
  if (npx > (size_t)0x7fffffff * 256) return fail(GPA_ERR_ARG, w + "npx is beyond one launch");
  if (overlaps(props, 4 * npx * dtype_size(dtype), jac, 4 * npx * dtype_size(dtype))) return fail(GPA_ERR_ARG, w + "props overlaps jac");
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
  const size_t plane = (size_t)nimg * n0 * n1 * dtype_size(dtype);
  DevBuf tmp;   // a temporary of this call
  HostStage st(tmp, nullptr);
  const int i_u = st.in(u, 2 * plane), i_j = st.out(J, 4 * plane), i_p = st.out(props, 4 * plane);
  HIP_TRY(st.upload());
  HIP_TRY(launch_field_jacobian(dtype, nimg, n0, n1, st.dev(i_u), nmperpixel, add_identity, st.dev(i_j), st.dev(i_p), refangle,
                                refscale, diff, nullptr));
  HIP_TRY(st.download());
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
  const size_t plane = (size_t)n0 * n1 * dtype_size(dtype);
  DevBuf tmp;   // a temporary of this call
  HostStage st(tmp, nullptr);
  const int i_ph = st.in(phases, P * plane), i_w = st.in(weights, P * plane), i_j = st.out(J, 4 * plane), i_p = st.out(props, 4 * plane);
  HIP_TRY(st.upload());
  HIP_TRY(launch_phases_jacobian(dtype, n0, n1, P, kvecs, st.dev(i_ph), st.dev(i_w), nmperpixel, add_identity, st.dev(i_j), st.dev(i_p),
                                 refangle, refscale, diff, nullptr));
  HIP_TRY(st.download());
  return GPA_OK;
}

int gpa_gradients_jacobian_dev(int device, int dtype, int nimg, int n0, int n1, int P, const double* kvecs, const double* dks,
                               const void* grads, const void* weights, double nmperpixel, int add_identity, void* J, void* props,
                               double refangle, double refscale, int diff, void* stream) {
  TRY(grads_check("gpa_gradients_jacobian_dev", true, dtype, nimg, n0, n1, P, kvecs, dks, grads, weights, nmperpixel, J, props));
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(launch_gradients_jacobian(dtype, nimg, n0, n1, P, kvecs, dks, grads, weights, nmperpixel, add_identity, J, props, refangle,
                                    refscale, diff, (hipStream_t)stream));
  return GPA_OK;
}

int gpa_gradients_jacobian(int device, int dtype, int nimg, int n0, int n1, int P, const double* kvecs, const double* dks,
                           const void* grads, const void* weights, double nmperpixel, int add_identity, void* J, void* props,
                           double refangle, double refscale, int diff) {
  TRY(grads_check("gpa_gradients_jacobian", false, dtype, nimg, n0, n1, P, kvecs, dks, grads, weights, nmperpixel, J, props));
  TRY(need_device("gpa_gradients_jacobian", device));
  const size_t plane = (size_t)nimg * n0 * n1 * dtype_size(dtype);
  DevBuf tmp;   // a temporary of this call
  HostStage st(tmp, nullptr);
  const int i_g = st.in(grads, 2 * P * plane), i_w = st.in(weights, P * plane), i_j = st.out(J, 4 * plane), i_p = st.out(props, 4 * plane);
  HIP_TRY(st.upload());
  HIP_TRY(launch_gradients_jacobian(dtype, nimg, n0, n1, P, kvecs, dks, st.dev(i_g), st.dev(i_w), nmperpixel, add_identity, st.dev(i_j),
                                    st.dev(i_p), refangle, refscale, diff, nullptr));
  HIP_TRY(st.download());
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
  const size_t bytes = 4 * npx * dtype_size(dtype);
  DevBuf tmp;   // a temporary of this call
  HostStage st(tmp, nullptr);
  const int i_jac = st.in(jac, bytes), i_props = st.out(props, bytes);
  HIP_TRY(st.upload());
  HIP_TRY(launch_phys_props(dtype, st.dev(i_jac), npx, add_identity, refangle, refscale, diff, poisson_ratio, st.dev(i_props), nullptr));
  HIP_TRY(st.download());
  return GPA_OK;
}
