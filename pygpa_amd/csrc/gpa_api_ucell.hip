// C ABI: unit-cell averaging and expansion (unit_cell_averaging.py:132-251), kernels in gpa_ucell.hip.
//
// The _dev entry points take device pointers and enqueue on the plan's stream without a host synchronisation (the
// scratch grows with one, the first time a shape or cell needs more); the host-pointer ones are these plus the copies: the
// plan-shaped operands in the plan's own d_image / d_u / d_wnorm, the cell-shaped ones in gpa_plan::host_stage.
#include "gpa_plan.h"

static int check_geom(const gpa_plan* p, const gpa_ucell_geom* gg, const char* who, UcellGeom* g) {
  if (!gg) return fail(GPA_ERR_ARG, std::string(who) + ": null geometry");
  const long long rs0 = gg->rsize[0], rs1 = gg->rsize[1];
  if (rs0 < 1 || rs1 < 1 || !(gg->z > 0.0))
    return fail(GPA_ERR_ARG, std::string(who) + ": need rsize >= 1 per axis and z > 0");
  if (rs0 * rs1 > UCELL_MAX_BINS)
    return fail(GPA_ERR_STATE, std::string(who) + ": a cell of " + std::to_string(rs0) + " x " + std::to_string(rs1) +
                                   " bins is beyond this build's limit of 2^24 (16777216) bins");
  if ((size_t)p->n0 * p->n1 >= ((size_t)1 << 31))
    return fail(GPA_ERR_STATE, std::string(who) + ": images of 2^31 pixels or more are beyond the int32 pixel lists");
  for (int k = 0; k < 4; ++k) {
    g->ks[k] = gg->ks[k];
    g->kinv[k] = gg->kinv[k];
  }
  g->rmin[0] = gg->rmin[0];
  g->rmin[1] = gg->rmin[1];
  g->z = gg->z;
  g->rs0 = (int)rs0;
  g->rs1 = (int)rs1;
  return GPA_OK;
}

int gpa_unit_cell_average_batch_dev(gpa_plan* p, const void* images_dev, int B, const void* u_dev, const gpa_ucell_geom* geom,
                                    double* res_dev, double* weights_dev) {
  if (!p || !images_dev || !res_dev) return fail(GPA_ERR_ARG, "gpa_unit_cell_average: null argument");
  if (B < 1 || B > UCELL_MAX_FRAMES)
    return fail(GPA_ERR_ARG, "gpa_unit_cell_average_batch_dev: need 1 <= B <= " + std::to_string(UCELL_MAX_FRAMES) +
                                 " frames per call (B = " + std::to_string(B) + "; split the stack)");
  UcellGeom g;
  TRY(check_geom(p, geom, "gpa_unit_cell_average", &g));
  HIP_TRY(hipSetDevice(p->device));
  ProfInstall prof(p);
  const hipError_t e = ucell_average(p->dtype, images_dev, B, u_dev, p->n0, p->n1, g, res_dev, weights_dev, p->stream, &p->ucell);
  if (e != hipSuccess) return fail(GPA_ERR_HIP, std::string("gpa_unit_cell_average: ") + hipGetErrorString(e));
  return prof_finish(p);
}

int gpa_unit_cell_average_dev(gpa_plan* p, const void* image_dev, const void* u_dev, const gpa_ucell_geom* geom, double* res_dev,
                              double* weights_dev) {
  return gpa_unit_cell_average_batch_dev(p, image_dev, 1, u_dev, geom, res_dev, weights_dev);
}

int gpa_unit_cell_average(gpa_plan* p, const void* image, const void* u, const gpa_ucell_geom* geom, double* res, double* weights) {
  if (!p || !image || !res) return fail(GPA_ERR_ARG, "gpa_unit_cell_average: null argument");
  UcellGeom g;
  TRY(check_geom(p, geom, "gpa_unit_cell_average", &g));
  HIP_TRY(hipSetDevice(p->device));
  const size_t plane = (size_t)p->n0 * p->n1 * p->rsz, cell = (size_t)g.rs0 * g.rs1 * sizeof(double);
  HostStage st(p->host_stage, p->stream, sizeof(double));   // res | weights back to back, as the plan has always counted them
  const int i_img = st.in(image, plane, p->d_image), i_u = st.in(u, 2 * plane, p->d_u);
  const int i_res = st.out(res, cell), i_w = st.out(weights, cell);
  HIP_TRY(st.upload());
  TRY(gpa_unit_cell_average_dev(p, st.dev(i_img), st.dev(i_u), geom, st.as<double>(i_res), st.as<double>(i_w)));
  HIP_TRY(st.download());
  return GPA_OK;
}

int gpa_expand_unitcell_dev(gpa_plan* p, const double* cell_dev, const gpa_ucell_geom* geom, double z2, const void* u_dev,
                            void* out_dev) {
  if (!p || !cell_dev || !out_dev) return fail(GPA_ERR_ARG, "gpa_expand_unitcell: null argument");
  if (!(z2 > 0.0)) return fail(GPA_ERR_ARG, "gpa_expand_unitcell: need z2 > 0");
  UcellGeom g;
  TRY(check_geom(p, geom, "gpa_expand_unitcell", &g));
  HIP_TRY(hipSetDevice(p->device));
  ProfInstall prof(p);
  const hipError_t e = ucell_expand(p->dtype, cell_dev, g, z2, u_dev, p->n0, p->n1, out_dev, p->stream, &p->ucell);
  if (e != hipSuccess) return fail(GPA_ERR_HIP, std::string("gpa_expand_unitcell: ") + hipGetErrorString(e));
  return prof_finish(p);
}

int gpa_expand_unitcell(gpa_plan* p, const double* cell, const gpa_ucell_geom* geom, double z2, const void* u, void* out) {
  if (!p || !cell || !out) return fail(GPA_ERR_ARG, "gpa_expand_unitcell: null argument");
  UcellGeom g;
  TRY(check_geom(p, geom, "gpa_expand_unitcell", &g));
  HIP_TRY(hipSetDevice(p->device));
  const size_t plane = (size_t)p->n0 * p->n1 * p->rsz;
  HostStage st(p->host_stage, p->stream);
  const int i_cell = st.in(cell, (size_t)g.rs0 * g.rs1 * sizeof(double)), i_u = st.in(u, 2 * plane, p->d_u);
  const int i_out = st.out(out, plane, p->d_wnorm);   // (n0 x n1 reals of the plan)
  HIP_TRY(st.upload());
  TRY(gpa_expand_unitcell_dev(p, st.as<double>(i_cell), geom, z2, st.dev(i_u), st.dev(i_out)));
  HIP_TRY(st.download());
  return GPA_OK;
}
