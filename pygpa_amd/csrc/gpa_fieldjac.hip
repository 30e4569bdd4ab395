// Displacement field or phases -> Jacobian J = grad(-u) and lattice properties in one pass: u2J, phases2J and
// calc_props_from_phases of pyGPA/property_extract.py:13-52, :258-278, and phys_props_from_Jac (:181-217).
//
// Streams.  Geometry, difference rule and index arithmetic are gpa_fieldjac.h (walked on the host by
// tests/host/fieldjac_check.cpp): one wave per tile of FJ_ROWS rows x 64 lanes x 16 bytes of columns, rows i-1, i, i+1 of every
// input plane rolling through registers, column neighbours from the lane's own vector and one cross-lane move per side.
// A lane loads 16 bytes per row and plane, stores each pixel's J as one Quad and its properties as 16 bytes per plane.
// Rows whose length is not a multiple of the vector (or unaligned bases) take the same path with element-wise accesses.
// The properties come from lattice_props of gpa_jacmath.h on the J that is stored (before add_identity), the function and the
// bits of props_kernel.
// The third source, phase gradients and weights of a stack (phasegradient2J, :69-101, calc_props_from_phasegradient, :234-255),
// has no stencil: gradients_jacobian_kernel is pointwise on the same geometry with a frame as one row of pixels.
#include "gpa_internal.h"
#include "gpa_fieldjac.h"
#include "gpa_jacmath.h"

namespace gpa {

namespace {

using namespace fieldjac;

template <class T> struct alignas(FJ_VEC_BYTES) Vec { T v[FJ_VEC_BYTES / sizeof(T)]; };

// the lane's columns [c, c + V) of row r of a plane; zeros beyond the frame
template <class T, bool WIDE>
__device__ __forceinline__ Vec<T> load_vec(const T* __restrict__ plane, const Geom& g, int r, int c) {
  constexpr int V = FJ_VEC_BYTES / sizeof(T);
  Vec<T> x;
  const T* p = plane + pixel_offset(g, r, c);
  if (WIDE) {   // n1 is a multiple of V here, so c < n1 puts the whole vector inside the row
    if (c < g.n1) x = *reinterpret_cast<const Vec<T>*>(p);
    else
      _Pragma("unroll") for (int k = 0; k < V; ++k) x.v[k] = T(0);
  } else {
    _Pragma("unroll") for (int k = 0; k < V; ++k) x.v[k] = c + k < g.n1 ? p[k] : T(0);
  }
  return x;
}

// the columns c - 1 and c + V of the row: from the neighbouring lanes, and for the wave's outer lanes from memory.  Outside the
// frame the value is unused (the difference rule takes the sample itself there).  Every lane of the wave must call this.
template <class T>
__device__ __forceinline__ void row_halo(const T* __restrict__ plane, const Geom& g, int r, int c, int lane, const Vec<T>& cur,
                                         T& left, T& right) {
  constexpr int V = FJ_VEC_BYTES / sizeof(T);
  left = __shfl_up(cur.v[V - 1], 1);
  right = __shfl_down(cur.v[0], 1);
  if (lane == 0) left = c > 0 && c - 1 < g.n1 ? plane[pixel_offset(g, r, c - 1)] : T(0);
  if (lane == FJ_LANES - 1) right = c + V < g.n1 ? plane[pixel_offset(g, r, c + V)] : T(0);
}

// the V values of one property plane of the lane's pixels
template <class T, bool WIDE>
__device__ __forceinline__ void store_props(T* __restrict__ props, const Geom& g, const Tile& t, int r, int c,
                                            const Vec<T> (&pv)[4]) {
  constexpr int V = FJ_VEC_BYTES / sizeof(T);
  _Pragma("unroll") for (int q = 0; q < 4; ++q) {
    T* dst = props + plane_offset(g, t.img, 4, q) + pixel_offset(g, r, c);
    if (WIDE) {
      if (c < g.n1) *reinterpret_cast<Vec<T>*>(dst) = pv[q];
    } else {
      _Pragma("unroll") for (int k = 0; k < V; ++k)
        if (c + k < g.n1) dst[k] = pv[q].v[k];
    }
  }
}

struct PropArgs { double refangle, refscale; int diff; };

// J (and its properties) of the V pixels of a lane in row r, from q[k] = the raw J of pixel k
template <class T, bool WIDE>
__device__ __forceinline__ void emit(const Geom& g, const Tile& t, int r, int c, Quad<T> (&q)[FJ_VEC_BYTES / sizeof(T)],
                                     T ident, Quad<T>* __restrict__ J, T* __restrict__ props, const PropArgs& pa) {
  constexpr int V = FJ_VEC_BYTES / sizeof(T);
  if (props)
    _Pragma("unroll") for (int k = 0; k < V; ++k) q[k] = Quad<T>{rounded(q[k].a), rounded(q[k].b), rounded(q[k].c), rounded(q[k].d)};
  if (J) {
    Quad<T>* dst = J + plane_offset(g, t.img, 1, 0) + pixel_offset(g, r, c);
    _Pragma("unroll") for (int k = 0; k < V; ++k)
      if (c + k < g.n1) dst[k] = Quad<T>{q[k].a + ident, q[k].b, q[k].c, q[k].d + ident};
  }
  if (props) {
    Vec<T> pv[4];
    _Pragma("unroll") for (int k = 0; k < V; ++k) {
      T p[4];
      lattice_props(q[k], T(1), (T)pa.refangle, (T)pa.refscale, pa.diff, p);
      _Pragma("unroll") for (int i = 0; i < 4; ++i) pv[i].v[k] = p[i];
    }
    store_props<T, WIDE>(props, g, t, r, c, pv);
  }
}

// u: nimg x 2 x n0 x n1 -> J: nimg x n0 x n1 x 2 x 2 with J[n, m, c, a] = np.gradient(-u_c, h, axis=a), props: nimg x 4 x n0 x n1
template <class T, bool WIDE>
__global__ __launch_bounds__(FJ_LANES * FJ_WAVES) void field_jacobian_kernel(const T* __restrict__ u, Geom g, T h1, T h2, T ident, Quad<T>* __restrict__ J,
                                                                             T* __restrict__ props, PropArgs pa) {
  constexpr int V = FJ_VEC_BYTES / sizeof(T);
  const int lane = threadIdx.x % FJ_LANES;
  const uint64_t tix = (uint64_t)blockIdx.x * FJ_WAVES + threadIdx.x / FJ_LANES;
  if (tix >= g.tiles) return;   // the whole wave
  const Tile t = tile_of(g, tix);
  const int c = lane_col(g, t, lane);
  const T* pl[2] = {u + plane_offset(g, t.img, 2, 0), u + plane_offset(g, t.img, 2, 1)};
  Vec<T> up[2], cur[2], dn[2];
  _Pragma("unroll") for (int i = 0; i < 2; ++i) {
    cur[i] = load_vec<T, WIDE>(pl[i], g, t.r0, c);
    up[i] = t.r0 > 0 ? load_vec<T, WIDE>(pl[i], g, t.r0 - 1, c) : cur[i];
  }
  for (int r = t.r0; r < t.r1; ++r) {
    const bool redge = is_edge(r, g.n0);
    Quad<T> q[V];
    T d[2][2][V];   // [component][axis][pixel]
    _Pragma("unroll") for (int i = 0; i < 2; ++i) {
      dn[i] = r + 1 < g.n0 ? load_vec<T, WIDE>(pl[i], g, r + 1, c) : cur[i];
      T left, right;
      row_halo(pl[i], g, r, c, lane, cur[i], left, right);
      _Pragma("unroll") for (int k = 0; k < V; ++k) {
        const int col = c + k;
        const T lo = col > 0 ? (k > 0 ? cur[i].v[k - 1] : left) : cur[i].v[k];
        const T hi = col < g.n1 - 1 ? (k < V - 1 ? cur[i].v[k + 1] : right) : cur[i].v[k];
        d[i][0][k] = field_diff(up[i].v[k], dn[i].v[k], redge, h1, h2);
        d[i][1][k] = field_diff(lo, hi, is_edge(col, g.n1), h1, h2);
      }
      up[i] = cur[i];
      cur[i] = dn[i];
    }
    _Pragma("unroll") for (int k = 0; k < V; ++k) q[k] = Quad<T>{d[0][0][k], d[0][1][k], d[1][0][k], d[1][1][k]};
    emit<T, WIDE>(g, t, r, c, q, ident, J, props, pa);
  }
}

struct KMat { double k[16]; };   // 2 pi kvecs, P x 2

// phases, weights: P x n0 x n1 -> J = -(weighted least squares of wrap(2 grad phases) / 2 / nmperpixel against kmat)
template <class T, int P, bool WIDE>
__global__ __launch_bounds__(FJ_LANES * FJ_WAVES) void phases_jacobian_kernel(const T* __restrict__ ph, const T* __restrict__ w,
                                                                              KMat km, Geom g, T nm, T ident,
                                                                              Quad<T>* __restrict__ J, T* __restrict__ props,
                                                                              PropArgs pa) {
  constexpr int V = FJ_VEC_BYTES / sizeof(T);
  const int lane = threadIdx.x % FJ_LANES;
  const uint64_t tix = (uint64_t)blockIdx.x * FJ_WAVES + threadIdx.x / FJ_LANES;
  if (tix >= g.tiles) return;   // the whole wave
  const Tile t = tile_of(g, tix);
  const int c = lane_col(g, t, lane);
  const size_t npx = (size_t)g.n0 * (size_t)g.n1;
  Vec<T> up[P], cur[P], dn[P];
  _Pragma("unroll") for (int p = 0; p < P; ++p) {
    cur[p] = load_vec<T, WIDE>(ph + p * npx, g, t.r0, c);
    up[p] = t.r0 > 0 ? load_vec<T, WIDE>(ph + p * npx, g, t.r0 - 1, c) : cur[p];
  }
  for (int r = t.r0; r < t.r1; ++r) {
    const bool redge = is_edge(r, g.n0);
    Vec<T> wv[P];
    T wmax[V];
    _Pragma("unroll") for (int k = 0; k < V; ++k) wmax[k] = T(0);
    _Pragma("unroll") for (int p = 0; p < P; ++p) {
      wv[p] = load_vec<T, WIDE>(w + p * npx, g, r, c);
      _Pragma("unroll") for (int k = 0; k < V; ++k) { const T a = wv[p].v[k] < T(0) ? -wv[p].v[k] : wv[p].v[k]; wmax[k] = a > wmax[k] ? a : wmax[k]; }
    }
    T ws[V], a00[V], a01[V], a11[V], rx0[V], rx1[V], ry0[V], ry1[V];
    _Pragma("unroll") for (int k = 0; k < V; ++k) ws[k] = wmax[k] > T(0) ? T(1) / wmax[k] : T(0);
    _Pragma("unroll") for (int k = 0; k < V; ++k) a00[k] = a01[k] = a11[k] = rx0[k] = rx1[k] = ry0[k] = ry1[k] = T(0);
    _Pragma("unroll") for (int p = 0; p < P; ++p) {
      dn[p] = r + 1 < g.n0 ? load_vec<T, WIDE>(ph + p * npx, g, r + 1, c) : cur[p];
      T left, right;
      row_halo(ph + p * npx, g, r, c, lane, cur[p], left, right);
      const T k0 = (T)km.k[2 * p], k1 = (T)km.k[2 * p + 1];
      _Pragma("unroll") for (int k = 0; k < V; ++k) {
        const int col = c + k;
        const T lo = col > 0 ? (k > 0 ? cur[p].v[k - 1] : left) : cur[p].v[k];
        const T hi = col < g.n1 - 1 ? (k < V - 1 ? cur[p].v[k + 1] : right) : cur[p].v[k];
        const T bx = wrap_to_pi_fast(phase_diff(up[p].v[k], dn[p].v[k], redge));              // along axis 0
        const T by = wrap_to_pi_fast(phase_diff(lo, hi, is_edge(col, g.n1)));                // along axis 1
        const T wn = wv[p].v[k] * ws[k], ww = wn * wn;
        a00[k] += ww * k0 * k0; a01[k] += ww * k0 * k1; a11[k] += ww * k1 * k1;
        rx0[k] += ww * k0 * bx; rx1[k] += ww * k1 * bx;
        ry0[k] += ww * k0 * by; ry1[k] += ww * k1 * by;
      }
      up[p] = cur[p];
      cur[p] = dn[p];
    }
    Quad<T> q[V];
    _Pragma("unroll") for (int k = 0; k < V; ++k) {
      T ux0, ux1, uy0, uy1;
      solve2(a00[k], a01[k], a11[k], rx0[k], rx1[k], ux0, ux1);   // d u_i / d axis 0
      solve2(a00[k], a01[k], a11[k], ry0[k], ry1[k], uy0, uy1);   // d u_i / d axis 1
      q[k] = Quad<T>{-(T(0.5) * ux0) / nm, -(T(0.5) * uy0) / nm, -(T(0.5) * ux1) / nm, -(T(0.5) * uy1) / nm};
    }
    emit<T, WIDE>(g, t, r, c, q, ident, J, props, pa);
  }
}

// 2 pi (kvecs + dks), P x 2, and with on != 0 the turn 2 pi dks the gradients are taken against (iso_ref of phasegradient2J)
struct GradK { double k[16], shift[16]; int on; };

// the V interleaved (d/d axis 0, d/d axis 1) pairs of the lane's pixels [c, c + V) of one peak: 2 V reals, two vectors
template <class T, bool WIDE>
__device__ __forceinline__ void load_pairs(const T* __restrict__ pairs, const Geom& g, int c, Vec<T> (&x)[2]) {
  constexpr int V = FJ_VEC_BYTES / sizeof(T);
  const T* p = pairs + 2 * pixel_offset(g, 0, c);
  if (WIDE) {   // the pixel count is a multiple of V here, so c < n1 puts both vectors inside the frame
    if (c < g.n1) {
      x[0] = reinterpret_cast<const Vec<T>*>(p)[0];
      x[1] = reinterpret_cast<const Vec<T>*>(p)[1];
      return;
    }
    _Pragma("unroll") for (int k = 0; k < 2 * V; ++k) x[k / V].v[k % V] = T(0);
  } else {
    _Pragma("unroll") for (int k = 0; k < 2 * V; ++k) x[k / V].v[k % V] = c + k / 2 < g.n1 ? p[k] : T(0);
  }
}

// grads: nimg x P x npx x 2, w: nimg x P x npx -> J[i, j] = (weighted least squares of grads[:, j] against gk.k)_i / nmperpixel:
// phasegradient2J (property_extract.py:69-101), the arithmetic of jacobian_kernel (gpa_reconstruct.hip) operation for operation.
// Pointwise: the geometry g is that of nimg frames of ONE row of npx pixels, a wave takes 64 x V consecutive pixels of a frame.
template <class T, int P, bool WIDE>
__global__ __launch_bounds__(FJ_LANES * FJ_WAVES) void gradients_jacobian_kernel(const T* __restrict__ grads, const T* __restrict__ w,
                                                                                 GradK gk, Geom g, T inv_nm, T ident,
                                                                                 Quad<T>* __restrict__ J, T* __restrict__ props,
                                                                                 PropArgs pa) {
  constexpr int V = FJ_VEC_BYTES / sizeof(T);
  const int lane = threadIdx.x % FJ_LANES;
  const uint64_t tix = (uint64_t)blockIdx.x * FJ_WAVES + threadIdx.x / FJ_LANES;
  if (tix >= g.tiles) return;   // the whole wave
  const Tile t = tile_of(g, tix);
  const int c = lane_col(g, t, lane);
  if (c >= g.n1) return;   // no cross-lane traffic here: a lane beyond the frame has nothing to do
  const size_t npx = (size_t)g.n1;
  const T* wf = w + plane_offset(g, t.img, P, 0);
  const T* gf = grads + 2 * plane_offset(g, t.img, P, 0);
  Vec<T> wv[P], gv[P][2];
  _Pragma("unroll") for (int p = 0; p < P; ++p) {
    wv[p] = load_vec<T, WIDE>(wf + p * npx, g, 0, c);
    load_pairs<T, WIDE>(gf + 2 * p * npx, g, c, gv[p]);
  }
  Quad<T> q[V];
  _Pragma("unroll") for (int k = 0; k < V; ++k) {
    T wmax = T(0);
    _Pragma("unroll") for (int p = 0; p < P; ++p) { const T a = wv[p].v[k] < T(0) ? -wv[p].v[k] : wv[p].v[k]; wmax = a > wmax ? a : wmax; }
    const T ws = wmax > T(0) ? T(1) / wmax : T(0);
    T a00 = 0, a01 = 0, a11 = 0, rx0 = 0, rx1 = 0, ry0 = 0, ry1 = 0;
    _Pragma("unroll") for (int p = 0; p < P; ++p) {
      const T k0 = (T)gk.k[2 * p], k1 = (T)gk.k[2 * p + 1], wn = wv[p].v[k] * ws, ww = wn * wn;
      T gx = gv[p][(2 * k) / V].v[(2 * k) % V], gy = gv[p][(2 * k + 1) / V].v[(2 * k + 1) % V];
      if (gk.on) {
        gx = wrap_to_pi(gx - (T)gk.shift[2 * p]);
        gy = wrap_to_pi(gy - (T)gk.shift[2 * p + 1]);
      }
      a00 += ww * k0 * k0; a01 += ww * k0 * k1; a11 += ww * k1 * k1;
      rx0 += ww * k0 * gx; rx1 += ww * k1 * gx;
      ry0 += ww * k0 * gy; ry1 += ww * k1 * gy;
    }
    T ux0, ux1, uy0, uy1;
    solve2(a00, a01, a11, rx0, rx1, ux0, ux1);   // d u_i / d axis 0
    solve2(a00, a01, a11, ry0, ry1, uy0, uy1);   // d u_i / d axis 1
    // (rounded: what is stored with add_identity is the J of phasegradient2J plus 1, not a product fused into that sum)
    q[k] = Quad<T>{rounded(ux0 * inv_nm), rounded(uy0 * inv_nm), rounded(ux1 * inv_nm), rounded(uy1 * inv_nm)};
  }
  emit<T, WIDE>(g, t, 0, c, q, ident, J, props, pa);
}

template <class T>
__global__ __launch_bounds__(256) void phys_props_kernel(const Quad<T>* __restrict__ jac, size_t npx, T ident, T refangle,
                                                        T refscale, int diff, T delta, T* __restrict__ out) {
  const size_t o = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (o >= npx) return;
  T p[4];
  lattice_phys_props(jac[o], ident, refangle, refscale, diff, delta, p);
  out[o] = p[0];
  out[npx + o] = p[1];
  out[2 * npx + o] = p[2];
  out[3 * npx + o] = p[3];
}

// 16-byte accesses need rows that start on 16 bytes: the row length a multiple of the vector and the bases aligned
bool wide_ok(const Geom& g, const void* a, const void* b, const void* props) {
  const uintptr_t bits = (uintptr_t)a | (uintptr_t)b | (uintptr_t)props;
  return g.n1 % g.vec == 0 && bits % FJ_VEC_BYTES == 0;
}

template <class T, int P>
void launch_phases_p(unsigned grid, const void* ph, const void* w, const KMat& km, const Geom& g, double nm, bool wide,
                     int add_identity, void* J, void* props, const PropArgs& pa, hipStream_t s) {
  const T ident = add_identity ? T(1) : T(0);
  if (wide)
    phases_jacobian_kernel<T, P, true><<<grid, FJ_LANES * FJ_WAVES, 0, s>>>((const T*)ph, (const T*)w, km, g, (T)nm, ident,
                                                                             (Quad<T>*)J, (T*)props, pa);
  else
    phases_jacobian_kernel<T, P, false><<<grid, FJ_LANES * FJ_WAVES, 0, s>>>((const T*)ph, (const T*)w, km, g, (T)nm, ident,
                                                                              (Quad<T>*)J, (T*)props, pa);
}

template <class T>
hipError_t launch_phases_t(int P, unsigned grid, const void* ph, const void* w, const KMat& km, const Geom& g, double nm, bool wide,
                           int add_identity, void* J, void* props, const PropArgs& pa, hipStream_t s) {
  switch (P) {
    case 2: launch_phases_p<T, 2>(grid, ph, w, km, g, nm, wide, add_identity, J, props, pa, s); break;
    case 3: launch_phases_p<T, 3>(grid, ph, w, km, g, nm, wide, add_identity, J, props, pa, s); break;
    case 4: launch_phases_p<T, 4>(grid, ph, w, km, g, nm, wide, add_identity, J, props, pa, s); break;
    case 5: launch_phases_p<T, 5>(grid, ph, w, km, g, nm, wide, add_identity, J, props, pa, s); break;
    case 6: launch_phases_p<T, 6>(grid, ph, w, km, g, nm, wide, add_identity, J, props, pa, s); break;
    case 7: launch_phases_p<T, 7>(grid, ph, w, km, g, nm, wide, add_identity, J, props, pa, s); break;
    case 8: launch_phases_p<T, 8>(grid, ph, w, km, g, nm, wide, add_identity, J, props, pa, s); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

template <class T, int P>
void launch_grads_p(unsigned grid, const void* gr, const void* w, const GradK& gk, const Geom& g, double nm, bool wide,
                    int add_identity, void* J, void* props, const PropArgs& pa, hipStream_t s) {
  const T ident = add_identity ? T(1) : T(0), inv_nm = (T)(1.0 / nm);
  if (wide)
    gradients_jacobian_kernel<T, P, true><<<grid, FJ_LANES * FJ_WAVES, 0, s>>>((const T*)gr, (const T*)w, gk, g, inv_nm, ident,
                                                                                (Quad<T>*)J, (T*)props, pa);
  else
    gradients_jacobian_kernel<T, P, false><<<grid, FJ_LANES * FJ_WAVES, 0, s>>>((const T*)gr, (const T*)w, gk, g, inv_nm, ident,
                                                                                 (Quad<T>*)J, (T*)props, pa);
}

template <class T>
hipError_t launch_grads_t(int P, unsigned grid, const void* gr, const void* w, const GradK& gk, const Geom& g, double nm, bool wide,
                          int add_identity, void* J, void* props, const PropArgs& pa, hipStream_t s) {
  switch (P) {
    case 2: launch_grads_p<T, 2>(grid, gr, w, gk, g, nm, wide, add_identity, J, props, pa, s); break;
    case 3: launch_grads_p<T, 3>(grid, gr, w, gk, g, nm, wide, add_identity, J, props, pa, s); break;
    case 4: launch_grads_p<T, 4>(grid, gr, w, gk, g, nm, wide, add_identity, J, props, pa, s); break;
    case 5: launch_grads_p<T, 5>(grid, gr, w, gk, g, nm, wide, add_identity, J, props, pa, s); break;
    case 6: launch_grads_p<T, 6>(grid, gr, w, gk, g, nm, wide, add_identity, J, props, pa, s); break;
    case 7: launch_grads_p<T, 7>(grid, gr, w, gk, g, nm, wide, add_identity, J, props, pa, s); break;
    case 8: launch_grads_p<T, 8>(grid, gr, w, gk, g, nm, wide, add_identity, J, props, pa, s); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

template <class T>
void launch_field_t(unsigned grid, const void* u, const Geom& g, double h, bool wide, int add_identity, void* J, void* props,
                    const PropArgs& pa, hipStream_t s) {
  const T h1 = (T)h, h2 = (T)(2.0 * h), ident = add_identity ? T(1) : T(0);   // each divisor rounded once, as NumPy rounds it
  if (wide)
    field_jacobian_kernel<T, true><<<grid, FJ_LANES * FJ_WAVES, 0, s>>>((const T*)u, g, h1, h2, ident, (Quad<T>*)J, (T*)props, pa);
  else
    field_jacobian_kernel<T, false><<<grid, FJ_LANES * FJ_WAVES, 0, s>>>((const T*)u, g, h1, h2, ident, (Quad<T>*)J, (T*)props, pa);
}

}  // namespace

hipError_t launch_field_jacobian(int dtype, int nimg, int n0, int n1, const void* u, double nmperpixel, int add_identity, void* J,
                                 void* props, double refangle, double refscale, int diff, hipStream_t s) {
  const Geom g = make_geom(nimg, n0, n1, dtype == 0 ? 4 : 8);
  const uint64_t grid = grid_blocks(g);
  if (nimg < 1 || n0 < 2 || n1 < 2 || grid == 0 || (!J && !props)) return hipErrorInvalidValue;
  const bool wide = wide_ok(g, u, nullptr, props);
  const PropArgs pa{refangle, refscale, diff};
  GPA_PROF("field_jacobian_kernel", s);
  if (dtype == 0) launch_field_t<float>((unsigned)grid, u, g, nmperpixel, wide, add_identity, J, props, pa, s);
  else launch_field_t<double>((unsigned)grid, u, g, nmperpixel, wide, add_identity, J, props, pa, s);
  return hipGetLastError();
}

hipError_t launch_phases_jacobian(int dtype, int n0, int n1, int P, const double* kvecs, const void* phases, const void* weights,
                                  double nmperpixel, int add_identity, void* J, void* props, double refangle, double refscale,
                                  int diff, hipStream_t s) {
  const Geom g = make_geom(1, n0, n1, dtype == 0 ? 4 : 8);
  const uint64_t grid = grid_blocks(g);
  if (n0 < 2 || n1 < 2 || P < 2 || P > 8 || grid == 0 || (!J && !props)) return hipErrorInvalidValue;
  KMat km{};
  for (int i = 0; i < 2 * P; ++i) km.k[i] = 6.283185307179586476925 * kvecs[i];
  const bool wide = wide_ok(g, phases, weights, props);
  const PropArgs pa{refangle, refscale, diff};
  GPA_PROF("phases_jacobian_kernel", s);
  if (dtype == 0)
    return launch_phases_t<float>(P, (unsigned)grid, phases, weights, km, g, nmperpixel, wide, add_identity, J, props, pa, s);
  return launch_phases_t<double>(P, (unsigned)grid, phases, weights, km, g, nmperpixel, wide, add_identity, J, props, pa, s);
}

// a frame is one row of n0 x n1 pixels to this pointwise kernel (gradients_geom of gpa_fieldjac.h)
hipError_t launch_gradients_jacobian(int dtype, int nimg, int n0, int n1, int P, const double* kvecs, const double* dks,
                                     const void* grads, const void* weights, double nmperpixel, int add_identity, void* J, void* props,
                                     double refangle, double refscale, int diff, hipStream_t s) {
  if (nimg < 1 || n0 < 1 || n1 < 1 || !gradients_fits(n0, n1) || P < 2 || P > 8 || (!J && !props)) return hipErrorInvalidValue;
  const Geom g = gradients_geom(nimg, n0, n1, dtype == 0 ? 4 : 8);
  const uint64_t grid = grid_blocks(g);
  if (grid == 0) return hipErrorInvalidValue;
  GradK gk{};
  gk.on = dks != nullptr;
  for (int i = 0; i < 2 * P; ++i) {   // the doubles gpa_phasegradient2J stages and passes
    gk.k[i] = 2.0 * M_PI * (kvecs[i] + (dks ? dks[i] : 0.0));
    gk.shift[i] = dks ? 6.283185307179586476925 * dks[i] : 0.0;
  }
  const bool wide = wide_ok(g, grads, weights, props);
  const PropArgs pa{refangle, refscale, diff};
  GPA_PROF("gradients_jacobian_kernel", s);
  if (dtype == 0)
    return launch_grads_t<float>(P, (unsigned)grid, grads, weights, gk, g, nmperpixel, wide, add_identity, J, props, pa, s);
  return launch_grads_t<double>(P, (unsigned)grid, grads, weights, gk, g, nmperpixel, wide, add_identity, J, props, pa, s);
}

hipError_t launch_phys_props(int dtype, const void* jac, size_t npx, int add_identity, double refangle, double refscale, int diff,
                             double poisson_ratio, void* out, hipStream_t s) {
  const unsigned grid = (unsigned)((npx + 255) / 256);
  GPA_PROF("phys_props_kernel", s);
  if (dtype == 0)
    phys_props_kernel<float><<<grid, 256, 0, s>>>((const Quad<float>*)jac, npx, add_identity ? 1.f : 0.f, (float)refangle,
                                                  (float)refscale, diff, (float)poisson_ratio, (float*)out);
  else
    phys_props_kernel<double><<<grid, 256, 0, s>>>((const Quad<double>*)jac, npx, add_identity ? 1.0 : 0.0, refangle, refscale,
                                                   diff, poisson_ratio, (double*)out);
  return hipGetLastError();
}

}  // namespace gpa
