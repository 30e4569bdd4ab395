// Geometry and difference rule of the field -> Jacobian kernels (gpa_fieldjac.hip): u2J and phases2J of
// pyGPA/property_extract.py:13-52.  Host and device: tests/host/fieldjac_check.cpp walks every tile of this header on the CPU.
//
// One WAVE owns one tile: FJ_ROWS rows of 64 lanes x (16 bytes of columns).  The wave walks its rows top to bottom and keeps the
// rows i-1, i, i+1 of every input plane in registers, so a plane is read once per tile plus one halo row above and below
// (2 / FJ_ROWS more, re-reads of lines a neighbouring tile fetches).  Column neighbours are the lane's own vector and, at its two
// ends, the neighbouring lane's (cross-lane move) or, for lanes 0 and 63, one scalar load.  No LDS, no barrier, no atomics.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define GPA_FJ_HD __host__ __device__ __forceinline__
#else
#define GPA_FJ_HD inline
#endif

namespace gpa {
namespace fieldjac {

constexpr int FJ_LANES = 64;       // lanes of the wave that walks a tile
constexpr int FJ_VEC_BYTES = 16;   // bytes of one row and plane a lane holds: 4 f32 or 2 f64 columns
constexpr int FJ_ROWS = 16;        // rows of a tile
constexpr int FJ_WAVES = 4;        // tiles (waves) per workgroup, neighbours along a row

struct Geom {
  int nimg, n0, n1;
  int vec;              // columns per lane
  int tile_w;           // columns per tile
  int col_tiles, row_bands;
  uint64_t tiles;       // nimg * row_bands * col_tiles
};

GPA_FJ_HD Geom make_geom(int nimg, int n0, int n1, int elem_size) {
  Geom g;
  g.nimg = nimg; g.n0 = n0; g.n1 = n1;
  g.vec = FJ_VEC_BYTES / elem_size;
  g.tile_w = FJ_LANES * g.vec;
  g.col_tiles = (n1 + g.tile_w - 1) / g.tile_w;
  g.row_bands = (n0 + FJ_ROWS - 1) / FJ_ROWS;
  g.tiles = (uint64_t)nimg * (uint64_t)g.row_bands * (uint64_t)g.col_tiles;
  return g;
}

// workgroups of a launch; 0 when they exceed what one grid dimension takes
GPA_FJ_HD uint64_t grid_blocks(const Geom& g) {
  const uint64_t b = (g.tiles + FJ_WAVES - 1) / FJ_WAVES;
  return b <= 0x7fffffffull ? b : 0;
}

struct Tile { int img, r0, r1, c0; };   // frame, rows [r0, r1), first column

// tile t of the launch: column tiles run fastest, then row bands, then frames
GPA_FJ_HD Tile tile_of(const Geom& g, uint64_t t) {
  Tile x;
  const uint64_t ct = t % (uint64_t)g.col_tiles, rest = t / (uint64_t)g.col_tiles;
  const uint64_t band = rest % (uint64_t)g.row_bands;
  x.img = (int)(rest / (uint64_t)g.row_bands);
  x.r0 = (int)band * FJ_ROWS;
  x.r1 = x.r0 + FJ_ROWS < g.n0 ? x.r0 + FJ_ROWS : g.n0;
  x.c0 = (int)ct * g.tile_w;
  return x;
}

// first column of a lane of the tile (may lie beyond the frame: the lane then loads and stores nothing)
GPA_FJ_HD int lane_col(const Geom& g, const Tile& t, int lane) { return t.c0 + lane * g.vec; }

// element offset of pixel (r, c) of plane `plane` out of `planes` per frame
GPA_FJ_HD size_t plane_offset(const Geom& g, int img, int planes, int plane) {
  return ((size_t)img * (size_t)planes + (size_t)plane) * ((size_t)g.n0 * (size_t)g.n1);
}
GPA_FJ_HD size_t pixel_offset(const Geom& g, int r, int c) { return (size_t)r * (size_t)g.n1 + (size_t)c; }

// The pointwise member of the family (gradients -> J, gradients_jacobian_kernel) has no stencil, so a frame is ONE row of
// n0 * n1 pixels to it: the same tiles, lanes and offsets, one row band per frame, a wave on 64 vectors of consecutive pixels.
// The row length is an int: frames of up to 2^31 - 1 pixels.
GPA_FJ_HD bool gradients_fits(int n0, int n1) { return (uint64_t)n0 * (uint64_t)n1 <= 0x7fffffffull; }
GPA_FJ_HD Geom gradients_geom(int nimg, int n0, int n1, int elem_size) { return make_geom(nimg, 1, n0 * n1, elem_size); }

// The samples a difference at index i of an axis of n >= 2 points reads: i - 1 and i + 1 inside, the sample itself in place of
// the missing neighbour at the two ends (np.gradient's first-order edges).  hi - lo is 2 inside and 1 at an end.
GPA_FJ_HD void stencil(int i, int n, int& lo, int& hi) {
  lo = i > 0 ? i - 1 : 0;
  hi = i < n - 1 ? i + 1 : n - 1;
}
GPA_FJ_HD bool is_edge(int i, int n) { return i == 0 || i == n - 1; }

// np.gradient(-f, h) at one sample: h1 = T(h), h2 = T(2 h), each rounded once; a true division
template <class T>
GPA_FJ_HD T field_diff(T flo, T fhi, bool edge, T h1, T h2) {
  return ((-fhi) - (-flo)) / (edge ? h1 : h2);
}

// 2 np.gradient(f) at one sample (unit spacing): f[i+1] - f[i-1] inside, twice the one-sided difference at an end
template <class T>
GPA_FJ_HD T phase_diff(T flo, T fhi, bool edge) {
  const T d = fhi - flo;
  return edge ? d + d : d;
}

}  // namespace fieldjac
}  // namespace gpa
