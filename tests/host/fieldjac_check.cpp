// Host walk of pygpa_amd/csrc/gpa_fieldjac.h, the geometry and difference rule of the field -> Jacobian kernels: every tile of a
// launch, every lane and column of it, as the kernels of gpa_fieldjac.hip step through them.  Checks that the tiles partition
// the frames (each output pixel written exactly once, by one lane), that every sample a lane reads lies inside its own frame and
// inside what the wave holds (its rows r0 - 1 ... r1, its own vector, one neighbour lane or one in-frame scalar), and the
// difference rule against a reference that walks the axis the way np.gradient is written.  Prints "OK <checks>".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gpa_fieldjac.h"

using namespace gpa::fieldjac;

static long checks = 0;
#define CHECK(cond, ...)                                   \
  do {                                                     \
    ++checks;                                              \
    if (!(cond)) {                                         \
      std::printf("FAIL %s:%d: ", __FILE__, __LINE__);     \
      std::printf(__VA_ARGS__);                            \
      std::printf("\n");                                   \
      std::exit(1);                                        \
    }                                                      \
  } while (0)

static void walk(int nimg, int n0, int n1, int elem) {
  const Geom g = make_geom(nimg, n0, n1, elem);
  CHECK(g.vec * elem == FJ_VEC_BYTES && g.tile_w == FJ_LANES * g.vec, "vector %d", g.vec);
  CHECK(g.col_tiles * g.tile_w >= n1 && (g.col_tiles - 1) * g.tile_w < n1, "column tiles %d for %d", g.col_tiles, n1);
  CHECK(g.row_bands * FJ_ROWS >= n0 && (g.row_bands - 1) * FJ_ROWS < n0, "row bands %d for %d", g.row_bands, n0);
  const uint64_t blocks = grid_blocks(g);
  CHECK(blocks > 0 && blocks * FJ_WAVES >= g.tiles && (blocks - 1) * FJ_WAVES < g.tiles, "grid");
  const size_t total = (size_t)nimg * n0 * n1;
  std::vector<unsigned char> written(total, 0);
  for (uint64_t tix = 0; tix < blocks * FJ_WAVES; ++tix) {
    if (tix >= g.tiles) continue;   // the wave leaves
    const Tile t = tile_of(g, tix);
    CHECK(t.img >= 0 && t.img < nimg && t.r0 >= 0 && t.r0 < t.r1 && t.r1 <= n0 && t.r1 - t.r0 <= FJ_ROWS && t.c0 >= 0 && t.c0 < n1,
          "tile %llu of %d x %d x %d", (unsigned long long)tix, nimg, n0, n1);
    const size_t frame = plane_offset(g, t.img, 1, 0);
    CHECK(frame == (size_t)t.img * n0 * n1 && plane_offset(g, t.img, 2, 1) == ((size_t)t.img * 2 + 1) * n0 * n1, "plane offset");
    for (int lane = 0; lane < FJ_LANES; ++lane) {
      const int c = lane_col(g, t, lane);
      for (int k = 0; k < g.vec; ++k) {
        const int col = c + k;
        if (col >= n1) continue;
        int clo, chi;
        stencil(col, n1, clo, chi);
        CHECK(clo >= 0 && chi < n1 && chi - clo == (is_edge(col, n1) ? 1 : 2) && clo <= col && col <= chi, "column stencil");
        // the left sample: the lane's own vector, the neighbour lane's last column, or (lane 0) one scalar of the frame
        if (clo < col) CHECK(k > 0 || lane > 0 || clo == t.c0 - 1, "left neighbour of column %d", col);
        if (chi > col) CHECK(k < g.vec - 1 || lane < FJ_LANES - 1 || chi == t.c0 + g.tile_w, "right neighbour of column %d", col);
        for (int r = t.r0; r < t.r1; ++r) {
          int rlo, rhi;
          stencil(r, n0, rlo, rhi);
          CHECK(rlo >= 0 && rhi < n0 && rhi - rlo == (is_edge(r, n0) ? 1 : 2), "row stencil");
          CHECK(rlo >= (t.r0 > 0 ? t.r0 - 1 : 0) && rhi <= (t.r1 < n0 ? t.r1 : n0 - 1), "row %d reads outside the wave's rows", r);
          const size_t o = frame + pixel_offset(g, r, col);
          CHECK(o < total, "offset");
          CHECK(frame + pixel_offset(g, rlo, clo) >= frame && frame + pixel_offset(g, rhi, chi) < frame + (size_t)n0 * n1,
                "a read leaves the frame");
          ++written[o];
        }
      }
    }
  }
  for (size_t i = 0; i < total; ++i) CHECK(written[i] == 1, "pixel %zu of %d x %d x %d written %d times", i, nimg, n0, n1, written[i]);
}

// the axis walked the way np.gradient is written: interior, then the first and the last sample
template <class T>
static void rule(int n, double h, unsigned seed) {
  std::vector<T> f(n), want(n), want2(n);
  std::srand(seed);
  for (int i = 0; i < n; ++i) f[i] = (T)((std::rand() % 20001 - 10000) * 1e-3);
  const T h1 = (T)h, h2 = (T)(2.0 * h);
  for (int i = 1; i < n - 1; ++i) {
    want[i] = ((-f[i + 1]) - (-f[i - 1])) / h2;
    want2[i] = f[i + 1] - f[i - 1];
  }
  want[0] = ((-f[1]) - (-f[0])) / h1;
  want[n - 1] = ((-f[n - 1]) - (-f[n - 2])) / h1;
  want2[0] = T(2) * (f[1] - f[0]);
  want2[n - 1] = T(2) * (f[n - 1] - f[n - 2]);
  for (int i = 0; i < n; ++i) {
    int lo, hi;
    stencil(i, n, lo, hi);
    CHECK(field_diff(f[lo], f[hi], is_edge(i, n), h1, h2) == want[i], "field rule at %d of %d", i, n);
    CHECK(phase_diff(f[lo], f[hi], is_edge(i, n)) == want2[i], "phase rule at %d of %d", i, n);
  }
}

int main() {
  const int elems[2] = {4, 8};
  for (int e = 0; e < 2; ++e) {
    const int tw = FJ_LANES * FJ_VEC_BYTES / elems[e];
    const int few1[] = {2, 5, 70}, few0[] = {2, 3, FJ_ROWS + 1, 37};
    for (int n0 = 2; n0 <= 300; ++n0)
      for (int n1 : few1) walk(1, n0, n1, elems[e]);
    for (int n1 = 2; n1 <= 300; ++n1)
      for (int n0 : few0) walk(1, n0, n1, elems[e]);
    const int wide[] = {tw - 1, tw, tw + 1, 2 * tw + 3};
    for (int n1 : wide)
      for (int n0 : few0) walk(n0 == 3 ? 3 : 1, n0, n1, elems[e]);
    walk(3, 2 * FJ_ROWS + 5, 70, elems[e]);
    walk(5, 2, 2, elems[e]);
  }
  // beyond 2^31 elements: the offsets are 64-bit and the grid is refused only beyond one grid dimension
  {
    const Geom g = make_geom(3, 40000, 40000, 4);
    CHECK(g.tiles == 3ull * 2500 * 157 && grid_blocks(g) == (g.tiles + FJ_WAVES - 1) / FJ_WAVES, "large geometry");
    const Tile t = tile_of(g, g.tiles - 1);
    CHECK(t.img == 2 && t.r0 == 39984 && t.r1 == 40000 && t.c0 == 156 * 256, "last tile");
    CHECK(plane_offset(g, 2, 4, 3) + pixel_offset(g, 39999, 39999) == 12ull * 1600000000ull - 1, "64-bit offset");
    CHECK(grid_blocks(make_geom(65535, 1 << 20, 1 << 12, 8)) == 0, "a launch beyond one grid dimension is refused");
  }
  for (int n = 2; n <= 40; ++n)
    for (double h : {1.0, 0.5, 3.7, 0.37}) {
      rule<float>(n, h, 17u * n);
      rule<double>(n, h, 29u * n);
    }
  std::printf("OK %ld\n", checks);
  return 0;
}
