// Host walk of the pointwise geometry of pygpa_amd/csrc/gpa_fieldjac.h (gradients_geom: a frame is one row of n0 * n1 pixels) as
// gradients_jacobian_kernel of gpa_fieldjac.hip steps through it: every wave of a launch, every lane and pixel of it.  Checks
// that each pixel of each frame is taken exactly once, that the weights, the interleaved gradient pairs, J and the property
// planes a lane touches lie inside its own frame, and that whole vectors are used only where they fit.  Prints "OK <checks>".
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

static void walk(int nimg, int n0, int n1, int P, int elem) {
  CHECK(gradients_fits(n0, n1), "%d x %d fits", n0, n1);
  const Geom g = gradients_geom(nimg, n0, n1, elem);
  const size_t npx = (size_t)n0 * n1;
  CHECK(g.n0 == 1 && (size_t)g.n1 == npx && g.row_bands == 1 && g.tiles == (uint64_t)nimg * g.col_tiles, "one row per frame");
  const bool wide = g.n1 % g.vec == 0;   // (and aligned bases: the launcher's test)
  const uint64_t blocks = grid_blocks(g);
  CHECK(blocks > 0 && blocks * FJ_WAVES >= g.tiles, "grid");
  std::vector<unsigned char> taken((size_t)nimg * npx, 0);
  for (uint64_t tix = 0; tix < blocks * FJ_WAVES; ++tix) {
    if (tix >= g.tiles) continue;   // the wave leaves
    const Tile t = tile_of(g, tix);
    CHECK(t.img >= 0 && t.img < nimg && t.r0 == 0 && t.r1 == 1, "tile %llu", (unsigned long long)tix);
    const size_t wbase = plane_offset(g, t.img, P, 0), jbase = plane_offset(g, t.img, 1, 0);
    CHECK(wbase == (size_t)t.img * P * npx && jbase == (size_t)t.img * npx, "frame offsets");
    for (int lane = 0; lane < FJ_LANES; ++lane) {
      const int c = lane_col(g, t, lane);
      if (c >= g.n1) continue;   // the lane leaves
      if (wide) CHECK((size_t)c + g.vec <= npx && c % g.vec == 0, "a whole vector at pixel %d of %zu", c, npx);
      for (int k = 0; k < g.vec; ++k) {
        if (c + k >= g.n1) continue;
        const size_t o = pixel_offset(g, 0, c + k);
        for (int p = 0; p < P; ++p) {
          CHECK(wbase + p * npx + o < (size_t)(t.img + 1) * P * npx, "weight of peak %d", p);
          CHECK(2 * (wbase + p * npx + o) + 1 < 2 * (size_t)(t.img + 1) * P * npx, "pair of peak %d", p);
        }
        CHECK(jbase + o < (size_t)(t.img + 1) * npx, "J");
        for (int q = 0; q < 4; ++q)
          CHECK(plane_offset(g, t.img, 4, q) + o >= (size_t)t.img * 4 * npx + q * npx && plane_offset(g, t.img, 4, q) + o < (size_t)t.img * 4 * npx + (q + 1) * npx, "property plane %d", q);
        ++taken[jbase + o];
      }
    }
  }
  for (size_t i = 0; i < taken.size(); ++i) CHECK(taken[i] == 1, "pixel %zu of %d x %d x %d taken %d times", i, nimg, n0, n1, taken[i]);
}

int main() {
  const int elems[2] = {4, 8};
  const int shapes[][2] = {{1, 1}, {3, 5}, {7, 64}, {9, 67}, {64, 64}, {1, 255}, {1, 256}, {1, 257}, {33, 31}, {2, 1024}, {5, 1025}};
  for (int e = 0; e < 2; ++e)
    for (const auto& s : shapes)
      for (int nimg : {1, 3})
        for (int P : {2, 3, 8}) walk(nimg, s[0], s[1], P, elems[e]);
  CHECK(gradients_fits(46340, 46340) && !gradients_fits(46341, 46341) && !gradients_fits(65536, 65536), "frames of up to 2^31 - 1 pixels");
  CHECK(grid_blocks(gradients_geom(4096, 4096, 4096, 4)) > 0, "a stack of 4096 frames of 4096^2 is one launch");
  std::printf("OK %ld\n", checks);
  return 0;
}
