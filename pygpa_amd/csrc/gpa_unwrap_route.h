// Which kernels a solve of the weighted unwrap runs: the one statement of the rules.  run_pcg (gpa_unwrap.hip) fills a
// RouteIn from the workspace and the option table, calls unwrap_route() once per solve and keeps the answer in Impl::route;
// the dispatchers of the row, column and stencil translation units switch on it.  gpa_unwrap_tables.hip asks the
// unwrap_builds_*() functions below which tables a shape gets, so the builder and the route read the same conditions.
// Plain C++17: no HIP header, no gpa_internal.h, no globals -- tests/host/unwrap_route_table.cpp compiles it with g++
// and tests/test_unwrap_route_host.py holds the result to a written-out table.
#pragma once
#include <stddef.h>

namespace gpa {

// One image per call and axes up to 1024: the fused kernels are bound by their chains of dependent memory round
// trips, not by bandwidth or occupancy, and run as latency-tuned instantiations (every input requested before the
// first wait: ~30 more registers).  Stacks of frames and larger images fill the GPU and keep the lean ones
// (measured: 64 frames of 512^2 2596 -> 2475 Mpix/s and 2048^2 2565 -> 2493 with the latency-tuned kernels).
// The two kinds evaluate the same formulas; the compiler contracts multiply-adds differently in places, so results
// agree to rounding, not to the bit (GPA_NO_LAT=1 runs the lean kernels everywhere: tests use it to compare a stack
// with single calls exactly).
#ifndef GPA_UNWRAP_LAT_MAXLG
#define GPA_UNWRAP_LAT_MAXLG 10
#endif
#ifndef GPA_ROWHALF_MINLG
#define GPA_ROWHALF_MINLG 13   // rows from 2^13 points on: one row per half-length transform (gpa_unwrap_rowhalf.hip)
#endif
#ifndef GPA_COLSTREAM_MIN
#define GPA_COLSTREAM_MIN 2048   // square images from this side on take the streamed column solve by default (2048^2: 26 -> 19 us per iteration, 3000^2: 58 -> 43; 1024^2: slower)
#endif
#ifndef GPA_ROWPQ_MAXLG
#define GPA_ROWPQ_MAXLG 9   // rows up to 512 pixels: row kernel and stencil in one launch (rowidct_pq_kernel)
#endif

// ---- which shapes the power-of-two kernels take (gpa_unwrap_tables.hip: Impl::generic is the negation) ----
// both axes powers of two of 64 .. 16384 points (lg = -1: no power of two).  Anything else -- 32 x 8192 as much as
// 1000 x 1000 -- is a generic shape: the mixed-radix engine where it has a plan, the plain scheme otherwise.
constexpr bool unwrap_pow2_shape(int lg0, int lg1) { return lg0 >= 6 && lg1 >= 6 && lg0 <= 14 && lg1 <= 14; }

// ---- which tables a workspace gets (gpa_unwrap_tables.hip builds exactly these) ----
// power-of-two shapes: twiddles of length n1 / 2 for the half-length row kernels (rows of 4096 points can be switched to
// them for measurements: ROWHALF_MINLG; f64 takes the forward one there by default)
constexpr bool unwrap_builds_rowhalf(int lg1) { return lg1 >= 12; }
// power-of-two shapes: the tables of the half-length column kernel -- f64 columns of 16384 points, the one length whose
// packed-pair transform (colsolve_kernel) does not fit LDS
constexpr bool unwrap_builds_colhalf(int dtype, int lg0) { return dtype == 1 && lg0 == 14; }
// the shapes for which build_tritab / build_streamtab are called: square images, on the fused path (the smooth sizes'
// streamed solve reads rows of whole 4-pixel vectors).  Either builder may still decline: build_tritab when the column
// does not fit one workgroup (tri_geometry), build_streamtab when colstream_chunk() answers 0.
constexpr bool unwrap_builds_tri(bool generic, bool mr_ok, int n0, int n1) { return n0 == n1 && (!generic || mr_ok); }
constexpr bool unwrap_builds_stream(bool generic, bool mr_ok, int n0, int n1) {
  return n0 == n1 && (!generic || (mr_ok && (n1 % 4) == 0));
}
// rows per thread of the transform-free column solve (triR of the table): the f32 tile of a thread (ROWS x 4 columns) has
// to leave room for the double-precision recursions within the 128 VGPRs that 1024 threads per workgroup allow: 8 rows
// (32 registers); f64: 16 rows x 2 columns (64).  Short columns take half as many rows per thread on twice the threads:
// with ~125 one-wavefront workgroups on 256 CUs the kernel is bound by the instruction stream of a wavefront (4089
// instructions at 8 rows x 4 columns, a quarter of them f64), not by anything the chip shares.  small = largest n0 that
// does (TRI_SMALL, diagnostic).
constexpr int tri_rows_for(size_t real_size, int n0, int small = 640) {
  const int base = real_size == 4 ? 8 : 16;
  if (real_size == 4 && n0 > 8192) return 2 * base;   // (1024 threads hold at most 1024 chunks)
  return n0 <= small ? base / 2 : base;
}

// ---- what the choice depends on, as values ----
struct RouteIn {
  int dtype = 0, n0 = 0, n1 = 0, lg0 = -1, lg1 = -1;   // dtype 0: f32, 1: f64; lg = -1: the axis is no power of two
  int nprob = 1;
  bool generic = false, mr_ok = false;
  // tables the workspace holds
  bool has_rowhalf = false;   // Impl::tw1h
  bool has_colhalf = false;   // Impl::wk0h
  bool has_tri = false;       // Impl::tritab, with its rows per thread
  int triR = 0;
  bool has_stream = false;    // Impl::strtab
  // options of the solve
  int col_mode = 0;           // COLSOLVE: 0 default, 1 tri, 2 fft, 3 stream
  bool no_lat = false, no_rowhalf = false;
  bool rowhalf_minlg_set = false;
  int rowhalf_minlg = GPA_ROWHALF_MINLG;   // ROWHALF_MINLG where set
  bool no_rowpers = false, no_rowpq = false, no_pqdct = false;
};

enum class RowFwd { packed, half, halfpers, mr };
enum class RowInv { packed, pers, half, halfpers, mr };
enum class ColSolve { dct, tri, stream, colhalf, mr };

struct Route {
  RowFwd fwd = RowFwd::packed;     // rowdct_fused: R -= alpha DCT_rows(q)
  RowInv inv = RowInv::packed;     // rowidct_p: Z -> p (not launched where rowpq)
  ColSolve cols = ColSolve::dct;   // R -> Z
  bool rowpq = false;              // rowidct_p and the stencil in one launch (rowidct_pq_kernel)
  bool fuse_pq = false;            // the stencil and the next rowdct in one launch (pqdct_kernel), R -= alpha D in the column solve
  bool lat_rows = false, lat_cols = false;   // latency-tuned instantiations of the packed row kernels / of colsolve_kernel
  bool lat_pq = false;             // pq_small_kernel allowed (pq_t adds the band height and pixel count of its grid)
};

inline const char* route_name(RowFwd v) {
  switch (v) {
    case RowFwd::packed: return "packed";
    case RowFwd::half: return "half";
    case RowFwd::halfpers: return "halfpers";
    case RowFwd::mr: return "mr";
  }
  return "?";
}
inline const char* route_name(RowInv v) {
  switch (v) {
    case RowInv::packed: return "packed";
    case RowInv::pers: return "pers";
    case RowInv::half: return "half";
    case RowInv::halfpers: return "halfpers";
    case RowInv::mr: return "mr";
  }
  return "?";
}
inline const char* route_name(ColSolve v) {
  switch (v) {
    case ColSolve::dct: return "dct";
    case ColSolve::tri: return "tri";
    case ColSolve::stream: return "stream";
    case ColSolve::colhalf: return "colhalf";
    case ColSolve::mr: return "mr";
  }
  return "?";
}

// The rules, in the order the dispatchers used to test them.  (A generic shape without a mixed-radix plan runs the plain
// scheme and reads no route; it gets the generic answers.)
inline Route unwrap_route(const RouteIn& in) {
  Route r;
  const bool lat = !in.no_lat && in.nprob <= 2;
  r.lat_rows = lat && in.lg1 <= GPA_UNWRAP_LAT_MAXLG;
  r.lat_cols = lat && in.lg0 <= GPA_UNWRAP_LAT_MAXLG;
  r.lat_pq = lat;

  // ---- rows ----
  if (in.generic) {
    r.fwd = RowFwd::mr;
    r.inv = RowInv::mr;
  } else {
    // rows of 8192 points and more take the half-length kernels (NO_ROWHALF: the packed ones, for tests and measurements;
    // ROWHALF_MINLG moves the threshold, never below the 4096 points the twiddles exist from)
    const bool want_half = in.lg1 >= in.rowhalf_minlg && in.lg1 >= 12 && in.has_rowhalf && !in.no_rowhalf;
    // f64 rows of 16384 points have no packed-pair kernel to fall back to (its transform does not fit LDS): the half-length
    // kernels run whatever NO_ROWHALF / ROWHALF_MINLG say
    const bool half_only = in.dtype == 1 && in.lg1 == 14 && in.has_rowhalf;
    const bool half_exists = in.lg1 >= 12 && in.lg1 <= 14 && in.has_rowhalf;
    const bool half = (want_half || half_only) && half_exists;
    // f32 rows of 8192 / 16384 points, at least 64 of them: the persistent, LDS-DMA-pipelined forms of the half-length
    // kernels (bit-equal to the one-row-per-workgroup ones; NO_ROWPERS keeps those)
    const bool halfpers = in.dtype == 0 && (in.lg1 == 13 || in.lg1 == 14) && in.has_rowhalf && in.n0 >= 64 && !in.no_rowpers;
    // f32 rows of 4096 points, at least 64 of them: the persistent, software-pipelined rowidct_p (NO_ROWPERS: the
    // one-pair-per-workgroup kernel)
    const bool pers = in.dtype == 0 && in.lg1 == 12 && (in.n0 % 2) == 0 && in.n0 >= 64 && !in.no_rowpers;
    r.inv = half ? (halfpers ? RowInv::halfpers : RowInv::half) : (pers ? RowInv::pers : RowInv::packed);
    r.fwd = half ? (halfpers ? RowFwd::halfpers : RowFwd::half) : RowFwd::packed;
    // f64 rows of 4096 points: the forward kernel alone gains from the half-length form (116 -> 99 us per launch; the inverse
    // loses, 95 -> 126, and stays packed).
    // (quirk, kept: ROWHALF_MINLG set to ANY value, its default 13 included, switches this off)
    if (in.dtype == 1 && in.lg1 == 12 && in.has_rowhalf && !in.no_rowhalf && !in.rowhalf_minlg_set) r.fwd = RowFwd::half;
    // (quirk, kept: NO_ROWHALF is ignored for f64 rows of 16384 points -- half_only above)
  }

  // ---- columns ----
  // Square images from 2048 points a side: the streamed recursion (gpa_unwrap_colstream.hip) -- three launches that
  // read 1 KiB row pieces at the streaming rate instead of one that holds whole columns and is down to 32 / 16 / 8-byte
  // pieces at 4096 / 8192 / 16384 points.  COLSOLVE=stream forces it wherever it is offered, =tri / =fft the resident kernels.
  const bool stream = in.has_stream && (in.col_mode == 3 || (in.col_mode == 0 && in.n0 >= GPA_COLSTREAM_MIN));
  if (stream) {
    r.cols = ColSolve::stream;
  } else if (in.generic) {
    // smooth sizes: the transform-free solve where it applies (square images; it is 2-3x faster than two mixed-radix
    // transforms per column pair), COLSOLVE=fft keeps the transforms
    r.cols = in.has_tri && in.col_mode != 2 ? ColSolve::tri : ColSolve::mr;
  } else {
    // Square images can solve the columns without a transform (colsolve_tri_kernel).  Measured at 4096^2 on MI355X
    // (profiles/r02_colsolve_tri.txt): f64 1.54 ms per step against 2.0 for the DCT kernel (whose f64 transforms
    // spill), f32 82 us per launch against 68 -- the f32 DCT kernel is the faster one.  So: f64 by default,
    // COLSOLVE=tri / fft forces one or the other (tests compare the two).
    // (f32 columns of 8192 points: the transform kernel is down to two column pairs -- 16-byte row segments -- per
    //  workgroup there and loses to the recursion: 453 against ~330 us per launch)
    // (quirk, kept: COLSOLVE=stream where no stream table exists is neither tri nor default -- the transform kernels)
    const bool want_tri = in.col_mode ? in.col_mode == 1 : (in.dtype != 0 || in.lg0 >= 13);
    if (in.has_tri && want_tri && in.n0 / in.triR <= 1024) r.cols = ColSolve::tri;
    // f64 columns of 16384 points: colsolve_kernel's packed-pair transform does not fit LDS (ColGeom::FITS) -- one column per
    // half-length transform instead (gpa_unwrap_colhalf.hip)
    else if (in.dtype == 1 && in.lg0 == 14 && in.has_colhalf) r.cols = ColSolve::colhalf;
    else r.cols = ColSolve::dct;
  }

  // ---- stencil fusions ----
  // one image with rows of at most 512 pixels: row kernel and stencil in one launch (rowidct_pq_kernel)
  r.rowpq = !in.generic && lat && in.lg1 <= GPA_ROWPQ_MAXLG && in.n0 >= 4 && !in.no_rowpq;
  // rows of 2048 / 4096 points with the streamed column solve: stencil and row transform in one launch (pqdct_kernel),
  // the residual update applied by the column solve's first launch -- five launches and 44 bytes per pixel per
  // iteration instead of six and 48 (NO_PQDCT keeps the separate kernels)
  r.fuse_pq = !r.rowpq && !in.generic && (in.lg1 == 11 || in.lg1 == 12) && (in.n0 % 2) == 0 && stream && !in.no_pqdct;
  return r;
}

}  // namespace gpa
