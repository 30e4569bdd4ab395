// Host check of pygpa_amd/csrc/gpa_unwrap_route.h (tests/test_unwrap_route_host.py).
//   unwrap_route_table            reads one case per line from stdin and prints its route:
//       <f32|f64> <n0> <n1> [nprob=<n>] [generic] [NO_LAT] [NO_ROWHALF] [ROWHALF_MINLG=<lg>] [NO_ROWPERS] [NO_ROWPQ]
//       [NO_PQDCT] [COLSOLVE=<tri|fft|stream>]
//     -> fwd inv cols rowpq fuse_pq lat_rows lat_cols lat_pq      (inv is "-" where rowpq: the kernel is not launched)
//     (a shape outside unwrap_pow2_shape() -- 1000 x 1000, but also 32 x 8192 -- is generic with or without the word)
//   unwrap_route_table coupling   every power-of-two shape 64 .. 16384 per axis, both dtypes, every option combination:
//     the route never names a family whose table the unwrap_builds_*() functions say is absent, or that has no
//     instantiation for the shape; prints "OK <calls>".
// The workspace's tables are taken present exactly where gpa_unwrap_tables.hip builds them under default table-time
// options: unwrap_builds_*(), triR = tri_rows_for().  (build_tritab / build_streamtab decline no shape used here: the
// recursion's column fits one workgroup up to 16384 points in both precisions, and a column has at most 256 chunks.)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <iostream>
#include <sstream>
#include <string>

#include "gpa_unwrap_route.h"

using namespace gpa;

static int ilog2_exact(int n) {
  int lg = 0;
  while ((1 << lg) < n) ++lg;
  return (1 << lg) == n ? lg : -1;
}

// shape and default tables; generic sizes are taken with a mixed-radix plan (mr_ok).  A shape is generic where the caller says
// so and wherever the workspace makes it so: unwrap_pow2_shape() -- a power-of-two axis under 64 points has no power-of-two kernels
static RouteIn workspace(int dtype, int n0, int n1, bool generic) {
  RouteIn in;
  in.dtype = dtype; in.n0 = n0; in.n1 = n1;
  in.lg0 = ilog2_exact(n0); in.lg1 = ilog2_exact(n1);
  generic = generic || !unwrap_pow2_shape(in.lg0, in.lg1);
  in.generic = generic; in.mr_ok = generic;
  in.has_rowhalf = !generic && unwrap_builds_rowhalf(in.lg1);
  in.has_colhalf = !generic && unwrap_builds_colhalf(dtype, in.lg0);
  in.has_tri = unwrap_builds_tri(generic, in.mr_ok, n0, n1);
  in.triR = in.has_tri ? tri_rows_for(dtype == 0 ? 4 : 8, n0) : 0;
  in.has_stream = unwrap_builds_stream(generic, in.mr_ok, n0, n1);
  return in;
}

static int fail(const RouteIn& in, const Route& r, const char* what) {
  printf("FAIL %s: dtype %d %dx%d nprob %d col_mode %d no_lat %d no_rowhalf %d minlg %d/%d no_rowpers %d no_rowpq %d no_pqdct %d"
         " -> %s %s %s rowpq %d fuse_pq %d\n", what, in.dtype, in.n0, in.n1, in.nprob, in.col_mode, in.no_lat, in.no_rowhalf,
         in.rowhalf_minlg_set, in.rowhalf_minlg, in.no_rowpers, in.no_rowpq, in.no_pqdct, route_name(r.fwd), route_name(r.inv),
         route_name(r.cols), r.rowpq, r.fuse_pq);
  return 1;
}

static int coupling() {
  long calls = 0;
  for (int dtype = 0; dtype < 2; ++dtype)
    for (int lg0 = 6; lg0 <= 14; ++lg0)
      for (int lg1 = 6; lg1 <= 14; ++lg1)
        for (int opts = 0; opts < 64; ++opts)
          for (int col_mode = 0; col_mode < 4; ++col_mode)
            for (int minlg = 11; minlg <= 15; ++minlg)   // 11: not set
              for (int nprob = 1; nprob <= 4; nprob += 3) {
                RouteIn in = workspace(dtype, 1 << lg0, 1 << lg1, false);
                in.nprob = nprob;
                in.col_mode = col_mode;
                in.no_lat = opts & 1; in.no_rowhalf = opts & 2; in.no_rowpers = opts & 4;
                in.no_rowpq = opts & 8; in.no_pqdct = opts & 16;
                if (opts & 32) in.has_tri = in.has_stream = false, in.triR = 0;   // (a builder that declined)
                if (minlg > 11) { in.rowhalf_minlg_set = true; in.rowhalf_minlg = minlg; }
                const Route r = unwrap_route(in);
                ++calls;
                const bool f64 = dtype == 1;
                const bool fh = r.fwd == RowFwd::half || r.fwd == RowFwd::halfpers;
                const bool ih = r.inv == RowInv::half || r.inv == RowInv::halfpers;
                if ((fh || ih) && !(in.has_rowhalf && lg1 >= 12)) return fail(in, r, "half-length rows without twiddles");
                if ((r.fwd == RowFwd::halfpers || r.inv == RowInv::halfpers) && !(!f64 && lg1 >= 13)) return fail(in, r, "halfpers");
                if (r.inv == RowInv::pers && !(!f64 && lg1 == 12)) return fail(in, r, "pers");
                if ((r.fwd == RowFwd::packed || r.inv == RowInv::packed) && f64 && lg1 == 14) return fail(in, r, "no packed f64 kernel at 16384");
                if (r.fwd == RowFwd::mr || r.inv == RowInv::mr || r.cols == ColSolve::mr) return fail(in, r, "mr on a power of two");
                if (r.cols == ColSolve::stream && !in.has_stream) return fail(in, r, "stream without table");
                if (r.cols == ColSolve::tri && !in.has_tri) return fail(in, r, "tri without table");
                if (r.cols == ColSolve::colhalf && !(in.has_colhalf && f64 && lg0 == 14)) return fail(in, r, "colhalf without tables");
                if (r.cols == ColSolve::dct && f64 && lg0 == 14) return fail(in, r, "no f64 dct kernel at 16384");
                if (r.fuse_pq && !(r.cols == ColSolve::stream && (lg1 == 11 || lg1 == 12) && !r.rowpq)) return fail(in, r, "fuse_pq");
                if (r.rowpq && lg1 > 9) return fail(in, r, "rowpq");
                if ((r.lat_rows && lg1 > 10) || (r.lat_cols && lg0 > 10)) return fail(in, r, "lat");
              }
  printf("OK %ld\n", calls);
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "coupling")) return coupling();
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream ss(line);
    std::string dt, tok;
    int n0 = 0, n1 = 0;
    if (!(ss >> dt >> n0 >> n1)) continue;
    std::string rest;
    std::getline(ss, rest);
    RouteIn in = workspace(dt == "f64" ? 1 : 0, n0, n1, rest.find("generic") != std::string::npos);
    std::istringstream rs(rest);
    while (rs >> tok) {
      if (tok == "generic") continue;
      else if (tok.rfind("nprob=", 0) == 0) in.nprob = atoi(tok.c_str() + 6);
      else if (tok == "NO_LAT") in.no_lat = true;
      else if (tok == "NO_ROWHALF") in.no_rowhalf = true;
      else if (tok.rfind("ROWHALF_MINLG=", 0) == 0) { in.rowhalf_minlg_set = true; in.rowhalf_minlg = atoi(tok.c_str() + 14); }
      else if (tok == "NO_ROWPERS") in.no_rowpers = true;
      else if (tok == "NO_ROWPQ") in.no_rowpq = true;
      else if (tok == "NO_PQDCT") in.no_pqdct = true;
      else if (tok == "COLSOLVE=tri") in.col_mode = 1;
      else if (tok == "COLSOLVE=fft") in.col_mode = 2;
      else if (tok == "COLSOLVE=stream") in.col_mode = 3;
      else { printf("unknown token %s\n", tok.c_str()); return 2; }
    }
    const Route r = unwrap_route(in);
    printf("%s %s %s %d %d %d %d %d\n", route_name(r.fwd), r.rowpq ? "-" : route_name(r.inv), route_name(r.cols), r.rowpq,
           r.fuse_pq, r.lat_rows, r.lat_cols, r.lat_pq);
  }
  return 0;
}
