"""Time GPA.iterate_GPA host-in / host-out, as one library call (fused=True) and as the host loop over the single entry points
(fused=False), on one GPU:

    python tools/iterate_timing.py [--out profiles/iterate_fused_timing.txt] [--calls 10] [--sizes 512 2048]

Per size (square frames) and dtype: 3 peaks, sigma 10, edge 5, iters 3, kmax_iter 25, kmax 200 (the defaults of the
reference).  Plans are warmed by two untimed calls of each route; then every call is timed on the host clock between two
synchronisations of both plans, and the median of `--calls` calls is reported.  The stage split of the fused call comes from
one further call with gpa_set_profiling on (gpa_last_stage_ms: every stage waited for, so the stages add up to a little more
than an unprofiled call)."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pygpa_amd import _lib                                        # noqa: E402
import pygpa_amd.geometric_phase_analysis as GPA                  # noqa: E402
from pygpa_amd.synthetic import hex_kvecs, gaussian_bump_displacement, hex_moire   # noqa: E402

EDGE, ITERS, SIGMA = 5, 3, 10


def timed(fn, plans, calls):
    ts = []
    for _ in range(calls):
        for p in plans:
            p.sync()
        t0 = time.perf_counter()
        out = fn()
        for p in plans:
            p.sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--sizes', type=int, nargs='+', default=[512, 2048])
    args = ap.parse_args()
    lines = ['iterate_GPA host-in / host-out, 3 peaks, sigma %d, edge %d, iters %d, kmax_iter 25, kmax 200; median [min .. max] of %d '
             'calls, ms' % (SIGMA, EDGE, ITERS, args.calls),
             '%-6s %-8s %28s %28s %7s   %s' % ('size', 'dtype', 'fused', 'fused=False', 'ratio',
                                               'fused stages: lock-ins / polar crop / unwraps / fits')]
    for n in args.sizes:
        true_ks = hex_kvecs(0.1, 7.0)
        start = true_ks * 1.004
        image = hex_moire((n, n), true_ks, gaussian_bump_displacement((n, n)), noise=0.05, seed=1)
        image = image - image.mean()
        for dtype in (np.float32, np.float64):
            img = np.ascontiguousarray(image, dtype=dtype)
            plan = _lib.get_plan((n, n), len(start), dtype)
            crop = _lib.get_plan((n - 2 * EDGE, n - 2 * EDGE), 1, dtype)
            routes = {}
            for fused in (True, False):
                fn = lambda: GPA.iterate_GPA(img, start, SIGMA, edge=EDGE, iters=ITERS, dtype=dtype, fused=fused)   # noqa: E731
                fn(), fn()
                routes[fused] = timed(fn, (plan, crop), args.calls)
            assert plan is _lib.get_plan((n, n), len(start), dtype)       # the timed calls ran on the warmed plans
            plan.set_profiling(True)
            GPA.iterate_GPA(img, start, SIGMA, edge=EDGE, iters=ITERS, dtype=dtype, fused=True)
            st = plan.last_stage_ms()
            plan.set_profiling(False)
            dk = np.abs(routes[True][3][2] - routes[False][3][2]).max()
            f, h = routes[True], routes[False]
            lines.append('%-6d %-8s %9.2f [%7.2f .. %7.2f] %9.2f [%7.2f .. %7.2f] %7.2f   %.2f / %.2f / %.2f / %.2f   (|corr diff| %.1e)'
                         % (n, np.dtype(dtype).name, f[0], f[1], f[2], h[0], h[1], h[2], h[0] / f[0], st[0], st[1], st[2], st[3], dk))
            print(lines[-1], flush=True)
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(text)


if __name__ == '__main__':
    main()
