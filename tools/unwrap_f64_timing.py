#!/usr/bin/env python
"""One weighted component solve of the unwrap (kmax = 10) on resident data at the shapes the f64 long-axis kernels opened:
16384^2 in f64 beside f32, 8192^2 f64 (kernels that existed before: the yardstick of the box), and the 16384 x 64 /
64 x 16384 strips in f64.  Per-kernel times from the library's own events (gpa_set_profiling / gpa_last_kernel_profile),
the whole solve from the plan's timer, device memory of the plan from gpa_plan_workspace_bytes.
    python tools/unwrap_f64_timing.py [--out profiles/unwrap_f64_16384.txt] [--reps 3] [--cases 16384f64 16384f32 8192f64 strips]
Input: the smooth field of the long-axis tests, wrapped, with a closed-form weight (separable factors: no random draws)."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from pygpa_amd import _lib   # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=3)
ap.add_argument('--kmax', type=int, default=10)
ap.add_argument('--cases', nargs='+', default=['8192f64', '16384f32', '16384f64', 'strips'])
ap.add_argument('--out', default=None, help='append the table to this file as well')
a = ap.parse_args()

CASES = {'8192f64': [((8192, 8192), np.float64)], '16384f32': [((16384, 16384), np.float32)],
         '16384f64': [((16384, 16384), np.float64)],
         'strips': [((16384, 64), np.float64), ((64, 16384), np.float64)]}
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def wrap(v):
    return v - 2 * np.pi * np.floor((v + np.pi) / (2 * np.pi))


def problem(shape, dtype):
    """dx, dy of the wrapped smooth field and the weight, built in row blocks"""
    n0, n1 = shape
    x, y = np.arange(n0) / float(n0), np.arange(n1) / float(n1)
    sa, ca = np.sin(3 * np.pi * x), np.cos(3 * np.pi * x)
    fb, gb = 6.0 * np.cos(np.pi * y) * np.cos(4 * np.pi * y), 6.0 * np.sin(np.pi * y) * np.cos(4 * np.pi * y)
    dx, dy = np.empty((n0, n1 - 1), dtype=dtype), np.empty((n0 - 1, n1), dtype=dtype)
    blk = 1024
    for r0 in range(0, n0, blk):
        r1 = min(r0 + blk + 1, n0)
        s = slice(r0, r1)
        psi = wrap(np.multiply.outer(sa[s], fb) + np.multiply.outer(ca[s], gb) + (40.0 * x[s])[:, None] + (25.0 * y)[None, :])
        dx[r0:min(r0 + blk, n0)] = np.diff(psi[:blk], axis=1)
        dy[r0:r1 - 1] = np.diff(psi, axis=0)
    w = (0.6 + 0.5 * np.multiply.outer(np.cos(6 * np.pi * x), np.cos(4 * np.pi * y))).astype(dtype)
    return dx, dy, w


say('weighted component solve, kmax %d, resident data; %d timed solves after one warm-up; ms: median of the solves' % (a.kmax, a.reps))
for case in a.cases:
    for shape, dt in CASES[case]:
        name = '%d x %d %s' % (shape + (np.dtype(dt).name,))
        t0 = time.time()
        dx, dy, w = problem(shape, dt)
        plan = _lib.Plan(shape, 1, dt)
        bufs = [_lib.DeviceBuffer(v.nbytes) for v in (dx, dy, w)] + [_lib.DeviceBuffer(w.nbytes)]
        for b, v in zip(bufs, (dx, dy, w)):
            b.upload(v)
        del dx, dy, w
        t_setup = time.time() - t0
        plan.unwrap_prediff_dev(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, kmax=a.kmax)   # warm-up (grows the ring)
        ws = plan.workspace_bytes
        tot, profs, its = [], [], []
        for _ in range(a.reps):
            plan.set_profiling(False)
            plan.timer_start()
            its.append(plan.unwrap_prediff_dev(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, kmax=a.kmax))
            tot.append(plan.timer_stop())
            plan.set_profiling(True)
            plan.unwrap_prediff_dev(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, kmax=a.kmax)
            profs.append(plan.last_kernel_profile())
        plan.set_profiling(False)
        say('%-22s solve %9.3f ms (min %9.3f)  iterations %s  plan workspace %.2f GiB (without the search-direction ring grown by the '
            'solve)  host set-up %.1f s' % (name, float(np.median(tot)), min(tot), sorted(set(its)), ws / 2.0 ** 30, t_setup))
        for k in sorted(profs[0], key=lambda k: -profs[0][k][1]):
            ms = float(np.median([p[k][1] for p in profs]))
            say('    %-26s %3d launches %9.3f ms  (%8.1f us each)' % (k, profs[0][k][0], ms, 1e3 * ms / profs[0][k][0]))
        plan.close()
        for b in bufs:
            b.free()
if a.out:
    with open(a.out, 'a') as f:
        f.write('\n'.join(lines) + '\n')
