#!/usr/bin/env python
"""Lawler-Fujita inversion per boundary mode on resident data (gpa_invert_u_mode_dev): prefilter time (fir_rows + fir_cols,
both components) and time of the fixed-point kernel (label invert_kernel) from the library's own per-kernel events
(gpa_set_profiling / gpa_last_kernel_profile), as warm medians.
    python tools/lf_modes_timing.py [--out profiles/lf_modes_timing.txt] [--label TEXT] [--modes nearest constant ...]
Field: gaussian_bump_displacement, invert_u_overlap with edge 0.  Every mode is warmed up; the timed calls of the modes
alternate (mode after mode, round after round), so that drift of the clocks falls on all of them alike.  The yardstick of the
folded modes is 'constant' of the same run: the same kernel shape (one pixel per lane, interior path with 16-byte gathers).
An older build of the library (GPA_HIP_LIB) is measured with --modes nearest constant: rows to hold this build's against."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from pygpa_amd import _lib   # noqa: E402
from pygpa_amd.synthetic import gaussian_bump_displacement   # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--size', type=int, default=4096)
ap.add_argument('--iters', type=int, default=35)
ap.add_argument('--reps', type=int, default=15)
ap.add_argument('--warmup', type=int, default=3)
ap.add_argument('--modes', nargs='+', default=['nearest', 'constant', 'reflect', 'mirror', 'grid-wrap'])
ap.add_argument('--label', default='')
ap.add_argument('--out', default=None, help='append the table to this file as well')
a = ap.parse_args()

# (the codes of gpa_invert_u_mode_dev, passed as such: a build from before the folded modes has no warp_mode_code)
CODES = {'nearest': 0, 'constant': 1, 'reflect': 2, 'mirror': 3, 'grid-wrap': 4}
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def quartiles(v):
    v = np.sort(np.asarray(v))
    return np.median(v), v[len(v) // 4], v[(3 * len(v)) // 4], v[0], v[-1]


n = a.size
shape = (n, n)
say('%s%d^2, %d rounds, invert_u_overlap edge 0, gaussian_bump_displacement; %d warm-up calls per mode, then %d timed rounds over the modes; '
    'ms per call: median (quartiles; min .. max)' % (a.label + ': ' if a.label else '', n, a.iters, a.warmup, a.reps))
for dt, name in ((np.float32, 'f32'), (np.float64, 'f64')):
    s = np.dtype(dt).itemsize
    u = gaussian_bump_displacement(shape).astype(dt)
    plan = _lib.Plan(shape, 1, dt)
    d_u, d_out = _lib.DeviceBuffer(u.nbytes), _lib.DeviceBuffer(u.nbytes)
    d_u.upload(u)

    def call(mode):
        _lib.check(plan.lib.gpa_invert_u_mode_dev(plan.handle, _lib._ptr(int(d_u.ptr)), 1.0, a.iters, 0, 1, CODES[mode], None, 0,
                                                  _lib._ptr(int(d_out.ptr))), 'gpa_invert_u_mode_dev')

    for mode in a.modes:
        for _ in range(a.warmup):
            call(mode)
    plan.sync()
    pre, inv = {m: [] for m in a.modes}, {m: [] for m in a.modes}
    plan.set_profiling(True)
    for _ in range(a.reps):
        for mode in a.modes:
            call(mode)
            prof = plan.last_kernel_profile()
            pre[mode].append(prof['fir_rows_kernel'][1] + prof['fir_cols_kernel'][1])
            inv[mode].append(prof['invert_kernel'][1])
    plan.set_profiling(False)
    base = np.median(inv['constant']) if 'constant' in inv else None
    for mode in a.modes:
        p, k = quartiles(pre[mode]), quartiles(inv[mode])
        say('%s %-9s  prefilter %7.3f (%7.3f .. %7.3f; %7.3f .. %7.3f)   invert_kernel %7.3f (%7.3f .. %7.3f; %7.3f .. %7.3f)%s'
            % ((name, mode) + p + k + ('   = %.3f x constant' % (k[0] / base) if base else '',)))
    plan.close()
    d_u.free()
    d_out.free()
if a.out:
    with open(a.out, 'a') as f:
        f.write('\n'.join(lines) + '\n')
