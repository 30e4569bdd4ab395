"""Undistorting a stack of frames: one stack call against the loop of single-image calls a user writes without it.

Resident on one GPU (frames, fields and results stay in device buffers), timed with HIP events on the plan's stream
(Plan.timer_start / timer_stop: the second event is synchronised on), profiling off.  Legs per shape:
    loop, shared      B x undistort_image_dev(frame b, u, scale)           -- every call uploads nothing, but prefilters and
                                                                              inverts u again
    loop, per frame   B x undistort_image_dev(frame b, u[b], scale)
    stack, shared     undistort_image_batch_dev(frames, u)                  -- one inversion, B gathers sharing the weights
    stack, per frame  undistort_image_batch_dev(frames, u, per_frame=True)  -- B inversions in one set of launches
All legs are warmed up, then alternate leg by leg within each repetition; median, quartiles and extremes per leg.  Before
the timing the stack results are compared with the loop's, bit for bit, at the timed size.
The loop legs use only entry points that exist without the stack call, so the same script times a library that lacks it
(GPA_HIP_LIB=<its libgpa_hip.so>; the stack legs are skipped there): the loop measured with the parent commit's library is
the behaviour the stack call is compared with.

    python tools/undistort_stack_timing.py [--cases 64x512:f32,16x2048:f32,64x512:f64] [--reps 30] [--label TEXT]
                                           [--out profiles/undistort_stack_timing.txt]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STACK_SYMBOLS = ('gpa_undistort_image_batch_dev', 'gpa_undistort_image_batch')


def stats(ts):
    a = np.sort(np.asarray(ts))
    q = lambda f: float(a[int(round(f * (len(a) - 1)))])   # noqa: E731
    return {'n': len(a), 'median_ms': q(0.5), 'q25_ms': q(0.25), 'q75_ms': q(0.75), 'min_ms': float(a[0]), 'max_ms': float(a[-1])}


def fmt(name, s):
    return '  %-18s n=%-3d median %8.3f ms   quartiles %8.3f .. %8.3f   min %8.3f  max %8.3f' % (
        name, s['n'], s['median_ms'], s['q25_ms'], s['q75_ms'], s['min_ms'], s['max_ms'])


def run_case(_lib, B, n, dt, reps, warmup, have_stack):
    from pygpa_amd.synthetic import hex_kvecs, gaussian_bump_displacement, hex_moire
    shape, npx, item = (n, n), n * n, np.dtype(dt).itemsize
    rng = np.random.default_rng(5)
    base = hex_moire(shape, hex_kvecs(0.1, 7.0), noise=0.0)
    frames = np.stack([base + 0.1 * rng.standard_normal(shape) for _ in range(B)]).astype(dt)
    u0 = gaussian_bump_displacement(shape)               # the benchmark's field: |u| up to n / 26 px
    us = np.stack([(1.0 + 0.02 * b) * u0 for b in range(B)]).astype(dt)
    plan = _lib.Plan(shape, 1, dt, device=0)
    d = {k: _lib.DeviceBuffer(m * npx * item) for k, m in (('fr', B), ('u', 2 * B), ('rec', B), ('uinv', 2 * B), ('ref', B))}
    d['fr'].upload(frames)
    d['u'].upload(us)

    def loop(per_frame, out='rec'):
        for b in range(B):
            plan.undistort_image_dev(d['fr'].ptr + b * npx * item, d['u'].ptr + (2 * b * npx * item if per_frame else 0),
                                     d[out].ptr + b * npx * item, uinv_ptr=d['uinv'].ptr, scale=1.0)

    def stack(per_frame):
        plan.undistort_image_batch_dev(d['fr'].ptr, B, d['u'].ptr, d['rec'].ptr, per_frame=per_frame, scale=1.0, uinv_ptr=d['uinv'].ptr)

    legs = [('loop, shared', lambda: loop(False)), ('loop, per frame', lambda: loop(True))]
    lines = ['%d frames of %d^2 %s' % (B, n, np.dtype(dt).name)]
    if have_stack:
        legs += [('stack, shared', lambda: stack(False)), ('stack, per frame', lambda: stack(True))]
        for per_frame in (False, True):
            loop(per_frame, 'ref')
            stack(per_frame)
            plan.sync()
            same = np.array_equal(d['ref'].download((B,) + shape, dt), d['rec'].download((B,) + shape, dt), equal_nan=True)
            lines.append('  stack == loop bit for bit (%s): %s' % ('per frame' if per_frame else 'shared', same))
    for _ in range(warmup):
        for _, f in legs:
            f()
    plan.sync()
    times = {name: [] for name, _ in legs}
    for _ in range(reps):
        for name, f in legs:
            plan.timer_start()
            f()
            times[name].append(plan.timer_stop())
    res = {name: stats(ts) for name, ts in times.items()}
    lines += [fmt(name, res[name]) for name, _ in legs]
    if have_stack:
        for kind in ('shared', 'per frame'):
            lines.append('  median loop / median stack, %-9s = %.2f' % (kind, res['loop, ' + kind]['median_ms'] / res['stack, ' + kind]['median_ms']))
    plan.close()
    for b in d.values():
        b.free()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='64x512:f32,16x2048:f32,64x512:f64')
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--label', default='', help='what to call the library in the report')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'undistort_stack_timing.txt'))
    a = ap.parse_args()
    from pygpa_amd import _lib
    import ctypes
    have_stack = hasattr(ctypes.CDLL(_lib.LIB_PATH), STACK_SYMBOLS[0])
    if not have_stack:          # a library from before the stack call: bind what it has
        for name in STACK_SYMBOLS:
            _lib.SIGNATURES.pop(name, None)
    lines = ['library: %s%s' % (a.label or _lib.LIB_PATH, '' if have_stack else '   (no stack call: loop legs only)')]
    for case in a.cases.split(','):
        bn, dt = case.split(':')
        B, n = (int(v) for v in bn.split('x'))
        lines += run_case(_lib, B, n, {'f32': np.float32, 'f64': np.float64}[dt], a.reps, a.warmup, have_stack)
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'a') as f:
        f.write(text)


if __name__ == '__main__':
    main()
