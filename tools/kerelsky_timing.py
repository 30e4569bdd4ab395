#!/usr/bin/env python
"""Timing of the per-pixel Kerelsky fits on one GPU: resident gpa_kerelsky_fit_dev at 4096^2 and 1024^2, in f32 and f64, on a
smooth J field and on a rough one (noise on A larger than the signal: many pixels without a root, further starts, divergence).

    python tools/kerelsky_timing.py [--sizes 4096 1024] [--reps 5] [--cpu-pixels 1024] [--out profiles/kerelsky_timing.txt]

Per case: ms of one call (HIP events on a plan's stream through gpa_timer_start / stop, device pointers, no copies; one warm-up
call, then the median of --reps) and ns per pixel, beside the byte model -- J in and X out, 8 elements per pixel, 32 B in f32 --
at 8000 GB/s.  The field is a 1024^2 tile repeated.  Trial evaluations per pixel, their mean and the mean and largest of the
per-wave maximum (64 consecutive pixels: what a wave executes), are counted by the same solver compiled for the host
(tests/host/kerelsky_check.cpp) on a 256^2 crop of the tile; the device runs the same state machine, so up to the maths libraries
these are its counts.  Beside them: SciPy's per-pixel fit as the reference runs it (bounded least_squares, numerical Jacobian,
second start above a cost of 1e-5) on --cpu-pixels pixels of the same fields on this machine's CPU, as measured, not scaled.
There is no pass mark, and nothing on the parent commit to compare with.
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import kerelsky_cases as kc  # noqa: E402

HBM_GBS = 8000.0
DTYPES = {'f32': np.float32, 'f64': np.float64}
TILE = 1024
NOISE = {'smooth': 1e-4, 'rough': 0.03}


def tile_inputs(kind, n=TILE, seed=3):
    """J (n, n, 2, 2), A0 and the start of a field like the fixtures': smooth theta, psi, eps, xi, A = model + noise"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:n, :n] / n
    x = np.empty((n, n, 4))
    x[..., 0] = 1.15 + 0.8 * np.sin(2.1 * xx + 0.3) * np.cos(1.7 * yy)
    x[..., 1] = 25 + 30 * np.sin(1.3 * yy - 0.5 * xx)
    x[..., 2] = 0.004 + 0.0035 * np.cos(2.5 * xx + 1.1 * yy)
    x[..., 3] = 12 + 4 * np.cos(1.9 * xx) * np.sin(2.3 * yy + 0.4)
    A = kc.model(x) + NOISE[kind] * rng.standard_normal((n, n, 2, 2))
    A0 = kc.a0_and_start(kc.kvecs_of(kc.GLOBAL_X), kc.NMPERPIXEL, kc.A_0)[0]
    return np.linalg.solve(A0, A - A0), A0, np.array(kc.GLOBAL_X)


def scipy_fit(A, refest):
    """the reference's worker (property_extract.py:863-883) on one pixel, with the restated model"""
    from scipy.optimize import least_squares
    bounds = np.full((2, 4), np.inf)
    bounds[0, :] = -np.inf
    bounds[0, [0, 2]] = 0

    def f(x):
        return ((kc.model(x) - A) * 1000).ravel()
    res = least_squares(f, refest, bounds=bounds, max_nfev=50)
    if res.cost > 1e-5:
        res2 = least_squares(f, refest + np.array([0, 90, 0, 0]), bounds=bounds, max_nfev=50)
        if res2.cost < res.cost:
            res = res2
    return res.x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='*', default=[4096, 1024])
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--cpu-pixels', type=int, default=1024, help='0 skips SciPy')
    ap.add_argument('--dtypes', nargs='*', default=['f32', 'f64'])
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'kerelsky_timing.txt'))
    a = ap.parse_args()
    from pygpa_amd import _lib
    lines = ['Kerelsky fits, resident gpa_kerelsky_fit_dev, max_nfev 50, retry_cost 1e-5; byte model: 8 elements per pixel at %.0f GB/s' % HBM_GBS]
    tmp = tempfile.mkdtemp()
    r, exe = kc.build_check(tmp, ['-O2'])
    if r.returncode != 0:
        raise RuntimeError(r.stderr)
    fields = {}
    for kind in NOISE:
        J, A0, x0 = tile_inputs(kind)
        fields[kind] = (J, A0, x0)
        crop = np.ascontiguousarray(J[:256, :256]).reshape(-1, 2, 2)
        X, cost, nfev = kc.host_solve(exe, tmp, crop, x0, a0=A0)
        wave = nfev.reshape(-1, 64).max(axis=1)
        lines.append('%-6s trial evaluations per pixel (host-compiled solver, 256^2 crop): mean %.2f, max %d; per wave of 64: mean of the maximum %.2f, '
                     'largest %d; %.1f %% of the pixels end above cost 1e-5' % (kind, nfev.mean(), nfev.max(), wave.mean(), wave.max(), 100 * (cost > 1e-5).mean()))
    plan = _lib.Plan((64, 64), 1, np.float64)      # for its stream and timer only
    try:
        for n in a.sizes:
            for name in a.dtypes:
                dt = DTYPES[name]
                item = np.dtype(dt).itemsize
                d_J, d_X = _lib.DeviceBuffer(4 * n * n * item), _lib.DeviceBuffer(4 * n * n * item)
                try:
                    for kind, (J, A0, x0) in fields.items():
                        reps = (n + TILE - 1) // TILE
                        d_J.upload(np.ascontiguousarray(np.tile(J.astype(dt), (reps, reps, 1, 1))[:n, :n]))

                        def run():
                            _lib.kerelsky_fit_dev(d_J.ptr, n * n, x0, d_X.ptr, a0=A0, dtype=dt, stream=plan.stream())
                        run()
                        plan.sync()
                        ts = []
                        for _ in range(a.reps):
                            plan.timer_start()
                            run()
                            ts.append(plan.timer_stop())
                        ms = float(np.median(ts))
                        model_mb = 8.0 * n * n * item / 1e6
                        lines.append('%s %5d^2 %-6s %9.3f ms (median of %d, min %.3f, max %.3f) = %.3f ns per pixel; byte model %.0f MB = %.3f ms: %.0f x the model'
                                     % (name, n, kind, ms, a.reps, min(ts), max(ts), 1e6 * ms / (n * n), model_mb, model_mb / HBM_GBS, ms / (model_mb / HBM_GBS)))
                finally:
                    d_J.free()
                    d_X.free()
    finally:
        plan.close()
    if a.cpu_pixels:
        for kind, (J, A0, x0) in fields.items():
            A = kc.form_A(A0, J[:1, :a.cpu_pixels]).reshape(-1, 2, 2)
            t0 = time.perf_counter()
            for m in A:
                scipy_fit(m, x0)
            dt_s = time.perf_counter() - t0
            lines.append('CPU (scipy.optimize.least_squares per pixel, one core) %-6s %d pixels: %.2f s = %.2f ms per pixel' % (kind, len(A), dt_s, 1e3 * dt_s / len(A)))
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
