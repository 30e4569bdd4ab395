#!/usr/bin/env python
"""Timing of windowed Fourier filtering on one GPU: 1024^2, sigma = 10 (s = 20, 40 taps), wl, wu = -2, 2 (41 x 41 frequency
pairs), one threshold, f32 and f64.

    python tools/wff_timing.py [--size 1024] [--sigma 10] [--range 2] [--reps 5] [--out profiles/wff_timing.txt]
    python tools/wff_timing.py --cpu-reference [--cpu-size 128]      # the reference's own wff on the CPU, no GPU needed

Per precision: ms of one gpa_wff_dev call (HIP events on the plan's stream through gpa_timer_start / stop, device pointers, no
copies; one warm-up call, then the median of --reps), the three kernels' shares of a separately profiled call (event pairs
around every launch, gpa_set_profiling), and the multiply-add floor of DESIGN 2.11's model at the vector peak: per pixel
Kx (1 + T) 2s complex multiply-adds in the row kernels and Kx Ky (1 + T) 2s in the column kernel (8 flop each), of which the
column kernel really does Kx Ky ((R + 2s - 1) / R + T) 2s -- a tile computes its sf rows' halo again.  The HBM model is printed
beside it: per wx, f in and A out; A in and T planes out; T planes in and T planes of g in and out.

--cpu-reference times pyGPA's own `wff` (imported through oracle.make_golden._import_reference) at --cpu-size with the same
sigma and range.  It is reported as measured at that size, never scaled.
"""
import argparse
import contextlib
import io
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_TF = {'f32': 157.3, 'f64': 78.6}   # MI355X vector peak, TFLOP/s
HBM_GBS = 8000.0
TILE_R = 64                             # rows of a column tile at s = 20 (gpa_wff.h: wff_tile)


def field(n, seed=0):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[:n, :n].astype(np.float64)
    phi = 0.35 * x - 0.2 * y + 2.5 * np.exp(-((x - n / 2) ** 2 + (y - n / 2) ** 2) / (2 * (0.3 * n) ** 2))
    return np.exp(1j * (phi + 0.6 * rng.standard_normal((n, n))))


def model(n, s, K, T, csz):
    W = 2 * s
    rows = K * (1 + T) * W
    cols = K * K * (1 + T) * W
    cols_done = K * K * ((TILE_R + W - 1) / TILE_R + T) * W
    bytes_ = K * n * n * csz * (2 + (1 + T) + (T + (1 if K == 1 else 2) * T))
    return dict(macs_px=rows + cols, macs_px_done=rows + cols_done, flop=8.0 * (rows + cols) * n * n,
                flop_done=8.0 * (rows + cols_done) * n * n, hbm_bytes=bytes_)


def gpu(a, lines):
    from pygpa_amd import _lib
    n, sigma = a.size, a.sigma
    s = round(2 * sigma)
    wi = 1 / sigma
    ws = np.arange(-a.range, a.range + wi / 2, wi)
    scale = wi * wi / (4 * np.pi ** 2)
    img = field(n)
    thr = [0.3 * np.sqrt(np.pi) * sigma]     # ~0.15 of the |sf| = 2 sqrt(pi) sigma of a pure carrier under this window
    for name, dt in (('f32', np.float32), ('f64', np.float64)):
        plan = _lib.Plan((n, n), 1, dt)
        x = np.ascontiguousarray(img, dtype=plan.cdtype)
        d_in, d_out = _lib.DeviceBuffer(x.nbytes), _lib.DeviceBuffer(x.nbytes)
        try:
            d_in.upload(x)

            def run():
                plan.wff_dev(d_in.ptr, d_out.ptr, sigma, ws, ws, thr, scale)
            run()
            plan.sync()
            ts = []
            for _ in range(a.reps):
                plan.timer_start()
                run()
                ts.append(plan.timer_stop())
            plan.set_profiling(True)
            run()
            prof = plan.last_kernel_profile()
            plan.set_profiling(False)
            kept = float((np.abs(d_out.download((n, n), plan.cdtype)) > 0).mean())
        finally:
            d_in.free()
            d_out.free()
            plan.close()
        m = model(n, s, len(ws), 1, x.itemsize)
        ms = float(np.median(ts))
        floor = m['flop'] / (PEAK_TF[name] * 1e12) * 1e3
        lines.append('%s  %d^2  sigma %g (s = %d)  %d x %d pairs  T = 1:  call %.2f ms (median of %d, min %.2f, max %.2f)'
                     % (name, n, sigma, s, len(ws), len(ws), ms, a.reps, min(ts), max(ts)))
        for k in ('wff_rows_kernel', 'wff_cols_kernel', 'wff_rows_acc_kernel'):
            calls, tot = prof.get(k, (0, float('nan')))
            lines.append('     %-20s %4d launches  %9.2f ms in the profiled call' % (k, calls, tot))
        lines.append('     model: %.0f complex multiply-adds per pixel (%.0f with the tiles\' halo rows), %.3f TFLOP -> floor %.2f ms at '
                     '%.1f TFLOP/s (%.1f %% of the vector peak reached; %.1f %% counting the halo work); HBM model %.2f GB -> %.2f ms'
                     % (m['macs_px'], m['macs_px_done'], m['flop'] / 1e12, floor, PEAK_TF[name], 100 * floor / ms,
                        100 * m['flop_done'] / (PEAK_TF[name] * 1e12) * 1e3 / ms, m['hbm_bytes'] / 1e9,
                        m['hbm_bytes'] / HBM_GBS / 1e6))
        lines.append('     output samples that are not zero: %.3f' % kept)


def cpu_reference(a, lines):
    from oracle.make_golden import _import_reference
    GPA, _ = _import_reference()
    n, sigma = a.cpu_size, a.sigma
    img = field(n)
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        GPA.wff(img, sigma, [0.3 * np.sqrt(np.pi) * sigma], -a.range, a.range)
    dt = time.perf_counter() - t0
    nws = len(np.arange(-a.range, a.range + 1 / sigma / 2, 1 / sigma))
    lines.append('reference wff on the CPU (scipy.ndimage.convolve, one process): %d^2, sigma %g, %d x %d pairs, T = 1: %.1f s '
                 '(measured at this size; not scaled)' % (n, sigma, nws, nws, dt))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=1024)
    ap.add_argument('--sigma', type=float, default=10.0)
    ap.add_argument('--range', type=float, default=2.0)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None)
    ap.add_argument('--cpu-reference', action='store_true')
    ap.add_argument('--cpu-size', type=int, default=128)
    a = ap.parse_args()
    lines = []
    (cpu_reference if a.cpu_reference else gpu)(a, lines)
    text = '\n'.join(lines)
    print(text, flush=True)
    if a.out:
        with open(a.out, 'a' if a.cpu_reference else 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
