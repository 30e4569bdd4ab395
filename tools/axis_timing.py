#!/usr/bin/env python
"""Timing of homogenize_per_axis on one GPU: resident gpa_homogenize_per_axis_dev at 4096^2 with sigma = 200, in f32 and f64,
with and without a mask, on a smooth image and on white noise.

    python tools/axis_timing.py [--size 4096] [--sigma 200] [--reps 7] [--cpu-size 4096] [--out profiles/axis_timing.txt]

Per case: ms of one call (HIP events on the plan's stream through gpa_timer_start / stop, device pointers, no copies, taps
already resident; one warm-up call, then the median of --reps), the kernels' times in a separately profiled call, and the HBM
model of DESIGN 2.13 -- the image crosses HBM four times in and twice out, 6 n^2 elements -- against what the measured time
implies.  The smooth image is the hazard the histogram scheme is built for (nearly all keys of a line share their upper bytes);
white noise is the easy case: the two must take comparable time.  Beside them: NumPy / SciPy's time for the same call on this
machine's CPU (the reference's own expression).  There is no pass mark, and nothing on the parent commit to compare with.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_GBS = 8000.0
DTYPES = {'f32': np.float32, 'f64': np.float64}


def inputs(n, kind, seed=0):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[:n, :n].astype(np.float32)
    if kind == 'smooth':     # an illumination field with stripes and a little noise: the keys of a line share two bytes or more
        img = 2000.0 * (0.85 + 0.15 * np.exp(-((x - 0.55 * n) ** 2 + (y - 0.45 * n) ** 2) / (0.5 * n * n)))
        img = img * (1.0 + 0.05 * np.cos(0.37 * x)) * (1.0 + 0.05 * np.sin(0.11 * y)) + rng.standard_normal((n, n)).astype(np.float32)
    else:                    # white noise over fourteen octaves, both signs: every byte of the key is spread out
        img = rng.standard_normal((n, n)) * np.exp2(rng.integers(-7, 8, size=(n, n)))
    mask = ((x - n / 2) ** 2 + (y - n / 2) ** 2) < (0.6 * n) ** 2       # a round field of view that reaches every line
    mask &= rng.random((n, n)) >= 0.05
    return img, mask


def reference(image, sigma, mask):
    """the reference's expression (imagetools.py:112-125) with NumPy and SciPy"""
    import scipy.ndimage as ndi
    res = image.copy()
    for axis in (0, 1):
        src = res if mask is None else np.where(mask, res, np.nan)
        profile = ndi.gaussian_filter(np.nanmedian(src, axis=axis, keepdims=True), sigma=sigma)
        res /= profile / profile.max()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=4096)
    ap.add_argument('--sigma', type=float, default=200.0)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--cpu-size', type=int, default=4096, help='0 skips the CPU reference')
    ap.add_argument('--dtypes', nargs='*', default=['f32', 'f64'])
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'axis_timing.txt'))
    a = ap.parse_args()
    from pygpa_amd import _lib
    import pygpa_amd.imagetools as IT
    n, sigma = a.size, a.sigma
    lines = ['homogenize_per_axis, resident, %d^2, sigma %g (R = %d); model: 6 n^2 elements through HBM at %.0f GB/s'
             % (n, sigma, int(4 * sigma + 0.5), HBM_GBS)]
    for name in a.dtypes:
        dt = DTYPES[name]
        item = np.dtype(dt).itemsize
        model_mb = 6.0 * n * n * item / 1e6
        plan = _lib.Plan((n, n), 1, dt)
        d_in, d_out, d_mask = _lib.DeviceBuffer(n * n * item), _lib.DeviceBuffer(n * n * item), _lib.DeviceBuffer(n * n)
        try:
            for kind in ('smooth', 'noise'):
                img, mask = inputs(n, kind)
                d_in.upload(np.ascontiguousarray(img, dtype=dt))
                d_mask.upload(mask.astype(np.uint8))
                for masked in (False, True):
                    def run():
                        IT.homogenize_per_axis_dev(plan, d_in.ptr, d_mask.ptr if masked else None, d_out.ptr, sigma)
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
                    ms = float(np.median(ts))
                    lines.append('%s %-6s %-7s %.3f ms (median of %d, min %.3f, max %.3f); model %.0f MB = %.3f ms, the time implies %.0f GB/s'
                                 % (name, kind, 'mask' if masked else 'no mask', ms, a.reps, min(ts), max(ts), model_mb,
                                    model_mb / HBM_GBS, model_mb / ms))
                    for k in sorted(prof):
                        lines.append('     %-24s %2d launches  %8.3f ms in the profiled call' % ((k,) + tuple(prof[k])))
        finally:
            for b in (d_in, d_out, d_mask):
                b.free()
            plan.close()
    if a.cpu_size:
        m = a.cpu_size
        for name in a.dtypes:
            img, mask = inputs(m, 'smooth')
            x = np.ascontiguousarray(img, dtype=DTYPES[name])
            for msk in (None, mask):
                t0 = time.perf_counter()
                reference(x, sigma, msk)
                lines.append('CPU (NumPy nanmedian + SciPy gaussian_filter) %s %d^2 %-7s %.1f ms'
                             % (name, m, 'no mask' if msk is None else 'mask', 1e3 * (time.perf_counter() - t0)))
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
