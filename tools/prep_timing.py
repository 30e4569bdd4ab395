#!/usr/bin/env python
"""Timing of the image preparation on one GPU: resident gauss_homogenize_dev at 4096^2 with sigma = 50 (R = 200), and
generate_mask with r = 20 on a 16-frame stack, in f32 and f64.

    python tools/prep_timing.py [--size 4096] [--sigma 50] [--frames 16] [--r 20] [--reps 5] [--out profiles/prep_timing.txt]
    python tools/prep_timing.py --once f32 [--size ...]      # two homogenisations and nothing else: the target of a counter pass
    python tools/prep_timing.py --pmc DIR [DIR ...] [--out ...]   # per-kernel HBM bytes from rocprofv3 --pmc csv directories
    python tools/prep_timing.py --cpu-reference [--cpu-size 2048]  # SciPy's gaussian_filter and binary_erosion on the CPU, no GPU needed

Per precision: ms of one gpa_gauss_homogenize_dev call (HIP events on the plan's stream through gpa_timer_start / stop, device
pointers, no copies, tables already resident; one warm-up call, then the median of --reps), the kernels' shares of a
separately profiled call, and beside it TWICE the time of the existing gauss_fft_cols_kernel + gauss_fft_rows_kernel pair at the
same sigma and size (read from a profiled gpa_find_peaks_dev call, whose smoothing is exactly that pair): what two separate
gaussian_filter calls would cost before the masking and the division.  Those two kernels are untouched by this feature.
generate_mask: ms of the resident any-equal pass over the stack plus the erosion, and of the mirror's call from host arrays.

The HBM model of DESIGN 2.12 is printed beside the measured time; --pmc turns counter passes (FETCH_SIZE and WRITE_SIZE in
passes of their own) into measured bytes per kernel, 2 x FETCH_SIZE + WRITE_SIZE as on gfx950 a wide streaming read is counted
at half its bytes.  There is no pass mark.
"""
import argparse
import collections
import csv
import glob
import re
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_GBS = 8000.0
PREP_KERNELS = ('prep_cov_cols_kernel', 'prep_cov_rows_kernel', 'prep_cols_kernel', 'prep_rows_kernel')
DTYPES = {'f32': np.float32, 'f64': np.float64}


def inputs(n, seed=0):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[:n, :n].astype(np.float32)
    img = 500.0 + 3500.0 * np.exp(-((x - 0.6 * n) ** 2 + (y - 0.4 * n) ** 2) / (2 * (0.8 * n) ** 2)) * (0.8 + 0.2 * np.cos(0.7 * x))
    mask = ((x - n / 2) ** 2 + (y - n / 2) ** 2) < (0.42 * n) ** 2       # a round field of view; the corners are out of reach
    img[(rng.random((n, n)) < 0.01) & ~mask] = np.nan
    return img, mask


def model_bytes(n, rsz, L0, S0, L1, S1, vv):
    """bytes of one homogenisation.  The column pass reads image + mask L0 / S0 times over (the overlap of the
    segments) and writes two planes; the row pass reads them L1 / S1 times over, the coverage and the image once, and
    writes out (and VV); the coverage reads the mask about three times (the running count enters and leaves every sample
    once, the first row of a chunk reads its whole interval) and passes one byte plane through HBM."""
    px = float(n) * n
    cols = px * ((rsz + 1) * L0 / S0 + 2 * rsz)
    rows = px * (2 * rsz * L1 / S1 + 1 + rsz + rsz * (2 if vv else 1))
    cov = px * (3 + 1 + 1 + 1)
    return cols, rows, cov


def homogenize(a, lines):
    from pygpa_amd import _lib
    import pygpa_amd.imagetools as IT
    n, sigma = a.size, a.sigma
    R = int(4 * sigma + 0.5)
    img, mask = inputs(n)
    for name in a.dtypes:
        dt = DTYPES[name]
        plan = _lib.Plan((n, n), 1, dt)
        x = np.ascontiguousarray(img, dtype=dt)
        m8 = mask.astype(np.uint8)
        d_in, d_out, d_mask = _lib.DeviceBuffer(x.nbytes), _lib.DeviceBuffer(x.nbytes), _lib.DeviceBuffer(m8.nbytes)
        try:
            d_in.upload(x)
            d_mask.upload(m8)

            def run():
                IT.gauss_homogenize_dev(plan, d_in.ptr, d_mask.ptr, d_out.ptr, sigma)
            run()
            plan.sync()
            if a.once:
                run()
                plan.sync()
                continue
            ts = []
            for _ in range(a.reps):
                plan.timer_start()
                run()
                ts.append(plan.timer_stop())
            plan.set_profiling(True)
            run()
            prof = plan.last_kernel_profile()
            # the existing pair at the same sigma: the smoothing of find_peaks
            plan.find_peaks_dev(d_in.ptr, sigma, 0.0, 0.5)
            pair = plan.last_kernel_profile()
            plan.set_profiling(False)
            out = d_out.download((n, n), dt)
        finally:
            d_in.free()
            d_out.free()
            d_mask.free()
            plan.close()
        if a.once:
            continue
        ms = float(np.median(ts))
        lines.append('%s  %d^2  sigma %g (R = %d)  gauss_homogenize_dev: %.3f ms (median of %d, min %.3f, max %.3f); NaN in out: %.3f'
                     % (name, n, sigma, R, ms, a.reps, min(ts), max(ts), float(np.isnan(out).mean())))
        for k in sorted(prof):
            lines.append('     %-26s %3d launches  %8.3f ms in the profiled call' % ((k,) + tuple(prof[k])))
        gc, gr = pair.get('gauss_fft_cols_kernel', (0, float('nan'))), pair.get('gauss_fft_rows_kernel', (0, float('nan')))
        lines.append('     existing pair at this sigma: gauss_fft_cols_kernel %.3f ms + gauss_fft_rows_kernel %.3f ms; twice the pair '
                     '(num and den as two gaussian_filter calls, no masking, no division): %.3f ms' % (gc[1], gr[1], 2 * (gc[1] + gr[1])))
        # gaussfft_choose_lg picks the cheapest segment length L >= 4 R (up to 2^14 in f32, 2^13 in f64): the model for each
        for Lk in [1 << k for k in range(6, {4: 14, 8: 13}[x.itemsize] + 1) if (1 << k) >= 4 * R]:
            S = Lk - 2 * R
            c, r, v = model_bytes(n, x.itemsize, Lk, S, Lk, S, False)
            lines.append('     HBM model with segments of %5d (%5d kept): column pass %.0f MB, row pass %.0f MB, coverage %.0f MB, '
                         'total %.0f MB -> %.3f ms at %.0f GB/s' % (Lk, S, c / 1e6, r / 1e6, v / 1e6, (c + r + v) / 1e6,
                                                                    (c + r + v) / HBM_GBS / 1e6, HBM_GBS))


def masks(a, lines):
    from pygpa_amd import _lib
    import pygpa_amd.imagetools as IT
    n, B, r = a.size, a.frames, a.r
    rng = np.random.default_rng(1)
    for name in a.dtypes:
        dt = DTYPES[name]
        frames = rng.integers(100, 4000, size=(B, n, n)).astype(dt)
        frames[:, :n // 16, :] = 0                       # a dead band
        frames[rng.integers(0, B, 64), rng.integers(n // 4, n // 2, 64), rng.integers(0, n, 64)] = 0   # and dead pixels
        plan = _lib.get_plan((n, n), 1, dt)
        d_frames, d_hit = _lib.DeviceBuffer(frames.nbytes), _lib.DeviceBuffer(n * n)
        try:
            d_frames.upload(frames)

            def run():
                plan.mask_any_equal_dev(d_frames.ptr, B, 0.0, d_hit.ptr)
                plan.mask_erode_disk_dev(d_hit.ptr, d_hit.ptr, r, invert=True)
            run()
            plan.sync()
            ts = []
            for _ in range(a.reps):
                plan.timer_start()
                run()
                ts.append(plan.timer_stop())
            kept = float(d_hit.download((n, n), np.uint8).mean())
        finally:
            d_frames.free()
            d_hit.free()
        import time
        t0 = time.perf_counter()
        m = IT.generate_mask(frames, 0.0, r, dtype=dt)
        host = time.perf_counter() - t0
        assert abs(m.mean() - kept) < 1e-12
        lines.append('%s  %d frames of %d^2, r = %d: any-equal + erosion resident %.3f ms (median of %d, min %.3f, max %.3f; the stack is '
                     '%.0f MB -> %.3f ms at %.0f GB/s); generate_mask from host arrays %.0f ms; kept %.3f'
                     % (name, B, n, r, float(np.median(ts)), a.reps, min(ts), max(ts), frames.nbytes / 1e6,
                        frames.nbytes / HBM_GBS / 1e6, HBM_GBS, 1e3 * host, kept))
        del frames


def pmc(dirs, lines):
    acc = collections.defaultdict(lambda: collections.defaultdict(list))
    for d in dirs:
        for f in glob.glob(os.path.join(d, '**', '*counter_collection.csv'), recursive=True):
            for row in csv.DictReader(open(f)):
                name = row['Kernel_Name']
                short = next((k for k in PREP_KERNELS if re.search(r'\b%s\b' % (k[5:] if 'cov' in k else k), name)), None)
                if short:
                    short += '<double>' if 'double' in name else '<float>' if 'float' in name else ''
                    acc[short][row['Counter_Name']].append(float(row['Counter_Value']))
    lines.append('HBM bytes per launch from counter passes (FETCH_SIZE and WRITE_SIZE in passes of their own; 2 x FETCH_SIZE + WRITE_SIZE):')
    total = collections.defaultdict(float)
    for k in sorted(acc):
        c = acc[k]
        if 'FETCH_SIZE' in c and 'WRITE_SIZE' in c:
            f, w = np.mean(c['FETCH_SIZE']) * 1024, np.mean(c['WRITE_SIZE']) * 1024
            lines.append('%-34s FETCH_SIZE %8.1f MB (x 2 = %8.1f MB)  WRITE_SIZE %8.1f MB  ->  %8.1f MB per launch (n = %d)'
                         % (k, f / 1e6, 2 * f / 1e6, w / 1e6, (2 * f + w) / 1e6, len(c['FETCH_SIZE'])))
            total['double' if 'double' in k else 'float' if 'float' in k else 'bytes'] += 2 * f + w
    for k, v in total.items():
        lines.append('sum of the %s kernels: %.1f MB' % (k, v / 1e6))


def cpu_reference(a, lines):
    """SciPy on the host, one process: what the reference's imagetools spends (measured at the sizes named, never scaled)"""
    import time
    import scipy.ndimage as ndi
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import prep_cases as pc
    img, mask = inputs(a.cpu_size)
    x = np.where(mask, img, 0).astype(np.float64)
    t0 = time.perf_counter()
    ndi.gaussian_filter(x, sigma=a.sigma)
    t1 = time.perf_counter()
    lines.append('scipy.ndimage.gaussian_filter on the CPU, %d^2 float64, sigma %g: %.2f s (gauss_homogenize2 calls it twice)'
                 % (a.cpu_size, a.sigma, t1 - t0))
    m = np.ones((a.cpu_size // 2, a.cpu_size // 2), dtype=bool)
    m[::97, ::89] = False
    t0 = time.perf_counter()
    ndi.binary_erosion(m, structure=pc.disk(a.r))
    t1 = time.perf_counter()
    lines.append('scipy.ndimage.binary_erosion with disk(%d) on the CPU, %d^2: %.2f s' % (a.r, a.cpu_size // 2, t1 - t0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=4096)
    ap.add_argument('--sigma', type=float, default=50.0)
    ap.add_argument('--frames', type=int, default=16)
    ap.add_argument('--r', type=int, default=20)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--once', default=None, choices=list(DTYPES))
    ap.add_argument('--pmc', nargs='*', default=None)
    ap.add_argument('--cpu-reference', action='store_true')
    ap.add_argument('--cpu-size', type=int, default=2048)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    a.dtypes = [a.once] if a.once else list(DTYPES)
    lines = []
    if a.cpu_reference:
        cpu_reference(a, lines)
    elif a.pmc is not None:
        pmc(a.pmc, lines)
    else:
        homogenize(a, lines)
        if not a.once:
            masks(a, lines)
    text = '\n'.join(lines)
    print(text, flush=True)
    if a.out and lines:
        with open(a.out, 'a' if (a.pmc is not None or a.cpu_reference) else 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
