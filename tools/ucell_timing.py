#!/usr/bin/env python
"""Timing of unit-cell averaging / expansion on one GPU (f32, hex lattice r_k = 0.02, z = 3, Gaussian-bump u).

    python tools/ucell_timing.py [--sizes 4096 16384] [--reps 5] [--json out.json]

Per size: ms per call (HIP events on the plan's stream, device pointers, no copies) of
  average    lists built + one frame summed (gpa_unit_cell_average_dev)
  sum        one more frame on the same lists: (batch of 4 frames - one frame) / 3 (gpa_unit_cell_average_batch_dev)
  expand     gpa_expand_unitcell_dev onto the full grid
and each one's bytes against the HBM rate (a model: the streams each kernel must move, gathers counted by element);
the base-bin list lengths (median / max) come from the host at the smallest size.  For per-kernel times run it under
rocprofv3 --kernel-trace --stats.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pygpa_amd import _lib  # noqa: E402
from pygpa_amd import unit_cell_averaging as uc  # noqa: E402
from pygpa_amd.synthetic import hex_kvecs, gaussian_bump_displacement  # noqa: E402

HBM_GBS = 8000.0   # MI355X peak HBM3E rate, GB/s


def timed(plan, fn, reps):
    fn()
    plan.sync()
    ts = []
    for _ in range(reps):
        plan.timer_start()
        fn()
        ts.append(plan.timer_stop())
    return float(np.median(ts))


def list_lengths(shape, ks, u, z):
    rmin, (rs0, rs1) = uc.calc_ucell_parameters(ks, z)
    i, j = np.indices(shape, dtype=np.float64)
    R = uc.cart_in_uc(np.stack([i + u[0], j + u[1]], -1), ks, rmin) * z
    b = np.floor(R).astype(np.int64) + 1
    cnt = np.bincount((b[..., 0] * (rs1 + 1) + b[..., 1]).ravel(), minlength=(rs0 + 1) * (rs1 + 1))
    nz = cnt[cnt > 0]
    return int(np.median(nz)), int(nz.max()), int(len(nz))


def run(n, reps, z=3, frames=4):
    shape = (n, n)
    ks = hex_kvecs(0.02, 7.0, 3)[:2]
    u = (0.05 * gaussian_bump_displacement(shape)).astype(np.float32)
    rmin, rsize = uc.calc_ucell_parameters(ks, z)
    geom = _lib.UcellGeom.make(ks, np.linalg.inv(ks), rmin, rsize, z)
    ncell = int(rsize[0]) * int(rsize[1])
    npx = n * n
    plan = _lib.Plan(shape, 1, np.float32)
    img = np.random.default_rng(0).random((frames,) + shape, dtype=np.float32)
    d_img = _lib.DeviceBuffer(img.nbytes, plan.device)
    d_u = _lib.DeviceBuffer(u.nbytes, plan.device)
    d_res = _lib.DeviceBuffer(frames * ncell * 8, plan.device)
    d_out = _lib.DeviceBuffer(npx * 4, plan.device)
    try:
        d_img.upload(img)
        d_u.upload(u)
        t1 = timed(plan, lambda: plan.unit_cell_average_dev(d_img.ptr, geom, d_res.ptr, d_u.ptr), reps)
        tb = timed(plan, lambda: plan.unit_cell_average_dev(d_img.ptr, geom, d_res.ptr, d_u.ptr, nframes=frames),
                   reps) if frames > 1 else None
        res = d_res.download((ncell,), np.float64).reshape(rsize)
        d_cell = _lib.DeviceBuffer(ncell * 8, plan.device)
        d_cell.upload(np.ascontiguousarray(res))
        te = timed(plan, lambda: plan.expand_unitcell_dev(d_cell.ptr, geom, d_out.ptr, 1, d_u.ptr), reps)
        d_cell.free()
    finally:
        for b in (d_img, d_u, d_res, d_out):
            b.free()
        plan.close()
    nkeys = (rsize[0] + 1) * (rsize[1] + 1)
    bits = int(nkeys).bit_length()
    passes = (bits + 3) // 4
    # bytes: key pass (u in, key out); per radix pass (key read for the histogram, key + index in and out); list starts
    # and f64 fractions (key, index, u gathered, two fractions out); sum (index, two fractions, image gathered); the expand
    lists_b = npx * (8 + 4) + passes * npx * (4 + 16) + npx * (4 + 4 + 8 + 16)
    sum_b = npx * (4 + 16 + 4)
    exp_b = npx * (8 + 4)
    sum_ms = (tb - t1) / (frames - 1) if tb is not None else float('nan')
    out = dict(size=n, z=z, rsize=[int(v) for v in rsize], radix_passes=passes, average_ms=t1, sum_ms=sum_ms,
               lists_ms=t1 - sum_ms, expand_ms=te,
               lists_GB=lists_b / 1e9, sum_GB=sum_b / 1e9, expand_GB=exp_b / 1e9,
               lists_hbm_ms=lists_b / HBM_GBS / 1e6, sum_hbm_ms=sum_b / HBM_GBS / 1e6, expand_hbm_ms=exp_b / HBM_GBS / 1e6)
    return out, u


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='+', default=[4096, 16384])
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--json', default=None)
    ap.add_argument('--frames', type=int, default=4, help='frames of the batched call (1: no batched call -- one average '
                    'and one expand per repetition, for a per-call kernel profile)')
    a = ap.parse_args()
    rows = []
    for n in a.sizes:
        r, u = run(n, a.reps, frames=a.frames)
        if n == min(a.sizes) and n <= 4096:     # (host arrays of the whole grid: not at 16384^2)
            r['list_median'], r['list_max'], r['lists_nonempty'] = list_lengths((n, n), hex_kvecs(0.02, 7.0, 3)[:2], u, 3)
        rows.append(r)
        print(json.dumps(r), flush=True)
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
