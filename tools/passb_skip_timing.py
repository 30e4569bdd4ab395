#!/usr/bin/env python
"""Pass B's HIP-event time in the fused driver (profiling on) and the (row, candidate) pairs its spectral bound skipped
(DESIGN 2.1b), on the benchmark's image and on the image where nothing can be skipped:

    python tools/passb_skip_timing.py [--size 4096] [--dtype f32] [--image moire|bands] [--kgrid 4x4] [--reps 6]
    GPA_NO_PB_SKIP=1 python tools/passb_skip_timing.py ...        # every candidate runs

moire: hex_moire, seed 100, noise 0.1 (bench.py's image).  bands: vertical bands of columns, band j carrying candidate j of
every peak at equal amplitude -- every candidate wins somewhere on every row, so the test costs its instructions and saves
nothing.  One line per call; the numbers of a comparison belong to one GPU and one visit (profiles/passB_skip.txt)."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from pygpa_amd import _lib   # noqa: E402
from pygpa_amd.synthetic import hex_kvecs, explicit_klists, gaussian_bump_displacement, hex_moire   # noqa: E402


def bands_image(shape, klists):
    x = np.arange(shape[0], dtype=np.float64)[:, None]
    y = np.arange(shape[1], dtype=np.float64)[None, :]
    img = np.zeros(shape)
    K = len(klists[0])
    for kl in klists:
        for j, k in enumerate(kl):
            sl = slice(j * shape[1] // K, (j + 1) * shape[1] // K)
            img[:, sl] += np.cos(2 * np.pi * (k[0] * x + k[1] * y[:, sl]))
    return img


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=4096)
    ap.add_argument('--dtype', default='f32', choices=['f32', 'f64'])
    ap.add_argument('--image', default='moire', choices=['moire', 'bands'])
    ap.add_argument('--kgrid', default='4x4')
    ap.add_argument('--reps', type=int, default=6)
    a = ap.parse_args()
    dt = np.float32 if a.dtype == 'f32' else np.float64
    knx, kny = (int(v) for v in a.kgrid.split('x'))
    kvecs = hex_kvecs(0.1, 7.0)
    sigma = int(np.ceil(1 / np.linalg.norm(kvecs, axis=1).min()))
    kw = np.linalg.norm(kvecs, axis=1).mean() / 2.5
    klists = np.stack(explicit_klists(kvecs, kw, knx, kny))
    shape = (a.size, a.size)
    if a.image == 'moire':
        img = hex_moire(shape, kvecs, gaussian_bump_displacement(shape), noise=0.1, seed=100, dtype=dt)
    else:
        img = bands_image(shape, klists).astype(dt)
    plan = _lib.Plan(shape, 3 * knx * kny, dt)
    plan.set_profiling(True)
    ms = []
    for _ in range(a.reps):
        plan.extract_displacement_field(img, kvecs, klists, sigma, 2 * sigma, kmax=10, want_kidx=True)
        ms.append(plan.last_kernel_profile()['passB_shared_kernel'][1])
    skipped, visited = plan.last_passb_skips()
    plan.close()
    print('%d^2 %s %s %s NO_PB_SKIP=%s: pass B min %.4f median %.4f ms, skipped %d of %d candidate rows (%.1f %%)'
          % (a.size, a.dtype, a.kgrid, a.image, _lib.get_option('NO_PB_SKIP'), min(ms), float(np.median(ms)), skipped, visited,
             100.0 * skipped / max(visited, 1)))


if __name__ == '__main__':
    main()
