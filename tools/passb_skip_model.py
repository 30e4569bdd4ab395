#!/usr/bin/env python
"""NumPy (f64) model of the row-wise skip test of the shared pass B (gpa_passb_shared.hip).

For every peak the candidates are visited in the kernel's order (visiting_order: the library's own rule through
gpa_passb_visiting_order; visiting_order_numpy is its transcription, tests/test_passb_skip_host.py holds the two to each other).  For a row x and a candidate c = (wx, wy)

    B_c = (1 / n1) sum_k |X_k| |h_c(k)|,   X = FFT_y of the x-plane's row,   h_c(k) = sum_m g(m) cos(2 pi (wy + k / n1) m)

bounds the circular part of the candidate's lock-in at every pixel of the row; the pair (row, candidate) is skippable when
1.001 B_c <= min_j |best(j)| with the running best of the candidates visited before it.  The model leaves out the Hankel end
correction and f32 rounding.  magnitude='l1' uses |Re X_k| + |Im X_k| (what the f64 kernel forms; the f32
kernel forms |X_k| with a square root) instead of |X_k|.

    python tools/passb_skip_model.py [--size 2048] [--rows 256] [--seed 100] [--kgrid 4x4]

prints the skippable share of the (row, later candidate) pairs for both magnitudes and the share that wins nowhere (the ceiling
of any row-wise test), on the benchmark's image (hex_moire, noise 0.1)."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))


def gaussian_kspace_1d(n, sigma):
    f = np.fft.fftfreq(n)
    e = 2.0 * np.pi ** 2 * sigma ** 2 * f * f
    return np.where(e > 50.0, 0.0, np.exp(-e))


def visiting_order(klist, kref):
    """the order the kernel visits `klist` in, from the library itself (gpa_passb_visiting_order: host only, needs no GPU)"""
    from pygpa_amd import _lib
    return _lib.passb_visiting_order(klist, kref)


def visiting_order_numpy(klist, kref):
    """positions of `klist` in the order the kernel visits them: x-planes (distinct wx, in order of first appearance) kept
    together and ordered by their nearest candidate (ties: first list position), candidates of a plane by distance to kref
    (stable); a list with two different k-vectors equal modulo whole cycles keeps its own order"""
    klist = np.asarray(klist, dtype=np.float64).reshape(-1, 2)
    K = len(klist)
    frac = klist - np.floor(klist)
    for a in range(K):
        for b in range(a + 1, K):
            if not np.array_equal(klist[a], klist[b]) and np.array_equal(frac[a], frac[b]):
                return list(range(K))
    planes = {}
    planeof = [planes.setdefault(float(k[0]), len(planes)) for k in klist]
    d2 = ((klist - np.asarray(kref, dtype=np.float64)) ** 2).sum(axis=1)
    pmin = [min(d2[k] for k in range(K) if planeof[k] == pl) for pl in range(len(planes))]
    pfirst = [min(k for k in range(K) if planeof[k] == pl) for pl in range(len(planes))]
    return sorted(range(K), key=lambda k: (pmin[planeof[k]], pfirst[planeof[k]], d2[k], k))


def skip_model(img0, klist, kref, sigma, magnitude='abs', margin=1.001):
    """-> dict: order (list positions in visiting order), skipped / wins [n0][K] booleans in visiting order, amp [K][n0][n1]
    |lock-in| of every candidate in LIST order (the circular filter, as the reference computes it)"""
    img0 = np.asarray(img0, dtype=np.float64)
    klist = np.asarray(klist, dtype=np.float64).reshape(-1, 2)
    n0, n1 = img0.shape
    K = len(klist)
    g0, g1 = gaussian_kspace_1d(n0, sigma), gaussian_kspace_1d(n1, sigma)
    taps = np.fft.ifft(g1).real                     # g(m mod n1), even
    lags = np.fft.fftfreq(n1, 1.0 / n1)             # signed lag of every index
    keep = np.abs(lags) <= 12 * sigma + 1           # (beyond: < exp(-72) of the centre tap)
    taps, lags = taps[keep], lags[keep]
    x, y = np.arange(n0)[:, None], np.arange(n1)
    order = visiting_order(klist, kref)
    planes, amp = {}, np.empty((K, n0, n1))
    bound = np.empty((K, n0))
    for k in range(K):
        wx, wy = klist[k]
        if wx not in planes:
            T = np.fft.ifft(g0[:, None] * np.fft.fft(img0 * np.exp(2j * np.pi * wx * x), axis=0), axis=0)
            X = np.fft.fft(T, axis=1)
            mag = np.abs(X) if magnitude == 'abs' else np.abs(X.real) + np.abs(X.imag)
            planes[wx] = (T, mag)
        T, mag = planes[wx]
        amp[k] = np.abs(np.fft.ifft(g1 * np.fft.fft(T * np.exp(2j * np.pi * wy * y), axis=1), axis=1))
        h = (taps[None, :] * np.cos(2 * np.pi * (wy + (np.arange(n1) / n1))[:, None] * lags[None, :])).sum(axis=1)
        bound[k] = (mag * np.abs(h)).sum(axis=1) / n1
    best = np.zeros((n0, n1))
    skipped, wins = np.zeros((n0, K), bool), np.zeros((n0, K), bool)
    for pos, k in enumerate(order):
        take = amp[k] > best
        wins[:, pos] = take.any(axis=1)
        if pos > 0:
            skipped[:, pos] = margin * bound[k] <= best.min(axis=1)
        best = np.where(take, amp[k], best)
    return {'order': order, 'skipped': skipped, 'wins': wins, 'amp': amp}


def main():
    from pygpa_amd.synthetic import hex_kvecs, explicit_klists, gaussian_bump_displacement, hex_moire
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=2048)
    ap.add_argument('--rows', type=int, default=256, help='rows of the image that are modelled (the first ones)')
    ap.add_argument('--seed', type=int, default=100)
    ap.add_argument('--kgrid', default='4x4')
    a = ap.parse_args()
    knx, kny = (int(v) for v in a.kgrid.split('x'))
    kvecs = hex_kvecs(0.1, 7.0)
    sigma = int(np.ceil(1 / np.linalg.norm(kvecs, axis=1).min()))
    kw = np.linalg.norm(kvecs, axis=1).mean() / 2.5
    klists = explicit_klists(kvecs, kw, knx, kny)
    n = a.size
    img = hex_moire((n, n), kvecs, gaussian_bump_displacement((n, n)), noise=0.1, seed=a.seed)
    img0 = img - img.mean()
    # (the x-filter is circular over all rows: model whole columns, report the first --rows rows)
    rows = slice(0, min(a.rows, n))
    tot = {'abs': 0, 'l1': 0, 'nowin': 0, 'pairs': 0}
    for p in range(3):
        for mag in ('abs', 'l1'):
            m = skip_model(img0, klists[p], kvecs[p], sigma, magnitude=mag)
            assert not (m['skipped'] & m['wins']).any(), 'a skipped pair wins somewhere'
            tot[mag] += int(m['skipped'][rows].sum())
        tot['nowin'] += int((~m['wins'][rows, 1:]).sum())
        tot['pairs'] += m['wins'][rows, 1:].size
    print('%d^2 seed %d grid %s, rows %d: skippable share of (row, later candidate) pairs  |X| %.3f   |Re|+|Im| %.3f   win nowhere %.3f'
          % (n, a.seed, a.kgrid, rows.stop, tot['abs'] / tot['pairs'], tot['l1'] / tot['pairs'], tot['nowin'] / tot['pairs']))


if __name__ == '__main__':
    main()
