#!/usr/bin/env python
"""Fixtures of windowed Fourier filtering: runs the reference's own `wff` (pyGPA/geometric_phase_analysis.py:551-580, imported
through oracle.make_golden._import_reference) on the cases of tests/wff_cases.py and writes tests/golden/wff_*.npz.

    python tools/make_wff_golden.py [--only NAME ...]

Data only: the input, sigma, wl, wu, the frequency-list length, the thresholds, the reference's output, and the numbers that
rule out a flipped keep / drop decision -- per threshold the smallest distance of any |sf| sample to it, and the largest
|sf_complex64 - sf_complex128| of the case.  A flipped sample changes the output over a whole 2 s x 2 s neighbourhood, so the
thresholds are CHOSEN: each sits at the centre of the widest gap of the sorted |sf| within +-2000 ranks of its quantile (0.5,
0.9), and the generator asserts half-gap >= 32 x the complex64 error (tests/test_wff_host.py asserts it again from the file).
It also prints, per case, the deviation of the restatement run in complex64: the number behind wff_cases.F32_MEASURED.
"""
import argparse
import contextlib
import io
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import wff_cases as wc  # noqa: E402

QUANTILES = (0.5, 0.9)
RANKS = 2000
MARGIN = 32.0


def choose_thresholds(mags):
    """per quantile: (threshold, half-gap), the centre of the widest gap of the sorted magnitudes near its rank"""
    v = np.sort(mags)
    out = []
    for q in QUANTILES:
        r = int(q * (len(v) - 1))
        lo, hi = max(r - RANKS, 0), min(r + RANKS, len(v) - 1)
        gaps = np.diff(v[lo:hi + 1])
        i = int(np.argmax(gaps))
        out.append((0.5 * (v[lo + i] + v[lo + i + 1]), 0.5 * gaps[i]))
    return out


def make(GPA, name, seed):
    shape, sigma, wl, wu = wc.CASES[name]
    image = wc.noisy_phasor(shape, seed)
    ws = wc.freq_list(sigma, wl, wu)
    m128 = np.stack([np.abs(sf) for _, _, sf in wc.spectra(image, sigma, ws, ws)])
    c64_err = max(np.abs(sf.astype(np.complex128) - sf2).max()
                  for (_, _, sf), (_, _, sf2) in zip(wc.spectra(image, sigma, ws, ws, np.complex64), wc.spectra(image, sigma, ws, ws)))
    picks = choose_thresholds(m128.ravel())
    thresholds = np.array([p[0] for p in picks])
    min_dist = np.array([np.abs(m128 - t).min() for t in thresholds])
    assert np.all(min_dist >= MARGIN * c64_err), (name, min_dist, c64_err)
    with contextlib.redirect_stdout(io.StringIO()):
        ref = GPA.wff(image, sigma, thresholds, wl, wu)
    mine = wc.restate(image, sigma, thresholds, ws, ws, wc.scale_of(sigma))
    m64 = wc.restate(image, sigma, thresholds, ws, ws, wc.scale_of(sigma), np.complex64)
    big = np.abs(ref).max()
    print('%-16s nws %d  sf_max %.4f  thresholds %s  half-gaps/sf_max %s  c64 sf err/sf_max %.2e  restatement vs reference %.2e  '
          'c64 restatement %.3e' % (name, len(ws), m128.max(), thresholds, min_dist / m128.max(), c64_err / m128.max(),
                                    np.abs(mine - ref).max() / big, np.abs(m64 - mine).max() / big))
    np.savez_compressed(os.path.join(wc.GOLDEN, name + '.npz'), image=image, sigma=np.float64(sigma), wl=np.float64(wl),
                        wu=np.float64(wu), nws=np.int64(len(ws)), thresholds=thresholds, out=ref, sf_max=np.float64(m128.max()),
                        min_dist=min_dist, c64_err=np.float64(c64_err))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--only', nargs='*', default=None)
    a = ap.parse_args()
    from oracle.make_golden import _import_reference
    GPA, _ = _import_reference()
    for seed, name in enumerate(wc.CASES):
        if a.only is None or name in a.only:
            make(GPA, name, 100 + seed)


if __name__ == '__main__':
    main()
