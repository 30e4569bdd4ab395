"""The row-wise skip test of the shared pass B on the CPU: the NumPy model of the spectral bound
(tools/passb_skip_model.py) against the oracle's lock-ins, and the ABI of the counter that reports what the kernel skipped."""
import os
import re
import sys

import numpy as np

from oracle import gpa_oracle as orc
from pygpa_amd import _lib
from pygpa_amd.synthetic import hex_kvecs, gaussian_bump_displacement, hex_moire, explicit_klists

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import passb_skip_model as model   # noqa: E402


def test_model_never_skips_a_pair_that_wins_under_the_oracle():
    """64 x 2048, the benchmark's kind of image, 4 x 4 candidates of every peak in the kernel's visiting order: a (row, candidate)
    pair whose bound 1.001 B_c lies below the smallest running best of the row never wins a pixel of that row when the selection
    runs on the ORACLE's lock-ins (strict '>' in visiting order); and the model does skip a share worth having."""
    shape = (64, 2048)
    kvecs = hex_kvecs(0.1, 7.0)
    img = hex_moire(shape, kvecs, gaussian_bump_displacement(shape), noise=0.1, seed=100)
    img0 = img - img.mean()
    kw, sigma, _ = orc.derive_params(kvecs)
    klists = explicit_klists(kvecs, kw, 4, 4)
    for magnitude in ('abs', 'l1'):
        skipped = pairs = 0
        for p in range(3):
            m = model.skip_model(img0, klists[p], kvecs[p], sigma, magnitude=magnitude)
            assert sorted(m['order']) == list(range(16))
            best = np.zeros(shape)
            for pos, k in enumerate(m['order']):
                amp = np.abs(orc.lockin(img0, klists[p][k], sigma))
                assert np.abs(amp - m['amp'][k]).max() < 1e-10 * amp.max()      # the model's lock-ins are the oracle's
                take = amp > best
                wins = take.any(axis=1)
                assert not (m['skipped'][:, pos] & wins).any(), (magnitude, p, pos)
                best = np.where(take, amp, best)
            assert not m['skipped'][:, 0].any()
            skipped += int(m['skipped'].sum())
            pairs += m['skipped'][:, 1:].size
        assert skipped > 0.2 * pairs, (magnitude, skipped, pairs)


def _built():
    if not os.path.exists(_lib.LIB_PATH):
        from pygpa_amd import build
        build.build(verbose=False)


def test_visiting_order_is_the_librarys_and_keeps_planes_together_nearest_first():
    """model.visiting_order IS the library's rule (gpa_passb_visiting_order, the function shared_prepare orders the kernel's
    tables with); its NumPy transcription agrees on a plain grid, a wy-outer list, a shuffled list, lists with duplicated and
    with aliased k-vectors, and under NO_REORDER"""
    _built()
    kvecs = hex_kvecs(0.1, 7.0)
    klist = explicit_klists(kvecs, 0.04, 4, 4)[1]
    order = model.visiting_order(klist, kvecs[1])
    assert order == _lib.passb_visiting_order(klist, kvecs[1])
    wx = [klist[k][0] for k in order]
    assert all(len(set(wx[4 * i:4 * i + 4])) == 1 for i in range(4)) and len(set(wx)) == 4
    d2 = ((klist - kvecs[1]) ** 2).sum(axis=1)
    assert order[0] == int(np.argmin(d2))
    for i in range(4):
        run = [d2[k] for k in order[4 * i:4 * i + 4]]
        assert run == sorted(run)
    wy_outer = klist.reshape(4, 4, 2).transpose(1, 0, 2).reshape(-1, 2).copy()
    shuffled = klist[np.random.default_rng(4).permutation(16)]
    dup = np.concatenate([klist, klist[5:7], klist[0:1]])
    aliased = np.concatenate([klist, [klist[3] + np.array([1.0, 0.0])]])
    for p in range(3):
        for kl in (explicit_klists(kvecs, 0.04, 4, 4)[p], explicit_klists(kvecs, 0.04, 4, 2)[p], explicit_klists(kvecs, 0.04, 3, 7)[p],
                   wy_outer, shuffled, dup, aliased):
            got = _lib.passb_visiting_order(kl, kvecs[p])
            assert sorted(got) == list(range(len(kl)))
            assert got == model.visiting_order_numpy(kl, kvecs[p]), (p, len(kl))
    # two different k-vectors equal modulo whole cycles: the list's own order; and the switch
    assert _lib.passb_visiting_order(aliased, kvecs[1]) == list(range(17))
    with _lib.options(NO_REORDER='1'):
        assert _lib.passb_visiting_order(klist, kvecs[1]) == list(range(16))
    assert _lib.passb_visiting_order(klist, kvecs[1]) == order
    lib = _lib.load()
    assert lib.gpa_passb_visiting_order(None, None, 4, None) == -1 and _lib.last_error().startswith('gpa_passb_visiting_order')


def test_passb_skip_counter_in_header_signatures_and_library():
    _built()
    lib = _lib.load()
    header = open(os.path.join(ROOT, 'include', 'gpa_hip.h')).read()
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    m = re.search(r'\bint\s+gpa_last_passb_skips\s*\(([^)]*)\)\s*;', header)
    assert m, 'gpa_last_passb_skips is not declared in gpa_hip.h'
    args = [a.strip() for a in m.group(1).split(',')]
    assert len(args) == 3 and args[0].startswith('gpa_plan*') and args[1].startswith('long long*') and args[2].startswith('long long*')
    res, sig = _lib.SIGNATURES['gpa_last_passb_skips']
    assert res is _lib._i and len(sig) == 3
    assert hasattr(lib, 'gpa_last_passb_skips') and hasattr(_lib.Plan, 'last_passb_skips')
    m = re.search(r'\bint\s+gpa_passb_visiting_order\s*\(([^)]*)\)\s*;', header)
    assert m and len(m.group(1).split(',')) == 4 == len(_lib.SIGNATURES['gpa_passb_visiting_order'][1])
    assert hasattr(lib, 'gpa_passb_visiting_order')
    assert lib.gpa_last_passb_skips(None, None, None) == -1          # GPA_ERR_ARG, before any device is touched
    assert _lib.last_error().startswith('gpa_last_passb_skips')
    # the switch is a known option
    _lib.set_option('NO_PB_SKIP', '1')
    _lib.set_option('NO_PB_SKIP', None)
