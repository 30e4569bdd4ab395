"""iterate_GPA as one library call (gpa_iterate_gpa and the device-pointer entry points it is made of), on the CPU: the ABI
against the header and the built library, and the routing of GPA.iterate_GPA with the device call replaced by a recording
stand-in for _lib.get_plan that answers from the oracle (as tests/test_onesweep_host.py does for the one-sweep driver)."""
import os
import re

import numpy as np
import pytest

from oracle import gpa_oracle as orc
from pygpa_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ['gpa_unwrap_dev', 'gpa_fit_planes_dev', 'gpa_lockin_polar_crop_dev', 'gpa_iterate_gpa_dev', 'gpa_iterate_gpa']


def _ensure_built():
    if not os.path.exists(_lib.LIB_PATH):
        from pygpa_amd import build
        build.build(verbose=False)


def _header_prototypes():
    header = open(os.path.join(ROOT, 'include', 'gpa_hip.h')).read()
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    return {m.group(1): [a for a in m.group(2).split(',') if a.strip() and a.strip() != 'void']
            for m in re.finditer(r'\b(gpa_[A-Za-z0-9_]+)\s*\(([^)]*)\)\s*;', header)}


def test_new_symbols_in_header_signatures_and_library():
    _ensure_built()
    lib = _lib.load()
    protos = _header_prototypes()
    for name in NEW:
        assert name in protos, name
        assert name in _lib.SIGNATURES, name
        assert len(protos[name]) == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(lib, name), name
    # the device forms take what the host forms take
    assert _lib.SIGNATURES['gpa_unwrap_dev'] == _lib.SIGNATURES['gpa_unwrap']
    assert _lib.SIGNATURES['gpa_iterate_gpa_dev'] == _lib.SIGNATURES['gpa_iterate_gpa']
    assert len(_lib.SIGNATURES['gpa_iterate_gpa'][1]) == 15
    assert len(_lib.SIGNATURES['gpa_fit_planes_dev'][1]) == 7
    assert len(_lib.SIGNATURES['gpa_lockin_polar_crop_dev'][1]) == 8


@pytest.mark.parametrize('name', NEW)
def test_null_plan_is_an_argument_error(name):
    _ensure_built()
    lib = _lib.load()
    ints = {'gpa_unwrap_dev': {3: 5, 5: 1}, 'gpa_fit_planes_dev': {2: 1, 3: 5}, 'gpa_lockin_polar_crop_dev': {2: 1, 3: 0},
            'gpa_iterate_gpa_dev': {4: 1, 6: 0, 7: 0, 8: 1, 9: 1}, 'gpa_iterate_gpa': {4: 1, 6: 0, 7: 0, 8: 1, 9: 1}}[name]
    args = []
    for i, t in enumerate(_lib.SIGNATURES[name][1]):
        args.append(ints.get(i, 1.0 if t is _lib._d else None) if t in (_lib._i, _lib._d) else None)
    assert getattr(lib, name)(*args) == -1         # GPA_ERR_ARG, before any device is touched
    assert _lib.last_error().startswith('gpa_')


def test_plan_methods_exist():
    import inspect
    for meth in ('unwrap_dev', 'fit_planes_dev', 'lockin_polar_crop_dev', 'iterate_gpa', 'iterate_gpa_dev'):
        assert callable(getattr(_lib.Plan, meth)), meth
    sig = inspect.signature(_lib.Plan.iterate_gpa)
    assert list(sig.parameters) == ['self', 'image', 'kvecs', 'sigma', 'edge', 'iters', 'kmax_iter', 'kmax', 'crop_plan']
    import pygpa_amd.geometric_phase_analysis as GPA
    sig = inspect.signature(GPA.iterate_GPA)
    assert sig.parameters['fused'].default is True and sig.parameters['dtype'].default is None
    # the reference's positional order is untouched
    assert list(sig.parameters)[:8] == ['image', 'kvecs', 'sigma', 'edge', 'iters', 'kmax_iter', 'kmax', 'verbose']


class _RecordingPlan:
    """stands in for _lib.Plan: records the calls, answers iterate_gpa from the oracle"""

    def __init__(self, log, shape, batch, dtype):
        self.log, self.shape, self.dtype = log, tuple(shape), np.dtype(dtype)
        self.rdtype = self.dtype.type

    def iterate_gpa(self, image, kvecs, sigma, edge=5, iters=3, kmax_iter=25, kmax=200, crop_plan=None):
        self.log.append(('iterate_gpa', self.shape, None if crop_plan is None else crop_plan.shape, self.dtype,
                         int(edge), int(iters), int(kmax_iter), int(kmax)))
        image = np.asarray(image, dtype=np.float64)
        prs, w, corr = orc.iterate_gpa(image, kvecs, sigma, edge=edge, iters=iters, kmax_iter=kmax_iter, kmax=kmax)
        # what each pass subtracted: replayed from shorter runs of the same oracle
        corrs = [np.zeros_like(corr)] + [orc.iterate_gpa(image, kvecs, sigma, edge=edge, iters=i, kmax_iter=kmax_iter,
                                                         kmax=kmax)[2] for i in range(1, iters + 1)]
        delta_ks = np.array([corrs[i] - corrs[i + 1] for i in range(iters)]).reshape(iters, len(corr), 2)
        return (prs.astype(self.rdtype), w.astype(self.rdtype), corr, delta_ks,
                np.full((iters + 1, len(corr)), kmax_iter, dtype=np.int32))

    # the host loop's entry points
    def lockin_batch(self, image, kvecs, sigma):
        self.log.append(('lockin_batch', self.shape))
        return orc.lockin_batch(np.asarray(image, dtype=np.float64), kvecs, sigma)

    def unwrap(self, psi, weight=None, kmax=100, eps=1e-9, axes_compat=True):
        self.log.append(('unwrap', self.shape))
        return orc.unwrap(np.asarray(psi, dtype=np.float64), weight, kmax=kmax), kmax

    def fit_plane(self, image, max_iter=200, tol=1e-12):
        self.log.append(('fit_plane', self.shape))
        return orc.fit_plane(np.asarray(image, dtype=np.float64)), 1


@pytest.fixture
def recorded(monkeypatch):
    log = []
    monkeypatch.setattr(_lib, 'get_plan', lambda shape, batch, dtype=np.float64, device=0: _RecordingPlan(log, shape, batch, dtype))
    return log


@pytest.fixture(scope='module')
def case(golden):
    g = golden('iterate_64')
    image = g['image'] - g['image'].mean()
    start, sigma = g['start_ks'], int(g['sigma'])
    return image, start, sigma, orc.iterate_gpa(image, start, sigma, edge=5, iters=2)


def test_fused_is_one_call_with_a_frame_and_a_window_plan(recorded, case):
    import pygpa_amd.geometric_phase_analysis as GPA
    image, start, sigma, (prs_o, w_o, corr_o) = case
    prs, w, corr = GPA.iterate_GPA(image, start, sigma, edge=5, iters=2)
    assert recorded == [('iterate_gpa', (64, 64), (54, 54), np.dtype(np.float64), 5, 2, 25, 200)]
    assert prs.shape == (3, 54, 54) and w.shape == (3, 54, 54) and corr.shape == (3, 2)
    assert prs.dtype == w.dtype == corr.dtype == np.float64
    assert np.array_equal(prs, prs_o) and np.array_equal(w, w_o) and np.array_equal(corr, corr_o)


def test_dtype_reaches_both_plans(recorded, case):
    import pygpa_amd.geometric_phase_analysis as GPA
    image, start, sigma, _ = case
    prs, w, corr = GPA.iterate_GPA(image, start, sigma, edge=3, iters=1, kmax_iter=4, kmax=6, dtype=np.float32)
    assert recorded == [('iterate_gpa', (64, 64), (58, 58), np.dtype(np.float32), 3, 1, 4, 6)]
    assert prs.dtype == w.dtype == np.float32 and corr.dtype == np.float64


def test_edge_zero_passes_one_shape(recorded, case):
    import pygpa_amd.geometric_phase_analysis as GPA
    image, start, sigma, _ = case
    prs, w, corr = GPA.iterate_GPA(image, start[:1], sigma, edge=0, iters=0, kmax=5)
    assert recorded == [('iterate_gpa', (64, 64), (64, 64), np.dtype(np.float64), 0, 0, 25, 5)]
    assert prs.shape == (1, 64, 64) and w.shape == (1, 64, 64)
    assert np.array_equal(corr, np.zeros((1, 2)))


def test_unfused_makes_no_such_call(recorded, case):
    import pygpa_amd.geometric_phase_analysis as GPA
    image, start, sigma, (prs_o, w_o, corr_o) = case
    prs, w, corr = GPA.iterate_GPA(image, start, sigma, edge=5, iters=2, fused=False)
    names = [c[0] for c in recorded]
    assert 'iterate_gpa' not in names
    assert names.count('lockin_batch') == 3 and names.count('unwrap') == 9 and names.count('fit_plane') == 6
    assert np.array_equal(w, w_o) and np.allclose(corr, corr_o, rtol=0, atol=1e-15) and np.allclose(prs, prs_o, rtol=0, atol=1e-9)


def test_verbose_prints_one_block_per_pass(recorded, case, capsys):
    import pygpa_amd.geometric_phase_analysis as GPA
    image, start, sigma, (_, _, corr_o) = case
    GPA.iterate_GPA(image, start[:1], sigma, edge=5, iters=2, verbose=True)
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    assert len(lines) == 2                       # P = 1: one line per pass, as the reference's print(delta_ks) gives
    printed = np.array([[float(v) for v in ln.replace('[', ' ').replace(']', ' ').split()] for ln in lines])
    assert printed.shape == (2, 2)
    # the two steps add up to the correction of peak 0 refined on its own
    corr1 = orc.iterate_gpa(image, start[:1], sigma, edge=5, iters=2)[2]
    assert np.allclose(-printed.sum(axis=0), corr1[0], rtol=0, atol=1e-7)


@pytest.mark.parametrize('kw', [dict(edge=32), dict(edge=-1), dict(iters=-1), dict(kvecs=np.zeros((3, 3))), dict(kvecs=np.zeros(4))])
def test_argument_errors_touch_neither_plan_nor_library(monkeypatch, case, kw):
    import pygpa_amd.geometric_phase_analysis as GPA
    image, start, sigma, _ = case

    def boom(*a, **k):
        raise AssertionError('a plan or the library was asked for')
    monkeypatch.setattr(_lib, 'get_plan', boom)
    monkeypatch.setattr(_lib, 'load', boom)
    args = dict(kvecs=start, edge=5, iters=1)
    args.update(kw)
    for fused in (True, False):
        with pytest.raises(ValueError):
            GPA.iterate_GPA(image, args['kvecs'], sigma, edge=args['edge'], iters=args['iters'], fused=fused)
