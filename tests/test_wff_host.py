"""Windowed Fourier filtering without a GPU: the restatement of tests/wff_cases.py against the fixtures the reference wrote,
the fixtures' own no-flip margins, the geometry header (tests/host/wff_geom_check.cpp, plain and under the host sanitizers --
an ordinary executable), the C ABI's two symbols, and the Python mirror against a recording stand-in for the library."""
import os
import re

import numpy as np
import pytest

from pygpa_amd import _lib
import pygpa_amd.geometric_phase_analysis as GPA

import wff_cases as wc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('name', list(wc.CASES))
def test_restatement_matches_the_reference(name):
    z = wc.load(name)
    shape, sigma, wl, wu = wc.CASES[name]
    assert z['image'].shape == shape and float(z['sigma']) == sigma and (float(z['wl']), float(z['wu'])) == (wl, wu)
    ws = wc.freq_list(sigma, wl, wu)
    assert len(ws) == int(z['nws'])
    assert z['out'].shape == (len(z['thresholds']),) + shape and z['out'].dtype == np.complex128
    mine = wc.restate(z['image'], sigma, z['thresholds'], ws, ws, wc.scale_of(sigma))
    assert np.abs(mine - z['out']).max() <= 1e-13 * np.abs(z['out']).max()


@pytest.mark.parametrize('name', list(wc.CASES))
def test_thresholds_sit_in_gaps(name):
    """no keep / drop decision may flip: every |sf| is at least 32 complex64 errors away from every threshold -- from the stored
    numbers, and the stored distances are those of the restatement's |sf|"""
    z = wc.load(name)
    assert np.all(z['min_dist'] >= 32 * float(z['c64_err'])) and float(z['c64_err']) > 0
    sigma = float(z['sigma'])
    ws = wc.freq_list(sigma, float(z['wl']), float(z['wu']))
    mags = np.stack([np.abs(sf) for _, _, sf in wc.spectra(z['image'], sigma, ws, ws)])
    assert np.isclose(mags.max(), float(z['sf_max']), rtol=1e-12)
    for t, d in zip(z['thresholds'], z['min_dist']):
        assert np.isclose(np.abs(mags - t).min(), d, rtol=1e-6)
        assert 0 < (mags >= t).mean() < 1


def test_rounding_dependent_list_length():
    # -0.7 + 6 / 3 = 1.3 lies above wu + wi / 2 = 1.2667 by a margin, 1.1 + 1 / 6 above -0.7 + 5 / 3: six entries; the
    # symmetric list ends ON wu (1.0 < 1 + 1 / 6): seven
    assert len(wc.freq_list(3.0, -0.7, 1.1)) == 6 and len(wc.freq_list(3.0, -1.0, 1.0)) == 7


def test_symbols_in_header_and_signatures():
    header = open(os.path.join(ROOT, 'include', 'gpa_hip.h')).read()
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    for name in ('gpa_wff', 'gpa_wff_dev'):
        m = re.search(r'\bint\s+%s\s*\(([^)]*)\)\s*;' % name, header)
        assert m, name
        nargs = len([a for a in m.group(1).split(',') if a.strip()])
        res, args = _lib.SIGNATURES[name]
        assert nargs == len(args) == 11 and res is _lib._i
    assert ('#define GPA_WFF_MAX_S %d' % _lib.WFF_MAX_S) in header and ('#define GPA_WFF_MAX_T %d' % _lib.WFF_MAX_T) in header


def _run_geom(tmp_path_factory, extra):
    r, out = wc.geom_check(tmp_path_factory.mktemp('wffgeom'), extra)
    if r.returncode != 0 and extra and ('asan' in r.stderr or 'ubsan' in r.stderr or 'sanitize' in r.stderr):
        pytest.skip('the host compiler has no sanitizer runtimes')
    assert r.returncode == 0, r.stderr[-2000:]
    assert out.returncode == 0, (out.stdout + out.stderr)[-2000:]
    assert out.stdout.startswith('OK ') and int(out.stdout.split()[1]) > 1000
    return out.stdout


def test_geometry_header(tmp_path_factory):
    text = _run_geom(tmp_path_factory, [])
    tiles = [ln.split() for ln in text.splitlines() if ln.startswith('TILE ')]
    assert {(t[1], int(t[2])) for t in tiles} >= {('f32', 6), ('f64', 6), ('f32', 5), ('f64', 5)}


def test_geometry_header_sanitized(tmp_path_factory):
    _run_geom(tmp_path_factory, ['-fsanitize=address,undefined', '-fno-sanitize-recover=all'])


def test_half_window_follows_python_rounding():
    # (the C side is checked in wff_geom_check.cpp; these are the values it is held to)
    assert [wc.half_window(s) for s in (1.25, 2.25, 2.5, 3, 10)] == [2, 4, 5, 6, 20]


class _RecordingLib:
    """stands in for libgpa_hip.so behind a Plan: records every gpa_wff call, fills the output with the call's number"""

    def __init__(self):
        self.calls = []

    def gpa_wff(self, handle, image, sigma, wxs, Kx, wys, Ky, thr, T, scale, out):
        import ctypes as C

        def arr(p, n):
            return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_double)), shape=(n,)).copy()
        self.calls.append(dict(sigma=sigma, wxs=arr(wxs, Kx), wys=arr(wys, Ky), thr=arr(thr, T), scale=scale, image=image, out=out))
        return 0


@pytest.fixture
def recording(monkeypatch):
    lib = _RecordingLib()
    plans = []

    def get_plan(shape, batch, dtype=np.float64, device=0):
        p = _lib.Plan.__new__(_lib.Plan)
        p.lib, p.handle, p.shape = lib, 1, (int(shape[0]), int(shape[1]))
        p.code = _lib.GPA_F32 if np.dtype(dtype) == np.float32 else _lib.GPA_F64
        p.rdtype, p.cdtype = _lib._DTYPES[p.code]
        plans.append(p)
        return p
    monkeypatch.setattr(_lib, 'get_plan', get_plan)
    yield lib, plans
    for p in plans:
        p.handle = None


def test_mirror_one_call_per_chunk(recording):
    lib, plans = recording
    sigma, wl, wu = 3.0, -0.7, 1.1
    image = wc.noisy_phasor((12, 9), 1)
    thr = np.linspace(0.1, 2.0, 2 * _lib.WFF_MAX_T + 3)
    out = GPA.wff(image, sigma, thr, wl, wu)
    assert out.shape == (len(thr),) + image.shape and out.dtype == np.complex128
    assert [len(c['thr']) for c in lib.calls] == [_lib.WFF_MAX_T, _lib.WFF_MAX_T, 3]
    assert np.array_equal(np.concatenate([c['thr'] for c in lib.calls]), thr)
    ws = np.arange(wl, wu + (1 / sigma) / 2, 1 / sigma)
    for c in lib.calls:
        assert np.array_equal(c['wxs'], ws) and np.array_equal(c['wys'], ws)     # the np.arange list, for both axes
        assert c['scale'] == (1 / sigma) ** 2 / (4 * np.pi ** 2) and c['sigma'] == sigma
    # one call for a list that fits
    lib.calls.clear()
    assert GPA.wff(image, sigma, thr[:2], wl, wu).shape == (2,) + image.shape and len(lib.calls) == 1


def test_mirror_promotes_a_real_image(recording):
    lib, plans = recording
    real = np.arange(20.0).reshape(4, 5)
    out = GPA.wff(real, 2.0, [0.5], -1, 1, dtype=np.float32)
    assert out.dtype == np.complex64 and out.shape == (1, 4, 5) and len(lib.calls) == 1
    assert plans[-1].cdtype == np.complex64
    # what the library received is the image as interleaved complex64 with zero imaginary parts
    import ctypes as C
    got = np.ctypeslib.as_array(C.cast(lib.calls[0]['image'], C.POINTER(C.c_float)), shape=(4, 5, 2))
    assert np.array_equal(got[..., 0], real.astype(np.float32)) and np.all(got[..., 1] == 0)


@pytest.mark.parametrize('kw', [dict(sigma=0), dict(sigma=-2.0), dict(sigma=float('nan')), dict(threshold=[]),
                                dict(threshold=[1.0, float('nan')]), dict(wl=float('inf')), dict(wl=1.0, wu=-1.0),
                                dict(image=np.zeros(5, complex)), dict(image=np.zeros((2, 3, 4), complex))])
def test_mirror_argument_errors_before_the_library(recording, kw):
    lib, plans = recording
    args = dict(image=np.ones((6, 6), complex), sigma=3.0, threshold=[1.0], wl=-1.0, wu=1.0)
    args.update(kw)
    with pytest.raises(ValueError):
        GPA.wff(args['image'], args['sigma'], args['threshold'], args['wl'], args['wu'])
    assert not lib.calls and not plans


def test_library_argument_errors_need_no_device():
    """the C entry points refuse bad arguments before they touch a device (a null plan among them)"""
    lib = _lib.load()
    one = np.array([0.5])
    img = np.ones((8, 8), complex)
    out = np.empty((1, 8, 8), complex)
    P = _lib._ptr
    for fn in (lib.gpa_wff, lib.gpa_wff_dev):
        assert fn(None, P(img), 3.0, P(one), 1, P(one), 1, P(one), 1, 1.0, P(out)) == -1
        assert 'plan' in _lib.last_error()


def test_no_cpu_fallback():
    lib = _lib.load()
    if lib.gpa_device_count() > 0:
        pytest.skip('a GPU is visible')
    with pytest.raises(_lib.GPAError):
        GPA.wff(wc.noisy_phasor((16, 16), 0), 3.0, [1.0], -1, 1)
