"""The boundary modes 'reflect' / 'grid-mirror', 'mirror' and 'grid-wrap' of invert_u / invert_u_overlap without a GPU:
the fold, weight and tap-extension arithmetic of pygpa_amd/csrc/gpa_spline.h, compiled for the host
(tests/host/spline_modes_emulator.cpp) and held to scipy.ndimage.map_coordinates; the mode codes of the ctypes layer;
and the refusal of the modes that are not provided, before the library is touched."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from pygpa_amd import _lib
import pygpa_amd.geometric_phase_analysis as GPA

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXT = {'reflect': 0, 'mirror': 1, 'grid-wrap': 2}
SHAPES = [(4, 5), (5, 7), (16, 23), (40, 33)]


@pytest.fixture(scope='module')
def emulator(tmp_path_factory):
    gxx = shutil.which('g++')
    if gxx is None:
        pytest.skip('g++ not available')
    exe = str(tmp_path_factory.mktemp('spline_modes') / 'spline_modes_emulator')
    src = os.path.join(ROOT, 'tests', 'host', 'spline_modes_emulator.cpp')
    subprocess.run([gxx, '-O2', '-std=c++17', '-I', os.path.join(ROOT, 'pygpa_amd', 'csrc'), src, '-o', exe], check=True)
    return exe


def axis_lists(n, rng):
    """coordinates along an axis of n samples: 400 random ones in +-5 n, every half-integer in +-3 n, the six fold points"""
    return (rng.uniform(-5.0 * n, 5.0 * n, 400), 0.5 * np.arange(-6 * n, 6 * n + 1), np.array([-0.5, n - 0.5, n - 1.0, 0.0, float(n), -1.0]))


def coordinates(n0, n1, rng):
    r0, h0, f0 = axis_lists(n0, rng)
    r1, h1, f1 = axis_lists(n1, rng)
    m = max(len(h0), len(h1))
    # random x random; the half-integers of each axis, each list shuffled and cycled to the longer one; every pair of fold points
    hx, hy = np.resize(rng.permutation(h0), m), np.resize(rng.permutation(h1), m)
    fx, fy = [v.ravel() for v in np.meshgrid(f0, f1, indexing='ij')]
    return np.stack([np.concatenate([r0, hx, fx, f0, h0[:6]]), np.concatenate([r1, hy, fy, r1[:6], f1])])


def run_emulator(exe, tmp_path, field, coords, mode):
    src, dst = str(tmp_path / 'in.bin'), str(tmp_path / 'out.bin')
    npts = coords.shape[1]
    np.concatenate([field.ravel(), [float(npts)], coords[0], coords[1]]).astype(np.float64).tofile(src)
    out = subprocess.run([exe, str(field.shape[0]), str(field.shape[1]), str(EXT[mode]), src, dst], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip().endswith('OK'), (out.stdout[-2000:], out.stderr[-2000:])
    got = np.fromfile(dst, dtype=np.float64)
    assert got.shape == (npts,)
    return got


def test_emulator_selfcheck(emulator):
    """NaN, infinite and huge coordinates fold to a point of the period; every tap index lies inside the axis"""
    out = subprocess.run([emulator, 'selfcheck'], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip().endswith('OK'), out.stdout[-2000:]


@pytest.mark.parametrize('mode', ['reflect', 'mirror', 'grid-wrap'])
@pytest.mark.parametrize('shape', SHAPES)
def test_folded_sampler_vs_scipy(emulator, tmp_path, shape, mode):
    """FIR prefilter with the mode's extension + fold + weights + extended taps (the host instantiation of the device's
    functions) against scipy.ndimage.map_coordinates(order=3, mode=mode) at 1e-12 max|field|.  'reflect' on the two short
    shapes is held to an exact identity instead -- 'grid-wrap' sampling of the symmetric doubling of the field -- because
    SciPy's own 'reflect' prefilter is approximate there (3.7e-6 of the field at n = 4, rounding from n = 12)."""
    import scipy.ndimage as ndi
    n0, n1 = shape
    rng = np.random.default_rng(100 * n0 + n1)
    field = rng.standard_normal(shape)
    coords = coordinates(n0, n1, rng)
    got = run_emulator(emulator, tmp_path, field, coords, mode)
    if mode == 'reflect' and min(shape) < 16:
        ref = ndi.map_coordinates(np.pad(field, ((0, n0), (0, n1)), mode='symmetric'), coords, order=3, mode='grid-wrap')
    else:
        ref = ndi.map_coordinates(field, coords, order=3, mode=mode)
    err = np.abs(got - ref).max()
    print('%s %s: max error %.3g of max|field| %.3g' % (shape, mode, err, np.abs(field).max()))
    assert np.all(np.isfinite(got))
    assert err <= 1e-12 * np.abs(field).max()


def test_warp_mode_code():
    codes = {'nearest': 0, 'constant': 1, 'reflect': 2, 'grid-mirror': 2, 'mirror': 3, 'grid-wrap': 4}
    for mode, code in codes.items():
        assert _lib.warp_mode_code(mode) == code
    for mode in ('wrap', 'grid-constant', 'bogus', '', None, 2):
        with pytest.raises(NotImplementedError):
            _lib.warp_mode_code(mode)
    with pytest.raises(NotImplementedError, match='grid-wrap'):
        _lib.warp_mode_code('wrap')
    with pytest.raises(NotImplementedError, match='NaN'):
        _lib.warp_mode_code('grid-constant')


@pytest.fixture
def no_library(monkeypatch):
    """any attempt to get a plan (and with it the library) fails the test"""
    def boom(*a, **k):
        raise AssertionError('the library was touched')
    monkeypatch.setattr(_lib, 'get_plan', boom)
    monkeypatch.setattr(_lib, 'load', boom)


@pytest.mark.parametrize('fn', [GPA.invert_u, GPA.invert_u_overlap])
def test_refused_modes_raise_before_the_library(no_library, fn):
    us = np.zeros((2, 8, 9))
    for mode in ('wrap', 'grid-constant', 'bogus'):
        with pytest.raises(NotImplementedError):
            fn(us, mode=mode)
    with pytest.raises(NotImplementedError, match='grid-wrap'):
        fn(us, mode='wrap')
    # an accepted mode goes on to the plan
    with pytest.raises(AssertionError, match='the library was touched'):
        fn(us, mode='grid-wrap')
