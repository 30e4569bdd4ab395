"""Image preparation without a GPU: the fixtures the reference's imagetools wrote against the NumPy restatement of
tests/prep_cases.py, the geometry header (tests/host/prep_check.cpp, plain and under the host sanitizers -- an ordinary
executable), the C ABI's symbols, and the Python mirror against a recording stand-in for the library."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from pygpa_amd import _lib
import pygpa_amd.imagetools as IT

import prep_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PREP_SYMBOLS = {'gpa_gauss_homogenize': 8, 'gpa_mask_any_equal': 6, 'gpa_mask_erode_disk': 5, 'gpa_mask_bounds': 3,
                'gpa_nan_lines': 4, 'gpa_nan_trim_lims': 3}


# ---- fixtures are self-consistent --------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(pc.H_CASES))
def test_homogenize_fixture_matches_the_restatement(name):
    z = pc.load(name)
    shape, sigma, _ = pc.H_CASES[name]
    image, mask, sigma2 = pc.homogenize_inputs(name)
    assert z['image'].shape == shape and float(z['sigma']) == sigma == sigma2 and z['mask'].dtype == np.bool_
    assert np.array_equal(z['image'], image, equal_nan=True) and np.array_equal(z['mask'], mask)
    assert os.path.getsize(os.path.join(pc.GOLDEN, name + '.npz')) < 512 * 1024
    # the cases' promises: values of 500 .. 4000 under the mask, NaNs only outside it
    assert np.all(np.isfinite(image[mask])) and image[mask].min() >= 500 and image[mask].max() <= 4000
    assert not np.any(np.isnan(image) & mask)
    out, VV, den = pc.restate_homogenize(image, mask, sigma)
    ok = ~np.isnan(z['VV'])
    assert np.array_equal(np.isnan(VV), ~ok)
    assert np.abs(VV[ok] - z['VV'][ok]).max() <= 1e-13 * np.abs(z['VV'][ok]).max()
    assert np.all(np.abs(VV[ok] - z['VV'][ok]) <= 1e-13 * np.abs(z['VV'][ok]))
    assert np.abs(den - z['den']).max() <= 1e-13
    both = ~np.isnan(z['out_none'])
    assert np.array_equal(np.isnan(out), ~both)
    assert np.all(np.abs(out[both] - z['out_none'][both]) <= 1e-13 * np.abs(z['out_none'][both]))
    out1, VV1, _ = pc.restate_homogenize(image, mask, sigma, nan_scale=1)
    fin = ~np.isnan(z['out_1'])
    assert np.array_equal(np.isnan(out1), ~fin) and np.array_equal(fin, ~np.isnan(image))
    assert np.all(np.abs(out1[fin] - z['out_1'][fin]) <= 1e-13 * np.abs(z['out_1'][fin]))


@pytest.mark.parametrize('name', list(pc.H_CASES))
def test_vv_is_nan_exactly_where_the_box_is_empty(name):
    z = pc.load(name)
    empty = pc.box_empty(z['mask'], float(z['sigma']))
    assert np.array_equal(np.isnan(z['VV']), empty)
    assert np.array_equal(z['den'] == 0, empty)
    # out: NaN where VV is or the image is; with nan_scale = 1 only where the image is
    assert np.array_equal(np.isnan(z['out_none']), empty | np.isnan(z['image']))
    assert np.array_equal(z['out_1'][empty], z['image'][empty], equal_nan=True)
    if name == 'prep_h_96x130_s3':
        assert 0.75 <= empty.mean() <= 0.85
    if name == 'prep_h_64x64_full_s4':
        assert not empty.any() and not np.isnan(z['image']).any()
    # den under the mask stays well above what f32 transforms resolve
    assert z['den'][z['mask']].min() >= 3e-3


def test_mask_fixture_matches_the_restatement():
    z = pc.load('prep_mask')
    stack = pc.mask_stack()
    assert np.array_equal(z['stack'], stack) and stack.shape == pc.MASK_SHAPE and float(z['mask_value']) == pc.MASK_VALUE
    assert tuple(z['radii']) == pc.MASK_RADII
    frames = stack.astype(np.float64)
    for r in pc.MASK_RADII:
        m = z['mask_r%d' % r]
        assert m.dtype == np.bool_ and np.array_equal(m, pc.restate_generate_mask(frames, pc.MASK_VALUE, r)), r
    assert np.array_equal(z['mask_r0'], ~np.any(stack == 0, axis=0))
    assert 0.02 <= z['mask_r20'].mean() <= 0.10 and not z['mask_r200'].any()
    # a NaN value hits nothing: the erosion of an all-true mask, eaten from the edges
    want = np.zeros(pc.MASK_SHAPE[1:], dtype=bool)
    want[20:-20, 20:-20] = True
    assert np.array_equal(z['mask_nan_r20'], want)
    assert np.array_equal(z['mask_nan_r20'], pc.restate_generate_mask(frames, np.nan, 20))
    for r in (3, 20):
        assert np.array_equal(z['cull_lims_r%d' % r], pc.restate_bounds(z['mask_r%d' % r]))


def test_disk_restatement():
    assert np.array_equal(pc.disk(1), [[0, 1, 0], [1, 1, 1], [0, 1, 0]])
    assert pc.disk(0).shape == (1, 1) and pc.disk(20).shape == (41, 41) and pc.disk(3).sum() == 29


def test_erosion_restatement_against_scipy():
    import scipy.ndimage as ndi
    rng = np.random.default_rng(5)
    mask = rng.random((60, 75)) > 0.004
    for r in (1, 2, 3, 7):
        assert np.array_equal(pc.restate_erosion(mask, r), ndi.binary_erosion(mask, structure=pc.disk(r))), r


def test_trim_fixture_matches_the_restatement():
    z = pc.load('prep_trim')
    for name in pc.TRIM_CASES:
        img = pc.trim_image(name)
        assert np.array_equal(z[name + '_image'], img, equal_nan=True)
        assert np.array_equal(z[name + '_trim_nans'], pc.restate_trim_nans(img), equal_nan=True)
        lims = pc.restate_trim_lims(img)
        if name + '_trim_nans2_empties' in z:
            assert lims[1] <= lims[0] or lims[3] <= lims[2]
            continue
        assert np.array_equal(z[name + '_lims'].ravel(), lims)
        assert np.array_equal(z[name + '_trim_nans2'], img[lims[0]:lims[1], lims[2]:lims[3]])
        assert not np.isnan(z[name + '_trim_nans2']).any()
    # unequal widths on all four sides; the tie went to the columns
    b = z['borders_lims']
    assert len({int(b[0, 0]), 48 - int(b[0, 1]), int(b[1, 0]), 56 - int(b[1, 1])}) == 4
    assert np.array_equal(z['tie_lims'], [[0, 12], [1, 8]])
    assert 'inner_trim_nans2_empties' in z and z['inner_trim_nans'].shape == (18, 15)


# ---- the geometry header -------------------------------------------------------------------------------------------------
def _run_check(tmp_path_factory, extra):
    if extra and not pc.host_compiler_links(tmp_path_factory.mktemp('probe'), extra):
        pytest.skip('the host compiler has no sanitizer runtimes')      # decided on an empty program, before the check is built
    r, out = pc.prep_check(tmp_path_factory.mktemp('prepcheck'), extra)
    assert r.returncode == 0, r.stderr[-2000:]
    assert out.returncode == 0, (out.stdout + out.stderr)[-2000:]
    assert out.stdout.startswith('OK ') and int(out.stdout.split()[1]) > 100000


def test_geometry_header(tmp_path_factory):
    _run_check(tmp_path_factory, [])


def test_geometry_header_sanitized(tmp_path_factory):
    _run_check(tmp_path_factory, ['-fsanitize=address,undefined', '-fno-sanitize-recover=all'])


# ---- the C ABI -------------------------------------------------------------------------------------------------------
def test_symbols_in_header_and_signatures():
    header = open(os.path.join(ROOT, 'include', 'gpa_hip.h')).read()
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    for base, n in PREP_SYMBOLS.items():
        for name in (base, base + '_dev'):
            m = re.search(r'\bint\s+%s\s*\(([^)]*)\)\s*;' % name, header)
            assert m, name
            nargs = len([a for a in m.group(1).split(',') if a.strip()])
            res, args = _lib.SIGNATURES[name]
            assert nargs == len(args) == n and res is _lib._i, name
    assert ('#define GPA_PREP_MAX_R %d' % _lib.PREP_MAX_R) in header and ('#define GPA_PREP_MAX_N1 %d' % _lib.PREP_MAX_N1) in header
    limits = open(os.path.join(ROOT, 'pygpa_amd', 'csrc', 'gpa_prep.h')).read()
    assert ('PREP_MAX_R = %d;' % _lib.PREP_MAX_R) in limits and ('PREP_MAX_N1 = %d;' % _lib.PREP_MAX_N1) in limits


def test_library_argument_errors_need_no_device():
    """the C entry points refuse bad arguments before they touch a device (a null plan among them)"""
    lib = _lib.load()
    P = _lib._ptr
    a = np.ones((8, 8))
    m = np.ones((8, 8), dtype=np.uint8)
    lims = np.zeros(4, dtype=np.int32)
    for sfx in ('', '_dev'):
        calls = [lambda f: f(None, P(a), P(m), 3.0, 0, 0.0, P(a), None), lambda f: f(None, P(a), 1, 0.0, 0, P(m)),
                 lambda f: f(None, P(m), 0, 1, P(m)), lambda f: f(None, P(m), P(lims)), lambda f: f(None, P(a), P(m), P(m)),
                 lambda f: f(None, P(a), P(lims))]
        for base, call in zip(PREP_SYMBOLS, calls):
            assert call(getattr(lib, base + sfx)) == -1
            assert 'plan' in _lib.last_error() and (base + sfx) in _lib.last_error()


# ---- the mirror against a recording stand-in ---------------------------------------------------------------------------
def _bytes(p, n):
    return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(n,))


class _RecordingLib:
    """stands in for libgpa_hip.so behind a Plan: records every call, answers with fixed lims / flags"""

    def __init__(self):
        self.calls = []
        self.lims = [1, 3, 2, 5]
        self.rows = self.cols = None

    def gpa_gauss_homogenize(self, handle, image, mask, sigma, use, ns, out, vv):
        self.calls.append(('homogenize', sigma, use, ns, vv is None))
        return 0

    def gpa_mask_any_equal(self, handle, frames, B, value, accumulate, hit):
        self.calls.append(('any_equal', B, value, accumulate))
        _bytes(hit, self.npx)[:] = 0
        _bytes(hit, self.npx)[B] = 1           # marks the chunk length in the plane it returns
        return 0

    def gpa_mask_erode_disk(self, handle, inp, invert, r, out):
        self.calls.append(('erode', invert, r, _bytes(inp, self.npx).copy()))
        _bytes(out, self.npx)[:] = 2           # not 0 / 1: the mirror must hand out bool
        return 0

    def gpa_mask_bounds(self, handle, mask, lims):
        self.calls.append(('bounds', _bytes(mask, self.npx).copy()))
        np.ctypeslib.as_array(C.cast(lims, C.POINTER(C.c_int32)), shape=(4,))[:] = self.lims
        return 0

    def gpa_nan_lines(self, handle, image, rows, cols):
        self.calls.append(('nan_lines',))
        _bytes(rows, len(self.rows))[:] = self.rows
        _bytes(cols, len(self.cols))[:] = self.cols
        return 0

    def gpa_nan_trim_lims(self, handle, image, lims):
        self.calls.append(('trim',))
        np.ctypeslib.as_array(C.cast(lims, C.POINTER(C.c_int32)), shape=(4,))[:] = self.lims
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
        lib.npx = p.shape[0] * p.shape[1]
        plans.append(p)
        return p
    monkeypatch.setattr(_lib, 'get_plan', get_plan)
    yield lib, plans
    for p in plans:
        p.handle = None


@pytest.mark.parametrize('kw, exc', [
    (dict(mask=np.ones((6, 7))), TypeError), (dict(mask=np.ones((6, 7), dtype=np.uint8)), TypeError),
    (dict(mask=np.ones((6, 6), dtype=bool)), ValueError), (dict(sigma=0), ValueError), (dict(sigma=-1.0), ValueError),
    (dict(sigma=float('nan')), ValueError), (dict(sigma=float('inf')), ValueError), (dict(sigma=[2.0, 3.0]), ValueError),
    (dict(image=np.ones((2, 6, 7))), ValueError), (dict(image=np.ones((6, 7), dtype=complex)), TypeError),
    (dict(image='nan_under_mask'), ValueError), (dict(image='inf_under_mask'), ValueError), (dict(dtype=np.int32), ValueError)])
def test_homogenize_argument_errors_before_the_library(recording, kw, exc):
    lib, plans = recording
    args = dict(image=np.full((6, 7), 5.0), mask=np.ones((6, 7), dtype=bool), sigma=2.0, dtype=None)
    args.update(kw)
    if isinstance(args['image'], str):
        bad = np.full((6, 7), 5.0)
        bad[2, 3] = np.nan if args['image'].startswith('nan') else np.inf
        args['image'] = bad
    with pytest.raises(exc):
        IT.gauss_homogenize2(args['image'], args['mask'], args['sigma'], dtype=args['dtype'])
    assert not lib.calls and not plans


def test_homogenize_mirror_calls(recording):
    lib, plans = recording
    img = np.arange(42.0).reshape(6, 7) + 1
    mask = np.ones((6, 7), dtype=bool)
    mask[0, 0] = False
    img[0, 0] = np.nan                      # a NaN outside the mask is the normal case
    out = IT.gauss_homogenize2(img, mask, 2.5)
    assert out.shape == (6, 7) and out.dtype == np.float64
    IT.gauss_homogenize2(img, mask, 2.5, nan_scale=7.0, dtype=np.float32)
    IT.gauss_homogenize3(img, mask, 2.5)
    ints = IT.gauss_homogenize3(np.arange(42).reshape(6, 7), mask, 2.5, dtype=np.float32)     # integers are converted
    assert ints.dtype == np.float32 and plans[-1].rdtype == np.float32
    assert lib.calls == [('homogenize', 2.5, 0, 0.0, True), ('homogenize', 2.5, 1, 7.0, True), ('homogenize', 2.5, 1, 1.0, True),
                         ('homogenize', 2.5, 1, 1.0, True)]


def test_generate_mask_chunks_and_bool(recording, monkeypatch):
    lib, plans = recording
    frames = np.ones((7, 4, 5))
    monkeypatch.setattr(IT, 'MASK_CHUNK_BYTES', 3 * 4 * 5 * 8)            # three frames per upload
    mask = IT.generate_mask(frames, 0.5, r=2)
    assert mask.dtype == np.bool_ and mask.shape == (4, 5) and mask.all()
    assert [c[:4] for c in lib.calls[:3]] == [('any_equal', 3, 0.5, 0), ('any_equal', 3, 0.5, 1), ('any_equal', 1, 0.5, 1)]
    kind, invert, r, plane = lib.calls[3]
    assert (kind, invert, r) == ('erode', 1, 2) and plane[1] == 1 and plane.sum() == 1     # the last chunk's plane, inverted there
    lib.calls.clear()
    IT.generate_mask(list(frames), np.nan)                                  # anything np.asarray makes a stack of; r = 20
    assert lib.calls[-1][1:3] == (1, 20)
    for bad in (dict(dataset=np.ones((4, 5))), dict(dataset=np.ones((0, 4, 5))), dict(r=-1), dict(r=_lib.PREP_MAX_R + 1)):
        lib.calls.clear()
        args = dict(dataset=frames, r=3)
        args.update(bad)
        with pytest.raises(ValueError):
            IT.generate_mask(args['dataset'], 0.0, args['r'])
        assert not lib.calls


def test_cull_and_trims_slice_from_lims(recording):
    lib, plans = recording
    data = np.arange(3 * 4 * 6).reshape(3, 4, 6)
    mask = np.zeros((4, 6))
    mask[1:3, 2:5] = 3.0                                                    # truth values, as np.sum takes them
    got = IT.cull_by_mask(data, mask)
    assert np.array_equal(got, data[:, 1:3, 2:5])
    assert np.array_equal(lib.calls[-1][1].reshape(4, 6), mask != 0)
    lib.lims = [4, 0, 6, 0]
    with pytest.raises(ValueError):
        IT.cull_by_mask(data, mask)
    with pytest.raises(ValueError):
        IT.cull_by_mask(data, np.zeros((4, 5)))
    img = np.arange(24.0).reshape(4, 6)
    lib.lims = [1, 3, 2, 5]
    t, lims = IT.trim_nans2(img, return_lims=True)
    assert np.array_equal(t, img[1:3, 2:5]) and np.array_equal(lims, [[1, 3], [2, 5]]) and t.base is None
    assert np.array_equal(IT.trim_nans2(img), img[1:3, 2:5])
    lib.lims = [2, 1, 0, 6]
    with pytest.raises(ValueError):
        IT.trim_nans2(img)
    lib.rows, lib.cols = [0, 1, 0, 0], [1, 0, 0, 0, 1, 0]
    assert np.array_equal(IT.trim_nans(img), img[[0, 2, 3]][:, [1, 2, 3, 5]])
    for f in (IT.trim_nans, IT.trim_nans2):
        with pytest.raises(NotImplementedError, match='colour'):
            f(np.zeros((4, 6, 3)))


def test_plan_masks_go_by_truth_value(recording):
    lib, plans = recording
    p = _lib.get_plan((2, 3), 1)
    assert np.array_equal(p._mask(np.array([[0.5, 0, 256], [0, -1, 1e-30]])), [[1, 0, 1], [0, 1, 1]])
    assert p._mask(np.ones((2, 3), dtype=bool)).dtype == np.uint8


def test_fftbounds_is_the_existing_mirror():
    import pygpa_amd.geometric_phase_analysis as GPA
    assert IT.fftbounds is GPA.fftbounds


def test_no_cpu_fallback():
    lib = _lib.load()
    if lib.gpa_device_count() > 0:
        pytest.skip('a GPU is visible')
    with pytest.raises(_lib.GPAError):
        IT.gauss_homogenize2(np.ones((16, 16)), np.ones((16, 16), dtype=bool), 2.0)
    with pytest.raises(_lib.GPAError):
        IT.trim_nans2(np.ones((16, 16)))
