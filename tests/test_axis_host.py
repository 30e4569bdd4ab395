"""homogenize_per_axis without a GPU: the fixtures the reference wrote against the NumPy restatement of tests/axis_cases.py and
its derived bound, the header of the selection kernels (tests/host/lines_check.cpp, plain and under the host sanitizers -- an
ordinary executable), the C ABI's symbols and argument errors, and the Python mirror against a recording stand-in."""
import os
import re

import numpy as np
import pytest

from pygpa_amd import _lib
import pygpa_amd.imagetools as IT

import axis_cases as ac
import prep_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LINES_SYMBOLS = {'gpa_line_nanmedian': 6, 'gpa_homogenize_per_axis': 8, 'gpa_homogenize_lines': 7}


# ---- fixtures ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(ac.CASES))
def test_fixture_promises_and_restatement(name):
    z = ac.load(name)
    shape, sigma, _ = ac.CASES[name]
    image, mask, sigma2 = ac.case_inputs(name)
    assert z['image'].shape == shape and float(z['sigma']) == sigma == sigma2 and z['mask'].dtype == np.bool_
    assert np.array_equal(z['image'], image) and np.array_equal(z['mask'], mask)
    assert os.path.getsize(os.path.join(ac.GOLDEN, name + '.npz')) < 1 << 20
    if name not in ac.THIN:     # the mask's special lines: a column with ONE valid sample, a row with TWO, none empty
        assert (mask.sum(axis=0) == 1).sum() == 1 and (mask.sum(axis=1) == 2).sum() == 1
    assert mask.sum(axis=0).min() >= 1 and mask.sum(axis=1).min() >= 1 and 0.75 <= mask.mean() <= 0.97
    for variant in ac.VARIANTS:
        img, m = ac.variant_inputs(z, variant)
        ref, p0, p1 = z['out_' + variant], z['p0_' + variant], z['p1_' + variant]
        assert ref.dtype == p0.dtype == p1.dtype == img.dtype and p0.shape == (shape[1],) and p1.shape == (shape[0],)
        # the promises the bound rests on: finite, positive profiles (so positive medians), q within 0.5 .. 1
        assert np.isfinite(ref).all() and p0.min() > 0 and p1.min() > 0
        for p in (p0, p1):
            q = p / p.max()
            assert 0.5 <= q.min() and q.max() <= 1.0
        out, r0, r1, res0 = ac.restate(img, sigma, m)
        src = img if m is None else np.where(m, img, np.nan)
        assert np.nanmedian(src, axis=0).min() > 0 and np.nanmedian(res0 if m is None else np.where(m, res0, np.nan), axis=1).min() > 0
        e0, e1, eo = ac.bounds(sigma, img.dtype)
        d = ac.rel_dev(r0, p0, img.dtype), ac.rel_dev(r1, p1, img.dtype), ac.rel_dev(out, ref, img.dtype)
        print('%s %s: restatement / reference in eps: profiles %.2f %.2f out %.2f (bounds %d %d %d)' % ((name, variant) + d + (e0, e1, eo)))
        assert d[0] <= e0 and d[1] <= e1 and d[2] <= eo


def test_nan_fixture_is_all_nan():
    z = ac.load(ac.NAN_CASE)
    image, mask, sigma = ac.case_inputs(ac.NAN_CASE)
    assert np.array_equal(z['image'], image) and np.array_equal(z['mask'], mask)
    assert (mask.sum(axis=0) == 0).sum() == 1
    for variant in ac.VARIANTS:
        img, m = ac.variant_inputs(z, variant)
        out = ac.restate(img, sigma, m)[0]
        if m is None:
            assert np.isfinite(z['out_' + variant]).all() and ac.rel_dev(out, z['out_' + variant], img.dtype) <= ac.bounds(sigma, img.dtype)[2]
        else:       # one line without a sample: the NaN median reaches every pixel through profile.max()
            assert np.isnan(z['out_' + variant]).all() and np.isnan(out).all() and z['out_' + variant].size == 2400


def test_bound_is_the_documented_chain():
    A = 2 * 800 + 2
    assert ac.bounds(200.0, np.float64) == (3 * A + 3, 9 * A + 15, 24 * A + 44)
    assert ac.bounds(200.0, np.float32) == (3, 15, 44) == ac.bounds(1.0, np.float32)
    e_p0 = 3 * A + 3
    e_q0 = 2 * e_p0 + 2
    e_r0 = e_q0 + 2
    e_m1 = e_r0 + 2 + 100
    e_p1 = e_m1 + 3 * A + 3
    assert ac.bounds(200.0, np.float64, m1_extra=100) == (e_p0, e_p1, e_r0 + 2 * e_p1 + 2 + 2)


def test_median_rule_is_numpys_bits():
    """fact 1 of the design: nanmedian is v[m // 2] or one rounded addition and an exact halving, in both precisions"""
    rng = np.random.default_rng(3)
    for dtype in (np.float32, np.float64):
        for m in range(1, 12):
            a = (2000 + rng.standard_normal((50, m))).astype(dtype)
            v = np.sort(a, axis=1)
            want = v[:, m // 2] if m % 2 else (v[:, m // 2 - 1] + v[:, m // 2]) * dtype(0.5)
            assert np.array_equal(np.nanmedian(a, axis=1), want)


# ---- the header ------------------------------------------------------------------------------------------------------------
def _run_check(tmp_path_factory, extra):
    if extra and not pc.host_compiler_links(tmp_path_factory.mktemp('probe'), extra):
        pytest.skip('the host compiler has no sanitizer runtimes')
    r, out = ac.lines_check(tmp_path_factory.mktemp('linescheck'), extra)
    assert r.returncode == 0, r.stderr[-2000:]
    assert out.returncode == 0, (out.stdout + out.stderr)[-2000:]
    assert out.stdout.startswith('OK ') and int(out.stdout.split()[1]) > 100000


def test_lines_header(tmp_path_factory):
    _run_check(tmp_path_factory, [])


def test_lines_header_sanitized(tmp_path_factory):
    _run_check(tmp_path_factory, ['-fsanitize=address,undefined', '-fno-sanitize-recover=all'])


def test_fold_matches_prep_cases():
    """the header's fold, evaluated by the host check against a walk, is the rule of prep_cases.fold: the same walk here"""
    for n in (1, 2, 5, 33):
        ext = np.concatenate([np.arange(n), np.arange(n)[::-1]])
        i = np.arange(-1700, 1700)
        assert np.array_equal(pc.fold(i, n), ext[np.mod(i, 2 * n)])


# ---- the C ABI -------------------------------------------------------------------------------------------------------------
def test_symbols_in_header_and_signatures():
    header = open(os.path.join(ROOT, 'include', 'gpa_hip.h')).read()
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    for base, n in LINES_SYMBOLS.items():
        for name in (base, base + '_dev'):
            m = re.search(r'\bint\s+%s\s*\(([^)]*)\)\s*;' % name, header)
            assert m, name
            nargs = len([a for a in m.group(1).split(',') if a.strip()])
            res, args = _lib.SIGNATURES[name]
            assert nargs == len(args) == n and res is _lib._i, name
    assert ('#define GPA_LINES_MAX_N %d' % _lib.LINES_MAX_N) in header
    assert ('LINES_MAX_N = %d;' % _lib.LINES_MAX_N) in open(os.path.join(ROOT, 'pygpa_amd', 'csrc', 'gpa_lines.h')).read()


def test_library_argument_errors_need_no_device():
    lib = _lib.load()
    P = _lib._ptr
    a = np.ones((8, 8))
    for sfx in ('', '_dev'):
        calls = [lambda f: f(None, P(a), None, 0, 0, P(a)), lambda f: f(None, P(a), None, 3.0, 0, 1, P(a), None),
                 lambda f: f(None, P(a), 3.0, P(a), None, P(a), None)]
        for base, call in zip(LINES_SYMBOLS, calls):
            assert call(getattr(lib, base + sfx)) == -1
            assert 'plan' in _lib.last_error() and (base + sfx) in _lib.last_error()


# ---- the mirror against a recording stand-in -------------------------------------------------------------------------------
class _RecordingLib:
    def __init__(self):
        self.calls = []

    def gpa_homogenize_per_axis(self, handle, image, mask, sigma, propagate, nb, out, prof):
        self.calls.append(('per_axis', sigma, propagate, nb, mask is None, prof is None))
        return 0

    def gpa_homogenize_lines(self, handle, image, sigma, line0, line1, out, prof):
        self.calls.append(('lines', sigma, line1 is None))
        return 0

    def gpa_line_nanmedian(self, handle, image, mask, axis, propagate, out):
        self.calls.append(('median', axis, propagate, mask is None))
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


@pytest.mark.parametrize('kw, exc', [
    (dict(mask=np.ones((6, 7))), TypeError), (dict(mask=np.ones((6, 7), dtype=np.uint8)), TypeError),
    (dict(mask=np.ones((6, 6), dtype=bool)), ValueError), (dict(sigma=0), ValueError), (dict(sigma=-1.0), ValueError),
    (dict(sigma=float('nan')), ValueError), (dict(sigma=float('inf')), ValueError), (dict(sigma=[2.0, 3.0]), ValueError),
    (dict(image=np.ones((2, 6, 7))), ValueError), (dict(image=np.ones((6, 7), dtype=complex)), TypeError),
    (dict(image=np.ones((3, 7))), ValueError), (dict(dtype=np.int32), ValueError), (dict(reducfunc=3), TypeError)])
def test_argument_errors_before_the_library(recording, kw, exc):
    lib, plans = recording
    args = dict(image=np.full((6, 7), 5.0), mask=np.ones((6, 7), dtype=bool), sigma=2.0, dtype=None, reducfunc=np.nanmedian)
    args.update(kw)
    with pytest.raises(exc):
        IT.homogenize_per_axis(args['image'], args['sigma'], args['mask'], args['reducfunc'], dtype=args['dtype'])
    assert not lib.calls and not plans
    if 'reducfunc' not in kw and 'image' not in kw:
        with pytest.raises(exc):
            IT.homogenize_per_axis_stack(np.full((2, 6, 7), 5.0), args['sigma'], args['mask'], dtype=args['dtype'])
        assert not lib.calls and not plans


def test_mirror_calls(recording, monkeypatch):
    lib, plans = recording
    img = np.arange(42.0).reshape(6, 7) + 1
    mask = np.ones((6, 7), dtype=bool)
    out = IT.homogenize_per_axis(img)                                     # the reference's defaults: sigma 200, no mask, nanmedian
    assert out.shape == (6, 7) and out.dtype == np.float64
    IT.homogenize_per_axis(img, 3, mask, np.median, dtype=np.float32)
    assert plans[-1].rdtype == np.float32
    assert lib.calls == [('per_axis', 200.0, 0, 1, True, True), ('per_axis', 3.0, 1, 1, False, True)]
    lib.calls.clear()
    # a foreign reducfunc is called on the host as the reference calls it, once per axis; only its lines go down
    seen = []

    def reduc(a, axis, keepdims):
        seen.append((a.shape, axis, keepdims, bool(np.isnan(a).any())))
        return np.nanmean(a, axis=axis, keepdims=keepdims)
    mask[2, 3] = False
    IT.homogenize_per_axis(img, 5, mask, reduc)
    assert seen == [((6, 7), 0, True, True), ((6, 7), 1, True, True)]
    assert lib.calls == [('lines', 5.0, True), ('lines', 5.0, False)]
    with pytest.raises(ValueError, match='shape'):
        IT.homogenize_per_axis(img, 5, mask, lambda a, axis, keepdims: np.nanmean(a, axis=axis))
    lib.calls.clear()
    # the stack goes down in chunks of whole frames
    monkeypatch.setattr(IT, 'AXIS_CHUNK_BYTES', 3 * 6 * 7 * 8)
    st = IT.homogenize_per_axis_stack(np.ones((7, 6, 7)), 4.0, mask)
    assert st.shape == (7, 6, 7) and [c[3] for c in lib.calls] == [3, 3, 1] and all(c[0] == 'per_axis' and c[2] == 0 for c in lib.calls)
    lib.calls.clear()
    # the primitive: short axes are repeated four times, the result keeps the reference's shapes
    m = IT.nanmedian_lines(np.ones((1, 7)), 0)
    assert m.shape == (1, 7) and plans[-1].shape == (4, 7)
    m = IT.nanmedian_lines(np.ones((7, 1)), 0, keepdims=False)
    assert m.shape == (1,) and plans[-1].shape == (7, 4)
    assert IT.nanmedian_lines(np.ones((9, 5)), 1, mask=np.ones((9, 5), dtype=bool)).shape == (9, 1)
    assert [c[1:] for c in lib.calls] == [(0, 0, True), (0, 0, True), (1, 0, False)]
    for bad, exc in ((dict(axis=2), ValueError), (dict(mask=np.ones((9, 5))), TypeError), (dict(image=np.ones((2, 9, 5))), NotImplementedError),
                     (dict(image=np.ones((9, _lib.LINES_MAX_N + 1)), axis=1), ValueError)):
        args = dict(image=np.ones((9, 5)), axis=1, mask=None)
        args.update(bad)
        with pytest.raises(exc):
            IT.nanmedian_lines(args['image'], args['axis'], mask=args['mask'])


def test_repeating_a_line_four_times_keeps_its_median():
    rng = np.random.default_rng(9)
    for m in range(1, 8):
        a = rng.standard_normal((20, m))
        a[rng.random(a.shape) < 0.2] = np.nan
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter('ignore', RuntimeWarning)
            assert np.array_equal(np.nanmedian(np.tile(a, (1, 4)), axis=1), np.nanmedian(a, axis=1), equal_nan=True)
            assert np.array_equal(np.median(np.tile(a, (1, 4)), axis=1), np.median(a, axis=1), equal_nan=True)


def test_no_cpu_fallback():
    lib = _lib.load()
    if lib.gpa_device_count() > 0:
        pytest.skip('a GPU is visible')
    with pytest.raises(_lib.GPAError):
        IT.homogenize_per_axis(np.ones((16, 16)), 2.0)
    with pytest.raises(_lib.GPAError):
        IT.nanmedian_lines(np.ones((16, 16)), 0)
