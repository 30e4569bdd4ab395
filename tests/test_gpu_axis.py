"""Per-line medians and homogenize_per_axis on the device (pygpa_amd.imagetools, gpa_line_nanmedian / gpa_homogenize_per_axis /
gpa_homogenize_lines).  Run with `-m gpu` on an MI355X.

Medians are held to NumPy bit for bit (np.nanmedian / np.median computed here).  homogenize_per_axis is held to the fixtures the
reference's own function wrote (tests/golden/axis_*.npz, tools/make_axis_golden.py): the NaN pattern exactly, the two profiles
and the output within the derived relative bounds of axis_cases.bounds; the measured figures are printed and recorded in
axis_cases.C_MEASURED."""
import warnings

import numpy as np
import pytest

from pygpa_amd import _lib
import pygpa_amd.imagetools as IT

import axis_cases as ac

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
SHAPES = [(1, 1), (1, 7), (7, 1), (5, 50), (50, 5), (33, 150), (64, 64), (257, 300)]
CONTENTS = ('smooth', 'bits', 'special', 'equal', 'ties')


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def content(kind, shape, dtype, rng):
    if kind == 'smooth':        # keys that share their top three bytes
        return (2000.0 + 1e-3 * (2.0 * rng.random(shape) - 1.0)).astype(dtype)
    if kind == 'bits':          # random bit patterns over all exponents (NaNs and infinities among them): every radix pass decides
        u = np.dtype(dtype).itemsize
        raw = rng.integers(0, 256, size=shape + (u,), dtype=np.uint8)
        return raw.view(dtype).reshape(shape)
    if kind == 'special':
        tiny = np.finfo(dtype).smallest_subnormal
        # (nothing above max / 2: where one sample is the middle, NumPy's small-array path forms (v + v) / 2, which overflows there)
        pool = np.array([-3.5, -1.0, -0.0, 0.0, 1.0, 1.0, 2.0, np.inf, -np.inf, np.nan, tiny, -tiny, 3 * tiny, np.finfo(dtype).tiny,
                         np.finfo(dtype).max / 4, -np.finfo(dtype).max / 4], dtype=dtype)
        return pool[rng.integers(0, len(pool), size=shape)]
    if kind == 'equal':         # all-equal lines along both axes, NaN sprinkled
        a = np.full(shape, 7.25, dtype=dtype)
        a[rng.random(shape) < 0.1] = np.nan
        return a
    a = rng.integers(1, 4, size=shape).astype(dtype)      # ties straddling the middle
    return a


def line_mask(shape, axis, rng):
    """30 % holes; along `axis`: line 0 without a sample, line 1 with ONE, line 2 with TWO, where the image has such lines"""
    mask = rng.random(shape) >= 0.3
    m = mask if axis == 1 else mask.T       # lines are rows of m
    n = m.shape[1]
    for line, count in ((0, 0), (1, 1), (2, 2)):
        if line < m.shape[0]:
            m[line, :] = False
            m[line, rng.permutation(n)[:min(count, n)]] = True
    return mask


def numpy_median(image, mask, axis, propagate):
    src = image if mask is None else np.where(mask, image, np.nan).astype(image.dtype)
    with warnings.catch_warnings(), np.errstate(all='ignore'):
        warnings.simplefilter('ignore', RuntimeWarning)
        return (np.median if propagate else np.nanmedian)(src, axis=axis, keepdims=True)


# ---- 1. medians, bit for bit -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%d' % s)
def test_medians_are_numpys_bits(shape, dtype):
    rng = np.random.default_rng(1000 * shape[0] + shape[1])
    for kind in CONTENTS:
        image = content(kind, shape, dtype, rng)
        for axis in (0, 1):
            for mask in (None, line_mask(shape, axis, rng)):
                got = IT.nanmedian_lines(image, axis, mask=mask, dtype=dtype)
                want = numpy_median(image, mask, axis, False)
                assert same(got, want), (kind, axis, mask is not None, np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))[:4])
                assert same(IT.nanmedian_lines(image, axis, mask=mask, keepdims=False, dtype=dtype), want.ravel())
                if min(shape) >= 4:     # np.median semantics through the plan (the mirror exposes nanmedian)
                    plan = _lib.get_plan(shape, 1, dtype)
                    got = plan.line_nanmedian(image, axis, mask, propagate_nan=True)
                    assert same(got, numpy_median(image, mask, axis, True).ravel()), (kind, axis, mask is not None)


@pytest.mark.parametrize('dtype', DTYPES)
def test_valid_counts_zero_to_nine(dtype):
    """rows with m = 0 .. 9 valid samples among NaNs, odd and even, from a small pool so that ties straddle the middle"""
    rng = np.random.default_rng(5)
    image = rng.integers(-2, 3, size=(40, 12)).astype(dtype) * dtype(0.5)
    for i in range(40):
        image[i, rng.permutation(12)[:12 - i % 10]] = np.nan
    assert same(IT.nanmedian_lines(image, 1, dtype=dtype), numpy_median(image, None, 1, False))
    assert same(IT.nanmedian_lines(image.T.copy(), 0, dtype=dtype), numpy_median(image.T, None, 0, False))


@pytest.mark.parametrize('dtype', DTYPES)
def test_longest_lines(dtype):
    """8 x 16384 and 16384 x 8: the LDS maximum; one more sample is refused with GPA_ERR_ARG"""
    rng = np.random.default_rng(6)
    n = _lib.LINES_MAX_N
    image = (2000.0 + 50.0 * rng.standard_normal((8, n))).astype(dtype)
    image[1] = content('smooth', (n,), dtype, rng)
    image[2] = content('bits', (n,), dtype, rng)
    image[3, rng.random(n) < 0.5] = np.nan
    image[4, 1:] = np.nan
    mask = rng.random((8, n)) >= 0.2
    for m in (None, mask):
        assert same(IT.nanmedian_lines(image, 1, mask=m, dtype=dtype), numpy_median(image, m, 1, False))
        mt = None if m is None else m.T.copy()
        assert same(IT.nanmedian_lines(image.T.copy(), 0, mask=mt, dtype=dtype), numpy_median(image.T, mt, 0, False))
    plan = _lib.Plan((8, n + 1), 1, dtype)
    try:
        with pytest.raises(_lib.GPAError, match=r'\(-1\).*GPA_LINES_MAX_N'):
            plan.line_nanmedian(np.ones((8, n + 1)), 1)
        assert plan.line_nanmedian(np.ones((8, n + 1)), 0).shape == (n + 1,)       # the other axis is not bound by the limit
        with pytest.raises(_lib.GPAError, match=r'\(-1\)'):
            plan.homogenize_per_axis(np.ones((8, n + 1)), 2.0)
    finally:
        plan.close()


# ---- 2. homogenize_per_axis against the reference's fixtures ---------------------------------------------------------------------
@pytest.fixture(scope='module')
def fixtures():
    return {name: ac.load(name) for name in list(ac.CASES) + [ac.NAN_CASE]}


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name', list(ac.CASES))
def test_homogenize_against_the_reference(fixtures, name, dtype):
    z = fixtures[name]
    sigma = float(z['sigma'])
    e0, e1, eo = ac.bounds(sigma, dtype)
    for variant in ac.VARIANTS:
        if not variant.startswith('f32' if dtype == np.float32 else 'f64'):
            continue
        img, mask = ac.variant_inputs(z, variant)
        out, p0, p1 = _lib.get_plan(img.shape, 1, dtype).homogenize_per_axis(img, sigma, mask, want_profiles=True)
        assert out.dtype == p0.dtype == p1.dtype == np.dtype(dtype) and out.shape == img.shape
        assert not np.isnan(out).any() and not np.isnan(p0).any() and not np.isnan(p1).any()
        d = ac.rel_dev(p0, z['p0_' + variant], dtype), ac.rel_dev(p1, z['p1_' + variant], dtype), ac.rel_dev(out, z['out_' + variant], dtype)
        print("MEASURED '%s': {'%s': (%.3f, %.3f, %.3f)}  bounds (%d, %d, %d)" % ((name, variant) + d + (e0, e1, eo)))
        assert d[0] <= e0 and d[1] <= e1 and d[2] <= eo, d
        assert same(IT.homogenize_per_axis(z['image'], sigma, mask, dtype=dtype), out)


@pytest.mark.parametrize('dtype', DTYPES)
def test_one_empty_line_turns_everything_nan(fixtures, dtype):
    z = fixtures[ac.NAN_CASE]
    sigma = float(z['sigma'])
    variant = 'f32' if dtype == np.float32 else 'f64'
    out = IT.homogenize_per_axis(z['image'], sigma, z['mask'], dtype=dtype)
    assert np.isnan(z['out_%s_mask' % variant]).all() and np.isnan(out).all() and out.shape == (40, 60)
    out = IT.homogenize_per_axis(z['image'], sigma, dtype=dtype)
    assert not np.isnan(out).any() and ac.rel_dev(out, z['out_%s_nomask' % variant], dtype) <= ac.bounds(sigma, dtype)[2]


# ---- 3. identities -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
def test_stack_dev_and_reuse(fixtures, dtype, monkeypatch):
    z = fixtures['axis_33x150_s10']
    image, mask, sigma = z['image'], z['mask'], float(z['sigma'])
    shape = image.shape
    rng = np.random.default_rng(8)
    frames = np.stack([image, image[::-1] * 1.25, image + 30.0 * rng.standard_normal(shape), image[:, ::-1]])
    singles = [IT.homogenize_per_axis(f, sigma, mask, dtype=dtype) for f in frames]
    # frame b of the stack equals the single call bit for bit: in one device call, and in chunks of two frames
    assert same(IT.homogenize_per_axis_stack(frames, sigma, mask, dtype=dtype), np.stack(singles))
    monkeypatch.setattr(IT, 'AXIS_CHUNK_BYTES', 2 * image.size * np.dtype(dtype).itemsize)
    assert same(IT.homogenize_per_axis_stack(frames, sigma, mask, dtype=dtype), np.stack(singles))
    assert same(IT.homogenize_per_axis_stack(frames, sigma, dtype=dtype), np.stack([IT.homogenize_per_axis(f, sigma, dtype=dtype) for f in frames]))
    plan = _lib.Plan(shape, 1, dtype)
    try:
        out, p0, p1 = plan.homogenize_per_axis(image, sigma, mask, want_profiles=True)
        assert same(out, singles[0])
        # work space is counted, and a repeated call leaves it alone
        item = np.dtype(dtype).itemsize
        before = plan.workspace_bytes
        outs, q0, q1 = plan.homogenize_per_axis(frames, sigma, mask, want_profiles=True)
        grown = plan.workspace_bytes
        assert grown - before >= 3 * image.size * item        # three more transposed planes, at the least
        assert same(outs, np.stack(singles)) and same(q0[0], p0) and same(q1[0], p1)
        plan.homogenize_per_axis(frames, sigma, mask)
        assert plan.workspace_bytes == grown
        # plan reuse: another sigma, another plan of a different shape in between, the same bits afterwards
        plan.homogenize_per_axis(image, 2.0, mask)
        IT.homogenize_per_axis(fixtures['axis_48x80_s3']['image'], 3.0, dtype=dtype)
        assert same(plan.homogenize_per_axis(image, sigma, mask), singles[0])
        # host form == _dev form, profiles included; the inputs stay as they were
        img_t, m8 = image.astype(dtype), mask.astype(np.uint8)
        bufs = [_lib.DeviceBuffer(img_t.nbytes), _lib.DeviceBuffer(img_t.nbytes), _lib.DeviceBuffer(m8.nbytes),
                _lib.DeviceBuffer((shape[0] + shape[1]) * item)]
        d_img, d_out, d_mask, d_prof = bufs
        try:
            d_img.upload(img_t)
            d_mask.upload(m8 * 200)         # a mask byte is true whatever its value
            IT.homogenize_per_axis_dev(plan, d_img.ptr, d_mask.ptr, d_out.ptr, sigma, profiles_ptr=d_prof.ptr)
            plan.sync()
            assert same(d_out.download(shape, dtype), singles[0])
            assert same(d_prof.download((shape[0] + shape[1],), dtype), np.concatenate([p0, p1]))
            assert same(d_img.download(shape, dtype), img_t) and np.array_equal(d_mask.download(shape, np.uint8), m8 * 200)
            IT.homogenize_per_axis_dev(plan, d_img.ptr, None, d_out.ptr, sigma)
            plan.sync()
            assert same(d_out.download(shape, dtype), IT.homogenize_per_axis(image, sigma, dtype=dtype))
            d_med = _lib.DeviceBuffer(shape[1] * item)
            bufs.append(d_med)
            plan.line_nanmedian_dev(d_img.ptr, d_mask.ptr, 0, d_med.ptr)
            plan.sync()
            assert same(d_med.download((shape[1],), dtype), plan.line_nanmedian(image, 0, mask))
        finally:
            for b in bufs:
                b.free()
    finally:
        plan.close()


@pytest.mark.parametrize('dtype', DTYPES)
def test_median_and_foreign_reducfunc(fixtures, dtype):
    import scipy.ndimage as ndi
    z = fixtures['axis_48x80_s3']
    image, mask, sigma = z['image'], z['mask'], float(z['sigma'])
    # np.median: without a mask and without NaNs it is the nanmedian; one hole in the mask turns everything NaN, as in the reference
    assert same(IT.homogenize_per_axis(image, sigma, reducfunc=np.median, dtype=dtype), IT.homogenize_per_axis(image, sigma, dtype=dtype))
    hole = np.ones(image.shape, dtype=bool)
    hole[20, 30] = False
    assert np.isnan(IT.homogenize_per_axis(image, sigma, hole, np.median, dtype=dtype)).all()
    assert not np.isnan(IT.homogenize_per_axis(image, sigma, hole, dtype=dtype)).any()
    # a foreign reducfunc: the reference's expression, evaluated here
    img_t = image.astype(dtype)
    ref = img_t.copy()
    for axis in (0, 1):
        prof = ndi.gaussian_filter(np.nanmean(np.where(mask, ref, np.nan), axis=axis, keepdims=True), sigma=sigma)
        ref /= prof / prof.max()
    got = IT.homogenize_per_axis(image, sigma, mask, np.nanmean, dtype=dtype)
    bound = ac.bounds(sigma, dtype, m1_extra=2 * image.shape[1])[2]
    d = ac.rel_dev(got, ref, dtype)
    print('nanmean %s: max relative deviation %.3f eps (bound %d)' % (np.dtype(dtype).name, d, bound))
    assert got.dtype == np.dtype(dtype) and d <= bound
    # the device's own medians handed back as lines give the device's result, bit for bit
    plan = _lib.get_plan(image.shape, 1, dtype)
    out = plan.homogenize_per_axis(image, sigma, mask)
    line0 = plan.line_nanmedian(image, 0, mask)
    res0 = plan.homogenize_lines(image, sigma, line0)
    line1 = plan.line_nanmedian(res0, 1, mask)
    assert same(plan.homogenize_lines(image, sigma, line0, line1), out)


# ---- 4. the fused loads are real ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name', ['axis_33x150_s10', 'axis_70x300_s1'])
def test_axis1_medians_are_those_of_the_divided_image(fixtures, name, dtype):
    """sigma = 0.1 gives R = 0, the one tap 1.0: the returned profiles ARE the medians.  res after axis 0, recomputed on the host
    as image / q0, has row medians equal to the device's axis-1 medians bit for bit, though the device never stored res."""
    z = fixtures[name]
    img_t = z['image'].astype(dtype)
    for mask in (None, z['mask']):
        plan = _lib.get_plan(img_t.shape, 1, dtype)
        out, p0, p1 = plan.homogenize_per_axis(img_t, 0.1, mask, want_profiles=True)
        assert same(p0, numpy_median(img_t, mask, 0, False).ravel())
        q0 = p0 / p0.max()
        res0 = img_t / q0[None, :]
        assert res0.dtype == np.dtype(dtype)
        assert same(p1, numpy_median(res0, mask, 1, False).ravel())
        assert not same(p1, numpy_median(img_t, mask, 1, False).ravel())       # ... and not those of the undivided image
        q1 = p1 / p1.max()
        assert same(out, res0 / q1[:, None])
