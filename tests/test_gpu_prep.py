"""Image preparation on the device (pygpa_amd.imagetools, gpa_gauss_homogenize / gpa_mask_* / gpa_nan_*) against
the fixtures the reference's own imagetools wrote (tests/golden/prep_*.npz, tools/make_prep_golden.py).  Run with `-m gpu` on
an MI355X.

Exact, in both precisions: the masks for every r, chunked == one call, the bounds, the trims, and the NaN / nan_scale pattern
of out and VV.  Accuracy, at every pixel where the reference's den > 0:

    |VV - VV_ref| <= b = 128 eps M / den_ref          M: the largest masked sample, eps: the unit round-off (2^-24 / 2^-53)
    |out - out_ref| <= |image| b / (VV_ref (VV_ref - b))    a pixel is left out only where b >= VV_ref / 2, never under the mask

on the FFT route (GAUSS_FFT_MINR = 1) and on the direct route (GAUSS_FFT_MINR = 100000) alike.  128 is derived (prep_cases.C_VV),
the measured figures are printed and recorded in prep_cases.C_MEASURED."""
import numpy as np
import pytest

from pygpa_amd import _lib
import pygpa_amd.geometric_phase_analysis as GPA
import pygpa_amd.imagetools as IT
from pygpa_amd.synthetic import hex_kvecs, explicit_klists, gaussian_bump_displacement, hex_moire

import prep_cases as pc
from test_gpu_plan_state import same

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
ROUTES = {'fft': '1', 'direct': '100000'}


ROUTE_KERNELS = {'fft': {'prep_cols_kernel', 'prep_rows_kernel'}, 'direct': {'prep_cols_direct_kernel', 'prep_rows_direct_kernel'}}
ALL_ROUTE_KERNELS = ROUTE_KERNELS['fft'] | ROUTE_KERNELS['direct'] | {'gauss_fft_rows_kernel', 'prep_finish_kernel'}


def _kernels_of_a_call(plan, image, mask, sigma):
    """names of the kernels one profiled homogenisation launched"""
    plan.set_profiling(True)
    try:
        plan.gauss_homogenize(image, mask, sigma)
        return set(plan.last_kernel_profile())
    finally:
        plan.set_profiling(False)


@pytest.fixture(scope='module')
def fixtures():
    return {name: pc.load(name) for name in list(pc.H_CASES) + ['prep_mask', 'prep_trim']}


def _check_homogenize(z, dtype, out_none, vv, out_1, label):
    eps = pc.EPS[np.dtype(dtype)]
    image, mask, VVr, den = z['image'], z['mask'], z['VV'], z['den']
    assert out_none.dtype == vv.dtype == out_1.dtype == np.dtype(dtype) and out_none.shape == vv.shape == image.shape
    # the patterns, exactly
    assert np.array_equal(np.isnan(vv), np.isnan(VVr))
    assert np.array_equal(np.isnan(out_none), np.isnan(z['out_none']))
    assert np.array_equal(np.isnan(out_1), np.isnan(z['out_1']))
    empty = np.isnan(VVr)
    img_t = image.astype(dtype)
    assert np.array_equal(out_1[empty], img_t[empty], equal_nan=True)       # image / nan_scale with nan_scale = 1
    # VV
    ok = den > 0
    assert np.array_equal(ok, ~empty)
    M = image[mask].max()
    b = pc.C_VV * eps * M / den[ok]
    err = np.abs(vv[ok].astype(np.float64) - VVr[ok])
    measured = (err * den[ok] / (eps * M)).max()
    print('%s: max |VV - VV_ref| den_ref / (eps M) = %.3f (bound %g)' % (label, measured, pc.C_VV))
    assert np.all(err <= b), measured
    # out, nan_scale None and 1
    bb = np.zeros(image.shape)
    bb[ok] = b
    use = ok & (bb < VVr / 2) & ~np.isnan(image)
    left_out = ok & ~(bb < VVr / 2)
    assert not np.any(left_out & mask)
    if np.dtype(dtype) == np.float64:
        assert not left_out.any()
    tol = np.abs(image[use]) * bb[use] / (VVr[use] * (VVr[use] - bb[use]))
    for got, ref in ((out_none, z['out_none']), (out_1, z['out_1'])):
        e = np.abs(got[use].astype(np.float64) - ref[use])
        print('%s: max |out - out_ref| / bound = %.4f' % (label, (e / tol).max()))
        assert np.all(e <= tol), (e / tol).max()
    return measured


@pytest.mark.parametrize('route', list(ROUTES))
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name', list(pc.H_CASES))
def test_homogenize_routes(fixtures, gpa_option, name, dtype, route):
    z = fixtures[name]
    gpa_option('GAUSS_FFT_MINR', ROUTES[route])
    plan = _lib.Plan(z['image'].shape, 1, dtype)
    try:
        out_none, vv = plan.gauss_homogenize(z['image'], z['mask'], float(z['sigma']), want_vv=True)
        out_1 = plan.gauss_homogenize(z['image'], z['mask'], float(z['sigma']), nan_scale=1)
        ran = _kernels_of_a_call(plan, z['image'], z['mask'], float(z['sigma']))
    finally:
        plan.close()
    # the switch chose the route: the kernels of one route and none of the other
    assert ran & ALL_ROUTE_KERNELS == ROUTE_KERNELS[route], ran
    _check_homogenize(z, dtype, out_none, vv, out_1, '%s %s %s' % (name, np.dtype(dtype).name, route))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name', list(pc.H_CASES))
def test_homogenize_mirror_default_route(fixtures, name, dtype):
    """through pygpa_amd.imagetools with no switch set: R = 10 runs direct, the others as FFT convolutions"""
    z = fixtures[name]
    sigma = float(z['sigma'])
    out_none = IT.gauss_homogenize2(z['image'], z['mask'], sigma, dtype=dtype)
    out_1 = IT.gauss_homogenize3(z['image'], z['mask'], sigma, dtype=dtype)
    assert np.array_equal(out_1, IT.gauss_homogenize2(z['image'], z['mask'], sigma, nan_scale=1, dtype=dtype), equal_nan=True)
    _, vv = _lib.get_plan(z['image'].shape, 1, dtype).gauss_homogenize(z['image'], z['mask'], sigma, want_vv=True)
    _check_homogenize(z, dtype, out_none, vv, out_1, '%s %s default' % (name, np.dtype(dtype).name))
    ran = _kernels_of_a_call(_lib.get_plan(z['image'].shape, 1, dtype), z['image'], z['mask'], sigma)
    assert ran & ALL_ROUTE_KERNELS == ROUTE_KERNELS['fft' if pc.radius(sigma) >= 12 else 'direct'], ran
    # another nan_scale only moves the uncovered pixels
    out_7 = IT.gauss_homogenize2(z['image'], z['mask'], sigma, nan_scale=7.0, dtype=dtype)
    empty = np.isnan(z['VV'])
    assert np.array_equal(out_7[~empty], out_1[~empty], equal_nan=True)
    assert np.array_equal(out_7[empty], (z['image'].astype(dtype) / dtype(7.0))[empty], equal_nan=True)


@pytest.mark.parametrize('dtype', DTYPES)
def test_homogenize_closed_forms_and_equivalences(fixtures, dtype):
    z = fixtures['prep_h_96x130_s3']
    image, mask, sigma = z['image'], z['mask'], float(z['sigma'])
    shape = image.shape
    img_t = image.astype(dtype)
    plan = _lib.Plan(shape, 1, dtype)
    try:
        # mask all false: nothing is covered
        none = np.zeros(shape, dtype=bool)
        assert np.isnan(plan.gauss_homogenize(image, none, sigma)).all()
        assert np.array_equal(plan.gauss_homogenize(image, none, sigma, nan_scale=4.0), img_t / dtype(4.0), equal_nan=True)
        # run == run; vv_out NULL == vv_out given
        out, vv = plan.gauss_homogenize(image, mask, sigma, want_vv=True)
        out2, vv2 = plan.gauss_homogenize(image, mask, sigma, want_vv=True)
        assert np.array_equal(out, out2, equal_nan=True) and np.array_equal(vv, vv2, equal_nan=True)
        assert np.array_equal(plan.gauss_homogenize(image, mask, sigma), out, equal_nan=True)
        # host form == _dev form (mirror's and the plan's), with and without VV; the inputs stay as they were
        m8 = mask.astype(np.uint8)
        bufs = [_lib.DeviceBuffer(img_t.nbytes) for _ in range(3)] + [_lib.DeviceBuffer(m8.nbytes)]
        d_img, d_out, d_vv, d_mask = bufs
        try:
            d_img.upload(img_t)
            d_mask.upload(m8)
            IT.gauss_homogenize_dev(plan, d_img.ptr, d_mask.ptr, d_out.ptr, sigma, vv_ptr=d_vv.ptr)
            plan.sync()
            assert np.array_equal(d_out.download(shape, dtype), out, equal_nan=True)
            assert np.array_equal(d_vv.download(shape, dtype), vv, equal_nan=True)
            plan.gauss_homogenize_dev(d_img.ptr, d_mask.ptr, d_out.ptr, sigma, nan_scale=1)
            plan.sync()
            assert np.array_equal(d_out.download(shape, dtype), plan.gauss_homogenize(image, mask, sigma, nan_scale=1), equal_nan=True)
            assert np.array_equal(d_img.download(shape, dtype), img_t, equal_nan=True)
            assert np.array_equal(d_mask.download(shape, np.uint8), m8)
            # a mask byte is true whatever its value
            d_mask.upload(m8 * 200)
            plan.gauss_homogenize_dev(d_img.ptr, d_mask.ptr, d_out.ptr, sigma)
            plan.sync()
            assert np.array_equal(d_out.download(shape, dtype), out, equal_nan=True)
            # the resident trims and bounds
            assert np.array_equal(plan.nan_trim_lims_dev(d_img.ptr), plan.nan_trim_lims(image))
            assert same(plan.nan_lines_dev(d_img.ptr), plan.nan_lines(image))
            assert np.array_equal(IT.mask_bounds_dev(plan, d_mask.ptr).ravel(), plan.mask_bounds(mask))
        finally:
            for b in bufs:
                b.free()
    finally:
        plan.close()


@pytest.mark.parametrize('route', list(ROUTES))
@pytest.mark.parametrize('dtype', DTYPES)
def test_non_finite_under_the_mask_spreads_over_the_box(fixtures, gpa_option, dtype, route):
    """the rule of the C forms, on both routes: NaN in VV and out on at least the reference's (2R+1)^2 box, and nowhere on the
    direct route but there; the mirror refuses such input"""
    z = fixtures['prep_h_64x64_full_s4']
    sigma = float(z['sigma'])
    image = z['image'].copy()
    image[30, 20] = np.nan
    with pytest.raises(ValueError, match='non-finite'):
        IT.gauss_homogenize2(image, z['mask'], sigma, dtype=dtype)
    R = pc.radius(sigma)
    box = np.zeros(image.shape, dtype=bool)
    box[30 - R:30 + R + 1, 20 - R:20 + R + 1] = True
    gpa_option('GAUSS_FFT_MINR', ROUTES[route])
    plan = _lib.Plan(image.shape, 1, dtype)
    try:
        out, vv = plan.gauss_homogenize(image, z['mask'], sigma, want_vv=True)
        ran = _kernels_of_a_call(plan, image, z['mask'], sigma)
    finally:
        plan.close()
    assert ran & ALL_ROUTE_KERNELS == ROUTE_KERNELS[route], ran
    assert np.isnan(vv[box]).all() and np.isnan(out[box]).all()
    if route == 'direct':
        assert not np.isnan(vv[~box]).any()


@pytest.mark.parametrize('dtype', DTYPES)
def test_longest_segments(dtype):
    """a sigma that only the longest transform serves (16384 points in f32, 8192 in f64), where each pass is two launches: a
    small image under a radius many times its size, against the restatement, with the bound of the fixtures"""
    sigma = 600.0 if dtype is np.float32 else 300.0
    shape = (12, 70)
    image = pc.lattice_image(shape, 41)
    mask = np.zeros(shape, dtype=bool)
    mask[2:9, 10:33] = True
    mask[11, 69] = True
    image[0, 50] = image[7, 60] = np.nan
    out_ref, vv_ref, den = pc.restate_homogenize(image, mask, sigma)
    assert not pc.box_empty(mask, sigma).any()
    plan = _lib.Plan(shape, 1, dtype)
    try:
        out, vv = plan.gauss_homogenize(image, mask, sigma, want_vv=True)
        ran = _kernels_of_a_call(plan, image, mask, sigma)
        assert np.array_equal(plan.gauss_homogenize(image, mask, sigma), out, equal_nan=True)
    finally:
        plan.close()
    assert ran & ALL_ROUTE_KERNELS == {'prep_cols_kernel', 'gauss_fft_rows_kernel', 'prep_finish_kernel'}, ran
    eps, M = pc.EPS[np.dtype(dtype)], image[mask].max()
    measured = (np.abs(vv.astype(np.float64) - vv_ref) * den / (eps * M)).max()
    print('longest segments %s sigma %g: max |VV - VV_ref| den_ref / (eps M) = %.3f' % (np.dtype(dtype).name, sigma, measured))
    assert measured <= pc.C_VV
    assert np.array_equal(np.isnan(out), np.isnan(image))
    b = pc.C_VV * eps * M / den
    ok = ~np.isnan(image)
    assert np.all(b < vv_ref / 2)
    assert np.all(np.abs(out[ok].astype(np.float64) - out_ref[ok]) <= (np.abs(image) * b / (vv_ref * (vv_ref - b)))[ok])


@pytest.mark.parametrize('dtype', DTYPES)
def test_masks_exact(fixtures, dtype):
    z = fixtures['prep_mask']
    frames = z['stack'].astype(np.float64)
    value = float(z['mask_value'])
    shape = frames.shape[1:]
    for r in pc.MASK_RADII:
        got = IT.generate_mask(frames, value, r, dtype=dtype)
        assert got.dtype == np.bool_ and np.array_equal(got, z['mask_r%d' % r]), r
    assert np.array_equal(IT.generate_mask(frames, np.nan, dtype=dtype), z['mask_nan_r20'])
    plan = _lib.Plan(shape, 1, dtype)
    try:
        # chunked == one call
        whole = plan.mask_any_equal(frames, value)
        assert np.array_equal(whole.astype(bool), ~z['mask_r0'])
        parts = plan.mask_any_equal(frames[3:], value, plan.mask_any_equal(frames[:3], value))
        assert np.array_equal(parts, whole) and set(np.unique(whole)) <= {0, 1}
        # erosion: of the mask itself, of the inverted hits, in place on the device
        for r in (1, 20):
            assert np.array_equal(plan.mask_erode_disk(z['mask_r0'], r).astype(bool), z['mask_r%d' % r])
        d_hit, d_frames = _lib.DeviceBuffer(whole.nbytes), _lib.DeviceBuffer(frames.size * np.dtype(dtype).itemsize)
        try:
            d_frames.upload(frames.astype(dtype))
            plan.mask_any_equal_dev(d_frames.ptr, 2, value, d_hit.ptr)
            plan.mask_any_equal_dev(d_frames.ptr + 2 * whole.size * np.dtype(dtype).itemsize, 3, value, d_hit.ptr, accumulate=True)
            plan.sync()
            assert np.array_equal(d_hit.download(shape, np.uint8), whole)
            plan.mask_erode_disk_dev(d_hit.ptr, d_hit.ptr, 3, invert=True)
            plan.sync()
            assert np.array_equal(d_hit.download(shape, np.uint8).astype(bool), z['mask_r3'])
            assert np.array_equal(plan.mask_bounds_dev(d_hit.ptr), z['cull_lims_r3'])
        finally:
            d_hit.free()
            d_frames.free()
        # cull_by_mask: the bounds and the slice
        for r in (3, 20):
            lims = z['cull_lims_r%d' % r]
            assert np.array_equal(plan.mask_bounds(z['mask_r%d' % r]), lims)
            assert np.array_equal(IT.cull_by_mask(frames, z['mask_r%d' % r]), frames[:, lims[0]:lims[1], lims[2]:lims[3]])
        assert np.array_equal(plan.mask_bounds(np.zeros(shape, dtype=bool)), [shape[0], 0, shape[1], 0])
        with pytest.raises(ValueError):
            IT.cull_by_mask(frames, z['mask_r200'])
    finally:
        plan.close()


@pytest.mark.parametrize('dtype', DTYPES)
def test_trims_exact(fixtures, dtype):
    z = fixtures['prep_trim']
    for name in pc.TRIM_CASES:
        img = z[name + '_image']
        assert np.array_equal(IT.trim_nans(img, dtype=dtype), z[name + '_trim_nans'], equal_nan=True)
        if name + '_trim_nans2_empties' in z:
            with pytest.raises(ValueError):
                IT.trim_nans2(img, dtype=dtype)
            continue
        got, lims = IT.trim_nans2(img, return_lims=True, dtype=dtype)
        assert np.array_equal(lims, z[name + '_lims']) and np.array_equal(got, z[name + '_trim_nans2'])
        assert np.array_equal(IT.trim_nans2(img, dtype=dtype), z[name + '_trim_nans2'])
    with pytest.raises(ValueError):
        IT.trim_nans2(np.full((9, 7), np.nan), dtype=dtype)
    clean = np.arange(63.0).reshape(9, 7)
    t, lims = IT.trim_nans2(clean, return_lims=True, dtype=dtype)
    assert np.array_equal(t, clean) and np.array_equal(lims, [[0, 9], [0, 7]])
    # wider than the trim kernel's workgroup, down to a window of one row; the NaN of the last column leaves with its row
    wide = np.zeros((5, 2500))
    wide[0, 2100] = wide[4, 7] = wide[1, 1500] = wide[3, 2499] = np.nan
    t, lims = IT.trim_nans2(wide, return_lims=True, dtype=dtype)
    assert np.array_equal(lims, pc.restate_trim_lims(wide).reshape(2, 2)) and np.array_equal(lims, [[2, 3], [0, 2500]])


def test_plan_state_and_accounting(fixtures):
    shape = (64, 48)
    kv = hex_kvecs(0.12, 11.0)
    kw = np.linalg.norm(kv, axis=1).mean() / 2.5
    klists = np.stack(explicit_klists(kv, kw, 2, 2))
    img = hex_moire(shape, kv, gaussian_bump_displacement(shape), noise=0.1, seed=1)
    img = img - img.mean()
    mask = np.zeros(shape, dtype=bool)
    mask[10:40, 5:30] = True
    frames = np.ones((3,) + shape)
    plan = _lib.Plan(shape, 12, np.float64)
    try:
        before = plan.extract_displacement_field(img, kv, klists, 6.0, 3, kmax=5)
        b0 = plan.workspace_bytes

        def calls():
            plan.gauss_homogenize(img + 5.0, mask, 3.0, want_vv=True)
            plan.gauss_homogenize(img + 5.0, mask, 2.0)
            plan.mask_erode_disk(plan.mask_any_equal(frames, 1.0), 3, invert=True)
            plan.mask_bounds(mask)
            plan.nan_lines(img)
            plan.nan_trim_lims(img)
        calls()
        b1 = plan.workspace_bytes
        npx = shape[0] * shape[1]
        # work: num, den and two byte planes; staging: image, out, VV and the mask, or three frames and the hit plane; the tables
        assert b1 - b0 >= (2 * 8 + 2) * npx + max((3 * 8 + 1) * npx, (3 * 8 + 1) * npx) + 2 * 64 * (8 + 16)
        calls()
        assert plan.workspace_bytes == b1
        after = plan.extract_displacement_field(img, kv, klists, 6.0, 3, kmax=5)
        assert same(before, after)
    finally:
        plan.close()


def test_argument_errors_name_the_argument():
    shape = (16, 16)
    plan = _lib.Plan(shape, 1, np.float64)
    img = np.ones(shape)
    out = np.empty(shape)
    m = np.ones(shape, dtype=np.uint8)
    frames = np.ones((2,) + shape)
    lims = np.zeros(4, dtype=np.int32)
    rows = np.zeros(16, dtype=np.uint8)
    P = _lib._ptr
    ARG = -1
    lib, h = plan.lib, plan.handle

    def homog(fn, image=img, mask=m, sigma=2.0, o=out):
        return getattr(lib, fn)(h, P(image), P(mask), sigma, 0, 0.0, P(o), None)

    def anyeq(fn, f=frames, B=2, hit=m):
        return getattr(lib, fn)(h, P(f), B, 1.0, 0, P(hit))

    def erode(fn, i=m, r=1, o=m):
        return getattr(lib, fn)(h, P(i), 0, r, P(o))

    def bounds(fn, mask=m, l=lims):
        return getattr(lib, fn)(h, P(mask), P(l))

    def lines(fn, image=img, r=rows, c=rows):
        return getattr(lib, fn)(h, P(image), P(r), P(c))

    def trim(fn, image=img, l=lims):
        return getattr(lib, fn)(h, P(image), P(l))
    table = [
        ('gpa_gauss_homogenize', homog, [(dict(image=None), 'image'), (dict(mask=None), 'mask'), (dict(o=None), 'out'),
                                         (dict(sigma=0.0), 'sigma'), (dict(sigma=-1.0), 'sigma'), (dict(sigma=float('nan')), 'sigma'),
                                         (dict(sigma=float('inf')), 'sigma'), (dict(sigma=5000.0), 'sigma')]),
        ('gpa_mask_any_equal', anyeq, [(dict(f=None), 'frames'), (dict(hit=None), 'hit'), (dict(B=0), 'B')]),
        ('gpa_mask_erode_disk', erode, [(dict(i=None), 'in'), (dict(o=None), 'out'), (dict(r=-1), 'r'),
                                        (dict(r=_lib.PREP_MAX_R + 1), 'GPA_PREP_MAX_R')]),
        ('gpa_mask_bounds', bounds, [(dict(mask=None), 'mask'), (dict(l=None), 'lims')]),
        ('gpa_nan_lines', lines, [(dict(image=None), 'image'), (dict(r=None), 'rows'), (dict(c=None), 'cols')]),
        ('gpa_nan_trim_lims', trim, [(dict(image=None), 'image'), (dict(l=None), 'lims')]),
    ]
    try:
        for base, call, bad in table:
            assert call(base) == 0, (base, _lib.last_error())
            for kw, word in bad:
                for fn in (base, base + '_dev'):
                    code = call(fn, **kw)
                    assert code == ARG, (fn, kw, code)
                    msg = _lib.last_error()
                    assert fn + ':' in msg and word in msg, (fn, kw, msg)
        # the largest radius runs (everything is eaten)
        assert not plan.mask_erode_disk(m, _lib.PREP_MAX_R).any()
    finally:
        plan.close()


def test_chain_mask_homogenize_primary_ks():
    """generate_mask -> gauss_homogenize3 -> extract_primary_ks on one plan: a moire under a vignette with a dead corner gives
    its k-vectors within the reference's bar of 1.5 / size"""
    size = 256
    shape = (size, size)
    kv = hex_kvecs(0.1, 7.0)
    y, x = np.mgrid[:size, :size]
    vignette = np.exp(-((x - 140.0) ** 2 + (y - 110.0) ** 2) / (2 * 90.0 ** 2))
    image = 1000.0 * (3.5 + hex_moire(shape, kv)) * vignette
    frames = np.stack([image, image * 0.9])
    frames[:, :40, :40] = 0.0                                    # the dead corner, the sentinel of the detector
    plan = _lib.get_plan(shape, 1, np.float64)
    mask = IT.generate_mask(frames, 0.0, r=5)
    assert not mask[:45, :40].any() and not mask[:40, :45].any() and mask[60:190, 60:190].all()
    flat = IT.gauss_homogenize3(frames[0], mask, 20.0)
    assert _lib.get_plan(shape, 1, np.float64) is plan
    ks, _ = GPA.extract_primary_ks(flat, DoG=False)
    both = np.concatenate([kv, -kv])
    assert len(ks) == 3
    assert np.all(np.linalg.norm(ks[None] - both[:, None], axis=-1).min(axis=0) < 1.5 / size)
    GPA.extract_primary_ks(frames[0], DoG=False)                  # the unhomogenised image only has to run
