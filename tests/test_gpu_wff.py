"""Windowed Fourier filtering on the device (gpa_wff / gpa_wff_dev) against the fixtures the reference's own
`wff` wrote (tests/golden/wff_*.npz, tools/make_wff_golden.py) and the NumPy / SciPy restatement of tests/wff_cases.py.
Run with `-m gpu` on an MI355X.

f64: within 1e-12 of the output's largest magnitude (the two formulations differ by 1e-15 on the CPU; the margin covers the
summation order and fused multiply-adds).  f32: within wff_cases.f32_bound -- 8 x the deviation of the restatement run in
complex64 -- of the fixture and of the f64 build.  Thresholds sit in gaps of |sf| at least 32 x the complex64 error wide, so
no keep / drop decision may flip."""
import numpy as np
import pytest

from pygpa_amd import _lib
import pygpa_amd.geometric_phase_analysis as GPA
from pygpa_amd.synthetic import hex_kvecs, explicit_klists, gaussian_bump_displacement, hex_moire

import wff_cases as wc
from test_gpu_plan_state import same

pytestmark = pytest.mark.gpu

F64_TOL = 1e-12


@pytest.fixture(scope='module')
def results():
    """every fixture through the mirror in both precisions, once: name -> (fixture, f64 result, f32 result)"""
    out = {}
    for name in wc.CASES:
        z = wc.load(name)
        args = (z['image'], float(z['sigma']), z['thresholds'], float(z['wl']), float(z['wu']))
        out[name] = (z, GPA.wff(*args), GPA.wff(*args, dtype=np.float32))
    return out


def _rel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


@pytest.mark.parametrize('name', list(wc.CASES))
def test_f64_matches_reference(results, name):
    z, g64, _ = results[name]
    assert g64.dtype == np.complex128 and g64.shape == z['out'].shape
    err = _rel(g64, z['out'])
    print('%s f64: %.3e of the largest magnitude' % (name, err))
    assert err <= F64_TOL


@pytest.mark.parametrize('name', list(wc.CASES))
def test_f32_matches_reference_and_f64(results, name):
    z, g64, g32 = results[name]
    assert g32.dtype == np.complex64 and g32.shape == z['out'].shape
    e_ref, e_64 = _rel(g32, z['out']), _rel(g32, g64)
    print('%s f32: %.3e of the fixture, %.3e of the f64 build (bound %.3e)' % (name, e_ref, e_64, wc.f32_bound(name)))
    assert e_ref <= wc.f32_bound(name)
    assert e_64 <= wc.f32_bound(name)


@pytest.fixture(scope='module')
def case():
    z = wc.load('wff_40x56')
    sigma = float(z['sigma'])
    return dict(z=z, image=z['image'], sigma=sigma, ws=wc.freq_list(sigma, float(z['wl']), float(z['wu'])),
                scale=wc.scale_of(sigma), thr=z['thresholds'])


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_equivalences(case, dtype):
    c = case
    shape = c['image'].shape
    plan = _lib.Plan(shape, 1, dtype)
    try:
        cd = plan.cdtype
        both = plan.wff(c['image'], c['sigma'], c['ws'], c['ws'], c['thr'], c['scale'])
        # two runs
        assert np.array_equal(both, plan.wff(c['image'], c['sigma'], c['ws'], c['ws'], c['thr'], c['scale']))
        # T = 2 == two calls with T = 1
        for t in range(2):
            one = plan.wff(c['image'], c['sigma'], c['ws'], c['ws'], c['thr'][t:t + 1], c['scale'])
            assert np.array_equal(one[0], both[t])
        # device pointers == host arrays
        img = np.ascontiguousarray(c['image'], dtype=cd)
        d_img, d_out = _lib.DeviceBuffer(img.nbytes), _lib.DeviceBuffer(2 * img.nbytes)
        try:
            d_img.upload(img)
            plan.wff_dev(d_img.ptr, d_out.ptr, c['sigma'], c['ws'], c['ws'], c['thr'], c['scale'])
            plan.sync()
            assert np.array_equal(d_out.download((2,) + shape, cd), both)
            assert np.array_equal(d_img.download(shape, cd), img)
            # ... and the mirror's device form
            assert GPA.wff_dev(plan, d_img.ptr, d_out.ptr, c['sigma'], c['thr'], float(c['z']['wl']), float(c['z']['wu'])) == 2
            plan.sync()
            assert np.array_equal(d_out.download((2,) + shape, cd), both)
        finally:
            d_img.free()
            d_out.free()
        # a threshold above every |sf|: exact zeros
        zero = plan.wff(c['image'], c['sigma'], c['ws'], c['ws'], [2.0 * float(c['z']['sf_max'])], c['scale'])
        assert np.all(zero == 0)
    finally:
        plan.close()


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_more_thresholds_than_one_call_takes(case, dtype):
    """T above the per-call limit, through the mirror's chunks, gives the planes of single-threshold calls"""
    c = case
    lo, hi = c['thr']
    thr = np.concatenate([np.linspace(lo, hi, _lib.WFF_MAX_T + 2), [-1.0]])
    assert len(thr) > _lib.WFF_MAX_T
    many = GPA.wff(c['image'], c['sigma'], thr, float(c['z']['wl']), float(c['z']['wu']), dtype=dtype)
    assert many.shape == (len(thr),) + c['image'].shape
    for t in (0, 3, _lib.WFF_MAX_T - 1, _lib.WFF_MAX_T, len(thr) - 1):
        one = GPA.wff(c['image'], c['sigma'], thr[t:t + 1], float(c['z']['wl']), float(c['z']['wu']), dtype=dtype)
        assert np.array_equal(one[0], many[t]), t


def test_negative_threshold_is_the_plain_double_convolution(case):
    c = case
    got = GPA.wff(c['image'], c['sigma'], [-1.0], float(c['z']['wl']), float(c['z']['wu']))
    want = wc.restate(c['image'], c['sigma'], [-1.0], c['ws'], c['ws'], c['scale'])
    assert _rel(got, want) <= F64_TOL
    # thr = 0 keeps everything as well
    assert np.array_equal(GPA.wff(c['image'], c['sigma'], [0.0], float(c['z']['wl']), float(c['z']['wu'])), got)


@pytest.mark.parametrize('sigma', [3.0, 2.5])
def test_tile_seams(tmp_path_factory, sigma):
    """wider and taller than one workgroup tile in both directions, ragged last tiles: tile width + 3 columns, 2 R + 1 rows,
    3 x 3 frequencies, f64 against the restatement.  The tile comes from gpa_wff.h (tests/host/wff_geom_check.cpp prints it)."""
    cols, R = wc.tile_geometry(tmp_path_factory.mktemp('wffgeom'))[('f64', wc.half_window(sigma))]
    shape = (2 * R + 1, cols + 3)
    image = wc.noisy_phasor(shape, 7)
    ws = np.array([-0.4, 0.0, 0.4])
    thr = [0.8, 3.0]
    want = wc.restate(image, sigma, thr, ws, ws, 1.0)
    # the thresholds must sit in gaps of |sf| (a flipped sample is not a rounding error)
    mags = np.stack([np.abs(sf) for _, _, sf in wc.spectra(image, sigma, ws, ws)])
    gap = min(np.abs(mags - t).min() for t in thr)
    assert gap > 1e-9 * mags.max()
    plan = _lib.Plan(shape, 1, np.float64)
    try:
        got = plan.wff(image, sigma, ws, ws, thr, 1.0)
    finally:
        plan.close()
    err = _rel(got, want)
    print('seams %s sigma %g: %.3e' % (shape, sigma, err))
    assert err <= F64_TOL
    # the f32 tile is twice as wide: its seam falls inside this image only when cols_f32 + 3 <= shape[1]; checked on its own
    cols32, R32 = wc.tile_geometry(None)[('f32', wc.half_window(sigma))]
    shape32 = (2 * R32 + 1, cols32 + 3)
    image32 = wc.noisy_phasor(shape32, 8)
    want32 = wc.restate(image32, sigma, [-1.0], ws, ws, 1.0)
    plan = _lib.Plan(shape32, 1, np.float32)
    try:
        got32 = plan.wff(image32, sigma, ws, ws, [-1.0], 1.0)
    finally:
        plan.close()
    # no threshold in play: the f32 rounding of four 2 s-tap passes and 9 sums, 64 eps of the largest magnitude
    err32 = _rel(got32, want32)
    print('seams f32 %s sigma %g: %.3e' % (shape32, sigma, err32))
    assert err32 <= 64 * np.finfo(np.float32).eps


def test_plan_state_and_accounting():
    shape = (64, 48)
    kv = hex_kvecs(0.12, 11.0)
    kw = np.linalg.norm(kv, axis=1).mean() / 2.5
    klists = np.stack(explicit_klists(kv, kw, 2, 2))
    img = hex_moire(shape, kv, gaussian_bump_displacement(shape), noise=0.1, seed=1)
    img = img - img.mean()
    field = wc.noisy_phasor(shape, 3)
    ws = wc.freq_list(3.0, -1.0, 1.0)
    plan = _lib.Plan(shape, 12, np.float64)
    try:
        before = plan.extract_displacement_field(img, kv, klists, 6.0, 3, kmax=5)
        b0 = plan.workspace_bytes
        plan.wff(field, 3.0, ws, ws, [1.0, 2.0, 3.0], wc.scale_of(3.0))
        b1 = plan.workspace_bytes
        npx = shape[0] * shape[1] * 16
        # the A plane and 3 B planes, the staged image and 3 output planes, the tables
        assert b1 - b0 >= (1 + 3) * npx + (1 + 3) * npx + 2 * len(ws) * 12 * 16
        plan.wff(field, 3.0, ws, ws, [1.0, 2.0, 3.0], wc.scale_of(3.0))
        assert plan.workspace_bytes == b1
        after = plan.extract_displacement_field(img, kv, klists, 6.0, 3, kmax=5)
        assert same(before, after)
    finally:
        plan.close()


def test_argument_errors_name_the_argument():
    shape = (16, 16)
    plan = _lib.Plan(shape, 1, np.float64)
    img = np.ones(shape, dtype=np.complex128)
    out = np.empty((1,) + shape, dtype=np.complex128)
    one = np.array([0.5])
    P = _lib._ptr
    ARG = -1

    def call(image=img, sigma=3.0, wxs=one, Kx=1, wys=one, Ky=1, thr=one, T=1, scale=1.0, o=out, fn='gpa_wff'):
        return getattr(plan.lib, fn)(plan.handle, P(image), sigma, P(wxs), Kx, P(wys), Ky, P(thr), T, scale, P(o))
    try:
        assert call() == 0
        nan, inf = np.array([np.nan]), np.array([np.inf])
        many = np.zeros(_lib.WFF_MAX_T + 1)
        for kw, word in ((dict(image=None), 'image'), (dict(o=None), 'out'), (dict(wxs=None), 'wxs'), (dict(wys=None), 'wys'),
                         (dict(thr=None), 'thresholds'), (dict(Kx=0), 'Kx'), (dict(Ky=0), 'Ky'), (dict(T=0), 'T'),
                         (dict(sigma=0.0), 'sigma'), (dict(sigma=-1.0), 'sigma'), (dict(sigma=float('nan')), 'sigma'),
                         (dict(wxs=nan), 'wxs'), (dict(wys=inf), 'wys'), (dict(thr=nan), 'thresholds'),
                         (dict(scale=float('inf')), 'scale'), (dict(sigma=0.1), 'sigma'),
                         (dict(sigma=(_lib.WFF_MAX_S + 1) / 2.0), 'GPA_WFF_MAX_S'), (dict(thr=many, T=len(many)), 'GPA_WFF_MAX_T')):
            for fn in ('gpa_wff', 'gpa_wff_dev'):
                code = call(fn=fn, **kw)
                assert code == ARG, (fn, kw, code)
                msg = _lib.last_error()
                assert fn in msg and word in msg, (fn, kw, msg)
        # the largest window and the largest T run
        assert call(sigma=_lib.WFF_MAX_S / 2.0) == 0
        with pytest.raises(_lib.GPAError, match='GPA_WFF_MAX_T'):
            plan.wff(img, 3.0, one, one, many, 1.0)
    finally:
        plan.close()
