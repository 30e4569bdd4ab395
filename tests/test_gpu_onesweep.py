"""The one-sweep form of the fused driver (gpa_extract_displacement_field_grad*): u AND, per peak, lock-in, winner, phase
gradient and |lock-in| from a single sweep -- against the reference's own numbers (tests/golden), against today's separate calls
(gpa_extract_displacement_field_dev + gpa_sweep_grad_dev per peak), against the oracle at the headline's size, and through the
mirror's `wfr_func` plug-ins.  Run with `-m gpu` on an MI355X.

Bounds are the ones the existing tests hold the separate calls to: TOL of tests/test_gpu_parity.py (lock-ins, PCG outputs,
amplitude ties), test_a4_grad's 1e-9 / 2e-3 rad modulo pi on pixels with the same winner and an amplitude above 1e-3 of the
maximum, tests/tolerances.py for u in pixels."""
import ctypes as C
import os

import numpy as np
import pytest

import tolerances
from oracle import gpa_oracle as orc
from pygpa_amd import _lib
from pygpa_amd.synthetic import hex_kvecs, gaussian_bump_displacement, hex_moire, explicit_klists
from test_gpu_parity import TOL, DeviceArray, check_kidx, rel, _pdiff

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
GRAD_TOL = {np.float64: 1e-9, np.float32: 2e-3}          # rad, test_a4_grad (tests/test_gpu_parity.py:224-229)


def _grad_err(grad, ref, ok):
    """largest difference modulo the pi-periodic wrap of wrapToPi(2 g) / 2 on the pixels `ok`"""
    d = orc.wrap_to_pi(2 * (np.asarray(grad, dtype=np.float64) - ref)) / 2
    return float(np.abs(d[ok]).max())


def _one_sweep(plan, image, kvecs, klists, sigma, grad_mode=0):
    return plan.extract_displacement_field(image, kvecs, klists, sigma, 2 * sigma, kmax=10, want_lockins=True, want_kidx=True,
                                           want_grads=True, want_weights=True, grad_mode=grad_mode)


def _demean(u):
    return u - u.mean(axis=(1, 2), keepdims=True)


# ---- 1. the reference's own numbers ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
def test_golden_all_peaks(golden, dtype):
    """hex_64: u, winners, lock-ins of the three peaks (a3), their phase gradients and weights (props_64: the same image and
    lists, oracle/make_golden.py:344-368) from ONE driver call.  64-point rows: the per-candidate pass B in its phases mode."""
    g, pr = golden('hex_64'), golden('props_64')
    sigma = int(g['sigma'])
    K = g['a3_klists'].shape[1]
    plan = _lib.Plan(g['image'].shape, 3 * K, dtype)
    u, lock, kidx, iters, grads, absw = _one_sweep(plan, g['image'], g['kvecs'], g['a3_klists'], sigma)
    plan.close()
    assert grads.shape == pr['grads'].shape and absw.shape == pr['weights'].shape
    assert grads.dtype == dtype and absw.dtype == dtype
    print('u rel', rel(u, g['u']), 'absw rel', rel(absw, pr['weights']))
    assert rel(u, g['u']) < TOL[dtype]['pcg']
    img0 = g['image'] - g['image'].mean()
    for p in range(3):
        check_kidx(kidx[p], g['a3_kidx'][p], img0, g['a3_klists'][p], sigma, TOL[dtype]['tie'])
        same = kidx[p] == g['a3_kidx'][p]
        amp = np.abs(g['a3_lockin'][p])
        ok = same & (amp > 1e-3 * amp.max())
        print('peak', p, 'lock rel', rel(lock[p][same], g['a3_lockin'][p][same]), 'grad', _grad_err(grads[p], pr['grads'][p], ok))
        assert rel(lock[p][same], g['a3_lockin'][p][same]) < TOL[dtype]['lock']
        assert _grad_err(grads[p], pr['grads'][p], ok) < GRAD_TOL[dtype]
    assert rel(absw, pr['weights']) < TOL[dtype]['lock']
    if dtype is np.float64:
        assert np.array_equal(kidx, g['a3_kidx']) and iters == (10, 10)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name', ['hex_48x80', 'hex_63x65'])
def test_golden_non_square_odd(golden, name, dtype):
    """non-square and odd sizes (zero-padded rows): peak 0 against a4_grad0, u and the winners of all peaks"""
    g = golden(name)
    sigma = int(g['sigma'])
    K = g['a3_klists'].shape[1]
    plan = _lib.Plan(g['image'].shape, 3 * K, dtype)
    u, lock, kidx, iters, grads, absw = _one_sweep(plan, g['image'], g['kvecs'], g['a3_klists'], sigma)
    plan.close()
    assert rel(u, g['u']) < TOL[dtype]['pcg']
    img0 = g['image'] - g['image'].mean()
    for p in range(3):
        check_kidx(kidx[p], g['a3_kidx'][p], img0, g['a3_klists'][p], sigma, TOL[dtype]['tie'])
        same = kidx[p] == g['a3_kidx'][p]
        assert rel(lock[p][same], g['a3_lockin'][p][same]) < TOL[dtype]['lock']
    assert rel(absw, np.abs(g['a3_lockin'])) < TOL[dtype]['lock']
    same = kidx[0] == g['a3_kidx'][0]
    amp = np.abs(g['a3_lockin'][0])
    err = _grad_err(grads[0], g['a4_grad0'], same & (amp > 1e-3 * amp.max()))
    print(name, 'grad0', err)
    assert err < GRAD_TOL[dtype]


# ---- 2. the shared-forward pass B: one sweep, against today's separate calls -----------------------------------------------
def _dev_one_sweep(plan, d_img, kvecs, klists, sigma, kmax, P, shape, dtype, grad_mode=0):
    cdt = np.complex64 if dtype is np.float32 else np.complex128
    d_u = DeviceArray(np.zeros((2,) + shape, dtype=dtype))
    d_lock = DeviceArray(np.zeros((P,) + shape, dtype=cdt))
    d_kidx = DeviceArray(np.zeros((P,) + shape, dtype=np.int32))
    d_grad = DeviceArray(np.zeros((P,) + shape + (2,), dtype=dtype))
    d_w = DeviceArray(np.zeros((P,) + shape, dtype=dtype))
    iters = plan.extract_displacement_field_dev(d_img.ptr, kvecs, klists, sigma, 2 * sigma, kmax, d_u.ptr, d_lock.ptr, d_kidx.ptr,
                                                grads_ptr=d_grad.ptr, weights_ptr=d_w.ptr, grad_mode=grad_mode)
    return d_u.get(), d_lock.get(), d_kidx.get(), d_grad.get(), d_w.get(), iters


@pytest.mark.parametrize('dtype', DTYPES)
def test_shared_route_2048_vs_separate_calls(dtype):
    """configs[1]'s image, 2048^2, 3 x 8: the new form against extract_displacement_field_dev (u) and sweep_grad_dev per peak on
    the image minus its mean, all on the same plan; and the profile of the call: ONE pass A, ONE shared pass B with phases"""
    n, P = 2048, 3
    shape = (n, n)
    kvecs = hex_kvecs(0.1, 7.0)
    img = hex_moire(shape, kvecs, gaussian_bump_displacement(shape), noise=0.1, seed=5).astype(dtype)
    kw, sigma, _ = orc.derive_params(kvecs)
    klists = np.stack(explicit_klists(kvecs, kw, 4, 2))
    cdt = np.complex64 if dtype is np.float32 else np.complex128
    plan = _lib.Plan(shape, 24, dtype)
    d_img = DeviceArray(img)
    u, lock, kidx, grads, absw, iters = _dev_one_sweep(plan, d_img, kvecs, klists, sigma, 10, P, shape, dtype)
    # today's calls
    d_u = DeviceArray(np.zeros((2,) + shape, dtype=dtype))
    iters0 = plan.extract_displacement_field_dev(d_img.ptr, kvecs, klists, sigma, 2 * sigma, 10, d_u.ptr)
    u0 = d_u.get()
    img0 = (img.astype(np.float64) - img.astype(np.float64).mean())
    d_img0 = DeviceArray(img0.astype(dtype))
    d_l1, d_k1 = DeviceArray(np.zeros(shape, dtype=cdt)), DeviceArray(np.zeros(shape, dtype=np.int32))
    d_g1 = DeviceArray(np.zeros(shape + (2,), dtype=dtype))
    f32 = dtype is np.float32
    d = _demean(u.astype(np.float64)) - _demean(u0.astype(np.float64))
    print('u max_px', np.abs(d).max(), 'rms_px', np.sqrt((d ** 2).mean()), iters, iters0)
    if f32:
        assert np.abs(d).max() < tolerances.F32['max_px'] and np.sqrt((d ** 2).mean()) < tolerances.F32['rms_px']
    else:
        assert np.abs(d).max() < tolerances.F64['max_px']
    for p in range(P):
        plan.sweep_grad_dev(d_img0.ptr, kvecs[p], klists[p], sigma, d_l1.ptr, d_g1.ptr, kidx_ptr=d_k1.ptr)
        plan.sync()
        l1, k1, g1 = d_l1.get(), d_k1.get(), d_g1.get()
        check_kidx(kidx[p], k1, img0, klists[p], sigma, TOL[dtype]['tie'])
        same = kidx[p] == k1
        amp = np.abs(l1)
        ok = same & (amp > 1e-3 * amp.max())
        print('peak', p, 'mismatch', int((~same).sum()), 'lock', rel(lock[p][same], l1[same]), 'grad', _grad_err(grads[p], g1, ok))
        assert rel(lock[p][same], l1[same]) < TOL[dtype]['lock']
        assert _grad_err(grads[p], g1.astype(np.float64), ok) < GRAD_TOL[dtype]
        assert rel(absw[p][same], amp[same]) < TOL[dtype]['lock']
    # which kernels the one-sweep call runs
    plan.set_profiling(True)
    _dev_one_sweep(plan, d_img, kvecs, klists, sigma, 10, P, shape, dtype)
    prof = plan.last_kernel_profile()
    plan.set_profiling(False)
    plan.close()
    assert prof['passA_kernel'][0] == 1, prof
    assert prof['passB_shared_phases_kernel'][0] == 1, prof
    assert prof['phasegrad_kernel'][0] == 1 and prof['lockin_abs_kernel'][0] == 1, prof
    assert 'passB_kernel' not in prof and 'passB_shared_kernel' not in prof, prof


@pytest.fixture(scope='module')
def oracle_4096():
    """configs[2]'s image and lists; the oracle's u and its wfr2_grad_opt of peak 0 (one run for the module)"""
    n = 4096
    kvecs = hex_kvecs(0.1, 7.0)
    img = hex_moire((n, n), kvecs, gaussian_bump_displacement((n, n)), noise=0.1, seed=100)
    kw, sigma, _ = orc.derive_params(kvecs)
    klists = np.stack(explicit_klists(kvecs, kw, 4, 4))
    cores = min(os.cpu_count() or 1, 16)
    u_ref, parts = orc.extract_displacement_field(img, kvecs, sigma=sigma, klists=klists, return_parts=True, workers=cores, pool=cores)
    g0 = orc.sweep(img - img.mean(), sigma, klists[0], kvecs[0], want_grad=True, workers=cores, pool=cores)
    ref_kidx = np.stack([g['kidx'] for g in parts['gs']])
    return img, kvecs, klists, sigma, u_ref, ref_kidx, g0


def test_headline_size_4096_f32_vs_oracle(oracle_4096):
    """4096^2 f32 3 x 16 (4096-point rows of the shared kernel): u within the stated f32 tolerances against the oracle
    (tests/tolerances.F32), winners up to ties, lock-in, gradient and weight of peak 0 against the oracle's wfr2_grad_opt"""
    img, kvecs, klists, sigma, u_ref, ref_kidx, g0 = oracle_4096
    shape, dtype = img.shape, np.float32
    plan = _lib.Plan(shape, 48, dtype)
    d_img = DeviceArray(img.astype(dtype))
    u, lock, kidx, grads, absw, iters = _dev_one_sweep(plan, d_img, kvecs, klists, sigma, 10, 3, shape, dtype)
    plan.close()
    d = _demean(u.astype(np.float64)) - _demean(u_ref)
    print('u max_px', np.abs(d).max(), 'rms_px', np.sqrt((d ** 2).mean()), iters)
    assert np.abs(d).max() < tolerances.F32['max_px'] and np.sqrt((d ** 2).mean()) < tolerances.F32['rms_px']
    img0 = img - img.mean()
    for p in range(3):
        assert (kidx[p] != ref_kidx[p]).mean() <= tolerances.F32['kidx_frac']
        check_kidx(kidx[p], ref_kidx[p], img0, klists[p], sigma, tolerances.F32['tie_rel'])
    same = kidx[0] == g0['kidx']
    amp = np.abs(g0['lockin'])
    ok = same & (amp > 1e-3 * amp.max())
    print('lock', rel(lock[0][same], g0['lockin'][same]), 'grad', _grad_err(grads[0], g0['grad'], ok))
    assert rel(lock[0][same], g0['lockin'][same]) < TOL[dtype]['lock']
    assert _grad_err(grads[0], g0['grad'], ok) < GRAD_TOL[dtype]
    assert rel(absw[0][same], amp[same]) < TOL[dtype]['lock']


# ---- 3. the other stencils ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('mode', [1, 2])
def test_grad_modes_vs_sweep_grad(dtype, mode):
    """forward differences (NaN at the last index of each axis) in both component orders, against gpa_sweep_grad per peak"""
    shape = (256, 256)
    kvecs = hex_kvecs(0.1, 7.0)
    img = hex_moire(shape, kvecs, gaussian_bump_displacement(shape), noise=0.1, seed=8)
    kw, sigma, _ = orc.derive_params(kvecs)
    klists = np.stack(explicit_klists(kvecs, kw, 3, 3))
    plan = _lib.Plan(shape, 27, dtype)
    u, lock, kidx, iters, grads, absw = _one_sweep(plan, img, kvecs, klists, sigma, grad_mode=mode)
    img0 = img - img.mean()
    for p in range(3):
        l1, k1, g1 = plan.sweep(img0, kvecs[p], klists[p], sigma, want_grad=True, grad_mode=mode)
        check_kidx(kidx[p], k1, img0, klists[p], sigma, TOL[dtype]['tie'])
        same = kidx[p] == k1
        assert np.array_equal(np.isnan(grads[p]), np.isnan(g1))
        nan = np.isnan(g1)
        # the NaNs sit at the last index of the differenced axis, wherever a candidate won
        along0, along1 = (0, 1) if mode == 1 else (1, 0)
        assert nan[..., along0][-1][k1[-1] >= 0].all() and nan[..., along1][:, -1][k1[:, -1] >= 0].all()
        amp = np.abs(l1)
        ok = (same & (amp > 1e-3 * amp.max()))[..., None] & ~nan
        d = orc.wrap_to_pi(2 * (np.where(nan, 0, grads[p]).astype(np.float64) - np.where(nan, 0, g1))) / 2
        print('mode', mode, 'peak', p, np.abs(d[ok]).max())
        assert np.abs(d[ok]).max() < GRAD_TOL[dtype]
        assert rel(lock[p][same], l1[same]) < TOL[dtype]['lock']
    plan.close()


# ---- 4. without gradients: the very launches of the plain driver; plan reuse ------------------------------------------------
def _grad_dev_raw(plan, d_img, kvecs, klists, sigma, kmax, d_u, grads=None, absw=None):
    """the new C entry point itself (the Python method calls the old one when no gradient pointer is given)"""
    kv = np.ascontiguousarray(kvecs, dtype=np.float64)
    kl = np.ascontiguousarray(klists, dtype=np.float64)
    iters = (C.c_int * 2)()
    vp = lambda a: None if a is None else C.c_void_p(a)   # noqa: E731
    rc = plan.lib.gpa_extract_displacement_field_grad_dev(plan.handle, vp(d_img.ptr), kv.ctypes.data_as(C.c_void_p), len(kv),
                                                          kl.ctypes.data_as(C.c_void_p), kl.shape[1], float(sigma), int(2 * sigma),
                                                          int(kmax), 0, vp(d_u.ptr), None, None, vp(grads), vp(absw), iters)
    _lib.check(rc, 'gpa_extract_displacement_field_grad_dev')
    return iters[0], iters[1]


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('n', [512, 2048])
def test_null_grads_are_the_old_bits_and_plans_are_reusable(n, dtype):
    shape = (n, n)
    kvecs = hex_kvecs(0.1, 7.0)
    img = hex_moire(shape, kvecs, gaussian_bump_displacement(shape), noise=0.1, seed=12).astype(dtype)
    kw, sigma, _ = orc.derive_params(kvecs)
    klists = np.stack(explicit_klists(kvecs, kw, 4, 2))
    d_img = DeviceArray(img)

    def plain(plan):
        d_u = DeviceArray(np.zeros((2,) + shape, dtype=dtype))
        it = plan.extract_displacement_field_dev(d_img.ptr, kvecs, klists, sigma, 2 * sigma, 10, d_u.ptr)
        return d_u.get(), it

    def new_null(plan):
        d_u = DeviceArray(np.zeros((2,) + shape, dtype=dtype))
        it = _grad_dev_raw(plan, d_img, kvecs, klists, sigma, 10, d_u)
        return d_u.get(), it

    def with_grads(plan):
        return _dev_one_sweep(plan, d_img, kvecs, klists, sigma, 10, 3, shape, dtype)

    # order 1: plain, new entry point without gradients, one sweep, plain again -- on one plan
    plan = _lib.Plan(shape, 24, dtype)
    ws0 = plan.workspace_bytes
    u_a, it_a = plain(plan)
    ws1 = plan.workspace_bytes
    u_b, it_b = new_null(plan)
    assert plan.workspace_bytes == ws1           # no phase scratch without gradients
    assert np.array_equal(u_a, u_b) and it_a == it_b
    g1 = with_grads(plan)
    item = np.dtype(dtype).itemsize
    assert plan.workspace_bytes >= ws0 + 24 * n * n * item      # the phase scratch is counted
    u_c, it_c = plain(plan)
    u_d, it_d = new_null(plan)
    assert np.array_equal(u_a, u_c) and np.array_equal(u_a, u_d) and it_a == it_c == it_d
    g2 = with_grads(plan)
    for a, b in zip(g1[:5], g2[:5]):
        assert np.array_equal(a, b, equal_nan=True)
    plan.close()
    # order 2: a fresh plan whose FIRST call asks for gradients, then plain
    plan = _lib.Plan(shape, 24, dtype)
    g3 = with_grads(plan)
    u_e, it_e = plain(plan)
    plan.close()
    assert np.array_equal(u_a, u_e) and it_a == it_e
    for a, b in zip(g1[:5], g3[:5]):
        assert np.array_equal(a, b, equal_nan=True)


# ---- 5. the mirror ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def mirror_case():
    shape = (512, 512)
    kvecs = hex_kvecs(0.1, 7.0)
    img = hex_moire(shape, kvecs, gaussian_bump_displacement(shape), noise=0.1, seed=3)
    kw, sigma, kstep = orc.derive_params(kvecs)
    return img, kvecs, kw, sigma, kstep


@pytest.mark.parametrize('which', ['cuGPA.wfr2_grad_opt', 'GPA.wfr2_grad_opt', 'cuGPA.wfr2_grad_single'])
def test_mirror_plugins_one_call(mirror_case, which):
    import pygpa_amd.geometric_phase_analysis as GPA
    from pygpa_amd import cuGPA, property_extract as pe
    func = {'cuGPA.wfr2_grad_opt': cuGPA.wfr2_grad_opt, 'GPA.wfr2_grad_opt': GPA.wfr2_grad_opt,
            'cuGPA.wfr2_grad_single': cuGPA.wfr2_grad_single}[which]
    f32 = func is cuGPA.wfr2_grad_single
    dtype = np.float32 if f32 else np.float64
    img, kvecs, kw, sigma, kstep = mirror_case
    u, gs = GPA.extract_displacement_field(img, kvecs, wfr_func=func, return_gs=True)
    img0 = img - img.mean()
    ref = [func(img0, sigma, pk[0], pk[1], kw=kw, kstep=kstep) for pk in kvecs]
    # winners of both routes (the plug-ins of cuGPA do not return kidx: the same sweeps through GPA.wfr2_grad_opt, which
    # are the same device calls in the same precision, do)
    _, gk = GPA.extract_displacement_field(img, kvecs, wfr_func=GPA.wfr2_grad_opt, return_gs=True, dtype=dtype)
    rk = [GPA.wfr2_grad_opt(img0, sigma, pk[0], pk[1], kw, kstep, dtype=dtype) for pk in kvecs]
    assert u.dtype == np.float64
    u_def = GPA.extract_displacement_field(img, kvecs)
    if f32:
        d = _demean(u) - _demean(u_def)
        print('u max_px', np.abs(d).max(), 'rms', np.sqrt((d ** 2).mean()))
        assert np.abs(d).max() < tolerances.F32['max_px'] and np.sqrt((d ** 2).mean()) < tolerances.F32['rms_px']
    else:
        assert rel(u, u_def) < 1e-9
    for p in range(3):
        assert set(gs[p]) == set(ref[p])
        assert np.array_equal(gs[p]['lockin'], gk[p]['lockin']) and np.array_equal(ref[p]['lockin'], rk[p]['lockin'])
        klist = GPA._sweep_list(kvecs[p][0], kvecs[p][1], kw, kstep)
        check_kidx(gk[p]['kidx'], rk[p]['kidx'], img0, klist, sigma, TOL[dtype]['tie'])
        same = gk[p]['kidx'] == rk[p]['kidx']
        amp = np.abs(ref[p]['lockin'])
        ok = same & (amp > 1e-3 * amp.max())
        assert gs[p]['lockin'].dtype == ref[p]['lockin'].dtype and gs[p]['grad'].dtype == ref[p]['grad'].dtype
        print(which, p, rel(gs[p]['lockin'][same], ref[p]['lockin'][same]), _grad_err(gs[p]['grad'], ref[p]['grad'].astype(np.float64), ok))
        assert rel(gs[p]['lockin'][same], ref[p]['lockin'][same]) < TOL[dtype]['lock']
        assert _grad_err(gs[p]['grad'], ref[p]['grad'].astype(np.float64), ok) < GRAD_TOL[dtype]
        if 'w' in ref[p]:
            assert np.array_equal(gs[p]['w'][:, same], ref[p]['w'][:, same])
    if f32:
        return
    # the lattice properties from this call's gradients and weights against the two-sweep route
    # (bounds: test_f2_fused_from_sweep_vs_oracle, tests/test_gpu_parity.py:589-592)
    props = pe.calc_props_from_phasegradient(kvecs, np.stack([g['grad'] for g in gs]), np.stack([np.abs(g['lockin']) for g in gs]), 1.0)
    two = pe.calc_props_from_phasegradient(kvecs, np.stack([g['grad'] for g in ref]), np.stack([np.abs(g['lockin']) for g in ref]), 1.0)
    print('props', np.abs(_pdiff(props[0], two[0], 360)).max(), np.abs(props[2] / two[2] - 1).max(), np.abs(props[3] / two[3] - 1).max())
    assert np.abs(_pdiff(props[0], two[0], 360)).max() < 1e-9
    assert np.allclose(props[2], two[2], rtol=1e-11) and np.allclose(props[3], two[3], rtol=1e-10)
    well = two[3] > 1.001
    assert np.abs(_pdiff(props[1], two[1], 180))[well].max() < 1e-6
