"""iterate_GPA as one device-resident call (gpa_iterate_gpa) and the entry points it is made of -- gpa_lockin_polar_crop_dev,
gpa_unwrap_dev, gpa_fit_planes_dev.  Run with `-m gpu` on an MI355X.

Every bound is one the suite already applies to this route: test_gpu_parity.py::test_a8_iterate_gpa (64^2, the reference's
outputs) and tolerances.C1_F64 / C1_F32 (512^2).  Where the fused call is held against the host loop (fused=False) the bounds
are doubled, since each side is held to the reference at once each."""
import ctypes as C

import numpy as np
import pytest

import tolerances as TOL
from oracle import gpa_oracle as orc
from pygpa_amd import _lib
from pygpa_amd.synthetic import hex_moire

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
C1_SL = (Ellipsis, slice(3, None, 7), slice(3, None, 7))      # oracle/make_golden.py: C1_STRIDE
TWO_PI = 2 * np.pi


def _GPA():
    import pygpa_amd.geometric_phase_analysis as GPA
    return GPA


def check_item1(prs, w, corr, prs_ref, w_ref, corr_ref, dtype, factor=1):
    """the bounds of test_a8_iterate_gpa (factor 2: two results that are each held to the reference)"""
    f = factor
    if dtype is np.float64:
        assert np.allclose(corr, corr_ref, rtol=f * 1e-5, atol=f * 1e-8), np.abs(corr - corr_ref).max()
        assert np.allclose(w, w_ref, rtol=f * 1e-8, atol=f * 1e-10), np.abs(w - w_ref).max()
        assert np.allclose(prs, prs_ref, rtol=f * 1e-5, atol=f * 1e-6), np.abs(prs - prs_ref).max()
    else:
        assert np.allclose(corr, corr_ref, rtol=0, atol=f * 2e-6), np.abs(corr - corr_ref).max()
        assert np.allclose(w, w_ref, rtol=f * 2e-5, atol=f * 1e-5), np.abs(w - w_ref).max()
        assert np.abs(prs - prs_ref).max() < f * 2e-3 * np.abs(prs_ref).max(), np.abs(prs - prs_ref).max()


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize('dtype', DTYPES)
def test_reference_vectors_64(golden, dtype):
    g = golden('iterate_64')
    prs, w, corr = _GPA().iterate_GPA(g['image'] - g['image'].mean(), g['start_ks'], int(g['sigma']), dtype=dtype, fused=True)
    assert prs.shape == g['prs'].shape and prs.dtype == dtype and w.dtype == dtype and corr.dtype == np.float64
    check_item1(prs, w, corr, g['prs'], g['w'], g['corr'], dtype)
    assert np.abs(g['start_ks'] + corr - g['true_ks']).max() < 5e-4


@pytest.mark.parametrize('dtype', DTYPES)
def test_reference_vectors_config1_512(golden, dtype):
    """512^2 against the fixture's subsample of the reference's outputs"""
    g = golden('config1_512')
    image = hex_moire((512, 512), g['it_true_ks'], None, noise=0.05, seed=21)
    start, sigma = g['it_start_ks'], int(g['it_sigma'])
    prs, w, corr = _GPA().iterate_GPA(image - image.mean(), start, sigma, dtype=dtype, fused=True)
    assert prs.shape == (3, 502, 502)
    k_err = np.abs(start + corr - g['it_true_ks']).max()
    corr_err = np.abs(corr - g['it_corr']).max()
    prs_err = np.abs(prs[C1_SL] - g['it_prs']).max()
    scale = np.abs(g['it_prs']).max()
    print('config1_512 fused %s: k_err %.3g corr_err %.3g prs_err %.3g (max|prs| %.3g)' % (np.dtype(dtype).name, k_err, corr_err,
                                                                                           prs_err, scale))
    assert k_err < 1e-6
    if dtype is np.float64:
        T = TOL.C1_F64
        assert corr_err < T['corr'] and prs_err < T['prs']
        assert np.allclose(w[C1_SL], g['it_w'], rtol=1e-9, atol=1e-12)
    else:
        T = TOL.C1_F32
        assert corr_err < T['corr'] and prs_err < T['prs_rel'] * scale
        assert np.allclose(w[C1_SL], g['it_w'], rtol=2e-5, atol=1e-5)


# ---------------------------------------------------------------------------------------------------------------- 2
_FRAMED = {}


def framed_case(golden, shape, edge):
    """sum of cosines at the fixture's true k-vectors, three times as bright on a 4-pixel frame: the largest |lock-in| of
    every peak lies outside the window.  Oracle results, computed once per (shape, edge)."""
    key = (shape, edge)
    if key not in _FRAMED:
        g = golden('iterate_64')
        x = np.arange(shape[0], dtype=np.float64)[:, None]
        y = np.arange(shape[1], dtype=np.float64)[None, :]
        img = sum(np.cos(TWO_PI * (kx * x + ky * y)) for kx, ky in g['true_ks'])
        frame = np.ones(shape)
        frame[:4] = frame[-4:] = 3
        frame[:, :4] = frame[:, -4:] = 3
        img = img * frame
        img -= img.mean()
        start, sigma = g['start_ks'].copy(), 7
        rs = orc.lockin_batch(img, start, sigma)
        it = orc.iterate_gpa(img, start, sigma, edge=edge, iters=2)
        for a in (img, start, rs) + tuple(it):
            a.setflags(write=False)
        _FRAMED[key] = (img, start, sigma, rs, it)
    return _FRAMED[key]


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('edge', [3, 5])
@pytest.mark.parametrize('shape', [(48, 80), (63, 65)])
def test_weights_use_the_windows_maximum(golden, shape, edge, dtype):
    img, start, sigma, rs, (prs_o, w_o, corr_o) = framed_case(golden, shape, edge)
    sl = (slice(None), slice(edge, -edge), slice(edge, -edge))
    a_full, a_win = np.abs(rs).max(axis=(1, 2)), np.abs(rs[sl]).max(axis=(1, 2))
    assert (a_full > 1.01 * a_win).all(), a_full / a_win      # the test's premise, from the oracle
    P, (n0, n1) = len(start), shape
    m0, m1 = n0 - 2 * edge, n1 - 2 * edge
    plan = _lib.Plan(shape, P, dtype)
    rsz = np.dtype(dtype).itemsize
    d_img = _lib.DeviceBuffer(n0 * n1 * rsz)
    d_lock = _lib.DeviceBuffer(P * n0 * n1 * 2 * rsz)
    d_psi, d_amp, d_wgt = (_lib.DeviceBuffer(P * m0 * m1 * rsz) for _ in range(3))
    d_amax = _lib.DeviceBuffer(P * rsz)
    d_img.upload(img.astype(dtype))
    plan.lockin_batch_dev(d_img.ptr, start, sigma, d_lock.ptr)
    plan.lockin_polar_crop_dev(d_lock.ptr, P, edge, d_psi.ptr, d_amp.ptr, d_amax.ptr, weight_ptr=d_wgt.ptr)
    plan.sync()
    lock = d_lock.download((P, n0, n1), plan.cdtype)[sl]
    psi, amp, wgt = (d.download((P, m0, m1), dtype) for d in (d_psi, d_amp, d_wgt))
    amax = d_amax.download((P,), dtype)
    assert np.array_equal(amax, amp.max(axis=(1, 2)))
    a_ref = np.abs(lock)
    w_ref = np.sqrt(a_ref / a_ref.max(axis=(1, 2), keepdims=True))
    if dtype is np.float64:
        assert np.allclose(amp, a_ref, rtol=1e-8, atol=1e-10) and np.allclose(wgt, w_ref, rtol=1e-8, atol=1e-10)
    else:
        assert np.allclose(amp, a_ref, rtol=2e-5, atol=1e-5) and np.allclose(wgt, w_ref, rtol=2e-5, atol=1e-5)
    d = psi.astype(np.float64) - np.angle(lock.astype(np.complex128))
    d = np.abs((d + np.pi) % TWO_PI - np.pi)
    assert d.max() < (1e-12 if dtype is np.float64 else 2e-6), d.max()
    # a second call must not inherit the first one's maximum: amax is zeroed by the call
    plan.lockin_polar_crop_dev(d_lock.ptr, P, edge, d_psi.ptr, d_amp.ptr, d_amax.ptr)
    plan.sync()
    assert np.array_equal(d_amax.download((P,), dtype), amax)
    plan.close()
    for b in (d_img, d_lock, d_psi, d_amp, d_wgt, d_amax):
        b.free()
    prs, w, corr = _GPA().iterate_GPA(img, start, sigma, edge=edge, iters=2, dtype=dtype, fused=True)
    check_item1(prs, w, corr, prs_o, w_o, corr_o, dtype)


# ---------------------------------------------------------------------------------------------------------------- 3
def _image(golden, shape):
    g = golden('iterate_64')
    if shape == (64, 64):
        return g['image'] - g['image'].mean(), g['start_ks'], int(g['sigma'])
    img = hex_moire(shape, g['true_ks'], None, noise=0.05, seed=3)
    return img - img.mean(), g['start_ks'], int(g['sigma'])


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shape,edge,P,iters', [((64, 64), 0, 3, 2), ((64, 64), 0, 1, 0), ((63, 65), 3, 1, 2), ((63, 65), 3, 2, 1),
                                                ((63, 65), 0, 2, 0), ((64, 64), 5, 2, 0)])
def test_edges_and_counts_against_the_host_loop(golden, shape, edge, P, iters, dtype):
    GPA = _GPA()
    img, start, sigma = _image(golden, shape)
    start = start[:P]
    kw = dict(edge=edge, iters=iters, kmax_iter=3, kmax=7)
    prs_h, w_h, corr_h = GPA.iterate_GPA(img, start, sigma, dtype=dtype, fused=False, **kw)
    prs, w, corr = GPA.iterate_GPA(img, start, sigma, dtype=dtype, fused=True, **kw)
    assert prs.shape == prs_h.shape == (P, shape[0] - 2 * edge, shape[1] - 2 * edge)
    assert prs.dtype == prs_h.dtype and w.dtype == w_h.dtype and corr.dtype == corr_h.dtype == np.float64
    check_item1(prs, w, corr, prs_h, w_h, corr_h, dtype, factor=2)
    plan = _lib.Plan(shape, P, dtype)
    crop = plan if edge == 0 else _lib.Plan((shape[0] - 2 * edge, shape[1] - 2 * edge), 1, dtype)
    out = plan.iterate_gpa(img, start, sigma, crop_plan=crop, **kw)
    assert np.array_equal(out[0], prs) and np.array_equal(out[1], w) and np.array_equal(out[2], corr)
    assert out[3].shape == (iters, P, 2) and out[4].shape == (iters + 1, P)
    c = np.zeros((P, 2))
    for dk in out[3]:
        c -= dk
    assert np.array_equal(c, corr)                                    # corr is the running difference of the steps, in f64
    # (a solve may stop before its limit: the stopping test and the breakdown guard are the unwrap's own)
    assert (out[4] >= 1).all() and (out[4][:-1] <= 3).all() and (out[4][-1] <= 7).all()
    if iters == 0:
        assert np.array_equal(corr, np.zeros((P, 2)))
        # the one pass is the last one: kmax governs it, kmax_iter is never looked at
        other = plan.iterate_gpa(img, start, sigma, crop_plan=crop, edge=edge, iters=0, kmax_iter=1, kmax=7)
        assert all(np.array_equal(a, b) for a, b in zip(out, other))
        fewer = plan.iterate_gpa(img, start, sigma, crop_plan=crop, edge=edge, iters=0, kmax_iter=3, kmax=2)
        assert (fewer[4] <= 2).all() and not np.array_equal(fewer[0], out[0])
    if edge == 0:
        none = plan.iterate_gpa(img, start, sigma, crop_plan=None, **kw)       # the frame's plan serves the window
        assert all(np.array_equal(a, b) for a, b in zip(out, none))
    else:
        crop.close()
    plan.close()


# ---------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize('dtype', DTYPES)
def test_driver_is_nothing_but_its_parts(golden, dtype):
    shape, edge, iters, kmax_iter, kmax = (63, 65), 3, 2, 6, 12
    img, start, sigma = _image(golden, shape)
    P, (n0, n1) = len(start), shape
    m0, m1 = n0 - 2 * edge, n1 - 2 * edge
    rsz = np.dtype(dtype).itemsize
    plan, crop = _lib.Plan(shape, P, dtype), _lib.Plan((m0, m1), 1, dtype)
    whole = plan.iterate_gpa(img, start, sigma, edge=edge, iters=iters, kmax_iter=kmax_iter, kmax=kmax, crop_plan=crop)
    d_img = _lib.DeviceBuffer(n0 * n1 * rsz)
    d_lock = _lib.DeviceBuffer(P * n0 * n1 * 2 * rsz)
    d_psi, d_amp, d_wgt, d_prs, d_w2 = (_lib.DeviceBuffer(P * m0 * m1 * rsz) for _ in range(5))
    d_amax = _lib.DeviceBuffer(P * rsz)
    d_img.upload(img.astype(dtype))
    # device form == host form
    corr_d, dk_d, uit_d = plan.iterate_gpa_dev(d_img.ptr, start, sigma, d_prs.ptr, d_w2.ptr, edge=edge, iters=iters,
                                               kmax_iter=kmax_iter, kmax=kmax, crop_plan=crop)
    assert np.array_equal(d_prs.download((P, m0, m1), dtype), whole[0])
    assert np.array_equal(d_w2.download((P, m0, m1), dtype), whole[1])
    assert np.array_equal(corr_d, whole[2]) and np.array_equal(dk_d, whole[3]) and np.array_equal(uit_d, whole[4])
    # the parts, on fresh plans, with corr kept in f64 here
    plan2, crop2 = _lib.Plan(shape, P, dtype), _lib.Plan((m0, m1), 1, dtype)
    corr = np.zeros((P, 2))
    dks, uits = [], []
    plane = m0 * m1 * rsz
    for i in range(iters + 1):
        plan2.lockin_batch_dev(d_img.ptr, start + corr, sigma, d_lock.ptr)
        plan2.lockin_polar_crop_dev(d_lock.ptr, P, edge, d_psi.ptr, d_amp.ptr, d_amax.ptr, weight_ptr=d_wgt.ptr)
        plan2.sync()
        last = i == iters
        uits.append([crop2.unwrap_dev(d_psi.ptr + q * plane, d_wgt.ptr + q * plane, d_prs.ptr + q * plane,
                                      kmax=kmax if last else kmax_iter) for q in range(P)])
        if not last:
            coef, _ = crop2.fit_planes_dev(d_prs.ptr, P)
            dks.append(coef[:, :2] / (2 * np.pi))
            corr -= dks[-1]
    assert np.array_equal(d_prs.download((P, m0, m1), dtype), whole[0])
    assert np.array_equal(d_amp.download((P, m0, m1), dtype), whole[1])
    assert np.array_equal(corr, whole[2]) and np.array_equal(np.array(dks), whole[3]) and np.array_equal(np.array(uits), whole[4])
    # gpa_unwrap_dev == gpa_unwrap
    psi, wgt = d_psi.download((P, m0, m1), dtype), d_wgt.download((P, m0, m1), dtype)
    phi_h, it_h = crop2.unwrap(psi[1], wgt[1], kmax=kmax)
    assert it_h == uits[-1][1] and np.array_equal(phi_h, whole[0][1])
    for p in (plan, crop, plan2, crop2):
        p.close()
    for b in (d_img, d_lock, d_psi, d_amp, d_wgt, d_prs, d_w2, d_amax):
        b.free()


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shape', [(57, 59), (300, 70), (1100, 37)])     # rows: below / above 256 columns, above 1024 workgroups
def test_fit_planes_equal_single_fits(shape, dtype):
    """planes that converge after different numbers of rounds: an exact plane, a plane with outliers, a noisy steep one"""
    rng = np.random.default_rng(11)
    x, y = np.arange(shape[0])[:, None], np.arange(shape[1])[None, :]
    exact = 0.02 * x - 0.013 * y + 0.4
    outl = 0.05 * x + 0.01 * y - 1.0 + 0.1 * rng.standard_normal(shape)
    outl[rng.random(shape) < 0.08] += 25.0
    steep = 0.9 * x - 0.7 * y + 3 * rng.standard_normal(shape)
    planes = np.ascontiguousarray(np.stack([exact, outl, steep, exact + 1.0]), dtype=dtype)
    P = len(planes)
    plan = _lib.Plan(shape, 1, dtype)
    buf = _lib.DeviceBuffer(planes.nbytes)
    buf.upload(planes)
    before = plan.workspace_bytes
    coef, its = plan.fit_planes_dev(buf.ptr, P)
    assert plan.workspace_bytes > before                  # the scratch the call grew is counted
    single = [plan.fit_plane_dev(buf.ptr + q * planes[0].nbytes) for q in range(P)]
    assert len(set(int(i) for i in its)) > 1, its          # they do stop after different numbers of rounds
    for q in range(P):
        assert np.array_equal(coef[q], single[q][0]) and its[q] == single[q][1], (q, coef[q], single[q])
    # ... and a subset gives the same bits as the whole set
    coef2, its2 = plan.fit_planes_dev(buf.ptr + planes[0].nbytes, 2, max_iter=3)
    s3 = [plan.fit_plane_dev(buf.ptr + q * planes[0].nbytes, max_iter=3) for q in (1, 2)]
    assert all(np.array_equal(coef2[i], s3[i][0]) and its2[i] == s3[i][1] for i in range(2))
    plan.close()
    buf.free()


# ---------------------------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize('dtype', DTYPES)
def test_plans_are_unchanged_by_a_fused_call(golden, dtype):
    from pygpa_amd.synthetic import explicit_klists, hex_kvecs
    shape, edge = (63, 65), 3
    win = (shape[0] - 2 * edge, shape[1] - 2 * edge)
    img, start, sigma = _image(golden, shape)
    kw = dict(edge=edge, iters=1, kmax_iter=4, kmax=6)
    kv = hex_kvecs(0.12, 11.0)
    klists = np.stack(explicit_klists(kv, np.linalg.norm(kv, axis=1).mean() / 2.5, 2, 2))
    rng = np.random.default_rng(2)
    dx = (0.2 * rng.standard_normal((win[0], win[1] - 1))).astype(dtype)
    dy = (0.2 * rng.standard_normal((win[0] - 1, win[1]))).astype(dtype)
    wt = rng.random(win).astype(dtype)
    other = start[::-1] * 1.01

    def after(plan, crop):
        u = plan.extract_displacement_field(img, kv, klists, 6.0, 3, 5)
        return (u[0], u[3], crop.unwrap_prediff(dx, dy, wt, kmax=5), crop.fit_plane(wt),
                plan.iterate_gpa(img, other, sigma, crop_plan=crop, **kw))

    plan, crop = _lib.Plan(shape, 12, dtype), _lib.Plan(win, 1, dtype)
    b0, c0 = plan.workspace_bytes, crop.workspace_bytes
    plan.iterate_gpa(img, start, sigma, crop_plan=crop, **kw)
    assert plan.workspace_bytes > b0 and crop.workspace_bytes > c0      # lock-in planes; psi / weight / Huber scratch
    used = after(plan, crop)
    fresh_plan, fresh_crop = _lib.Plan(shape, 12, dtype), _lib.Plan(win, 1, dtype)
    fresh = after(fresh_plan, fresh_crop)

    def same(a, b):
        if isinstance(a, (tuple, list)):
            return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
        if isinstance(a, np.ndarray):
            return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)
        return a == b
    for name, a, b in zip(('u', 'iters', 'unwrap_prediff', 'fit_plane', 'second fused call'), used, fresh):
        assert same(a, b), name
    for p in (plan, crop, fresh_plan, fresh_crop):
        p.close()


# ---------------------------------------------------------------------------------------------------------------- 6
def _raw(plan, crop, image, kvecs, P, sigma, edge, iters, kmax_iter, kmax, prs, w, corr, form='gpa_iterate_gpa'):
    ptr = lambda a: None if a is None else (C.c_void_p(a) if isinstance(a, int) else a.ctypes.data_as(C.c_void_p))
    fn = getattr(_lib.load(), form)
    rc = fn(plan.handle if plan is not None else None, crop.handle if crop is not None else None, ptr(image), ptr(kvecs), P,
            float(sigma), edge, iters, kmax_iter, kmax, ptr(prs), ptr(w), ptr(corr), None, None)
    return rc, _lib.last_error()


@pytest.mark.parametrize('dtype', DTYPES)
def test_errors_name_their_argument_and_launch_nothing(golden, dtype):
    shape, edge = (63, 65), 3
    win = (shape[0] - 2 * edge, shape[1] - 2 * edge)
    img, start, sigma = _image(golden, shape)
    img = np.ascontiguousarray(img, dtype=dtype)
    kvecs = np.ascontiguousarray(start, dtype=np.float64)
    P = len(kvecs)
    plan, crop = _lib.Plan(shape, P, dtype), _lib.Plan(win, 1, dtype)
    wrong_shape = _lib.Plan((win[0] + 1, win[1]), 1, dtype)
    wrong_dtype = _lib.Plan(win, 1, np.float32 if dtype is np.float64 else np.float64)
    prs, w = np.empty((P,) + win, dtype=dtype), np.empty((P,) + win, dtype=dtype)
    corr = np.zeros((P, 2))
    ok = dict(plan=plan, crop=crop, image=img, kvecs=kvecs, P=P, sigma=sigma, edge=edge, iters=1, kmax_iter=4, kmax=6, prs=prs,
              w=w, corr=corr)
    ARG, STATE = -1, -4
    cases = [(dict(plan=None), ARG, 'plan'), (dict(image=None), ARG, 'image'), (dict(kvecs=None), ARG, 'kvecs'),
             (dict(prs=None), ARG, 'prs'), (dict(w=None), ARG, 'w is null'), (dict(corr=None), ARG, 'corr'),
             (dict(P=0), ARG, 'P must'), (dict(P=P + 1), ARG, 'max_batch'), (dict(iters=-1), ARG, 'iters'),
             (dict(edge=-1), ARG, 'edge'), (dict(edge=31), ARG, 'edge'), (dict(crop=None), ARG, 'crop_plan'),
             (dict(crop=wrong_shape), ARG, 'crop_plan'), (dict(crop=wrong_dtype), ARG, 'crop_plan'),
             (dict(crop=plan), ARG, 'crop_plan')]
    for form in ('gpa_iterate_gpa', 'gpa_iterate_gpa_dev'):
        for change, code, word in cases:
            args = dict(ok)
            args.update(change)
            rc, msg = _raw(form=form, **args)
            assert rc == code and word in msg and msg.startswith('gpa_iterate_gpa:'), (form, change, rc, msg)
    # refusals of the two plans (nothing of either is ever launched: the frames are never uploaded)
    if dtype is np.float64:
        big = _lib.Plan((8, 4097), 1, dtype)                  # 4097 points: beyond the f64 sweep's 4096 for other lengths
        nowin = _lib.Plan((4, 8192), 1, dtype)                # the sweep takes it, the unwrap has no kernels: the smallest such shape
    else:
        big = _lib.Plan((8, 8193), 1, dtype)
        nowin = _lib.Plan((4, 16384), 1, dtype)
    for p, word in ((big, 'plan (the frame)'), (nowin, 'unwrap kernels')):
        n = p.shape[0] * p.shape[1]
        z = np.zeros(n, dtype=dtype)
        rc, msg = _raw(p, None, z, kvecs[:1], 1, sigma, 0, 0, 4, 6, z.copy(), z.copy(), np.zeros(2))
        assert rc == STATE and word in msg, (rc, msg)
        rc, msg = _raw(p, p, z, kvecs[:1], 1, sigma, 0, 0, 4, 6, z.copy(), z.copy(), np.zeros(2))
        assert rc == STATE and word in msg, (rc, msg)
        p.close()
    # after all those refusals the pair answers like a fresh one
    got = plan.iterate_gpa(img, kvecs, sigma, edge=edge, iters=1, kmax_iter=4, kmax=6, crop_plan=crop)
    fp, fc = _lib.Plan(shape, P, dtype), _lib.Plan(win, 1, dtype)
    fresh = fp.iterate_gpa(img, kvecs, sigma, edge=edge, iters=1, kmax_iter=4, kmax=6, crop_plan=fc)
    assert all(np.array_equal(a, b) for a, b in zip(got, fresh))
    for p in (plan, crop, wrong_shape, wrong_dtype, fp, fc):
        p.close()
