"""The per-pixel weighted solve of a5 / a6 on the device, at every P = 2 ... 8, in both precisions, kernel by kernel against
LAPACK (tests/lstsq_cases.py: cases, reference, derived bound), and the fused driver at P != 3 against the oracle's pieces and the
library's own unfused route.  Run with `-m gpu` on an MI355X.

Every check prints a line 'CMEAS kernel P class dtype figure' before it asserts (pytest -s shows them); lstsq_cases.C_MEASURED is
made of those lines.

Shapes.  A plan needs both sides >= 4 (gpa_plan_create), so the smallest shape is (4, 4) and the thin one (4, 257): one pixel
row per workgroup row in prediff_kernel, a second 256-thread block with one live thread in all the kernels.  (17, 70) is ragged
in both directions.  For reconstruct_kernel: (4, 4); (16, 64) and (17, 65) around the band of REC_ROWS = 16 rows and lane 63's
reload of its right neighbour from memory; (33, 257) a third band and a second workgroup along the row.
"""
import ctypes as C

import numpy as np
import pytest

import lstsq_cases as lc
from oracle import gpa_oracle as orc
from pygpa_amd import _lib
from pygpa_amd.synthetic import gaussian_bump_displacement, hex_moire, explicit_klists

pytestmark = pytest.mark.gpu

SOLVE_SHAPES = [(4, 4), (4, 257), (17, 70)]
REC_SHAPES = [(4, 4), (16, 64), (17, 65), (33, 257)]
REC_FULL = (17, 65)                   # the shape at which reconstruct_kernel sees every class; the others: REC_FEW
REC_FEW = ('equal', 'one_nonzero')    # and the smallest graded ratio of the precision
NM = 3.7


def name_of(dtype):
    return np.dtype(dtype).name


def report(kernel, P, cls, dtype, figure):
    print('CMEAS %s %d %s %s %.4g' % (kernel, P, cls, name_of(dtype), figure))


def check_solution(kernel, kset, cls, dtype, x, x_ref, x_r1, b, w, K, tag=''):
    """one kernel's answer (2, ...) for one class against LAPACK: the bound, the stability condition or exact zeros"""
    P = len(K)
    x = np.asarray(x, dtype=np.float64)
    assert x.shape == x_ref.shape
    assert np.isfinite(x).all(), (kernel, kset, cls, tag)
    if cls == 'all_zero':
        report(kernel, P, cls, dtype, float(np.abs(x).max()))
        assert not x.any(), (kernel, kset, tag)
    elif cls == 'beyond':
        q = lc.stability_ratio(x, x_ref, x_r1)
        report(kernel, P, cls, dtype, q)
        # which pixels kept the dominant direction only: those that equal the rank-1 answer to rounding
        r1 = lc.norm2(x - x_r1) <= lc.bound(x_r1, b, K, w, dtype, db=lc.DB[kernel], deficient=True, extra=lc.EXTRA[kernel])
        print('RANK1 %s %d %s %s %.3f' % (kernel, P, tag, name_of(dtype), r1.mean()))
        assert q <= 2.0, (kernel, kset, tag, q)
    else:
        bnd = lc.bound(x_ref, b, K, w, dtype, db=lc.DB[kernel], deficient=cls in lc.DEFICIENT, extra=lc.EXTRA[kernel])
        q = lc.ratio(x, x_ref, bnd)
        report(kernel, P, cls, dtype, q)
        if cls == 'graded':      # the share of pixels that kept the dominant direction only (none but at f32's smallest ratio)
            r1 = lc.norm2(x - x_r1) <= lc.bound(x_r1, b, K, w, dtype, db=lc.DB[kernel], deficient=True, extra=lc.EXTRA[kernel])
            print('RANK1 %s %d %s %s %.3f' % (kernel, P, tag, name_of(dtype), r1.mean()))
        assert q <= 1.0, (kernel, kset, cls, tag, q)


# ---- wlstsq_kernel and prediff_kernel -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', lc.DTYPES)
@pytest.mark.parametrize('shape', SOLVE_SHAPES)
@pytest.mark.parametrize('kset', lc.KSET_NAMES)
def test_weighted_lstsq_vs_lapack(kset, shape, dtype):
    kvecs = lc.KSETS[kset]
    plan = _lib.get_plan(shape, len(kvecs), dtype)
    for label, cls, r in lc.class_list(kset, dtype):
        c = lc.solve_case(kset, label, shape, name_of(dtype))
        x = plan.weighted_lstsq(c['b'], c['w'], kvecs)
        assert x.dtype == np.dtype(dtype)
        check_solution('wlstsq', kset, cls, dtype, x, c['x_ref'], c['x_r1'], c['b'], c['w'], c['K'], label)


def prediff_inputs(kset, label, shape, dtype):
    """grads (P, n0, n1, 2) in the dtype: the class's right-hand sides (another draw for the second component) shifted by
    0, +-2 pi, +-4 pi from pixel to pixel; f64: a few samples exactly at +-pi.  Returns grads and their wrapped float64 values"""
    c = lc.solve_case(kset, label, shape, name_of(dtype))
    b2 = lc.rhs(kset, shape, (label, 'axis0'))
    n = shape[0] * shape[1]
    turns = (np.arange(n) % 5 - 2).reshape(shape)
    g = np.stack([c['b'] + lc.TWO_PI * turns, b2 + lc.TWO_PI * np.roll(turns, 2)], axis=-1)
    if np.dtype(dtype) == np.float64:
        flat = g.reshape(len(c['K']), n, 2)
        flat[0, 0::7, 0] = np.pi
        flat[1, 3::7, 0] = -np.pi
        flat[-1, 5::7, 1] = np.pi
    g = lc.rounded(g, dtype)
    wrapped = lc.wrap_to_pi(g)
    if np.dtype(dtype) == np.float64:
        assert (wrapped == -np.pi).sum() >= 3 and not (wrapped == np.pi).any()     # wrapToPi: +pi -> -pi
        rest = np.abs(np.abs(g.reshape(len(c['K']), n, 2)) - np.pi) > 0
        assert np.abs(wrapped.reshape(len(c['K']), n, 2)[rest]).max() < np.pi - 0.4
    else:
        assert np.abs(wrapped).max() < np.pi - 0.4 > lc.SEAM_MARGIN
    return c, g, wrapped


@pytest.mark.parametrize('dtype', lc.DTYPES)
@pytest.mark.parametrize('shape', SOLVE_SHAPES)
@pytest.mark.parametrize('kset', lc.KSET_NAMES)
def test_reconstruct_prediff_vs_lapack(kset, shape, dtype):
    kvecs = lc.KSETS[kset]
    plan = _lib.get_plan(shape, len(kvecs), dtype)
    u = lc.U[np.dtype(dtype)]
    for label, cls, r in lc.class_list(kset, dtype):
        c, g, wrapped = prediff_inputs(kset, label, shape, dtype)
        dudx, dudy, wn = plan.reconstruct_prediff(g, c['w'], kvecs)
        bx, wx = wrapped[..., 0][:, :, :-1], c['w'][:, :, :-1]
        by, wy = wrapped[..., 1][:, :-1, :], c['w'][:, :-1, :]
        K = c['K']
        check_solution('prediff', kset, cls, dtype, dudx, lc.lapack(bx, K, wx), lc.rank1(bx, K, wx), bx, wx, K, label + ' dx')
        check_solution('prediff', kset, cls, dtype, dudy, lc.lapack(by, K, wy), lc.rank1(by, K, wy), by, wy, K, label + ' dy')
        # wnorm = ||w||_2: P squares and sums, a root, the normalisation and its undoing
        ref = lc.norm2(c['w'])
        assert np.all(np.abs(wn - ref) <= (len(K) + 6) * u * ref), label


# ---- jacobian_kernel ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', lc.DTYPES)
@pytest.mark.parametrize('kset', lc.KSET_NAMES)
def test_phasegradient2J_vs_lapack(kset, dtype):
    """J[n, m, i, j] = + (lstsq of grads[:, n, m, j])_i / nmperpixel, the sign of the reference's phasegradient2J
    (property_extract.py:97-99; the minus belongs to phases2J, :50)"""
    shape = (17, 70)
    kvecs = lc.KSETS[kset]
    plan = _lib.get_plan(shape, len(kvecs), dtype)
    for label, cls, r in lc.class_list(kset, dtype, signed=False):
        c = lc.solve_case(kset, label, shape, name_of(dtype))
        b2 = lc.rounded(lc.rhs(kset, shape, (label, 'axis0')), dtype)
        J = plan.phasegradient2J(kvecs, np.stack([c['b'], b2], axis=-1), c['w'], NM)
        assert J.shape == shape + (2, 2) and J.dtype == np.dtype(dtype)
        # (J nm is x with two more roundings, 1 / nm and the product: far inside a bound of C(P) >= 22 roundings times kappa^2;
        #  a zero stays a zero)
        for j, b in ((0, c['b']), (1, b2)):
            x = np.moveaxis(J[..., j].astype(np.float64), -1, 0) * NM
            x_ref = c['x_ref'] if j == 0 else lc.lapack(b, c['K'], c['w'])
            check_solution('jacobian', kset, cls, dtype, x, x_ref, lc.rank1(b, c['K'], c['w']), b, c['w'], c['K'], label + ' j%d' % j)


# ---- reconstruct_kernel<T, P> ---------------------------------------------------------------------------------------------------
def rec_labels(kset, dtype, shape):
    labels = lc.class_list(kset, dtype, signed=False)
    if shape == REC_FULL:
        return labels
    few = REC_FEW + ('graded_%g' % lc.GRADED[np.dtype(dtype)][-1],)
    return [t for t in labels if t[0] in few]


def check_reconstruct(kset, cls, label, dtype, c, dudx, dudy, tag):
    check_solution('reconstruct', kset, cls, dtype, dudx, c['dx'], c['dx_r1'], c['bx'], c['wx'], c['K'], '%s dx %s' % (label, tag))
    check_solution('reconstruct', kset, cls, dtype, dudy, c['dy'], c['dy_r1'], c['by'], c['wy'], c['K'], '%s dy %s' % (label, tag))


@pytest.mark.parametrize('dtype', lc.DTYPES)
@pytest.mark.parametrize('shape', REC_SHAPES)
@pytest.mark.parametrize('kset', lc.KSET_NAMES)
def test_reconstruct_grad_vs_lapack(kset, shape, dtype):
    """lock-ins w exp(i phi): the device's wrapped differences of atan2 against np.angle of the same numbers, solved per pixel.
    mask_border 0 and 3, and a border wider than half the image: there every weight carries the 1e-6 factor and the answers are
    those of border 0 within the same bound"""
    kvecs = lc.KSETS[kset]
    P = len(kvecs)
    plan = _lib.get_plan(shape, P, dtype)
    u = lc.U[np.dtype(dtype)]
    n0, n1 = shape
    wide = max(n0, n1) // 2 + 1
    for label, cls, r in rec_labels(kset, dtype, shape):
        c = lc.lockin_case(kset, label, shape, name_of(dtype))
        for border in (0, 3, wide):
            dudx, dudy, wn = plan.reconstruct_grad(c['z'], kvecs, border)
            check_reconstruct(kset, cls, label, dtype, c, dudx, dudy, 'border %d' % border)
            # wnorm = || |z| (mask + 1e-6) ||_2 with the factor as the kernel forms it in T
            i, j = np.meshgrid(np.arange(n0), np.arange(n1), indexing='ij')
            inside = (i >= border) & (i < n0 - border) & (j >= border) & (j < n1 - border)
            T = np.dtype(dtype).type
            mfac = (np.where(inside, T(1), T(0)) + T(1e-6)).astype(np.float64)
            ref = lc.norm2(c['amp']) * mfac
            assert np.all(np.abs(wn - ref) <= (P + 8) * u * ref), (label, border)
            if border == wide:
                assert not inside.any()


@pytest.mark.parametrize('dtype', lc.DTYPES)
@pytest.mark.parametrize('kset', lc.KSET_NAMES)
def test_reconstruct_grad_dev_equals_host_form(kset, dtype):
    """gpa_reconstruct_grad_dev on device pointers: the bits of the host form"""
    shape = REC_FULL
    kvecs = np.ascontiguousarray(lc.KSETS[kset], dtype=np.float64)
    P = len(kvecs)
    plan = _lib.get_plan(shape, P, dtype)
    c = lc.lockin_case(kset, 'equal', shape, name_of(dtype))
    n0, n1 = shape
    rsz = np.dtype(dtype).itemsize
    dudx, dudy, wn = plan.reconstruct_grad(c['z'], kvecs, 3)
    d_z = _lib.DeviceBuffer(c['z'].nbytes)
    d_dx, d_dy, d_w = (_lib.DeviceBuffer(k * rsz) for k in (2 * n0 * (n1 - 1), 2 * (n0 - 1) * n1, n0 * n1))
    try:
        d_z.upload(c['z'])
        _lib.check(plan.lib.gpa_reconstruct_grad_dev(plan.handle, C.c_void_p(d_z.ptr), kvecs.ctypes.data_as(C.c_void_p), P, 3,
                                                     C.c_void_p(d_dx.ptr), C.c_void_p(d_dy.ptr), C.c_void_p(d_w.ptr)),
                   'gpa_reconstruct_grad_dev')
        plan.sync()
        assert np.array_equal(d_dx.download((2, n0, n1 - 1), dtype), dudx)
        assert np.array_equal(d_dy.download((2, n0 - 1, n1), dtype), dudy)
        assert np.array_equal(d_w.download((n0, n1), dtype), wn)
    finally:
        for buf in (d_z, d_dx, d_dy, d_w):
            buf.free()


# ---- reconstruct_setup_kernel<T, P>: the fused driver at P != 3 ----------------------------------------------------------------------
DRIVER_SETS = ['hex2', 'sq2', 'sq4', 'hex6', 'sq8']
DRIVER_SHAPES = [(48, 80), (63, 65)]
_driver_cache = {}


def driver_case(kset, shape):
    """image of the set's P cosines, 2 x 2 k-lists, and the oracle's pieces run once: sweep -> phases_weights ->
    reconstruct_gradients -> unwrap_prediff"""
    key = (kset, shape)
    if key not in _driver_cache:
        kvecs = lc.KSETS[kset]
        img = hex_moire(shape, kvecs, gaussian_bump_displacement(shape), noise=0.1, seed=9)
        _, sigma, _ = orc.derive_params(kvecs)
        # candidates within 0.4 of the shortest vector: the sets with second-order peaks have neighbours 1 |k| apart
        klists = np.stack(explicit_klists(kvecs, np.linalg.norm(kvecs, axis=1).min() / 2.5, 2, 2))
        gs = [orc.sweep(img - img.mean(), sigma, klists[p], kvecs[p]) for p in range(len(kvecs))]
        phases, weights, _ = orc.phases_weights(np.stack([g['lockin'] for g in gs]), sigma)
        dudx, dudy = orc.reconstruct_gradients(kvecs, phases, weights)
        wn = np.linalg.norm(weights, axis=0)
        u_ref = np.stack([orc.unwrap_prediff(dudx[c], dudy[c], wn, kmax=10) for c in range(2)])
        _driver_cache[key] = dict(kvecs=kvecs, img=img, sigma=sigma, klists=klists, u_ref=u_ref)
    return _driver_cache[key]


def rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


@pytest.mark.parametrize('dtype', lc.DTYPES)
@pytest.mark.parametrize('shape', DRIVER_SHAPES)
@pytest.mark.parametrize('kset', DRIVER_SETS)
def test_fused_driver_at_every_P(kset, shape, dtype):
    """extract_displacement_field with P = 2 (hex pair, square pair), 4, 6 and 8 peaks, max_batch = 4 P: against the oracle's
    pieces with the tolerances of test_fused_driver_rectangular_pow2, and against the library's own unfused route sweep ->
    reconstruct_grad -> unwrap_prediff (f64: equal iteration counts and u within 1e-9, the fused kernel's arithmetic being that
    of the two separate kernels; f32: the 2e-5 of test_fused_driver_golden)"""
    d = driver_case(kset, shape)
    kvecs, img, sigma, klists = d['kvecs'], d['img'], d['sigma'], d['klists']
    P = len(kvecs)
    plan = _lib.get_plan(shape, 4 * P, dtype)
    assert plan.max_batch >= 4 * P
    u, lock, kidx, iters = plan.extract_displacement_field(img, kvecs, klists, sigma, 2 * sigma, kmax=10, want_lockins=True, want_kidx=True)
    assert np.isfinite(u).all()
    print('DRIVER %s %s %s oracle %.3g' % (kset, shape, name_of(dtype), rel(u, d['u_ref'])))
    if np.dtype(dtype) == np.float64:
        assert rel(u, d['u_ref']) < 1e-8
    else:
        e = (u - u.mean(axis=(1, 2), keepdims=True)) - (d['u_ref'] - d['u_ref'].mean(axis=(1, 2), keepdims=True))
        assert np.sqrt((e ** 2).mean()) / np.abs(d['u_ref']).max() < 3e-3
    img0 = img - img.mean()
    locks = np.stack([plan.sweep(img0, kvecs[p], klists[p], sigma)[0] for p in range(P)])
    dudx, dudy, wn = plan.reconstruct_grad(locks, kvecs, 2 * sigma)
    parts = [plan.unwrap_prediff(dudx[c], dudy[c], wn, kmax=10) for c in range(2)]
    u2 = np.stack([p[0] for p in parts])
    print('DRIVER %s %s %s unfused %.3g iters %s %s' % (kset, shape, name_of(dtype), rel(u, u2), iters, [p[1] for p in parts]))
    if np.dtype(dtype) == np.float64:
        assert tuple(iters) == tuple(p[1] for p in parts)
        assert rel(u, u2) < 1e-9
    else:
        assert rel(u, u2) < 2e-5


@pytest.mark.parametrize('dtype', lc.DTYPES)
@pytest.mark.parametrize('kset', ['hex2', 'sq8'])
def test_stack_call_equals_single_calls(kset, dtype, gpa_option):
    """B = 2 frames through the batched driver (reconstruct_setup_kernel with blockIdx.z = image) at P = 2 and P = 8: the bits and
    iteration counts of the single calls (GPA_NO_LAT as in test_image_stack_equals_single_images: same kernels on both sides)"""
    gpa_option('NO_LAT', '1')
    shape = (63, 65)
    d = driver_case(kset, shape)
    kvecs, sigma, klists = d['kvecs'], d['sigma'], d['klists']
    frames = np.stack([d['img'], hex_moire(shape, kvecs, 0.5 * gaussian_bump_displacement(shape), noise=0.2, seed=4)])
    plan = _lib.get_plan(shape, 4 * len(kvecs), dtype)
    us, its = plan.extract_displacement_field_stack(frames, kvecs, klists, sigma, 2 * sigma, kmax=10)
    for f in range(2):
        u, _, _, it = plan.extract_displacement_field(frames[f], kvecs, klists, sigma, 2 * sigma, kmax=10)
        assert np.array_equal(us[f], u), f
        assert tuple(its[f]) == tuple(it), f


@pytest.mark.parametrize('dtype', lc.DTYPES)
def test_tile_window_at_P2(dtype):
    """one gpa_tile_gradients_dev window at P = 2 (reconstruct_kernel<T, 2> in tile mode, storing an interior rectangle into
    pitched blocks) against the interior of reconstruct_grad on the same window's lock-ins, with the project's tolerance for
    gradients (test_a5_a6_reconstruct: 1e-11 / 2e-5 of the largest value)"""
    shape = (48, 80)
    d = driver_case('hex2', shape)
    kvecs, img, sigma, klists = d['kvecs'], d['img'], d['sigma'], d['klists']
    n0, n1 = shape
    plan = _lib.get_plan(shape, 4 * len(kvecs), dtype)
    rsz = np.dtype(dtype).itemsize
    i0, j0, t0, t1 = 5, 7, 38, 66            # interior rectangle: rows 5 ... 42, columns 7 ... 72
    image = np.ascontiguousarray(img, dtype=dtype)
    d_img = _lib.DeviceBuffer(image.nbytes)
    d_dx, d_dy, d_w = (_lib.DeviceBuffer(k * t0 * t1 * rsz) for k in (2, 2, 1))
    try:
        d_img.upload(image)
        for buf, k in ((d_dx, 2), (d_dy, 2), (d_w, 1)):
            buf.upload(np.full(k * t0 * t1, -7.0, dtype=dtype))
        mean = float(image.astype(np.float64).mean())
        plan.tile_gradients_dev(d_img.ptr, n1, 0, 0, mean, kvecs, klists, sigma, 2 * sigma, (i0, j0, t0, t1),
                                (d_dx.ptr, t1, t0 * t1), (d_dy.ptr, t1, t0 * t1), (d_w.ptr, t1))
        plan.sync()
        tdx, tdy, tw = d_dx.download((2, t0, t1), dtype), d_dy.download((2, t0, t1), dtype), d_w.download((t0, t1), dtype)
    finally:
        for buf in (d_img, d_dx, d_dy, d_w):
            buf.free()
    img0 = image.astype(np.float64) - mean
    locks = np.stack([plan.sweep(img0, kvecs[p], klists[p], sigma)[0] for p in range(len(kvecs))])
    dudx, dudy, wn = plan.reconstruct_grad(locks, kvecs, 2 * sigma)
    tol = 1e-11 if np.dtype(dtype) == np.float64 else 2e-5
    sl = (slice(None), slice(i0, i0 + t0), slice(j0, j0 + t1))
    print('TILE %s dx %.3g dy %.3g w %.3g' % (name_of(dtype), rel(tdx, dudx[sl]), rel(tdy, dudy[sl]), rel(tw, wn[sl[1:]])))
    assert rel(tdx, dudx[sl]) < tol and rel(tdy, dudy[sl]) < tol
    assert rel(tw, wn[sl[1:]]) < (1e-11 if np.dtype(dtype) == np.float64 else 2e-6)


# ---- limits ---------------------------------------------------------------------------------------------------------------------
def test_P_limits_are_refused():
    """P = 1 and P = 9 are refused by all five entry points with the message they document ('need 2 <= P <= 8'), and so is
    P > max_batch"""
    shape = (16, 20)
    rng = np.random.default_rng(1)

    def calls(plan, P):
        k = 0.1 * rng.normal(size=(P, 2))
        real = rng.random((P,) + shape)
        cx = (real * np.exp(1j * real)).astype(plan.cdtype)
        g2 = rng.random((P,) + shape + (2,))
        klists = np.repeat(k[:, None, :], 1, axis=1)
        img = rng.random(shape)
        return {
            'gpa_reconstruct_grad': lambda: plan.reconstruct_grad(cx, k, 0),
            'gpa_extract_displacement_field': lambda: plan.extract_displacement_field(img, k, klists, 3, 2, want_lockins=True),
            'gpa_weighted_lstsq': lambda: plan.weighted_lstsq(real, real, k),
            'gpa_reconstruct_prediff': lambda: plan.reconstruct_prediff(g2, real, k),
            'gpa_phasegradient2J': lambda: plan.phasegradient2J(k, g2, real, NM),
        }

    for dtype in lc.DTYPES:
        plan = _lib.Plan(shape, 16, dtype)
        for P in (1, 9):
            for name, call in calls(plan, P).items():
                with pytest.raises(_lib.GPAError, match='need 2 <= P <= 8'):
                    call()
        for name, call in calls(plan, 8).items():       # the largest P is taken
            call()
        plan.close()
        small = _lib.Plan(shape, 3, dtype)               # max_batch = 3: P = 4 does not fit
        for name, call in calls(small, 4).items():
            with pytest.raises(_lib.GPAError, match='need 2 <= P <= 8|exceeds max_batch'):
                call()
        for name, call in calls(small, 3).items():
            call()
        small.close()
