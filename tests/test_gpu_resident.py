"""The device-pointer entry points (`*_dev`, `*_enqueue_dev`, `unwrap_finish`) on caller-owned buffers against their host
forms on a FRESH plan, bit for bit, and the bench's resident pipeline (bench.py `pipeline_end_to_end`) replayed stage by
stage and held to the oracle.  Run with `-m gpu` on an MI355X.

Every operand sits at a nonzero offset of a whole number of planes inside a larger buffer, as the bench places its lock-ins
and gradients; the planes around it are filled with NaN so that a read outside the operand shows up in the result.

Also here: ADVICE r06's find_peaks_dev truncation (more candidates than max_out came back as an arbitrary subset)."""
import numpy as np
import pytest

from oracle import gpa_oracle as orc
from pygpa_amd import _lib
from pygpa_amd.synthetic import hex_kvecs, explicit_klists, gaussian_bump_displacement, hex_moire
from test_gpu_parity import TOL
import tolerances as TOLS

pytestmark = pytest.mark.gpu
DTYPES = [np.float64, np.float32]
SHAPES = [(128, 256), (96, 80)]          # powers of two; mixed radix (96 = 2^5 3, 80 = 2^4 5)


class Slot:
    """one operand of `shape` / `dtype` at an offset of `lead` whole planes (n0 x n1 elements of its type) inside a buffer
    whose other bytes are all ones (NaN as f32 and f64, -1 as int32)"""

    def __init__(self, plane_px, shape, dtype, lead=1, host=None):
        self.shape, self.dtype = tuple(shape), np.dtype(dtype)
        self.off = lead * plane_px * self.dtype.itemsize
        self.nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        total = self.off + self.nbytes + plane_px * self.dtype.itemsize
        self.buf = _lib.DeviceBuffer(total)
        self.buf.upload(np.full(total, 0xFF, dtype=np.uint8))
        if host is not None:
            self.set(host)

    @property
    def ptr(self):
        return self.buf.ptr + self.off

    def set(self, host):
        host = np.ascontiguousarray(host, dtype=self.dtype)
        assert host.shape == self.shape
        self.buf.upload_at(host, self.off)

    def get(self):
        raw = self.buf.download((self.buf.nbytes,), np.uint8)
        # the bytes after the operand are still all ones: nothing wrote past it
        assert np.all(raw[self.off + self.nbytes:] == 0xFF) and np.all(raw[:self.off] == 0xFF)
        return raw[self.off:self.off + self.nbytes].view(self.dtype).reshape(self.shape).copy()

    def free(self):
        self.buf.free()


def _case(shape, seed=3, K=(2, 2)):
    kvecs = hex_kvecs(0.12, 11.0)
    img = hex_moire(shape, kvecs, gaussian_bump_displacement(shape), noise=0.1, seed=seed)
    img = img - img.mean()
    kw = np.linalg.norm(kvecs, axis=1).mean() / 2.5
    klists = np.stack(explicit_klists(kvecs, kw, *K))
    return img, kvecs, klists


def same(a, b):
    """bit-for-bit equality, NaN in the same places"""
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


# ---- A: find_peaks_dev with more candidates than max_out --------------------------------------------------
def _many_candidates_image():
    # counted with the oracle: 5180 candidates at sigma 1, no DoG, threshold_rel 0.01 (more than find_peaks' 4096)
    return hex_moire((512, 512), hex_kvecs(0.12, 17.0), noise=5.0, seed=9)


@pytest.mark.parametrize('dtype', DTYPES)
def test_find_peaks_dev_keeps_every_candidate(dtype):
    """find_peaks_dev used to keep min(count, 4096) candidates in the device's atomic-append order: an arbitrary subset.
    Now it fetches all of them like find_peaks does: dev == host exactly, in f64 the oracle's list; and
    extract_primary_ks_dev == extract_primary_ks, once on a first evaluation above 4096 candidates and once on a
    relaxation loop that walks the threshold down to 0.00625 (6942 candidates, through find_peaks_again)"""
    import pygpa_amd.geometric_phase_analysis as GPA
    img = _many_candidates_image()
    shape = img.shape
    d_img = Slot(img.size, shape, dtype, host=img)
    plan = _lib.Plan(shape, 1, dtype)
    c_dev, v_dev = plan.find_peaks_dev(d_img.ptr, 1.0, 0.0, 0.01)
    host = _lib.Plan(shape, 1, dtype)
    c_host, v_host = host.find_peaks(img, 1.0, 0.0, 0.01)
    print('find_peaks_dev %s: %d candidates (host %d)' % (np.dtype(dtype).name, len(c_dev), len(c_host)))
    assert len(c_host) > 4096
    assert np.array_equal(c_dev, c_host) and np.array_equal(v_dev, v_host)
    assert np.all(np.diff(v_dev) <= 0)
    if dtype is np.float64:
        ref = orc.smoothed_spectrum(img, 1, DoG=False)
        ref_c = orc.peak_local_max(ref, 0.01)
        # |p_hat(k)| = |p_hat(-k)| up to rounding: the order inside such a pair is not defined (find_peaks' docstring)
        assert {tuple(c) for c in c_dev} == {tuple(c) for c in ref_c}
        assert np.allclose(v_dev, ref[tuple(c_dev.T)], rtol=1e-10, atol=0)
    for kw in (dict(threshold=0.01, DoG=False, pix_norm_range=(59, 64)),     # 62 of the 5180 in the ring
               dict(pix_norm_range=(2, 6))):                                # relaxes: sigma 0.37, threshold 0.00625
        ks_dev, all_dev = GPA.extract_primary_ks_dev(_lib.Plan(shape, 1, dtype), d_img.ptr, **kw)
        ks_host, all_host = GPA._primary_ks(GPA._reusing(host, lambda s, d, t: host.find_peaks(img, s, d, t)), shape,
                                            False, kw.get('threshold', 0.7), kw['pix_norm_range'], 1, kw.get('DoG', True))
        assert np.array_equal(all_dev, all_host) and np.array_equal(ks_dev, ks_host), kw
        assert len(all_dev) >= 3
        if dtype is np.float64:
            ref_ks, ref_all = orc.extract_primary_ks(img, **kw)
            assert np.array_equal(ks_dev, ref_ks) and np.array_equal(all_dev, ref_all), kw
    plan.close()
    host.close()
    d_img.free()


# ---- B: every _dev entry point against its host form on a fresh plan --------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shape', SHAPES)
def test_dev_spectral_and_plane_fit(shape, dtype):
    """per_dft_dev, fit_plane_dev (coefficients and iteration count), gaussian_deconvolve_dev out of place and in place"""
    img, _, _ = _case(shape)
    ramp = img + 0.03 * np.arange(shape[0])[:, None] - 0.02 * np.arange(shape[1])[None, :]
    npx = img.size
    plan = _lib.Plan(shape, 1, dtype)
    d_img = Slot(npx, shape, dtype, lead=2, host=ramp)
    d_out = Slot(npx, shape, np.complex128 if dtype is np.float64 else np.complex64, lead=3)
    plan.per_dft_dev(d_img.ptr, d_out.ptr)
    plan.sync()                    # the _dev calls only enqueue; Slot.get copies on the null stream
    assert same(d_out.get(), _lib.Plan(shape, 1, dtype).per_dft(ramp))
    coef, it = plan.fit_plane_dev(d_img.ptr)
    coef_h, it_h = _lib.Plan(shape, 1, dtype).fit_plane(ramp)
    assert np.array_equal(coef, coef_h) and it == it_h
    assert same(d_img.get(), np.ascontiguousarray(ramp, dtype=dtype))          # the image is not modified
    # gaussian_deconvolve: this plan's shape is the padded one (m + 4 dr)
    dr, sigma = 4, 3.0
    m = (shape[0] - 4 * dr, shape[1] - 4 * dr)
    field = img[:m[0], :m[1]] * 0.5
    ref = _lib.Plan(shape, 1, dtype).gaussian_deconvolve(field, dr, sigma, 5000)
    d_f = Slot(npx, m, dtype, lead=1, host=field)
    d_g = Slot(npx, m, dtype, lead=2)
    plan.gaussian_deconvolve_dev(d_f.ptr, dr, sigma, 5000, d_g.ptr)
    plan.sync()
    assert same(d_g.get(), ref)
    assert same(d_f.get(), np.ascontiguousarray(field, dtype=dtype))
    plan.gaussian_deconvolve_dev(d_f.ptr, dr, sigma, 5000, d_f.ptr)             # out_ptr == data_ptr (docstring)
    plan.sync()
    assert same(d_f.get(), ref)
    for s in (d_img, d_out, d_f, d_g):
        s.free()
    plan.close()


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shape', SHAPES)
def test_dev_sweep_weights_jacobian_props(shape, dtype):
    """sweep_grad_dev (grad_mode 0 / 1 / 2, with and without kidx) vs sweep(want_grad=True); lockin_weights_dev vs np.abs
    of the lock-ins; phasegradient2J_dev (with and without dks) vs phasegradient2J; props_from_jac_dev vs props_from_jac"""
    img, kvecs, klists = _case(shape)
    P, npx = len(kvecs), img.size
    cdt = np.complex128 if dtype is np.float64 else np.complex64
    sigma = 6
    plan = _lib.Plan(shape, klists.shape[1] * P, dtype)
    d_img = Slot(npx, shape, dtype, lead=1, host=img)
    d_lock = Slot(npx, (P,) + shape, cdt, lead=2)
    d_grad = Slot(npx, (P,) + shape + (2,), dtype, lead=2)
    d_kidx = Slot(npx, shape, np.int32, lead=4)
    d_w = Slot(npx, (P,) + shape, dtype, lead=1)
    d_J = Slot(npx, shape + (2, 2), dtype, lead=3)
    d_props = Slot(npx, (4,) + shape, dtype, lead=1)
    item = np.dtype(dtype).itemsize
    for mode in (0, 1, 2):
        for with_kidx in (True, False):
            for p in range(P):
                plan.sweep_grad_dev(d_img.ptr, kvecs[p], klists[p], sigma, d_lock.ptr + p * 2 * npx * item,
                                    d_grad.ptr + p * 2 * npx * item, kidx_ptr=d_kidx.ptr if with_kidx else None, grad_mode=mode)
                plan.sync()
                lock, kidx, grad = _lib.Plan(shape, P * klists.shape[1], dtype).sweep(img, kvecs[p], klists[p], sigma,
                                                                                   want_grad=True, grad_mode=mode)
                assert same(d_lock.get()[p], lock) and same(d_grad.get()[p], grad), (mode, with_kidx, p)
                if with_kidx:
                    assert np.array_equal(d_kidx.get(), kidx), (mode, p)
    # the lock-ins of grad_mode 0 (the bench's) feed the rest
    for p in range(P):
        plan.sweep_grad_dev(d_img.ptr, kvecs[p], klists[p], sigma, d_lock.ptr + p * 2 * npx * item, d_grad.ptr + p * 2 * npx * item)
    plan.sync()
    lock, grads = d_lock.get(), d_grad.get()
    plan.lockin_weights_dev(d_lock.ptr, P, d_w.ptr)
    plan.sync()
    w = d_w.get()
    # the kernel takes hypot() of the device's math library, NumPy that of the host's C library; each is within one ulp of
    # |z|, so the two are at most two ulps apart (measured on MI355X: two ulps occur, in both precisions)
    ref_w = np.abs(lock)
    assert w.dtype == ref_w.dtype
    ulps = np.abs(w.view(np.int64 if dtype is np.float64 else np.int32).astype(np.int64)
                  - ref_w.view(np.int64 if dtype is np.float64 else np.int32).astype(np.int64))
    assert ulps.max() <= 2
    print('lockin_weights_dev %s: %.4f of the weights differ from np.abs (at most %d ulps)' % (np.dtype(dtype).name, (ulps > 0).mean(), ulps.max()))
    dks = np.array([[0.001, -0.002], [0.0005, 0.001], [-0.001, 0.0]])
    for d in (None, dks):
        plan.phasegradient2J_dev(kvecs, d_grad.ptr, d_w.ptr, 0.7, d_J.ptr, dks=d)
        plan.sync()
        J = _lib.Plan(shape, P * klists.shape[1], dtype).phasegradient2J(kvecs, grads, w, 0.7, dks=d)
        assert same(d_J.get(), J)
    Jh = d_J.get()
    for kw in (dict(add_identity=True), dict(add_identity=True, refangle=12.5, refscale=0.3),
               dict(add_identity=True, diff=True), dict(refangle=-3.0, refscale=2.0, diff=True)):
        plan.props_from_jac_dev(d_J.ptr, d_props.ptr, **kw)
        plan.sync()
        assert same(d_props.get(), _lib.props_from_jac(Jh, dtype=dtype, **kw)), kw
    for s in (d_img, d_lock, d_grad, d_kidx, d_w, d_J, d_props):
        s.free()
    plan.close()


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shape', SHAPES)
def test_dev_unwrap_and_extraction(shape, dtype):
    """unwrap_prediff_dev and unwrap_prediff_enqueue_dev + unwrap_finish vs unwrap_prediff (phi and iteration counts);
    extract_displacement_field_dev vs extract_displacement_field (u, lock-ins, kidx, iterations)"""
    img, kvecs, klists = _case(shape)
    P, K, npx = len(kvecs), klists.shape[1], img.size
    sigma = 6
    host = _lib.Plan(shape, P * K, dtype)
    dudx, dudy, wnorm = host.extract_gradients(img, kvecs, klists, sigma, 2 * sigma)
    plan = _lib.Plan(shape, P * K, dtype)
    d_dx = Slot(npx, dudx.shape[1:], dtype, lead=1, host=dudx[0])
    d_dy = Slot(npx, dudy.shape[1:], dtype, lead=2, host=dudy[0])
    d_wt = Slot(npx, shape, dtype, lead=1, host=wnorm)
    d_phi = Slot(npx, shape, dtype, lead=3)
    for weight, kmax in ((wnorm, 10), (None, 3)):
        phi_h, it_h = _lib.Plan(shape, 1, dtype).unwrap_prediff(dudx[0], dudy[0], weight, kmax=kmax)
        wptr = None if weight is None else d_wt.ptr
        it = plan.unwrap_prediff_dev(d_dx.ptr, d_dy.ptr, wptr, d_phi.ptr, kmax=kmax)
        assert same(d_phi.get(), phi_h) and it == it_h
        d_phi.set(np.zeros(shape))
        plan.unwrap_prediff_enqueue_dev(d_dx.ptr, d_dy.ptr, wptr, d_phi.ptr, kmax=kmax)
        assert plan.unwrap_finish() == it_h
        assert same(d_phi.get(), phi_h)
    cdt = np.complex128 if dtype is np.float64 else np.complex64
    d_img = Slot(npx, shape, dtype, lead=2, host=img)
    d_u = Slot(npx, (2,) + shape, dtype, lead=1)
    d_lock = Slot(npx, (P,) + shape, cdt, lead=2)
    d_kidx = Slot(npx, (P,) + shape, np.int32, lead=1)
    u, lock, kidx, iters = _lib.Plan(shape, P * K, dtype).extract_displacement_field(img, kvecs, klists, sigma, 2 * sigma,
                                                                                     want_lockins=True, want_kidx=True)
    it = plan.extract_displacement_field_dev(d_img.ptr, kvecs, klists, sigma, 2 * sigma, 10, d_u.ptr, d_lock.ptr, d_kidx.ptr)
    assert same(d_u.get(), u) and same(d_lock.get(), lock) and np.array_equal(d_kidx.get(), kidx) and it == iters
    u2, _, _, it2 = _lib.Plan(shape, P * K, dtype).extract_displacement_field(img, kvecs, klists, sigma, 2 * sigma)
    assert same(u2, u) and it2 == iters
    for s in (d_dx, d_dy, d_wt, d_phi, d_img, d_u, d_lock, d_kidx):
        s.free()
    plan.close()
    host.close()


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shape', SHAPES)
def test_dev_lawler_fujita(shape, dtype):
    """invert_u_dev (scale -1) vs invert_u_overlap of the negated field; undistort_image_dev with uinv_ptr and scale -1
    vs undistort_image(img, -u) and invert_u_overlap(u)"""
    img, kvecs, klists = _case(shape)
    npx = img.size
    u = _lib.Plan(shape, klists.size // 2, dtype).extract_displacement_field(img, kvecs, klists, 6, 12)[0]
    plan = _lib.Plan(shape, 1, dtype)
    d_img = Slot(npx, shape, dtype, lead=1, host=img)
    d_u = Slot(npx, (2,) + shape, dtype, lead=2, host=u)
    d_rec = Slot(npx, shape, dtype, lead=1)
    d_uinv = Slot(npx, (2,) + shape, dtype, lead=3)
    plan.invert_u_dev(d_u.ptr, d_uinv.ptr, scale=-1.0)
    plan.sync()
    assert same(d_uinv.get(), _lib.Plan(shape, 1, dtype).invert_u_overlap(-u))
    d_uinv.set(np.zeros((2,) + shape))
    plan.undistort_image_dev(d_img.ptr, d_u.ptr, d_rec.ptr, uinv_ptr=d_uinv.ptr, scale=-1.0)
    plan.sync()
    assert same(d_rec.get(), _lib.Plan(shape, 1, dtype).undistort_image(img, -u))
    assert same(d_uinv.get(), _lib.Plan(shape, 1, dtype).invert_u_overlap(u))
    for s in (d_img, d_u, d_rec, d_uinv):
        s.free()
    plan.close()


# ---- the bench's resident pipeline (bench.py pipeline_end_to_end), replayed -------------------------------------------
def _pipeline(n, dtype, img, knx=4, kny=4, kmax=10):
    """bench.py pipeline_end_to_end's stages in its order, on one plan with P * K = 48 and caller-owned buffers at plane
    offsets (copied, not imported: bench.py is the yardstick and does not change for a test).  Returns every product."""
    import pygpa_amd.geometric_phase_analysis as GPA
    P, K = 3, knx * kny
    s = np.dtype(dtype).itemsize
    npx = n * n
    plan = _lib.Plan((n, n), P * K, dtype, device=0)
    bufs = {k: _lib.DeviceBuffer(v * npx * s) for k, v in dict(img=1, u=2, rec=1, uinv=2, lock=2 * P, grad=2 * P, w=P, J=4, props=4).items()}
    bufs['img'].upload(img)
    ks, _ = GPA.extract_primary_ks_dev(plan, bufs['img'].ptr, pix_norm_range=(2, 0.2 * n))
    sigma = int(np.ceil(1 / np.linalg.norm(ks, axis=1).min()))
    kw = np.linalg.norm(ks, axis=1).mean() / 2.5
    klists = np.stack(explicit_klists(ks, kw, knx, kny))
    iters = plan.extract_displacement_field_dev(bufs['img'].ptr, ks, klists, sigma, 2 * sigma, kmax, bufs['u'].ptr)
    plan.undistort_image_dev(bufs['img'].ptr, bufs['u'].ptr, bufs['rec'].ptr, uinv_ptr=bufs['uinv'].ptr, scale=-1.0)
    for p_ in range(P):
        plan.sweep_grad_dev(bufs['img'].ptr, ks[p_], klists[p_], sigma, bufs['lock'].ptr + p_ * 2 * npx * s,
                            bufs['grad'].ptr + p_ * 2 * npx * s)
    plan.lockin_weights_dev(bufs['lock'].ptr, P, bufs['w'].ptr)
    plan.phasegradient2J_dev(ks, bufs['grad'].ptr, bufs['w'].ptr, 1.0, bufs['J'].ptr)
    plan.props_from_jac_dev(bufs['J'].ptr, bufs['props'].ptr, add_identity=True)
    plan.sync()
    cdt = np.complex128 if dtype is np.float64 else np.complex64
    out = dict(ks=ks, klists=klists, sigma=sigma, iters=iters,
               u=bufs['u'].download((2, n, n), dtype), rec=bufs['rec'].download((n, n), dtype),
               uinv=bufs['uinv'].download((2, n, n), dtype), lock=bufs['lock'].download((P, n, n), cdt),
               grad=bufs['grad'].download((P, n, n, 2), dtype), w=bufs['w'].download((P, n, n), dtype),
               J=bufs['J'].download((n, n, 2, 2), dtype), props=bufs['props'].download((4, n, n), dtype))
    for b in bufs.values():
        b.free()
    plan.close()
    return out


def _bench_image(n, dtype):
    img = hex_moire((n, n), hex_kvecs(0.1, 7.0), gaussian_bump_displacement((n, n)), noise=0.1, seed=100, dtype=np.float64)
    return (img - img.mean()).astype(dtype)


_ORACLE = {}


def _oracle_chain(img64, ks, klists, sigma):
    """the oracle's u, and per peak its sweep with gradients and a mask of the pixels whose two best candidates' amplitudes
    tie to 4e-6 of the largest (an f32 winner may flip there: tests/tolerances.py F32 tie_rel)"""
    key = (img64.tobytes(), ks.tobytes(), sigma)
    if key not in _ORACLE:
        _ORACLE.clear()
        u = orc.extract_displacement_field(img64, ks, sigma=sigma, klists=list(klists), workers=8)
        img0 = img64 - img64.mean()
        sweeps, ties = [], []
        for p in range(len(ks)):
            sweeps.append(orc.sweep(img0, sigma, klists[p], ks[p], want_grad=True, workers=8))
            amps = np.sort(np.abs(orc.lockin_batch(img0, klists[p], sigma, workers=8)), axis=0)
            ties.append(amps[-1] - amps[-2] <= TOLS.F32['tie_rel'] * amps[-1].max())
        _ORACLE[key] = (u, sweeps, ties)
    return _ORACLE[key]


def _pdiff(a, b, period):
    return (a - b + period / 2) % period - period / 2


@pytest.mark.parametrize('dtype', DTYPES)
def test_bench_pipeline_vs_oracle(dtype):
    """every product of the resident pipeline at 512^2 against the oracle chain: k-vectors within 1.5 / n of the
    generator's, u at tests/tolerances.py's F64 / F32, the undistorted image and u_inv at LF_4096's bounds against
    orc.undistort_image(img, -u) / orc.invert_u_overlap(u) of the device's u, per-peak gradients against the oracle
    sweep (wfr2_grad_opt on the explicit list), J and props against orc.phasegradient2J + orc.props_from_jac of the
    device's own gradients / weights / J with test_f2_*'s tolerances"""
    n = 512
    img = _bench_image(n, np.float32)            # one image for both precisions: the oracle runs once
    img64 = img.astype(np.float64)
    r = _pipeline(n, dtype, img.astype(dtype))
    ks, klists, sigma = r['ks'], r['klists'], r['sigma']
    for k in hex_kvecs(0.1, 7.0):
        d = np.minimum(np.linalg.norm(ks - k, axis=1), np.linalg.norm(ks + k, axis=1))
        assert d.min() < 1.5 / n
    u_ref, sw, ties = _oracle_chain(img64, ks, klists, sigma)
    du = (r['u'] - r['u'].mean(axis=(1, 2), keepdims=True)) - (u_ref - u_ref.mean(axis=(1, 2), keepdims=True))
    if dtype is np.float64:
        assert np.abs(du).max() < TOLS.F64['max_px']
    else:
        assert np.abs(du).max() < TOLS.F32['max_px'] and np.sqrt((du ** 2).mean()) < TOLS.F32['rms_px']
    # Lawler-Fujita of the device's own field (the resampling is what is compared, not the field)
    u_dev = r['u'].astype(np.float64)
    lf = TOLS.LF_4096[np.dtype(dtype).name]
    uinv_ref = orc.invert_u_overlap(u_dev)
    assert np.array_equal(np.isnan(r['uinv']), np.isnan(uinv_ref))
    ok = ~np.isnan(uinv_ref)
    assert np.abs(r['uinv'][ok] - uinv_ref[ok]).max() < lf['u_inv_px']
    rec_ref = orc.undistort_image(img64, -u_dev)
    # mode='constant' is discontinuous where r + u_inv leaves [0, n - 1]: in f32 compare away from that border (as
    # test_gpu_pins.py's 4096^2 check does)
    xx, yy = np.mgrid[:n, :n]
    cx, cy = xx + uinv_ref[0], yy + uinv_ref[1]
    margin = 0.0 if dtype is np.float64 else 2e-3
    ok = (cx >= margin) & (cx <= n - 1 - margin) & (cy >= margin) & (cy <= n - 1 - margin)
    ok |= (cx < -margin) | (cx > n - 1 + margin) | (cy < -margin) | (cy > n - 1 + margin)
    assert ok.mean() > 0.99
    assert np.abs(r['rec'] - rec_ref)[ok].max() < lf['rec_rel'] * np.abs(rec_ref).max()
    # per-peak lock-ins and gradients against the oracle sweep, away from amplitude ties; the phase error of a lock-in
    # grows as its amplitude falls: |d grad| <= 2 (two phases) x 4 x lock-in tolerance x max|lockin| / |lockin|
    for p in range(3):
        ref = sw[p]
        amp = np.abs(ref['lockin'])
        amax = amp.max()
        keep = ~ties[p] if dtype is np.float32 else np.ones(amp.shape, bool)
        assert keep.mean() > 0.999
        d = np.abs(_pdiff(r['grad'][p].astype(np.float64), ref['grad'], np.pi))
        ok = keep & (amp > 1e-3 * amax)
        assert np.all(d[ok] <= 8 * TOL[dtype]['lock'] * amax / amp[ok][:, None]), p
        assert np.abs(r['lock'][p] - ref['lockin'])[keep].max() < TOL[dtype]['lock'] * amax, p
        assert np.abs(r['w'][p].astype(np.float64) - np.abs(r['lock'][p])).max() <= 2 * np.finfo(dtype).eps * amax
    # J and props of the device's own inputs
    f32 = dtype is np.float32
    J_ref = orc.phasegradient2J(ks, r['grad'], r['w'], 1.0, iso_ref=False)
    assert np.abs(r['J'] - J_ref).max() <= (2e-5 if f32 else 1e-11) * np.abs(J_ref).max()
    props_ref = orc.props_from_jac(np.eye(2) + r['J'].astype(np.float64))
    props = r['props']
    kap = props_ref[3]
    tol_ani = (2e-5 if f32 else 1e-11) * (1 + 1 / (kap - 1)) * 57.3
    assert np.all(np.abs(_pdiff(props[0], props_ref[0], 360)) <= (1e-4 if f32 else 1e-10))
    assert np.all(np.abs(_pdiff(props[1], props_ref[1], 180)) <= tol_ani)
    assert np.allclose(props[2], props_ref[2], rtol=1e-5 if f32 else 1e-12,
                       atol=(2e-6 if f32 else 1e-13) * np.abs(props_ref[2] * kap).max())
    assert np.allclose(props[3], props_ref[3], rtol=(2e-5 if f32 else 1e-11) * kap.max())


def test_bench_pipeline_headline_size_vs_fresh_plans():
    """the resident pipeline at the headline's size (4096^2, f32): every stage equals the host entry point on a fresh
    plan fed the same inputs, bit for bit (the oracle is too slow at this size)"""
    import pygpa_amd.geometric_phase_analysis as GPA
    n, dtype = 4096, np.float32
    img = _bench_image(n, dtype)
    r = _pipeline(n, dtype, img)
    ks, klists, sigma = r['ks'], r['klists'], r['sigma']
    P, K = klists.shape[:2]
    fresh = _lib.Plan((n, n), 1, dtype)
    ks_h, _ = GPA._primary_ks(GPA._reusing(fresh, lambda s, d, t: fresh.find_peaks(img, s, d, t)), (n, n), False, 0.7,
                              (2, 0.2 * n), 1, True)
    fresh.close()
    assert np.array_equal(ks, ks_h)
    plan = _lib.Plan((n, n), P * K, dtype)
    u, _, _, iters = plan.extract_displacement_field(img, ks, klists, sigma, 2 * sigma, kmax=10)
    plan.close()
    assert np.array_equal(r['u'], u) and tuple(r['iters']) == tuple(iters)
    plan = _lib.Plan((n, n), 1, dtype)
    assert np.array_equal(r['rec'], plan.undistort_image(img, -u), equal_nan=True)
    assert np.array_equal(r['uinv'], plan.invert_u_overlap(u), equal_nan=True)
    plan.close()
    for p in range(P):
        plan = _lib.Plan((n, n), K, dtype)
        lock, _, grad = plan.sweep(img, ks[p], klists[p], sigma, want_grad=True)
        plan.close()
        assert np.array_equal(r['lock'][p], lock) and np.array_equal(r['grad'][p], grad), p
        del lock, grad
    plan = _lib.Plan((n, n), P, dtype)
    assert np.array_equal(r['J'], plan.phasegradient2J(ks, r['grad'], r['w'], 1.0))
    plan.close()
    assert np.array_equal(r['props'], _lib.props_from_jac(r['J'], add_identity=True, dtype=dtype))
