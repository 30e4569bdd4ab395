"""A plan's history must not change a result.  Run with `-m gpu` on an MI355X.

One long-lived `_lib.Plan` carries caches from call to call: the sigma of its filter tables and the compact axes
(ensure_filters), the staged k-lists and carrier tables (stage_kvectors), the shared pass-B tables keyed by sh_epoch
(shared_prepare), the 2 pi k matrix (stage_kmat), two slots of Gaussian-FFT tables (gauss_tables), the smoothed spectrum of
the last find_peaks, the batched-unwrap capacity -- and its entry points borrow each other's buffers as scratch.  The
state machine below drives one such plan through a drawn sequence of entry points whose parameters come from small pools
(so that every cache both hits and misses) and compares every result with the same call on a FRESH plan of the same
shape, dtype and max_batch, bit for bit.  Asynchronous calls (extract_displacement_field_async,
unwrap_prediff_enqueue_dev) are left in flight while later rules re-stage tables; `sync` and the teardown check them.

Pinned history dependence (by design, not tolerated): last_iters() / unwrap_finish() report the LATEST driver call / solve
of the plan, so the iteration counts of a pending call are only compared when nothing of its kind ran after it."""
import numpy as np
import pytest
from hypothesis import HealthCheck, settings
from hypothesis import strategies as st
from hypothesis.stateful import RuleBasedStateMachine, initialize, invariant, precondition, rule

from pygpa_amd import _lib
from pygpa_amd.synthetic import hex_kvecs, explicit_klists, gaussian_bump_displacement, hex_moire

pytestmark = pytest.mark.gpu

SIGMAS = (4.0, 6.0, 9.0)
BORDERS = (1, 3, 10)
KMAXES = (1, 3, 10)
MAX_BATCH = 18          # P x K of the largest k-list of the pool (3 x 6)


def _pools():
    """k-vector / k-list pool: (kvecs (P, 2), klists (P, K, 2)) pairs"""
    kv = hex_kvecs(0.12, 11.0)
    kw = np.linalg.norm(kv, axis=1).mean() / 2.5
    l22 = np.stack(explicit_klists(kv, kw, 2, 2))                 # 3 x 4
    l32 = np.stack(explicit_klists(kv, kw, 3, 2))                 # 3 x 6
    kv2 = hex_kvecs(0.115, 13.0)
    l22b = np.stack(explicit_klists(kv2, kw, 2, 2))
    return [
        (kv, l22),
        (kv, l32),
        (kv + 0.002, l22),                                          # the same lists with other reference vectors
        (kv[:2], l22.reshape(2, 6, 2)),                             # the same concatenated list split as 2 x 6
        (kv2, l22b),
        (kv[:2] * 1.01, l32[:2]),                                   # the same P, other k-vectors (d_kmat must change)
    ]


POOL = _pools()


def same(a, b):
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if a is None or b is None:
        return a is None and b is None
    if isinstance(a, np.ndarray):
        return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)
    return a == b


class PlanHistory(RuleBasedStateMachine):
    SHAPE = (96, 80)
    DTYPE = np.float64

    @initialize()
    def setup(self):
        n0, n1 = self.SHAPE
        dt = self.DTYPE
        self.plan = _lib.Plan(self.SHAPE, MAX_BATCH, dt)
        self.item = np.dtype(dt).itemsize
        self.npx = n0 * n1
        kv = POOL[0][0]
        self.imgs = [hex_moire(self.SHAPE, kv, gaussian_bump_displacement(self.SHAPE), noise=0.1, seed=s) for s in (1, 2, 3)]
        self.imgs = [(im - im.mean()).astype(dt) for im in self.imgs]
        self.d_imgs = _lib.DeviceBuffer(3 * self.npx * self.item)
        self.d_imgs.upload(np.stack(self.imgs))
        rng = np.random.default_rng(7)
        self.grads = rng.uniform(-0.3, 0.3, (3, n0, n1, 2)).astype(dt)
        self.weights = rng.uniform(0.1, 1.0, (3, n0, n1)).astype(dt)
        self.lockins = (self.weights * np.exp(1j * rng.uniform(-3, 3, (3, n0, n1)))).astype(np.complex128 if dt is np.float64 else np.complex64)
        self.dx = rng.uniform(-1, 1, (n0, n1 - 1)).astype(dt)
        self.dy = rng.uniform(-1, 1, (n0 - 1, n1)).astype(dt)
        x, y = np.meshgrid(np.arange(n0) - n0 / 2, np.arange(n1) - n1 / 2, indexing='ij')
        self.u = np.stack([1.5 * np.exp(-(x ** 2 + y ** 2) / (0.1 * n0 * n1)), 0.8 * np.sin(y / 9.0)]).astype(dt)
        self.d_unwrap_in = _lib.DeviceBuffer(3 * self.npx * self.item)
        self.d_unwrap_in.upload(np.concatenate([self.dx.ravel(), np.zeros(n0), self.dy.ravel(), np.zeros(n1),
                                                self.weights[0].ravel()]).astype(dt))
        self.pending = []          # (kind, device buffer, shape, expected, expected iterations)
        self.prev = 0
        self.peaks = None          # (sigma, dog) of the long-lived plan's last find_peaks
        self.since_unwrap = None   # the pending unwrap that is the plan's latest solve
        self.since_extract = None  # the pending extraction that is the plan's latest driver call

    def fresh(self):
        return _lib.Plan(self.SHAPE, MAX_BATCH, self.DTYPE)

    def both(self, fn):
        """fn(plan) on the long-lived plan and on a fresh one: equal bit for bit"""
        got = fn(self.plan)
        f = self.fresh()
        try:
            want = fn(f)
        finally:
            f.close()
        assert same(got, want), 'result depends on the plan history'
        return got

    def pick(self, k):
        if k < 0:
            return POOL[self.prev]
        self.prev = k
        return POOL[k]

    # ---- rules --------------------------------------------------------------------------------------------------------
    lists = st.sampled_from([-1] + list(range(len(POOL))))     # -1: the previous list again
    sigmas = st.sampled_from(SIGMAS)

    def _ran(self, kind):
        if kind == 'unwrap':
            self.since_unwrap = None
        self.since_extract = None if kind == 'extract' else self.since_extract

    @rule(k=lists, sigma=sigmas, img=st.integers(0, 2))
    def lockin_batch(self, k, sigma, img):
        kv, _ = self.pick(k)
        self.both(lambda p: p.lockin_batch(self.imgs[img], kv, sigma))

    @rule(k=lists, sigma=sigmas, peak=st.integers(0, 1), mode=st.sampled_from([None, 0, 1, 2]), want_kidx=st.booleans())
    def sweep(self, k, sigma, peak, mode, want_kidx):
        kv, kl = self.pick(k)
        self.both(lambda p: p.sweep(self.imgs[0], kv[peak], kl[peak], sigma, want_kidx=want_kidx, want_grad=mode is not None,
                                    grad_mode=mode or 0))

    @rule(k=lists, sigma=sigmas)
    def sweep_gated(self, k, sigma):
        kv, kl = self.pick(k)
        gate = np.linalg.norm(kl[0][:, None] - kl[0][None], axis=-1) < 0.03
        self.both(lambda p: p.sweep_gated(self.imgs[1], kv[0], kl[0], sigma, gate))

    @rule(k=lists, sigma=sigmas, border=st.sampled_from(BORDERS))
    def extract_gradients(self, k, sigma, border):
        kv, kl = self.pick(k)
        self.both(lambda p: p.extract_gradients(self.imgs[0], kv, kl, sigma, border))

    @rule(k=lists, sigma=sigmas, border=st.sampled_from(BORDERS), kmax=st.sampled_from(KMAXES), img=st.integers(0, 2),
          extras=st.booleans())
    def extract_host(self, k, sigma, border, kmax, img, extras):
        kv, kl = self.pick(k)
        self.both(lambda p: p.extract_displacement_field(self.imgs[img], kv, kl, sigma, border, kmax=kmax,
                                                         want_lockins=extras, want_kidx=extras))
        self._ran('extract')
        self._ran('unwrap')

    @rule(k=lists, sigma=sigmas, border=st.sampled_from(BORDERS), kmax=st.sampled_from(KMAXES), img=st.integers(0, 2))
    def extract_dev(self, k, sigma, border, kmax, img):
        kv, kl = self.pick(k)
        ptr = self.d_imgs.ptr + img * self.npx * self.item

        def call(p):
            out = _lib.DeviceBuffer(2 * self.npx * self.item)
            try:
                it = p.extract_displacement_field_dev(ptr, kv, kl, sigma, border, kmax, out.ptr)
                return out.download((2,) + self.SHAPE, self.DTYPE), it
            finally:
                out.free()
        self.both(call)
        self._ran('extract')
        self._ran('unwrap')

    @precondition(lambda self: len(self.pending) < 3)
    @rule(k=lists, sigma=sigmas, border=st.sampled_from(BORDERS), kmax=st.sampled_from(KMAXES), img=st.integers(0, 2))
    def extract_async(self, k, sigma, border, kmax, img):
        """enqueued and left in flight; the expected field comes from a fresh plan now"""
        kv, kl = self.pick(k)
        ptr = self.d_imgs.ptr + img * self.npx * self.item
        # (the same device-pointer form on the fresh plan: the host form with want_lockins takes another pass B on the
        #  shared-forward shapes, equal only to rounding)
        f = self.fresh()
        ref = _lib.DeviceBuffer(2 * self.npx * self.item)
        try:
            want_it = f.extract_displacement_field_dev(ptr, kv, kl, sigma, border, kmax, ref.ptr)
            want = ref.download((2,) + self.SHAPE, self.DTYPE)
        finally:
            ref.free()
            f.close()
        out = _lib.DeviceBuffer(2 * self.npx * self.item)
        self.plan.extract_displacement_field_async(ptr, kv, kl, sigma, border, kmax, out.ptr)
        entry = ['extract', out, (2,) + self.SHAPE, want, want_it]
        self.pending.append(entry)
        self._ran('unwrap')
        self.since_extract = entry

    @precondition(lambda self: self.plan.lib.gpa_supports_batch(self.plan.handle) != 0)
    @rule(k=lists, sigma=sigmas, nimg=st.integers(1, 3), kmax=st.sampled_from(KMAXES))
    def extract_batch_dev(self, k, sigma, nimg, kmax):
        kv, kl = self.pick(k)

        def call(p):
            out = _lib.DeviceBuffer(2 * nimg * self.npx * self.item)
            try:
                it = p.extract_displacement_field_batch_dev(self.d_imgs.ptr, nimg, kv, kl, sigma, 2 * int(sigma), kmax, out.ptr)
                return out.download((nimg, 2) + self.SHAPE, self.DTYPE), it
            finally:
                out.free()
        self.both(call)
        self._ran('extract')
        self._ran('unwrap')

    @rule(k=lists, border=st.sampled_from(BORDERS))
    def reconstruct_grad(self, k, border):
        kv, _ = self.pick(k)
        P = len(kv)
        self.both(lambda p: p.reconstruct_grad(self.lockins[:P], kv, border))

    @rule(k=lists)
    def reconstruct_prediff(self, k):
        kv, _ = self.pick(k)
        P = len(kv)
        self.both(lambda p: p.reconstruct_prediff(self.grads[:P], self.weights[:P], kv))

    @rule(k=lists)
    def weighted_lstsq(self, k):
        kv, _ = self.pick(k)
        P = len(kv)
        self.both(lambda p: p.weighted_lstsq(self.grads[:P, ..., 0], self.weights[:P], kv))

    @rule(kmax=st.sampled_from(KMAXES), weighted=st.booleans(), wrapped=st.booleans())
    def unwrap(self, kmax, weighted, wrapped):
        w = self.weights[1] if weighted else None
        if wrapped:
            self.both(lambda p: p.unwrap(self.grads[0, ..., 0] * 10, w, kmax=kmax))
        else:
            self.both(lambda p: p.unwrap_prediff(self.dx, self.dy, w, kmax=kmax))
        self._ran('unwrap')

    @precondition(lambda self: len(self.pending) < 3)
    @rule(kmax=st.sampled_from(KMAXES), weighted=st.booleans())
    def unwrap_enqueue(self, kmax, weighted):
        """the solve left in flight on the plan's stream"""
        n0, n1 = self.SHAPE
        f = self.fresh()
        want = f.unwrap_prediff(self.dx, self.dy, self.weights[0] if weighted else None, kmax=kmax)
        f.close()
        base = self.d_unwrap_in.ptr
        out = _lib.DeviceBuffer(self.npx * self.item)
        self.plan.unwrap_prediff_enqueue_dev(base, base + self.npx * self.item, base + 2 * self.npx * self.item if weighted else None,
                                             out.ptr, kmax=kmax)
        entry = ['unwrap', out, self.SHAPE, want[0], want[1]]
        self.pending.append(entry)
        self.since_unwrap = entry

    @rule(img=st.integers(0, 2), inverse=st.booleans())
    def per(self, img, inverse):
        if inverse:
            self.both(lambda p: p.per(self.imgs[img], inverse_dft=True))
        else:
            self.both(lambda p: p.per_dft(self.imgs[img]))

    @rule(sigma=st.sampled_from([1.0, 2.5]), dog=st.sampled_from([0.0, 20.0]), thr=st.sampled_from([0.05, 0.3]),
          img=st.integers(0, 2), dev=st.booleans())
    def find_peaks(self, sigma, dog, thr, img, dev):
        if dev:
            ptr = self.d_imgs.ptr + img * self.npx * self.item
            self.both(lambda p: p.find_peaks_dev(ptr, sigma, dog, thr))
        else:
            self.both(lambda p: p.find_peaks(self.imgs[img], sigma, dog, thr, want_smooth=True))
        self.peaks = (img, sigma, dog)

    @precondition(lambda self: self.peaks is not None)
    @rule(thr=st.sampled_from([0.01, 0.1, 0.5]))
    def find_peaks_again(self, thr):
        img, sigma, dog = self.peaks
        got = self.plan.find_peaks_again(thr)
        f = self.fresh()
        f.find_peaks(self.imgs[img], sigma, dog, 0.9)
        want = f.find_peaks_again(thr)
        f.close()
        assert same(got, want)

    @rule(img=st.integers(0, 2))
    def fit_plane(self, img):
        ramp = self.imgs[img] + np.arange(self.SHAPE[0])[:, None] * 0.01
        self.both(lambda p: p.fit_plane(ramp))

    @rule(k=lists, with_dks=st.booleans())
    def phasegradient2J(self, k, with_dks):
        kv, _ = self.pick(k)
        P = len(kv)
        dks = np.full((P, 2), 0.001) * np.arange(1, P + 1)[:, None] if with_dks else None
        self.both(lambda p: p.phasegradient2J(kv, self.grads[:P], self.weights[:P], 0.5, dks=dks))

    @rule(scale=st.sampled_from([1.0, -1.0]), undistort=st.booleans())
    def lawler_fujita(self, scale, undistort):
        if undistort:
            self.both(lambda p: p.undistort_image(self.imgs[0], scale * self.u))
        else:
            self.both(lambda p: p.invert_u_overlap(scale * self.u))

    @rule(sigma=sigmas)
    def gaussian_deconvolve(self, sigma):
        dr = 4                      # this plan's shape is then the padded one of an (n0 - 16) x (n1 - 16) field
        n0, n1 = self.SHAPE
        field = self.imgs[2][:n0 - 4 * dr, :n1 - 4 * dr]
        self.both(lambda p: p.gaussian_deconvolve(field, dr, sigma, 5000))

    @rule()
    def sync(self):
        self.plan.sync()
        pending, self.pending = self.pending, []
        got = []
        for kind, buf, shape, want, want_it in pending:
            got.append(buf.download(shape, self.DTYPE))
            buf.free()
        last_unwrap, last_extract = self.since_unwrap, self.since_extract
        self.since_unwrap = self.since_extract = None
        for (kind, _, _, want, _), g in zip(pending, got):
            assert same(g, want), 'the %s left in flight does not equal a fresh plan\'s' % kind
        if last_unwrap is not None:
            assert self.plan.unwrap_finish() == last_unwrap[4]
        if last_extract is not None:
            assert tuple(self.plan.last_iters()) == tuple(last_extract[4])

    @invariant()
    def few_pending(self):
        assert len(getattr(self, 'pending', [])) <= 3

    def teardown(self):
        if getattr(self, 'plan', None) is None:
            return
        try:
            self.sync()
        finally:
            self.plan.close()
            self.d_imgs.free()
            self.d_unwrap_in.free()


STATE_SETTINGS = settings(max_examples=6, stateful_step_count=12, deadline=None, derandomize=True,
                          suppress_health_check=[HealthCheck.too_slow, HealthCheck.data_too_large,
                                                 HealthCheck.filter_too_much])


def _machine(shape, dtype):
    name = 'PlanHistory_%dx%d_%s' % (shape[0], shape[1], np.dtype(dtype).name)
    m = type(name, (PlanHistory,), dict(SHAPE=shape, DTYPE=dtype))
    case = m.TestCase
    case.settings = STATE_SETTINGS
    return pytest.mark.gpu(case)


# rows of 2048 points: the shared-forward pass B engages (sh_epoch, sh_built_*); a small power-of-two shape; a mixed-radix
# shape whose padded axes change their compact length with sigma
TestPlanHistory64x2048F32 = _machine((64, 2048), np.float32)
TestPlanHistory64x2048F64 = _machine((64, 2048), np.float64)
TestPlanHistory64F64 = _machine((64, 64), np.float64)
TestPlanHistory96x80F64 = _machine((96, 80), np.float64)
TestPlanHistory96x80F32 = _machine((96, 80), np.float32)


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_mirror_calls_do_not_depend_on_the_cached_plans(dtype):
    """the user-facing consequence: a fixed interleaving of mirror calls on one image size (they share
    _lib.get_plan's cached plans) gives what each call gives after _lib._plans.clear()"""
    import pygpa_amd.geometric_phase_analysis as GPA
    import pygpa_amd.phase_unwrap as pu
    from pygpa_amd import mathtools, property_extract
    shape = (192, 160)
    kvecs = hex_kvecs(0.11, 9.0)
    img = hex_moire(shape, kvecs, gaussian_bump_displacement(shape), noise=0.2, seed=12)
    img2 = hex_moire(shape, hex_kvecs(0.13, 2.0), noise=0.5, seed=13)
    psi = np.angle(np.exp(1j * (np.arange(shape[0])[:, None] * 0.21 + np.arange(shape[1])[None, :] * 0.13)))
    calls = [
        ('ks', lambda: GPA.extract_primary_ks(img, dtype=dtype)),
        ('grad0', lambda: GPA.wfr2_grad_opt(img - img.mean(), 8, kvecs[0][0], kvecs[0][1], 0.02, 0.01, dtype=dtype)),
        ('unwrap', lambda: pu.phase_unwrap(psi, kmax=5, dtype=dtype)),
        ('u', lambda: GPA.extract_displacement_field(img, kvecs, dtype=dtype)),
        ('ks2', lambda: GPA.extract_primary_ks(img2, dtype=dtype)),
        ('plane', lambda: mathtools.fit_plane(img + np.arange(shape[0])[:, None] * 0.02, dtype=dtype)),
        ('grad1', lambda: GPA.wfr2_grad_opt(img - img.mean(), 10, kvecs[1][0], kvecs[1][1], 0.03, 0.01, dtype=dtype)),
        ('u_sigma', lambda: GPA.extract_displacement_field(img, kvecs, sigma=12, dtype=dtype)),
        ('props', lambda: property_extract.calc_props_from_phasegradient(
            kvecs, np.stack([GPA.wfr2_grad_opt(img - img.mean(), 8, k[0], k[1], 0.02, 0.01, dtype=dtype)['grad'] for k in kvecs]),
            np.stack([np.abs(GPA.wfr2_grad_opt(img - img.mean(), 8, k[0], k[1], 0.02, 0.01, dtype=dtype)['lockin']) for k in kvecs]),
            1.0, dtype=dtype)),
        ('u_again', lambda: GPA.extract_displacement_field(img, kvecs, dtype=dtype)),
    ]
    _lib._plans.clear()
    interleaved = {name: fn() for name, fn in calls}
    for name, fn in calls:
        _lib._plans.clear()
        alone = fn()
        if isinstance(alone, dict):
            assert all(same(interleaved[name][k], alone[k]) for k in alone), name
        else:
            assert same(interleaved[name], alone), name
    assert same(interleaved['u'], interleaved['u_again'])
    _lib._plans.clear()
