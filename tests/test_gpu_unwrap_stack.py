"""A stack of phase maps unwrapped in one device call (gpa_unwrap_batch[_dev], Plan.unwrap_stack, phase_unwrap_stack): every
map's phi and iteration count equal the single call's bit for bit under the same kernels, from psi and from pre-differenced
gradients, unweighted, with one shared weight and with one weight per map; against the CPU oracle and the golden unwrap;
through chunks and a workspace shared with the batched driver; device-resident; on a shape without a batched unwrap; and the
refusals of bad arguments."""
import ctypes as C

import numpy as np
import pytest

from oracle import gpa_oracle as orc
from pygpa_amd import _lib
from pygpa_amd import phase_unwrap as PU
from pygpa_amd.synthetic import hex_kvecs, gaussian_bump_displacement, hex_moire, explicit_klists

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
# the `pcg` tolerance of tests/test_gpu_parity.py (TOL), relative to max |phi| (rel below, as there)
PCG_TOL = {np.float64: 1e-9, np.float32: 2e-5}
B = 5
GPA_ERR_ARG, GPA_ERR_STATE = -1, -4


def rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def _wrap(x):
    return (x + np.pi) % (2 * np.pi) - np.pi


_STACKS = {}


def make_stack(shape):
    """B = 5 wrapped phase maps and their weights (f64; computed once per shape and never written).  Plane 0 is all zeros:
    r0 == 0, the solve ends at 0 iterations.  Plane 1 a wrapped ramp, planes 2 - 4 ramp + ripple + growing noise."""
    if shape not in _STACKS:
        n0, n1 = shape
        x, y = np.meshgrid(np.arange(n0), np.arange(n1), indexing='ij')
        rng = np.random.default_rng(7)
        psi = np.zeros((B,) + shape)
        psi[1] = _wrap(0.31 * x - 0.23 * y)
        for i in range(2, 5):
            a, b = rng.uniform(-0.4, 0.4, 2)
            psi[i] = _wrap(a * x + b * y + 1.5 * np.sin(x / 9 + y / 13) + 0.03 * (i + 1) * rng.standard_normal(shape))
        W = 0.3 + rng.random((B,) + shape)
        psi.setflags(write=False)
        W.setflags(write=False)
        _STACKS[shape] = (psi, W)
    return _STACKS[shape]


def weight_modes(W):
    return (('none', None), ('shared', W[0]), ('own', W))


def weight_of(w, b):
    return None if w is None else (w if w.ndim == 2 else w[b])


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shape, kmax', [((64, 64), 40), ((128, 256), 12), ((100, 60), 12), ((64, 2048), 12), ((1024, 128), 12)])
def test_stack_equals_singles_bit_for_bit(shape, kmax, dtype, gpa_option):
    """Stack == singles, bit for bit, phi and iteration counts, for weight None / W[0] shared / W own, from psi and from
    np.diff pairs.  NO_LAT=1: the same kernels on both sides -- a single small power-of-two frame otherwise runs latency-tuned
    instantiations whose multiply-adds the compiler contracts differently (tests/test_gpu_parity.py,
    test_image_stack_equals_single_images).  W[1] != W[0] pixel for pixel, so a problem that read another problem's weight
    (a left-over `pb >> 1`) cannot give the single call's bits.  f64 with own weights: the problems of one launch set stop at
    different iterations (CPU oracle, 64 x 64, kmax = 40: 0, 38, 40, 39, 39)."""
    gpa_option('NO_LAT', '1')
    psi, W = make_stack(shape)
    assert not np.any(W[1] == W[0])
    dx, dy = np.diff(psi, axis=2), np.diff(psi, axis=1)
    plan = _lib.Plan(shape, 1, dtype)
    for mode, w in weight_modes(W):
        phi_s, it_s = plan.unwrap_stack(psi, w, kmax=kmax)
        phi_d, it_d = plan.unwrap_prediff_stack(dx, dy, w, kmax=kmax)
        assert phi_s.shape == (B,) + shape and phi_s.dtype == dtype and it_s.shape == (B,)
        for b in range(B):
            phi1, it1 = plan.unwrap(psi[b], weight_of(w, b), kmax=kmax)
            assert np.array_equal(phi_s[b], phi1), (shape, mode, b, float(np.abs(phi_s[b] - phi1).max()))
            assert it_s[b] == it1, (shape, mode, b, it_s, it1)
            phi1, it1 = plan.unwrap_prediff(dx[b], dy[b], weight_of(w, b), kmax=kmax)
            assert np.array_equal(phi_d[b], phi1), (shape, mode, 'prediff', b, float(np.abs(phi_d[b] - phi1).max()))
            assert it_d[b] == it1, (shape, mode, 'prediff', b, it_d, it1)
        assert it_s[0] == 0 and not phi_s[0].any()          # plane 0: r0 == 0
        assert np.isfinite(phi_s).all() and np.isfinite(phi_d).all()
        if dtype is np.float64 and mode == 'own':
            assert len(set(it_s.tolist())) > 1, it_s        # the problems of one launch set end at different iterations
    plan.close()


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('nb', [1, 2])
def test_one_and_two_maps_with_the_default_kernels(nb, dtype):
    """nprob <= 2 takes the route of a single solve (unwrap_route): bit for bit against plan.unwrap with no option set"""
    shape = (128, 128)
    psi, W = make_stack(shape)
    plan = _lib.Plan(shape, 1, dtype)
    for mode, w in weight_modes(W[1:1 + nb]):
        phi_s, it_s = plan.unwrap_stack(psi[1:1 + nb], w, kmax=12)
        for b in range(nb):
            phi1, it1 = plan.unwrap(psi[1 + b], weight_of(w, b), kmax=12)
            assert np.array_equal(phi_s[b], phi1), (nb, mode, b, float(np.abs(phi_s[b] - phi1).max()))
            assert it_s[b] == it1
    plan.close()


@pytest.mark.parametrize('dtype', DTYPES)
def test_stack_against_the_oracle(golden, dtype):
    """the three phase maps of hex_64 with the weights iterate_GPA hands to its unwraps, sqrt(w_p / max w_p), kmax = 10,
    default kernels: each plane within the pcg tolerance of the oracle, plane 0 also of the golden unwrap"""
    g = golden('hex_64')
    psi = g['a5_phases']
    w = np.stack([np.sqrt(wp / wp.max()) for wp in g['a5_weights']])
    plan = _lib.Plan(psi.shape[1:], 1, dtype)
    phi, iters = plan.unwrap_stack(psi, w, kmax=10)
    for p in range(3):
        ref = orc.unwrap(psi[p], w[p], kmax=10)
        assert rel(phi[p], ref) < PCG_TOL[dtype], (p, rel(phi[p], ref))
    assert rel(phi[0], g['a7_psi_unwrap_kmax10']) < PCG_TOL[dtype]
    plan.close()


@pytest.mark.parametrize('dtype', DTYPES)
def test_chunks_and_shared_workspace(dtype, gpa_option):
    """UNWRAP_STACK_BYTES makes B = 5 run as chunks of 2, 2 and 1 with the bits of the unchunked call; a call of 2 reuses the
    workspace, a call of 7 grows it; the batched driver, which shares the workspace, returns identical u and counts before
    and after; gpa_plan_workspace_bytes never decreases and covers the grown workspace."""
    shape, kmax = (64, 64), 12
    psi, W = make_stack(shape)
    kvecs = hex_kvecs(0.12, 5.0)
    sigma = 5
    klists = np.stack(explicit_klists(kvecs, 0.04, 2, 2))
    imgs = np.stack([hex_moire(shape, kvecs, (0.3 + 0.2 * i) * gaussian_bump_displacement(shape), noise=0.05 * (i + 1), seed=i)
                     for i in range(3)])
    plan = _lib.Plan(shape, 12, dtype)
    sizes = [plan.workspace_bytes]
    u0, itu0 = plan.extract_displacement_field_stack(imgs, kvecs, klists, sigma, 2 * sigma, kmax=10)    # 6 problems
    sizes.append(plan.workspace_bytes)
    phi_ref, it_ref = plan.unwrap_stack(psi, W, kmax=kmax)           # unchunked: the 6-problem workspace serves 5
    sizes.append(plan.workspace_bytes)
    per = plan.unwrap_batch_problem_bytes(kmax)
    assert per >= (3 + 10) * shape[0] * shape[1] * np.dtype(dtype).itemsize
    gpa_option('UNWRAP_STACK_BYTES', str(2 * per + per // 2))        # two problems and a half: 2 + 2 + 1
    phi_c, it_c = plan.unwrap_stack(psi, W, kmax=kmax)
    assert np.array_equal(phi_c, phi_ref) and np.array_equal(it_c, it_ref)
    phi_p, it_p = plan.unwrap_prediff_stack(np.diff(psi, axis=2), np.diff(psi, axis=1), W[0], kmax=kmax)
    gpa_option('UNWRAP_STACK_BYTES', None)
    phi_q, it_q = plan.unwrap_prediff_stack(np.diff(psi, axis=2), np.diff(psi, axis=1), W[0], kmax=kmax)
    assert np.array_equal(phi_p, phi_q) and np.array_equal(it_p, it_q)
    sizes.append(plan.workspace_bytes)
    phi_2, it_2 = plan.unwrap_stack(psi[1:3], W[1:3], kmax=kmax)     # reuses the workspace
    assert plan.workspace_bytes == sizes[-1]
    psi7 = np.concatenate([psi, psi[3:5]])
    W7 = np.concatenate([W, W[3:5]])
    phi_7, it_7 = plan.unwrap_stack(psi7, W7, kmax=kmax)             # grows it to 7 problems
    sizes.append(plan.workspace_bytes)
    assert sizes[-1] >= sizes[-2] + per - 4096, sizes               # (one problem more than the six before)
    assert sizes[-1] >= sizes[0] + 7 * per - 4096, sizes            # covers the grown workspace, ring included
    assert all(b >= a for a, b in zip(sizes, sizes[1:])), sizes
    u1, itu1 = plan.extract_displacement_field_stack(imgs, kvecs, klists, sigma, 2 * sigma, kmax=10)
    assert np.array_equal(u1, u0) and np.array_equal(itu1, itu0)
    assert plan.workspace_bytes == sizes[-1]
    plan.close()
    # on a fresh plan the chunked call builds a workspace of two problems, not of five
    plan = _lib.Plan(shape, 1, dtype)
    base = plan.workspace_bytes
    gpa_option('UNWRAP_STACK_BYTES', str(2 * per + per // 2))
    phi_f, it_f = plan.unwrap_stack(psi, W, kmax=kmax)
    gpa_option('UNWRAP_STACK_BYTES', None)
    grown = plan.workspace_bytes - base
    assert 2 * per - 4096 <= grown < 3 * per + 5 * psi[0].size * 8 * 3, (grown, per)    # (+ the staging of a chunk)
    plan.close()
    # the same stack under the same kernels on every plan: one set of bits (the single calls of this configuration)
    gpa_option('NO_LAT', '1')
    plan = _lib.Plan(shape, 1, dtype)
    for b in range(B):
        phi1, it1 = plan.unwrap(psi[b], W[b], kmax=kmax)
        assert np.array_equal(phi_ref[b], phi1) and np.array_equal(phi_f[b], phi1) and it_ref[b] == it1 == it_f[b]
    for b in range(2):
        assert np.array_equal(phi_7[5 + b], phi_ref[3 + b]) and it_7[5 + b] == it_ref[3 + b]
    plan.close()
    # two maps take the single solve's default (latency-tuned) kernels
    gpa_option('NO_LAT', None)
    plan = _lib.Plan(shape, 1, dtype)
    for b in range(2):
        phi1, it1 = plan.unwrap(psi[1 + b], W[1 + b], kmax=kmax)
        assert np.array_equal(phi_2[b], phi1) and it_2[b] == it1
    plan.close()


@pytest.mark.parametrize('dtype', DTYPES)
def test_device_resident_form(dtype):
    """unwrap_batch_dev with iters_out = NULL only enqueues; unwrap_batch_finish waits and hands over the counts: the bits and
    counts of the host form, the inputs untouched"""
    shape, kmax = (128, 256), 12
    psi, W = make_stack(shape)
    psi_t, W_t = psi.astype(dtype), W.astype(dtype)
    plan = _lib.Plan(shape, 1, dtype)
    phi_h, it_h = plan.unwrap_stack(psi, W, kmax=kmax)
    d_psi = _lib.DeviceBuffer(psi_t.nbytes)
    d_w = _lib.DeviceBuffer(W_t.nbytes)
    d_phi = _lib.DeviceBuffer(psi_t.nbytes)
    try:
        d_psi.upload(psi_t)
        d_w.upload(W_t)
        assert plan.unwrap_batch_dev(d_psi.ptr, B, d_w.ptr, B, d_phi.ptr, kmax=kmax, want_iters=False) is None
        it_d = plan.unwrap_batch_finish(B)
        assert np.array_equal(it_d, it_h)
        assert np.array_equal(d_phi.download(psi_t.shape, dtype), phi_h)
        assert np.array_equal(d_psi.download(psi_t.shape, dtype), psi_t)
        assert np.array_equal(d_w.download(W_t.shape, dtype), W_t)
        # the waiting form, one shared weight, and the gradients
        it_w = plan.unwrap_batch_dev(d_psi.ptr, B, d_w.ptr, 1, d_phi.ptr, kmax=kmax)
        phi_sh, it_sh = plan.unwrap_stack(psi, W[0], kmax=kmax)
        assert np.array_equal(it_w, it_sh) and np.array_equal(d_phi.download(psi_t.shape, dtype), phi_sh)
    finally:
        for buf in (d_psi, d_w, d_phi):
            buf.free()
    plan.close()


@pytest.mark.parametrize('dtype', DTYPES)
def test_shape_without_a_batched_unwrap(dtype, gpa_option, monkeypatch):
    """63 x 65.  A plan whose unwrap has no fused iteration has no batched unwrap: the C entry says so (GPA_ERR_STATE, with
    the reason) and the mirror, which asks gpa_supports_batch once, loops over the single call and returns its bits.
    As the library stands the mixed-radix engine gives 63 x 65 a fused iteration (chirp-z on a smooth length that fits LDS, as
    for every shape a plan offers an unwrap for), so only a plan built under NO_MR=1 -- the Bluestein kernels of
    test_mixed_radix_fused_unwrap_vs_oracle -- is without one; the default plan runs the stack, bit for bit like any other."""
    shape, kmax = (63, 65), 10
    psi, W = make_stack(shape)
    dx, dy = np.diff(psi, axis=2), np.diff(psi, axis=1)
    gpa_option('NO_LAT', '1')
    plan = _lib.Plan(shape, 1, dtype)
    assert plan.lib.gpa_supports_batch(plan.handle)
    phi_s, it_s = plan.unwrap_stack(psi, W, kmax=kmax)
    for b in range(B):
        phi1, it1 = plan.unwrap(psi[b], W[b], kmax=kmax)
        assert np.array_equal(phi_s[b], phi1) and it_s[b] == it1, b
    plan.close()
    gpa_option('NO_MR', '1')
    monkeypatch.setattr(_lib, '_plans', {})                 # the drop-in functions build their plan under NO_MR too
    plan = _lib.Plan(shape, 1, dtype)
    assert not plan.lib.gpa_supports_batch(plan.handle)
    psi_t = np.ascontiguousarray(psi, dtype=dtype)
    phi = np.full_like(psi_t, 7.5)
    it = (C.c_int * B)()
    for code in (plan.lib.gpa_unwrap_batch(plan.handle, _lib._ptr(psi_t), B, None, 0, kmax, 1e-9, 1, _lib._ptr(phi), it),
                 plan.lib.gpa_unwrap_batch_dev(plan.handle, _lib._ptr(psi_t), B, None, 0, kmax, 1e-9, 1, _lib._ptr(phi), None)):
        assert code == GPA_ERR_STATE
        assert 'no batched unwrap' in _lib.last_error() and 'gpa_unwrap_batch' in _lib.last_error()
    assert np.all(phi == 7.5)
    phi_l, it_l = plan.unwrap_stack(psi, W, kmax=kmax)      # the mirror's loop
    for b in range(B):
        phi1, it1 = plan.unwrap(psi[b], W[b], kmax=kmax)
        assert np.array_equal(phi_l[b], phi1) and it_l[b] == it1, b
    plan.close()
    out = PU.phase_unwrap_stack(psi, W, kmax=kmax, dtype=dtype)
    out_d = PU.phase_unwrap_prediff_stack(dx, dy, W[0], kmax=kmax, dtype=dtype)
    assert not _lib.get_plan(shape, 1, dtype).lib.gpa_supports_batch(_lib.get_plan(shape, 1, dtype).handle)
    for b in range(B):
        assert np.array_equal(out[b], PU.phase_unwrap(psi[b], W[b], kmax=kmax, dtype=dtype))
        assert np.array_equal(out[b], phi_l[b])
        assert np.array_equal(out_d[b], PU.phase_unwrap_prediff(dx[b], dy[b], W[0], kmax=kmax, dtype=dtype))
    for pl in _lib._plans.values():
        pl.close()


def test_refusals_name_the_argument_and_launch_nothing(gpa_option):
    """Refusals only: every bad argument is GPA_ERR_ARG naming it, raised before anything is launched -- phi keeps its
    sentinel -- and a valid call on the same plan afterwards gives the bits of the single calls."""
    gpa_option('NO_LAT', '1')
    shape, kmax, dtype = (64, 64), 12, np.float64
    psi, W = make_stack(shape)
    psi_t, W_t = np.ascontiguousarray(psi), np.ascontiguousarray(W)
    plan = _lib.Plan(shape, 1, dtype)
    lib, h = plan.lib, plan.handle
    phi = np.full_like(psi_t, 7.5)
    it = (C.c_int * (_lib.UNWRAP_BATCH_MAX + 1))()
    P, Wp, F = _lib._ptr(psi_t), _lib._ptr(W_t), _lib._ptr(phi)
    dx, dy = np.ascontiguousarray(np.diff(psi, axis=2)), np.ascontiguousarray(np.diff(psi, axis=1))
    cases = [
        ('nb', lambda: lib.gpa_unwrap_batch(h, P, 0, None, 0, kmax, 1e-9, 1, F, it)),
        ('nb', lambda: lib.gpa_unwrap_batch(h, P, _lib.UNWRAP_BATCH_MAX + 1, None, 0, kmax, 1e-9, 1, F, it)),
        ('nb', lambda: lib.gpa_unwrap_batch(h, P, -1, None, 0, kmax, 1e-9, 1, F, it)),
        ('weight_planes', lambda: lib.gpa_unwrap_batch(h, P, B, Wp, 2, kmax, 1e-9, 1, F, it)),
        ('weight_planes', lambda: lib.gpa_unwrap_batch(h, P, B, Wp, B + 1, kmax, 1e-9, 1, F, it)),
        ('weight_planes', lambda: lib.gpa_unwrap_batch(h, P, B, Wp, -1, kmax, 1e-9, 1, F, it)),
        ('weight', lambda: lib.gpa_unwrap_batch(h, P, B, Wp, 0, kmax, 1e-9, 1, F, it)),          # a pointer without planes
        ('weight', lambda: lib.gpa_unwrap_batch(h, P, B, None, B, kmax, 1e-9, 1, F, it)),        # planes without a pointer
        ('weight', lambda: lib.gpa_unwrap_batch(h, P, B, None, 1, kmax, 1e-9, 1, F, it)),
        ('kmax', lambda: lib.gpa_unwrap_batch(h, P, B, Wp, B, 0, 1e-9, 1, F, it)),
        ('psi', lambda: lib.gpa_unwrap_batch(h, None, B, Wp, B, kmax, 1e-9, 1, F, it)),
        ('phi', lambda: lib.gpa_unwrap_batch(h, P, B, Wp, B, kmax, 1e-9, 1, None, it)),
        ('phi', lambda: lib.gpa_unwrap_batch(h, P, B, Wp, B, kmax, 1e-9, 1, P, it)),             # phi on top of psi
        ('dy', lambda: lib.gpa_unwrap_prediff_batch(h, _lib._ptr(dx), None, B, Wp, B, kmax, 1e-9, 1, F, it)),
        ('dx', lambda: lib.gpa_unwrap_prediff_batch(h, None, _lib._ptr(dy), B, Wp, B, kmax, 1e-9, 1, F, it)),
        ('nb', lambda: lib.gpa_unwrap_prediff_batch(h, _lib._ptr(dx), _lib._ptr(dy), 0, Wp, B, kmax, 1e-9, 1, F, it)),
        # the device forms check before they touch a pointer: the host arrays' addresses are never dereferenced
        ('nb', lambda: lib.gpa_unwrap_batch_dev(h, P, 0, None, 0, kmax, 1e-9, 1, F, None)),
        ('weight_planes', lambda: lib.gpa_unwrap_batch_dev(h, P, B, Wp, 3, kmax, 1e-9, 1, F, None)),
        ('kmax', lambda: lib.gpa_unwrap_prediff_batch_dev(h, _lib._ptr(dx), _lib._ptr(dy), B, None, 0, 0, 1e-9, 1, F, None)),
        ('nb', lambda: lib.gpa_unwrap_batch_finish(h, 1, it)),                                   # no batch call yet
    ]
    ws = plan.workspace_bytes
    for name, call in cases:
        code = call()
        assert code == GPA_ERR_ARG, (name, code)
        assert name in _lib.last_error(), (name, _lib.last_error())
        with pytest.raises(_lib.GPAError, match=name):
            _lib.check(code, 'gpa_unwrap_batch')
    assert np.all(phi == 7.5) and plan.workspace_bytes == ws          # nothing ran, nothing was built
    # ... and the mirror raises them as GPAError too
    with pytest.raises(_lib.GPAError, match='kmax'):
        plan.unwrap_stack(psi, W, kmax=0)
    # a valid call on the same plan afterwards
    phi_s, it_s = plan.unwrap_stack(psi, W, kmax=kmax)
    for b in range(B):
        phi1, it1 = plan.unwrap(psi[b], W[b], kmax=kmax)
        assert np.array_equal(phi_s[b], phi1) and it_s[b] == it1
    with pytest.raises(_lib.GPAError, match='nb'):
        plan.unwrap_batch_finish(B + 1)
    assert np.array_equal(plan.unwrap_batch_finish(B), it_s)
    plan.close()
