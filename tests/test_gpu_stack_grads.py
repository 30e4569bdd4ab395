"""The stack driver with the one-sweep outputs (gpa_extract_displacement_field_grad_batch_dev): u and, per frame and peak,
lock-in, winner, phase gradient and |lock-in| of a whole stack from one set of launches per chunk -- against the single-image
one-sweep driver frame by frame (bit for bit, with NO_LAT=1 as in test_image_stack_equals_single_images: a single small
power-of-two image otherwise runs latency-tuned instantiations of the unwrap's kernels), against the reference's own numbers
(tests/golden) and through the mirror's `wfr_func` plug-ins.  Run with `-m gpu` on an MI355X.

Which kernels ran is not checked here: the batched driver installs no per-kernel profiler (gpa_set_profiling reaches the
single-image entry points only), so a stack call leaves no kernel profile to read."""
import functools

import numpy as np
import pytest

from oracle import gpa_oracle as orc
from pygpa_amd import _lib, cuGPA
from pygpa_amd import geometric_phase_analysis as GPA
from pygpa_amd.synthetic import hex_kvecs, gaussian_bump_displacement, hex_moire, explicit_klists
from test_gpu_onesweep import GRAD_TOL, _grad_err
from test_gpu_parity import TOL, DeviceArray, check_kidx, rel

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
NAMES = ('u', 'lockins', 'kidx', 'grads', 'weights')


def _golden_frames(g):
    """(flipped image, the golden image, the image + 0.3 noise): the golden one at position 1"""
    img = g['image']
    noise = np.random.default_rng(11).normal(size=img.shape)
    return np.stack([img[::-1, ::-1], img, img + 0.3 * noise])


def _case(name, golden):
    """(frames (3, N, M), kvecs, klists (3, K, 2), sigma)"""
    if name == 'wide':   # 2048-point rows: the shared-forward pass B; shape and 4 x 4 lists of tests/test_gpu_shared_passb.py::_case
        shape = (64, 2048)
        kvecs = hex_kvecs(0.1, 7.0)
        kw, sigma, _ = orc.derive_params(kvecs)
        frames = np.stack([hex_moire(shape, kvecs, (0.5 + 0.25 * i) * gaussian_bump_displacement(shape), noise=0.2, seed=5 + i)
                           for i in range(3)])
        return frames, kvecs, np.stack(explicit_klists(kvecs, kw, 4, 4)), int(sigma)
    g = golden(name)
    return _golden_frames(g), g['kvecs'], g['a3_klists'], int(g['sigma'])


def _stack(plan, frames, kvecs, klists, sigma, grad_mode=0, chunk=None):
    """{name: array} and the iteration counts of one stack call with every optional output"""
    res = plan.extract_displacement_field_stack(frames, kvecs, klists, sigma, 2 * sigma, kmax=10, chunk=chunk, want_lockins=True,
                                                want_kidx=True, want_grads=True, want_weights=True, grad_mode=grad_mode)
    return dict(zip(NAMES, (res[0],) + res[2:])), res[1]


def _single(plan, image, kvecs, klists, sigma, grad_mode=0):
    u, lock, kidx, iters, grads, absw = plan.extract_displacement_field(image, kvecs, klists, sigma, 2 * sigma, kmax=10,
                                                                         want_lockins=True, want_kidx=True, want_grads=True,
                                                                         want_weights=True, grad_mode=grad_mode)
    return dict(zip(NAMES, (u, lock, kidx, grads, absw))), iters


def _assert_frames_equal(out, iters, singles, frames_of, what):
    for i, f in enumerate(frames_of):
        ref, it = singles[f]
        for k in NAMES:
            assert out[k][i].dtype == ref[k].dtype and out[k][i].shape == ref[k].shape, (what, k)
            assert np.array_equal(out[k][i], ref[k], equal_nan=True), (what, 'frame', f, k)
        assert tuple(iters[i]) == tuple(it), (what, 'frame', f, 'iterations')


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name', ['hex_64', 'wide', 'hex_48x80'])
def test_stack_equals_single_calls(golden, gpa_option, name, dtype):
    """every output and the iteration counts of B = 3 frames, as one chunk and as chunks of 2 and 1, then a shorter stack on the
    same plan (capacity reuse), equal the single one-sweep call per frame.  hex_64: 64-point rows, the per-candidate pass B in
    its phases mode (and the three stencils); 64 x 2048: the shared-forward pass B with phases; 48 x 80: zero-padded rows and a
    mixed-radix unwrap."""
    gpa_option('NO_LAT', '1')
    frames, kvecs, klists, sigma = _case(name, golden)
    plan = _lib.Plan(frames.shape[1:], 3 * klists.shape[1], dtype)
    assert plan.lib.gpa_supports_batch(plan.handle)
    try:
        for grad_mode in ((0, 1, 2) if name == 'hex_64' else (0,)):
            singles = [_single(plan, f, kvecs, klists, sigma, grad_mode) for f in frames]
            assert not np.array_equal(singles[0][0]['grads'], singles[1][0]['grads'])   # frames differ
            out, iters = _stack(plan, frames, kvecs, klists, sigma, grad_mode)
            _assert_frames_equal(out, iters, singles, (0, 1, 2), (name, grad_mode, 'one chunk'))
            out, iters = _stack(plan, frames, kvecs, klists, sigma, grad_mode, chunk=2)
            _assert_frames_equal(out, iters, singles, (0, 1, 2), (name, grad_mode, 'chunks of 2 and 1'))
            out, iters = _stack(plan, frames[1:], kvecs, klists, sigma, grad_mode)
            _assert_frames_equal(out, iters, singles, (1, 2), (name, grad_mode, 'shorter stack'))
        # caller's buffers, and a subset of the outputs
        og = np.empty((3, 3) + frames.shape[1:] + (2,), dtype=dtype)
        res = plan.extract_displacement_field_stack(frames, kvecs, klists, sigma, 2 * sigma, kmax=10, out_grads=og, want_weights=True)
        singles = [_single(plan, f, kvecs, klists, sigma) for f in frames]
        assert res[4] is og and res[2] is None and res[3] is None
        for i in range(3):
            assert np.array_equal(og[i], singles[i][0]['grads']) and np.array_equal(res[5][i], singles[i][0]['weights'])
            assert np.array_equal(res[0][i], singles[i][0]['u'])
    finally:
        plan.close()


@pytest.mark.parametrize('dtype', DTYPES)
def test_reference_numbers(golden, dtype):
    """frame 1 of the hex_64 stack against hex_64 / props_64 exactly as test_gpu_onesweep.py::test_golden_all_peaks holds the
    single call (same TOL and GRAD_TOL); the golden image is not the first frame, so a wrong frame stride cannot pass"""
    g, pr = golden('hex_64'), golden('props_64')
    sigma = int(g['sigma'])
    K = g['a3_klists'].shape[1]
    plan = _lib.Plan(g['image'].shape, 3 * K, dtype)
    out, iters = _stack(plan, _golden_frames(g), g['kvecs'], g['a3_klists'], sigma)
    plan.close()
    u, lock, kidx, grads, absw = (out[k][1] for k in NAMES)
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
        assert np.array_equal(kidx, g['a3_kidx']) and tuple(iters[1]) == (10, 10)
    assert not np.array_equal(out['kidx'][0], out['kidx'][1])


@pytest.mark.parametrize('dtype', DTYPES)
def test_nothing_asked_nothing_changed(golden, dtype):
    """with every optional output NULL, u and the iteration counts are extract_displacement_field_batch_dev's bit for bit; a call
    with gradients in between leaves the plain call's u as it was"""
    frames, kvecs, klists, sigma = _case('hex_48x80', golden)
    frames = frames.astype(dtype)
    B = len(frames)
    plan = _lib.Plan(frames.shape[1:], 3 * klists.shape[1], dtype)
    d_img = DeviceArray(frames)
    d_u = [DeviceArray(np.zeros((B, 2) + frames.shape[1:], dtype=dtype)) for _ in range(4)]
    d_g = DeviceArray(np.zeros((B, 3) + frames.shape[1:] + (2,), dtype=dtype))
    it0 = plan.extract_displacement_field_batch_dev(d_img.ptr, B, kvecs, klists, sigma, 2 * sigma, 10, d_u[0].ptr)
    it1 = plan.extract_displacement_field_grad_batch_dev(d_img.ptr, B, kvecs, klists, sigma, 2 * sigma, 10, d_u[1].ptr)
    it2 = plan.extract_displacement_field_grad_batch_dev(d_img.ptr, B, kvecs, klists, sigma, 2 * sigma, 10, d_u[2].ptr,
                                                         grads_ptr=d_g.ptr)
    it3 = plan.extract_displacement_field_grad_batch_dev(d_img.ptr, B, kvecs, klists, sigma, 2 * sigma, 10, d_u[3].ptr,
                                                         want_iters=False)
    it3 = plan._batch_iters(B)   # iters_out NULL: no synchronisation, gpa_last_batch_iters reads the counts
    u0, u1, u2, u3 = (d.get() for d in d_u)
    plan.close()
    assert u0.any() and d_g.get().any()
    assert np.array_equal(u1, u0) and np.array_equal(it1, it0)
    assert np.array_equal(u3, u0) and np.array_equal(it3, it0)
    assert u2.any() and it2.shape == it0.shape   # (held to the single one-sweep call in test_stack_equals_single_calls)


def test_stack_call_refuses_what_the_single_call_refuses(golden):
    frames, kvecs, klists, sigma = _case('hex_64', golden)
    plan = _lib.Plan(frames.shape[1:], 3 * klists.shape[1], np.float32)
    d_img = DeviceArray(frames.astype(np.float32))
    d_u = DeviceArray(np.zeros((3, 2) + frames.shape[1:], dtype=np.float32))
    d_g = DeviceArray(np.zeros((3, 3) + frames.shape[1:] + (2,), dtype=np.float32))
    with pytest.raises(_lib.GPAError, match='grad_mode'):
        plan.extract_displacement_field_grad_batch_dev(d_img.ptr, 3, kvecs, klists, sigma, 2 * sigma, 10, d_u.ptr, grads_ptr=d_g.ptr,
                                                       grad_mode=3)
    with pytest.raises(_lib.GPAError, match='images'):
        plan.extract_displacement_field_grad_batch_dev(d_img.ptr, 0, kvecs, klists, sigma, 2 * sigma, 10, d_u.ptr, grads_ptr=d_g.ptr)
    plan.close()


# ---- the mirror ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def movie():
    shape = (128, 128)
    kvecs = hex_kvecs(0.1, 7.0)
    return np.stack([hex_moire(shape, kvecs, (0.5 + 0.3 * i) * gaussian_bump_displacement(shape), noise=0.1, seed=20 + i)
                     for i in range(3)]), kvecs


@pytest.mark.parametrize('wfr_func', [GPA.wfr2_grad_opt, cuGPA.wfr2_grad_opt, cuGPA.wfr2_grad_single],
                         ids=['GPA.wfr2_grad_opt', 'cuGPA.wfr2_grad_opt', 'cuGPA.wfr2_grad_single'])
def test_mirror_return_gs(movie, gpa_option, wfr_func):
    """extract_displacement_field_stack(frames, ks, return_gs=True, wfr_func=f): us and gs[b][p] -- keys in the single call's
    order, dtypes and every array -- equal the single call's per frame; the arrays are views of the stacked outputs"""
    gpa_option('NO_LAT', '1')
    frames, kvecs = movie
    us, gs = GPA.extract_displacement_field_stack(frames, kvecs, return_gs=True, wfr_func=wfr_func)
    assert us.shape == (3, 2, 128, 128) and len(gs) == 3
    for b in range(3):
        u, g1 = GPA.extract_displacement_field(frames[b], kvecs, return_gs=True, wfr_func=wfr_func)
        assert us[b].dtype == u.dtype and np.array_equal(us[b], u), b
        assert len(gs[b]) == len(g1) == 3
        for p in range(3):
            assert list(gs[b][p]) == list(g1[p])
            for k in g1[p]:
                assert gs[b][p][k].dtype == g1[p][k].dtype and gs[b][p][k].shape == g1[p][k].shape, (b, p, k)
                assert np.array_equal(gs[b][p][k], g1[p][k], equal_nan=True), (b, p, k)
    assert not np.array_equal(gs[0][0]['lockin'], gs[1][0]['lockin'])
    for k in ('lockin', 'grad'):
        assert gs[0][0][k].base is not None and gs[0][0][k].base is gs[2][1][k].base, k   # no per-frame copies


def test_mirror_default_and_refusals(movie, gpa_option):
    gpa_option('NO_LAT', '1')
    frames, kvecs = movie
    us = GPA.extract_displacement_field_stack(frames, kvecs)
    assert isinstance(us, np.ndarray) and us.shape == (3, 2, 128, 128) and us.dtype == GPA.DEFAULT_DTYPE
    for b in range(3):
        assert np.array_equal(us[b], GPA.extract_displacement_field(frames[b], kvecs))
    assert np.array_equal(GPA.extract_displacement_field_stack(frames, kvecs, None, 2.5, 3, None, None), us)   # positional, as before
    part = functools.partial(GPA.wfr2_grad_opt)
    with pytest.raises(ValueError, match='partial'):
        GPA.extract_displacement_field_stack(frames, kvecs, return_gs=True, wfr_func=part)
    with pytest.raises(ValueError):
        GPA.extract_displacement_field_stack(frames, kvecs, wfr_func=lambda *a, **k: None)
