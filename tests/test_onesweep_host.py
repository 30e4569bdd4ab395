"""The one-sweep driver (gpa_extract_displacement_field_grad*) and the routing of the mirror's `wfr_func` plug-ins onto it,
on the CPU: the ABI is checked against the built library, the routing with the device call replaced by a recording stand-in
for _lib.get_plan that answers from the oracle (as tests/test_host_logic.py does for find_peaks), so that the per-peak results
the mirror assembles are checked too."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import gpa_oracle as orc
from pygpa_amd import _lib
from pygpa_amd.synthetic import hex_kvecs, gaussian_bump_displacement, hex_moire

NEW = ['gpa_extract_displacement_field_grad', 'gpa_extract_displacement_field_grad_dev',
       'gpa_extract_displacement_field_grad_async']


def _ensure_built():
    import os
    if not os.path.exists(_lib.LIB_PATH):
        from pygpa_amd import build
        build.build(verbose=False)


def test_new_symbols_exported_with_prototypes():
    _ensure_built()
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    # the async form is the synchronising one without iters_out
    assert _lib.SIGNATURES[NEW[2]][1] == _lib.SIGNATURES[NEW[1]][1][:-1]
    assert _lib.SIGNATURES[NEW[0]] == _lib.SIGNATURES[NEW[1]]


@pytest.mark.parametrize('name', NEW)
def test_null_plan_is_an_argument_error(name):
    _ensure_built()
    lib = _lib.load()
    nargs = len(_lib.SIGNATURES[name][1])
    args = [None, None, None, 3, None, 9, 5.0, 10, 10, 0] + [None] * (nargs - 10)
    assert getattr(lib, name)(*args) == -1         # GPA_ERR_ARG
    assert name + ':' in _lib.last_error()


class _RecordingPlan:
    """stands in for _lib.Plan: records the calls, answers the driver from the oracle"""

    def __init__(self, log, shape, batch, dtype):
        self.log, self.shape, self.dtype = log, tuple(shape), np.dtype(dtype)
        self.rdtype = self.dtype.type
        self.cdtype = np.complex64 if self.dtype == np.float32 else np.complex128

    def extract_displacement_field(self, image, kvecs, klists, sigma, mask_border, kmax=10, want_lockins=False,
                                   want_kidx=False, out=None, want_grads=False, want_weights=False, grad_mode=0):
        self.log.append(('extract', self.dtype, bool(want_grads), bool(want_weights), int(grad_mode)))
        image = np.asarray(image, dtype=np.float64)
        u = orc.extract_displacement_field(image, kvecs, sigma=sigma, klists=list(klists))
        img0 = image - image.mean()
        gs = [orc.sweep(img0, sigma, klists[p], kvecs[p], want_grad=True) for p in range(len(kvecs))]
        lock = np.stack([g['lockin'] for g in gs]).astype(self.cdtype) if want_lockins else None
        kidx = np.stack([g['kidx'] for g in gs]) if want_kidx else None
        res = (u.astype(self.rdtype), lock, kidx, (10, 10))
        if want_grads or want_weights:
            grads = np.stack([g['grad'] for g in gs]).astype(self.rdtype) if want_grads else None
            absw = np.stack([np.abs(g['lockin']) for g in gs]).astype(self.rdtype) if want_weights else None
            res += (grads, absw)
        return res

    # the old branch: per-peak sweeps of the plug-in, reconstruction and unwraps as separate calls
    def sweep(self, image, kref, klist, sigma, want_kidx=True, want_grad=False, grad_mode=0):
        self.log.append(('sweep', self.dtype))
        g = orc.sweep(np.asarray(image, dtype=np.float64), sigma, klist, kref, want_grad=want_grad)
        return (g['lockin'].astype(self.cdtype), g['kidx'] if want_kidx else None,
                g['grad'].astype(self.rdtype) if want_grad else None)

    def reconstruct_grad(self, lockins, kvecs, mask_border):
        self.log.append(('reconstruct_grad', self.dtype))
        n0, n1 = self.shape
        return np.zeros((2, n0, n1 - 1)), np.zeros((2, n0 - 1, n1)), np.ones((n0, n1))

    def unwrap_prediff(self, dx, dy, weight=None, kmax=10):
        self.log.append(('unwrap_prediff', self.dtype))
        return np.zeros(self.shape), kmax


@pytest.fixture
def recorded(monkeypatch):
    log = []
    monkeypatch.setattr(_lib, 'get_plan', lambda shape, batch, dtype=np.float64, device=0: _RecordingPlan(log, shape, batch, dtype))
    return log


@pytest.fixture(scope='module')
def case():
    shape = (48, 40)
    kvecs = hex_kvecs(0.15, 7.0)
    img = hex_moire(shape, kvecs, gaussian_bump_displacement(shape), noise=0.1, seed=5)
    kw, sigma, kstep = orc.derive_params(kvecs)
    img0 = img - img.mean()
    ref = [orc.wfr2_grad_opt(img0, sigma, pk[0], pk[1], kw, kstep) for pk in kvecs]
    lists = [orc.sweep_grid(pk[0], pk[1], kw, kstep) for pk in kvecs]
    u = orc.extract_displacement_field(img, kvecs)
    return img, kvecs, ref, lists, u


def _routed():
    import pygpa_amd.geometric_phase_analysis as GPA
    from pygpa_amd import cuGPA
    return [(GPA.wfr2_grad_opt, {'lockin', 'w', 'grad', 'kidx'}, np.float64),
            (GPA.wfr2_grad_vec, {'lockin', 'w', 'grad', 'kidx'}, np.float64),
            (cuGPA.wfr2_grad_opt, {'w', 'lockin', 'grad'}, np.float64),
            (cuGPA.wfr2_grad_single, {'lockin', 'grad'}, np.float32)]


@pytest.mark.parametrize('which', range(4))
def test_plugin_with_return_gs_is_one_driver_call(recorded, case, which):
    import pygpa_amd.geometric_phase_analysis as GPA
    func, keys, plan_dtype = _routed()[which]
    img, kvecs, ref, lists, u_ref = case
    u, gs = GPA.extract_displacement_field(img, kvecs, wfr_func=func, return_gs=True)
    # exactly one driver call, gradients requested, plain np.gradient stencil; no per-peak sweep, no separate unwrap
    assert recorded == [('extract', np.dtype(plan_dtype), True, False, 0)]
    f32 = plan_dtype is np.float32
    assert u.dtype == np.float64 and u.shape == (2,) + img.shape
    assert np.abs(u - u_ref).max() <= (1e-5 if f32 else 0) * np.abs(u_ref).max()
    assert len(gs) == len(kvecs)
    for p, g in enumerate(gs):
        assert set(g) == keys
        assert g['lockin'].dtype == (np.complex64 if f32 else np.complex128)
        assert g['grad'].dtype == (np.float32 if f32 else np.float64) and g['grad'].shape == img.shape + (2,)
        assert np.allclose(g['lockin'], ref[p]['lockin'], rtol=0, atol=(1e-6 if f32 else 0) * np.abs(ref[p]['lockin']).max())
        assert np.allclose(g['grad'], ref[p]['grad'], rtol=0, atol=1e-6 if f32 else 0)
        if 'kidx' in keys:
            assert np.array_equal(g['kidx'], ref[p]['kidx'])
        if 'w' in keys:
            # 'w' is built from the winners and the (padded) k-list of the peak
            kidx = ref[p]['kidx']
            w = np.zeros((2,) + img.shape)
            won = kidx >= 0
            w[0][won], w[1][won] = lists[p][kidx[won], 0], lists[p][kidx[won], 1]
            assert np.array_equal(g['w'], w) and np.array_equal(g['w'], ref[p]['w'])


def test_padded_lists_build_w_from_the_padded_list(recorded, case):
    """k-lists of unequal length are padded with repeats of their last candidate; 'w' follows the padded list"""
    import pygpa_amd.geometric_phase_analysis as GPA
    img, kvecs, ref, lists, _ = case
    short = [lists[0][:5], lists[1], lists[2][:7]]
    u, gs = GPA.extract_displacement_field(img, kvecs, wfr_func=GPA.wfr2_grad_opt, return_gs=True, klists=short)
    assert [c[0] for c in recorded] == ['extract'] and recorded[0][2]
    for p, g in enumerate(gs):
        kidx = g['kidx']
        assert kidx.max() < len(short[p])         # a repeat never wins a strict '>'
        assert np.array_equal(g['w'][0], short[p][kidx, 0]) and np.array_equal(g['w'][1], short[p][kidx, 1])


@pytest.mark.parametrize('which', range(4))
def test_without_return_gs_no_gradients(recorded, case, which):
    import pygpa_amd.geometric_phase_analysis as GPA
    func, _, plan_dtype = _routed()[which]
    img, kvecs, _, _, u_ref = case
    u = GPA.extract_displacement_field(img, kvecs, wfr_func=func)
    assert recorded == [('extract', np.dtype(plan_dtype), False, False, 0)]
    assert u.dtype == np.float64
    assert np.abs(u - u_ref).max() <= (1e-5 if plan_dtype is np.float32 else 0) * np.abs(u_ref).max()


def test_optwfr2_keeps_the_fused_path(recorded, case):
    import pygpa_amd.geometric_phase_analysis as GPA
    img, kvecs, ref, _, _ = case
    u, gs = GPA.extract_displacement_field(img, kvecs, return_gs=True)
    assert recorded == [('extract', np.dtype(np.float64), False, False, 0)]
    for p, g in enumerate(gs):
        assert set(g) == {'lockin', 'w', 'kidx'}
        assert np.array_equal(g['kidx'], ref[p]['kidx'])


def test_other_callables_take_the_old_branch(recorded, case):
    import pygpa_amd.geometric_phase_analysis as GPA
    from pygpa_amd import cuGPA
    img, kvecs, _, _, _ = case

    def mine(image, sigma, kx, ky, kw, kstep):
        return GPA.wfr2_grad_opt(image, sigma, kx, ky, kw, kstep)

    for func in (functools.partial(cuGPA.wfr2_grad_opt), functools.partial(cuGPA.wfr2_grad_opt, grad='diff'),
                 functools.partial(GPA.wfr2_grad_opt), mine):
        del recorded[:]
        u, gs = GPA.extract_displacement_field(img, kvecs, wfr_func=func, return_gs=True)
        names = [c[0] for c in recorded]
        assert names == ['sweep'] * 3 + ['reconstruct_grad', 'unwrap_prediff', 'unwrap_prediff'], names
        assert all('grad' in g for g in gs)


def test_plan_methods_take_the_new_arguments():
    """the binding layer: new keywords exist, old positional call sites keep their meaning"""
    import inspect
    sig = inspect.signature(_lib.Plan.extract_displacement_field)
    assert list(sig.parameters)[:10] == ['self', 'image', 'kvecs', 'klists', 'sigma', 'mask_border', 'kmax', 'want_lockins',
                                         'want_kidx', 'out']
    for name, default in (('want_grads', False), ('want_weights', False), ('grad_mode', 0)):
        assert sig.parameters[name].default == default
    for meth in (_lib.Plan.extract_displacement_field_dev, _lib.Plan.extract_displacement_field_async):
        sig = inspect.signature(meth)
        assert list(sig.parameters)[:10] == ['self', 'image_ptr', 'kvecs', 'klists', 'sigma', 'mask_border', 'kmax', 'u_ptr',
                                             'lockins_ptr', 'kidx_ptr']
        for name, default in (('grads_ptr', None), ('weights_ptr', None), ('grad_mode', 0)):
            assert sig.parameters[name].default == default
    assert C.sizeof(C.c_void_p) == 8
