"""gpa_gradients_jacobian: phase gradients and weights of a stack -> J and lattice properties in one pass, without a plan.
J is held to Plan.phasegradient2J bit for bit, the properties to props_from_jac(J, add_identity=True) bit for bit, the reference's
numbers (tests/golden/props_64.npz) to the bounds of tests/test_gpu_parity.py::test_f2_jacobian_and_props_golden, and the mirror's
stack functions to the single functions frame by frame.  Run with `-m gpu` on an MI355X."""
import numpy as np
import pytest

import gradjac_cases as gc
from pygpa_amd import _lib
from pygpa_amd import property_extract as pe
from test_gpu_parity import _pdiff

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]


@pytest.fixture(scope='module')
def chain():
    """(J, props) of today's two-kernel chain for one frame, computed once per (dtype, P, shape, dks?, props arguments)"""
    cache = {}

    def get(dtype, P, shape, grads, weights, dks, pargs):
        key = (np.dtype(dtype).name, P, shape, dks is not None, grads.shape[0])
        if key not in cache:
            # phasegradient2J differentiates nothing: a frame below the smallest shape a plan takes (4 x 4) goes through a plan
            # of that shape, padded with pixels nobody compares
            n0, n1 = max(shape[0], 4), max(shape[1], 4)
            plan = _lib.get_plan((n0, n1), max(P, 2), dtype)
            Js = []
            for b in range(grads.shape[0]):
                g = np.zeros((P, n0, n1, 2), dtype=dtype)
                w = np.zeros((P, n0, n1), dtype=dtype)
                g[:, :shape[0], :shape[1]] = grads[b]
                w[:, :shape[0], :shape[1]] = weights[b]
                Js.append(plan.phasegradient2J(gc.kvecs_of(P), g, w, gc.NMPERPIXEL, dks=dks)[:shape[0], :shape[1]])
            cache[key] = np.stack(Js)
        J = cache[key]
        return J, np.stack([_lib.props_from_jac(j, add_identity=True, dtype=dtype, **pargs) for j in J])
    return get


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('nimg', [1, 3])
@pytest.mark.parametrize('P', gc.PEAKS)
@pytest.mark.parametrize('shape', gc.SHAPES)
def test_bits_of_the_two_kernel_chain(chain, shape, P, nimg, dtype):
    """J equals Plan.phasegradient2J, props equals props_from_jac(J, add_identity=True), with and without dks, asking for J only,
    props only and both; the pixel of every frame whose weights are all 0 has J = 0; frames differ, so a wrong frame stride
    cannot pass."""
    grads, weights = gc.inputs(nimg, P, shape, dtype)
    assert nimg == 1 or not np.array_equal(grads[0], grads[1])
    kvecs = gc.kvecs_of(P)
    pargs = dict(refangle=3.0, refscale=2.0, diff=True)
    for dks in (None, gc.dks_of(P)):
        J_ref, props_ref = chain(dtype, P, shape, grads, weights, dks, pargs)
        if dks is not None and shape[0] * shape[1] >= 15:   # the turn has to fold some gradients back, or wrapToPi is not exercised
            assert (np.abs(grads.astype(np.float64) - 2 * np.pi * dks[None, :, None, None, :]) > np.pi).any()
        for want_J, want_props in ((True, False), (False, True), (True, True)):
            J, props = _lib.gradients_jacobian(kvecs, grads, weights, gc.NMPERPIXEL, dks=dks, want_J=want_J, want_props=want_props,
                                               dtype=dtype, **pargs)
            if want_J:
                assert J.dtype == dtype and J.shape == (nimg,) + shape + (2, 2)
                assert np.array_equal(J, J_ref), (shape, P, nimg, dks is not None, float(np.abs(J - J_ref).max()))
                for b in range(nimg):
                    assert not J[(b,) + tuple(gc.zero_pixel(shape, b))].any()
            else:
                assert J is None
            if want_props:
                assert props.dtype == dtype and props.shape == (nimg, 4) + shape
                assert np.array_equal(props, props_ref, equal_nan=True), (shape, P, nimg, dks is not None)
            else:
                assert props is None
    # a single frame without the frame axis, and I + J
    J1, _ = _lib.gradients_jacobian(kvecs, grads[0], weights[0], gc.NMPERPIXEL, dtype=dtype)
    J_ref, _ = chain(dtype, P, shape, grads, weights, None, pargs)
    assert J1.shape == shape + (2, 2) and np.array_equal(J1, J_ref[0])
    Jac, _ = _lib.gradients_jacobian(kvecs, grads[0], weights[0], gc.NMPERPIXEL, add_identity=True, dtype=dtype)
    assert np.array_equal(Jac, J_ref[0] + np.eye(2, dtype=dtype))


@pytest.mark.parametrize('dtype', DTYPES)
def test_device_pointers_unaligned_rows(dtype):
    """the device form on buffers whose bases are not 16-byte aligned (element-wise accesses) equals the host form"""
    from test_gpu_parity import DeviceArray
    P, shape, nimg = 3, (7, 64), 2
    grads, weights = gc.inputs(nimg, P, shape, dtype)
    J_ref, props_ref = _lib.gradients_jacobian(gc.kvecs_of(P), grads, weights, gc.NMPERPIXEL, want_props=True, dtype=dtype)
    item = np.dtype(dtype).itemsize
    pad = np.zeros(2, dtype=dtype)   # weights and props start one pair (8 bytes in f32) into their buffers
    d_g = DeviceArray(grads)
    d_w = DeviceArray(np.concatenate([pad, weights.ravel()]))
    d_J = DeviceArray(np.zeros(J_ref.shape, dtype=dtype))
    d_p = DeviceArray(np.zeros(props_ref.size + 2, dtype=dtype))
    pe.phasegradient2J_dev(gc.kvecs_of(P), d_g.ptr, d_w.ptr + 2 * item, grads.shape, gc.NMPERPIXEL, J_ptr=d_J.ptr,
                           props_ptr=d_p.ptr + 2 * item, iso_ref=False, dtype=dtype)
    out_p = d_p.get()
    assert np.array_equal(d_J.get(), J_ref)
    assert np.array_equal(out_p[2:].reshape(props_ref.shape), props_ref, equal_nan=True) and not out_p[:2].any()


@pytest.mark.parametrize('dtype', DTYPES)
def test_reference_numbers(golden, dtype):
    """props_64 (J, J_iso, props of the reference) to the bounds of test_f2_jacobian_and_props_golden: 1e-11 / 2e-5 of max|J|,
    and for the properties of the J computed here the kappa-dependent bound of the anisotropy angle; the golden frame is the
    second of two, so that a wrong frame stride cannot pass"""
    g = golden('props_64')
    f32 = dtype == np.float32
    bound = 2e-5 if f32 else 1e-11
    grads = np.stack([g['grads'][:, ::-1, ::-1], g['grads']])
    weights = np.stack([g['weights'][:, ::-1], g['weights']])
    J = pe.phasegradient2J_stack(g['kvecs'], grads, weights, 0.5, iso_ref=False, dtype=dtype)
    J_iso = pe.phasegradient2J_stack(g['aniks'], grads, weights, 0.5, dtype=dtype)
    print('J', np.abs(J[1] - g['J']).max() / np.abs(g['J']).max(), 'J_iso', np.abs(J_iso[1] - g['J_iso']).max() / np.abs(g['J_iso']).max())
    assert J.shape == (2,) + g['J'].shape and J.dtype == dtype
    assert np.abs(J[1] - g['J']).max() <= bound * np.abs(g['J']).max()
    assert np.abs(J_iso[1] - g['J_iso']).max() <= bound * np.abs(g['J_iso']).max()
    assert not np.array_equal(J[0], J[1])
    # g['props'] = props_from_J(g['J']): the fused properties of the same gradients, no reference angle (iso_ref=False)
    props = _lib.gradients_jacobian(g['kvecs'], grads, weights, 0.5, want_J=False, want_props=True, dtype=dtype)[1][1]
    ref = g['props']
    kap = ref[3]
    tol_ani = bound * (1 + 1 / (kap - 1)) * 57.3
    assert props.shape == ref.shape
    assert np.all(np.abs(_pdiff(props[0], ref[0], 360)) <= (1e-4 if f32 else 1e-10))
    assert np.all(np.abs(_pdiff(props[1], ref[1], 180)) <= tol_ani)
    assert np.allclose(props[2], ref[2], rtol=1e-5 if f32 else 1e-12, atol=(2e-6 if f32 else 1e-13) * np.abs(ref[2] * kap).max())
    assert np.allclose(props[3], ref[3], rtol=bound * kap.max())


@pytest.mark.parametrize('dtype', DTYPES)
def test_mirror_stack_equals_single_functions(golden, dtype):
    """calc_props_from_phasegradient_stack and phasegradient2J_stack (sort = 0, 1, -1; with and without iso_ref) frame by frame
    against the single functions, bit for bit"""
    g = golden('props_64')
    rng = np.random.default_rng(3)
    grads = np.stack([g['grads'], g['grads'][:, ::-1], g['grads'] + 0.1 * rng.normal(size=g['grads'].shape)])
    weights = np.stack([g['weights'], g['weights'][:, :, ::-1], g['weights'] * rng.random(g['weights'].shape)])
    props = pe.calc_props_from_phasegradient_stack(g['aniks'], grads, weights, 0.5, dtype=dtype)
    assert props.shape == (3, 4) + g['weights'].shape[1:] and props.dtype == dtype
    for b in range(3):
        assert np.array_equal(props[b], pe.calc_props_from_phasegradient(g['aniks'], grads[b], weights[b], 0.5, dtype=dtype),
                              equal_nan=True), b
    for sort in (0, 1, -1):
        for iso_ref in (True, False):
            J = pe.phasegradient2J_stack(g['aniks'], grads, weights, 0.5, iso_ref=iso_ref, sort=sort, dtype=dtype)
            for b in range(3):
                ref = pe.phasegradient2J(g['aniks'], grads[b], weights[b], 0.5, iso_ref=iso_ref, sort=sort, dtype=dtype)
                assert np.array_equal(J[b], ref), (sort, iso_ref, b)
