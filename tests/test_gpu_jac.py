"""Jacobian and property maps from a displacement field or from phases on the device (gpa_field_jacobian, gpa_phases_jacobian,
gpa_phys_props_from_jac; pygpa_amd.property_extract.u2J, phases2J, calc_props_from_phases, phys_props_from_Jac) against
np.gradient BIT FOR BIT and against the fixtures the reference wrote (tests/golden/jac_*.npz, tools/make_jac_golden.py).
Run with `-m gpu` on an MI355X.

Shapes: axes of two points (edges only), fewer rows than a tile, row lengths that are and are not a multiple of the 16-byte
vector (the two access paths), and a shape read from the tile constants of csrc/gpa_fieldjac.h: two tiles plus a ragged
remainder along both axes, once with an odd row length and once with one that takes the 16-byte path."""
import functools

import numpy as np
import pytest

from pygpa_amd import _lib
import pygpa_amd.property_extract as pe
from pygpa_amd.synthetic import hex_kvecs, hex_moire, explicit_klists

import jac_cases as jc

pytestmark = pytest.mark.gpu
DTYPES = [np.float64, np.float32]
RAGGED = jc.ragged_shape()
RAGGED_WIDE = (RAGGED[0], RAGGED[1] + 1)          # a multiple of the vector: the 16-byte path across more than two tiles
U_SHAPES = jc.U_SHAPES + [RAGGED, RAGGED_WIDE]
H = 0.37                                           # a Python float that neither f32 nor f64 holds exactly


def field(shape, dtype, seed=0):
    """an f32 field, so that the f64 and the f32 run see the same numbers"""
    return jc.field_input(shape, seed).astype(np.float32).astype(dtype)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shape', U_SHAPES)
def test_u2J_is_np_gradient(shape, dtype):
    """every value is one correctly rounded subtraction and one correctly rounded division by the divisor rounded once"""
    assert RAGGED[1] % 4 != 0 and RAGGED_WIDE[1] % 4 == 0
    U = field(shape, dtype, seed=shape[0] + 7 * shape[1])
    for h in (H, 1, 3.7):
        J = pe.u2J(U, h, dtype=dtype)
        assert J.dtype == dtype and J.shape == shape + (2, 2)
        np.testing.assert_array_equal(J, jc.u2J_gradient(U, h))


@pytest.mark.parametrize('dtype', DTYPES)
def test_u2J_nan_is_numpys(dtype):
    U = field((37, 72), dtype, seed=5)
    for c, i, j in [(0, 0, 0), (1, 36, 71), (0, 15, 3), (1, 16, 4), (0, 20, 64), (1, 0, 40)]:
        U[c, i, j] = np.nan
    J, want = pe.u2J(U, H, dtype=dtype), jc.u2J_gradient(U, H)
    assert np.isnan(want).sum() >= 20
    np.testing.assert_array_equal(J, want)               # NaN exactly where NumPy has it, every other pixel to the bit


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shape', [(37, 70), (18, 72)])
def test_u2J_stack_frames_equal_single_calls(shape, dtype):
    us = np.stack([field(shape, dtype, seed=b) for b in range(3)])
    Js = pe.u2J_stack(us, H, dtype=dtype)
    assert Js.shape == (3,) + shape + (2, 2)
    for b in range(3):
        assert np.array_equal(Js[b], pe.u2J(us[b], H, dtype=dtype)), b       # no frame reads another's rows
    np.testing.assert_array_equal(Js[1], jc.u2J_gradient(us[1], H))


class Buffers:
    def __init__(self, **arrays_or_sizes):
        self.b = {}
        for k, v in arrays_or_sizes.items():
            self.b[k] = _lib.DeviceBuffer(v if isinstance(v, int) else v.nbytes)
            if not isinstance(v, int):
                self.b[k].upload(v)

    def __getitem__(self, k):
        return self.b[k].ptr

    def get(self, k, shape, dtype):
        return self.b[k].download(shape, dtype)

    def free(self):
        for b in self.b.values():
            b.free()


def props_from_jac_dev(J_ptr, npx, dtype, props_ptr, refangle=0., refscale=1., diff=False):
    """gpa_props_from_jac_dev(add_identity = 1) on the default stream"""
    _lib.check(_lib.load().gpa_props_from_jac_dev(0, 0 if dtype == np.float32 else 1, npx, _lib._ptr(int(J_ptr)), 1, float(refangle),
                                                  float(refscale), int(diff), _lib._ptr(int(props_ptr)), None), 'gpa_props_from_jac_dev')


def sync():
    d = _lib.DeviceBuffer(8)
    d.download((1,), np.float64)          # a blocking copy on the default stream
    d.free()


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shape', [(37, 70), (37, 72), RAGGED])
def test_u2J_dev_identity_and_fused_props(shape, dtype):
    U = 0.05 * field(shape, dtype, seed=11)
    npx, item = shape[0] * shape[1], np.dtype(dtype).itemsize
    J = pe.u2J(U, H, dtype=dtype)
    assert np.array_equal(J, pe.u2J(U, H, dtype=dtype))                                    # rerun
    Jac = pe.u2Jac(U, H, dtype=dtype)
    assert np.array_equal(Jac, np.eye(2, dtype=dtype) + J)
    d = Buffers(u=U, J=4 * npx * item, p=4 * npx * item, p2=4 * npx * item, p3=4 * npx * item)
    try:
        pe.u2J_dev(d['u'], U.shape, H, J_ptr=d['J'], props_ptr=d['p'], dtype=dtype, refangle=3., refscale=2., diff=True)
        props_from_jac_dev(d['J'], npx, dtype, d['p2'], 3., 2., True)
        pe.u2J_dev(d['u'], U.shape, H, props_ptr=d['p3'], dtype=dtype, refangle=3., refscale=2., diff=True)       # J NULL
        sync()
        assert np.array_equal(d.get('J', J.shape, dtype), J)                               # _dev == host form
        props = d.get('p', (4,) + shape, dtype)
        assert np.isfinite(props).all() and props[3].min() >= 1
        assert np.array_equal(props, d.get('p2', (4,) + shape, dtype))                     # one device function on the same bits
        assert np.array_equal(props, d.get('p3', (4,) + shape, dtype))
        # add_identity changes what is stored in J, not the properties
        pe.u2J_dev(d['u'], U.shape, H, J_ptr=d['J'], props_ptr=d['p3'], add_identity=True, dtype=dtype, refangle=3., refscale=2., diff=True)
        sync()
        assert np.array_equal(d.get('J', J.shape, dtype), Jac) and np.array_equal(props, d.get('p3', (4,) + shape, dtype))
    finally:
        d.free()
    Jh, ph = _lib.field_jacobian(U, H, want_props=True, refangle=3., refscale=2., diff=True, dtype=dtype)
    assert np.array_equal(Jh, J) and np.array_equal(ph, props)


@functools.lru_cache(maxsize=None)
def fixture(name):
    z = jc.load(name)
    for v in z.values():
        v.setflags(write=False)
    return z


def phase_args(z):
    return z['kvecs'], z['phases'], z['weights'], float(z['nmperpixel'])


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name', list(jc.CASES))
def test_phases2J_fixtures(name, dtype):
    z = fixture(name)
    margin, share = jc.seam_margin_and_share(z['phases'])
    assert margin >= jc.SEAM_MARGIN and (share >= jc.WRAP_SHARE or not jc.CASES[name][2])
    J = pe.phases2J(*phase_args(z), dtype=dtype)
    assert J.dtype == dtype and J.shape == z['J'].shape
    dev = np.abs(J - z['J']).max() / np.abs(z['J']).max()
    print('%s %s: |J - reference| = %.3g max|J| (bound %g)' % (name, np.dtype(dtype).name, dev, jc.j_bound(dtype)))
    assert dev <= jc.j_bound(dtype)
    zero_px = jc.CASES[name][3]
    if zero_px is not None:
        assert not J[zero_px].any()                       # every weight zero: J = 0
    assert np.array_equal(pe.phases2Jac(*phase_args(z), dtype=dtype), np.eye(2, dtype=dtype) + J)
    assert np.array_equal(J, pe.phases2J(*phase_args(z), dtype=dtype))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shape', [RAGGED, RAGGED_WIDE])
def test_phases2J_beyond_two_tiles(shape, dtype):
    kvecs, phases, weights, nm = jc.phase_inputs('hex_37x70', shape=shape)
    margin, share = jc.seam_margin_and_share(phases)
    assert margin >= jc.SEAM_MARGIN and share >= jc.WRAP_SHARE
    want = jc.phases2J_np(kvecs, phases, weights, nm)
    J = pe.phases2J(kvecs, phases, weights, nm, dtype=dtype)
    dev = np.abs(J - want).max() / np.abs(want).max()
    print('%s %s: |J - restatement| = %.3g max|J| (bound %g)' % (shape, np.dtype(dtype).name, dev, jc.j_bound(dtype)))
    assert dev <= jc.j_bound(dtype)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name', ['hex_37x70', 'p8_24x20', 'p2_9x2', 'zero_weight_13x11'])
def test_phases_fused_props(name, dtype):
    z = fixture(name)
    kvecs, phases, weights, nm = phase_args(z)
    P, shape = len(kvecs), phases.shape[1:]
    npx, item = shape[0] * shape[1], np.dtype(dtype).itemsize
    d = Buffers(ph=phases.astype(dtype), w=weights.astype(dtype), J=4 * npx * item, p=4 * npx * item, p2=4 * npx * item, p3=4 * npx * item)
    try:
        pe.phases2J_dev(kvecs, d['ph'], d['w'], (P,) + shape, nm, J_ptr=d['J'], props_ptr=d['p'], dtype=dtype, refangle=5.)
        props_from_jac_dev(d['J'], npx, dtype, d['p2'], 5.)
        pe.phases2J_dev(kvecs, d['ph'], d['w'], (P,) + shape, nm, props_ptr=d['p3'], dtype=dtype, refangle=5.)      # J NULL
        sync()
        J, props = d.get('J', shape + (2, 2), dtype), d.get('p', (4,) + shape, dtype)
        assert np.array_equal(J, pe.phases2J(kvecs, phases, weights, nm, dtype=dtype))     # _dev == host form
        assert np.array_equal(props, d.get('p2', (4,) + shape, dtype))                     # one device function on the same bits
        assert np.array_equal(props, d.get('p3', (4,) + shape, dtype))
    finally:
        d.free()


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name', list(jc.CASES))
def test_calc_props_from_phases_fixtures(name, dtype):
    z = fixture(name)
    props = pe.calc_props_from_phases(*phase_args(z), dtype=dtype)
    assert props.dtype == dtype
    jc.check_props(props, z['props'], dtype)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name', list(jc.CASES))
def test_phys_props_fixtures(name, dtype):
    z = fixture(name)
    Jac = np.eye(2) + z['J']
    kap = z['props'][3]
    jc.check_props(pe.phys_props_from_Jac(Jac, poisson_ratio=jc.POISSON, dtype=dtype), z['phys'], dtype, last='epsilon', kappa=kap)
    jc.check_props(pe.phys_props_from_Jac(Jac, refangle=3.0, refscale=2.0, diff=True, poisson_ratio=jc.POISSON, dtype=dtype),
                   z['phys_diff'], dtype, last='epsilon', kappa=kap)
    # the identity added in the kernel is the identity added on the host
    assert np.array_equal(_lib.phys_props_from_jac(Jac - np.eye(2), add_identity=True, dtype=np.float64),
                          pe.phys_props_from_Jac(np.eye(2) + (Jac - np.eye(2)), dtype=np.float64))


@pytest.mark.parametrize('dtype', DTYPES)
def test_resident_chain(dtype):
    """extract_displacement_field of a stack, its u left on the device, through u2J_dev with properties: nothing is downloaded in
    between, and the result equals the host-array route on the downloaded u"""
    B, shape, nm = 2, (64, 64), 0.5
    npx, item = shape[0] * shape[1], np.dtype(dtype).itemsize
    kvecs = hex_kvecs(0.12, 11.0)
    x, y = np.mgrid[:64, :64] / 64. - 0.5
    imgs = np.stack([hex_moire(shape, kvecs, np.stack([(1.5 + b) * np.exp(-8 * (x * x + y * y)), 2. * x * y]), noise=0.05, seed=b)
                     for b in range(B)])
    imgs = (imgs - imgs.mean(axis=(1, 2), keepdims=True)).astype(dtype)
    klists = np.stack(explicit_klists(kvecs, np.linalg.norm(kvecs, axis=1).mean() / 2.5, 2, 2))
    plan = _lib.Plan(shape, klists.shape[0] * klists.shape[1], dtype)
    d = Buffers(img=imgs, u=2 * B * npx * item, J=4 * B * npx * item, p=4 * B * npx * item)
    try:
        plan.extract_displacement_field_batch_dev(d['img'], B, kvecs, klists, 8, 16, 10, d['u'], want_iters=False)
        pe.u2J_dev(d['u'], (B, 2) + shape, nm, J_ptr=d['J'], props_ptr=d['p'], stream=plan.stream(), dtype=dtype)
        plan.sync()
        u = d.get('u', (B, 2) + shape, dtype)
        J, props = d.get('J', (B,) + shape + (2, 2), dtype), d.get('p', (B, 4) + shape, dtype)
    finally:
        d.free()
        plan.close()
    assert np.isfinite(u).all() and np.abs(u).max() > 0.5                # the chain did run
    Jh = pe.u2J_stack(u, nm, dtype=dtype)
    assert np.array_equal(J, Jh)
    np.testing.assert_array_equal(J[1], jc.u2J_gradient(u[1], nm))
    for b in range(B):
        assert np.array_equal(props[b], pe.props_from_J(Jh[b], dtype=dtype)), b


def test_argument_errors_name_the_argument():
    lib = _lib.load()
    buf = jc.error_buffers()
    for base, table in jc.ERROR_TABLES.items():
        for sfx, tail in (('', ()), ('_dev', (None,))):
            f = getattr(lib, base + sfx)
            for args, word in table(_lib._ptr, buf):
                assert f(*((0,) + args + tail)) == -1, (base + sfx, word)
                assert word in _lib.last_error() and (base + sfx + ':') in _lib.last_error(), (word, _lib.last_error())
    assert not any(v.any() for k, v in buf.items() if k != 'k')
    with pytest.raises(ValueError):
        pe.u2J(np.zeros((2, 1, 8)), 0.5)
    with pytest.raises(ValueError):
        pe.phases2J(np.zeros((3, 2)), np.zeros((3, 4, 5)), np.zeros((3, 4, 4)), 0.5)
