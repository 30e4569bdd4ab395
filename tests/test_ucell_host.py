"""CPU checks of the unit-cell averaging mirror (pygpa_amd.unit_cell_averaging): its host helpers equal the reference's
values recorded in tests/golden/ucell_*.npz, and the library exports the unit-cell entry points."""
import os

import numpy as np
import pytest

from pygpa_amd import _lib
from pygpa_amd import unit_cell_averaging as uc
from pygpa_amd.synthetic import hex_kvecs

CASES = ['hex200_z2', 'hex200_z3', 'def200_z3', 'def151x233_z2', 'hex160_rk05_z8']
SYMBOLS = ['gpa_unit_cell_average', 'gpa_unit_cell_average_dev', 'gpa_unit_cell_average_batch_dev',
           'gpa_expand_unitcell', 'gpa_expand_unitcell_dev']


@pytest.mark.parametrize('name', CASES)
def test_host_helpers_match_reference(golden, name):
    g = golden('ucell_' + name)
    ks = hex_kvecs(float(g['r_k']), 7.0, 3)[:2]
    rmin, rsize = uc.calc_ucell_parameters(ks, int(g['z']))
    assert np.array_equal(rmin, g['rmin'])
    assert tuple(rsize) == tuple(g['rsize']) == g['res'].shape
    # (per axis without fused operations, as the kernels compute it; the reference's matmul rounds the last bits differently)
    assert np.allclose(uc.cart_in_uc(g['pts'], ks, rmin), g['pts_cart'], rtol=0, atol=1e-11)
    for f, ov in zip(g['fr'], g['fr_overlap']):
        assert np.array_equal(uc.float_overlap(f), ov)


def test_tiny_negative_lattice_coordinate_folds_to_one():
    ks = hex_kvecs(0.02, 7.0, 3)[:2]
    lat = np.array([-1e-300, 0.5])
    assert (lat % 1.)[0] == 1.0           # NumPy's remainder, which the kernels restate
    v = uc.backward_transform(lat, ks)
    assert np.allclose(uc.forward_transform(v, ks), lat, atol=1e-12)


def test_add_to_position_wraps_negative_index():
    res, w = np.zeros((3, 4)), np.zeros((3, 4))
    uc.add_to_position(2.0, np.array([-0.25, 1.5]), res, w)
    # base row -1 -> the last row, as NumPy indexes; float_overlap's layout: the row offset takes the second fraction
    ov = uc.float_overlap(np.array([0.75, 0.5]))
    assert np.allclose(w[-1, 1:3], ov[0]) and np.allclose(w[0, 1:3], ov[1])
    assert np.isclose(res.sum(), 2.0) and np.isclose(w.sum(), 1.0)


def test_geometry_struct_layout():
    ks = hex_kvecs(0.02, 7.0, 3)[:2]
    rmin, rsize = uc.calc_ucell_parameters(ks, 3)
    geo = _lib.UcellGeom.make(ks, np.linalg.inv(ks), rmin, rsize, 3)
    assert list(geo.ks) == list(ks.reshape(4)) and tuple(geo.rsize) == tuple(rsize) and geo.z == 3.0
    # double ks[4], kinv[4], rmin[2]; int32 rsize[2]; double z
    assert _lib.C.sizeof(_lib.UcellGeom) == 10 * 8 + 8 + 8


def test_unit_cell_symbols_exported():
    if not os.path.exists(_lib.LIB_PATH):
        from pygpa_amd import build
        build.build(verbose=False)
    lib = _lib.load()
    for name in SYMBOLS:
        assert name in _lib.SIGNATURES
        assert hasattr(lib, name)
    for name in uc.__all__:
        assert callable(getattr(uc, name))
