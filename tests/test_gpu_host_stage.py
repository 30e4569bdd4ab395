"""One staging buffer under every host-pointer form of wff, image preparation, the per-line medians and the unit-cell calls
(gpa_plan::host_stage, csrc/gpa_hoststage.h).  Run with `-m gpu` on an MI355X.

One plan of shape (20, 12) makes all of these calls in turn and then again in reverse order, so that every family runs once on
a buffer another family left larger.  A real plane is 960 bytes in f32 and 1920 in f64, a mask 240: none is a multiple of the
256 bytes the slots are aligned to, so a wrong offset overlaps a neighbour.  Every result of both passes must equal, bit for
bit, the same call on a fresh plan that makes only that call; the second pass must leave workspace_bytes alone; and the fused
driver must return the same bits before and after."""
import numpy as np
import pytest

from pygpa_amd import _lib
from pygpa_amd import unit_cell_averaging as uc
from pygpa_amd.synthetic import hex_kvecs, explicit_klists, gaussian_bump_displacement, hex_moire

import prep_cases as pc
import wff_cases as wc
from test_gpu_plan_state import same

pytestmark = pytest.mark.gpu

SHAPE = (20, 12)
MAX_BATCH = 12


def _calls(dtype):
    """[(name, fn(plan))] in the order of the first pass, and the driver call"""
    n0, n1 = SHAPE
    rng = np.random.default_rng(5)
    img = pc.lattice_image(SHAPE, 3).astype(dtype)
    mask = pc._disk_at(SHAPE, 8, 5, 4) | pc._disk_at(SHAPE, 16, 9, 2)
    holes = rng.random(SHAPE) >= 0.1
    holes[0, :] = holes[:, 0] = True                             # no empty line
    frames = np.stack([img, img[::-1] * 1.25, img[:, ::-1] + 7.0])
    nanimg = img.copy()
    nanimg[0] = nanimg[7] = nanimg[:, 11] = nanimg[3, 5] = np.nan
    counts = rng.integers(0, 6, size=(3,) + SHAPE).astype(dtype)     # about a sixth of the samples equal 0
    hit = (rng.random(SHAPE) < 0.1).astype(np.uint8)
    phasor = wc.noisy_phasor(SHAPE, 9)
    ws = wc.freq_list(3.0, -1.0, 1.0)
    kv = hex_kvecs(0.25, 11.0)
    kw = np.linalg.norm(kv, axis=1).mean() / 2.5
    klists = np.stack(explicit_klists(kv, kw, 2, 2))
    moire = hex_moire(SHAPE, kv, gaussian_bump_displacement(SHAPE), noise=0.1, seed=1)
    moire = (moire - moire.mean()).astype(dtype)
    x, y = np.meshgrid(np.arange(n0) - n0 / 2, np.arange(n1) - n1 / 2, indexing='ij')
    u = np.stack([0.8 * np.exp(-(x ** 2 + y ** 2) / (0.1 * n0 * n1)), 0.4 * np.sin(y / 3.0)]).astype(dtype)
    rmin, rsize = uc.calc_ucell_parameters(kv[:2], 2)
    geom = _lib.UcellGeom.make(kv[:2], np.linalg.inv(kv[:2]), rmin, rsize, 2)
    cell = rng.random(tuple(rsize))
    calls = [
        ('wff', lambda p: p.wff(phasor, 3.0, ws, ws, [0.4, 1.5], wc.scale_of(3.0))),
        ('gauss_homogenize', lambda p: p.gauss_homogenize(img, mask, 1.5, want_vv=True)),
        ('homogenize_per_axis', lambda p: p.homogenize_per_axis(frames, 2.0, holes, want_profiles=True)),
        ('line_nanmedian 0', lambda p: p.line_nanmedian(img, 0, holes)),
        ('line_nanmedian 1', lambda p: p.line_nanmedian(img, 1, holes)),
        ('mask_any_equal', lambda p: p.mask_any_equal(counts, 0.0, hit=hit)),
        ('mask_erode_disk', lambda p: p.mask_erode_disk(mask, 1)),
        ('mask_bounds', lambda p: p.mask_bounds(mask)),
        ('nan_lines', lambda p: p.nan_lines(nanimg)),
        ('nan_trim_lims', lambda p: p.nan_trim_lims(nanimg)),
        ('unit_cell_average', lambda p: p.unit_cell_average(moire, geom, u, want_weights=True)),
        ('expand_unitcell', lambda p: p.expand_unitcell(cell, geom, 1, u)),
    ]
    return calls, lambda p: p.extract_displacement_field(moire, kv, klists, 2.0, 1, kmax=3)


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_host_forms_share_one_staging_buffer(dtype):
    calls, driver = _calls(dtype)
    want = {}
    for name, fn in calls:
        fresh = _lib.Plan(SHAPE, MAX_BATCH, dtype)
        try:
            want[name] = fn(fresh)
        finally:
            fresh.close()
    plan = _lib.Plan(SHAPE, MAX_BATCH, dtype)
    try:
        before = driver(plan)
        for name, fn in calls:
            assert same(fn(plan), want[name]), '%s: the first pass differs from a fresh plan' % name
        grown = plan.workspace_bytes
        for name, fn in reversed(calls):
            assert same(fn(plan), want[name]), '%s: the reversed pass differs from a fresh plan' % name
        assert plan.workspace_bytes == grown
        assert same(driver(plan), before)
    finally:
        plan.close()
