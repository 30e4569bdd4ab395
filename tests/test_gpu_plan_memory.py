"""The plan's grown buffers (csrc/gpa_devbuf.h): regrowing one changes no result, gpa_plan_workspace_bytes counts them and
repeating a call allocates nothing.  Run with `-m gpu` on an MI355X.

tests/test_gpu_plan_state.py draws its sequences; this one is fixed so that every grow-on-demand buffer of the plan does grow
on the long-lived plan: the x-planes past their initial four (a sweep of 2 planes, then one of 6), the phase scratch of the
gradient form, the Lawler-Fujita scratch, the DFT work and the Gaussian-FFT tables (two sigmas, then a third that evicts a
slot), the unit-cell scratch and staging, the iterate_GPA scratch of a plan and its cropped plan, the batched driver's buffers.
Every result is compared bit for bit with the same call on a fresh plan that runs only that call."""
import numpy as np
import pytest

from pygpa_amd import _lib
from pygpa_amd import unit_cell_averaging as uc
from pygpa_amd.synthetic import hex_kvecs, explicit_klists, gaussian_bump_displacement, hex_moire

from test_gpu_plan_state import same

pytestmark = pytest.mark.gpu

MAX_BATCH = 18
EDGE = 3


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('shape', [(64, 64), (96, 80)])
def test_regrown_buffers_same_bits_counted_and_stable(shape, dtype):
    n0, n1 = shape
    item = np.dtype(dtype).itemsize
    kv = hex_kvecs(0.12, 11.0)
    kw = np.linalg.norm(kv, axis=1).mean() / 2.5
    l2 = explicit_klists(kv, kw, 2, 2)[0]                       # 2 x-planes
    l6 = explicit_klists(kv, kw, 6, 2)[0]                       # 6: more than the four the plan starts with
    l22 = np.stack(explicit_klists(kv, kw, 2, 2))
    imgs = [hex_moire(shape, kv, gaussian_bump_displacement(shape), noise=0.1, seed=s) for s in (1, 2, 3)]
    imgs = [(im - im.mean()).astype(dtype) for im in imgs]
    img = imgs[0]
    x, y = np.meshgrid(np.arange(n0) - n0 / 2, np.arange(n1) - n1 / 2, indexing='ij')
    u = np.stack([1.5 * np.exp(-(x ** 2 + y ** 2) / (0.1 * n0 * n1)), 0.8 * np.sin(y / 9.0)]).astype(dtype)
    rmin, rsize = uc.calc_ucell_parameters(kv[:2], 2)
    geom = _lib.UcellGeom.make(kv[:2], np.linalg.inv(kv[:2]), rmin, rsize, 2)
    d_imgs = _lib.DeviceBuffer(3 * n0 * n1 * item)
    d_imgs.upload(np.stack(imgs))
    win = (n0 - 2 * EDGE, n1 - 2 * EDGE)

    def batch(p, crop):
        out = _lib.DeviceBuffer(3 * 2 * n0 * n1 * item)
        try:
            it = p.extract_displacement_field_batch_dev(d_imgs.ptr, 3, kv, l22, 6.0, 3, 5, out.ptr)
            return out.download((3, 2) + shape, dtype), it
        finally:
            out.free()

    calls = [
        ('sweep of 2 planes', lambda p, crop: p.sweep(img, kv[0], l2, 6.0)),
        ('sweep of 6 planes', lambda p, crop: p.sweep(img, kv[0], l6, 6.0)),
        ('gradient sweep', lambda p, crop: p.sweep(img, kv[0], l6, 6.0, want_grad=True)),
        ('undistort', lambda p, crop: p.undistort_image(img, u)),
        ('find_peaks, two sigmas', lambda p, crop: p.find_peaks(img, 3.0, 4.0, 0.05, want_smooth=True)),
        ('find_peaks, a third sigma', lambda p, crop: p.find_peaks(img, 5.0, 0.0, 0.05, want_smooth=True)),
        ('unit-cell average', lambda p, crop: p.unit_cell_average(img, geom, u, want_weights=True)),
        ('iterate_gpa', lambda p, crop: p.iterate_gpa(img, kv, 6.0, edge=EDGE, iters=1, kmax_iter=4, kmax=6, crop_plan=crop)),
        # (the single-image driver first: the workspaces of its two unwraps are then there, and what the batched call adds is its own)
        ('extract', lambda p, crop: p.extract_displacement_field(img, kv, l22, 6.0, 3, kmax=5)),
        ('batched extract', batch),
    ]
    plan, crop = _lib.Plan(shape, MAX_BATCH, dtype), _lib.Plan(win, 1, dtype)
    try:
        assert plan.lib.gpa_supports_batch(plan.handle) != 0
        grew = {}
        for name, fn in calls:
            before = plan.workspace_bytes + crop.workspace_bytes
            got = fn(plan, crop)
            ws = plan.workspace_bytes, crop.workspace_bytes
            grew[name] = sum(ws) - before
            again = fn(plan, crop)
            assert (plan.workspace_bytes, crop.workspace_bytes) == ws, '%s: repeating the call changed workspace_bytes' % name
            fresh, fresh_crop = _lib.Plan(shape, MAX_BATCH, dtype), _lib.Plan(win, 1, dtype)
            try:
                want = fn(fresh, fresh_crop)
            finally:
                fresh.close()
                fresh_crop.close()
            assert same(got, want), '%s: the result depends on the plan history' % name
            assert same(again, want), '%s: the repeated call differs' % name
        # the buffers every one of these calls needs beyond what the calls before it left are counted
        assert grew['sweep of 6 planes'] >= 2 * n0 * n1 * 2 * item           # x-planes 5 and 6
        # a phase per candidate and the gradient staging by the end of the gradient sweep (the sweeps before it may have
        # grown the same scratch already: the split pass B of small images borrows it)
        swept = grew['sweep of 2 planes'] + grew['sweep of 6 planes'] + grew['gradient sweep']
        assert swept >= 2 * n0 * n1 * 2 * item + len(l6) * n0 * n1 * item + 2 * n0 * n1 * item
        assert grew['undistort'] > 0 and grew['unit-cell average'] > 0 and grew['iterate_gpa'] > 0
        assert grew['find_peaks, two sigmas'] > 0
        # the batched driver: the weights of the three frames alone are 3 n0 n1 reals (its x-planes, lock-ins and the unwrap
        # workspace of the six problems come on top)
        assert grew['batched extract'] >= 3 * n0 * n1 * item
    finally:
        plan.close()
        crop.close()
        d_imgs.free()
