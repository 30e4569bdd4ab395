"""u AND the lattice properties of one image: two sweeps (today's sequence) against the one-sweep driver.

Resident on one GPU, 4096^2 f32, 3 x 16, kmax = 10, the image and k-lists of bench.py's `pipeline_end_to_end`.
    leg A  extract_displacement_field_dev, sweep_grad_dev x 3, lockin_weights_dev, phasegradient2J_dev, props_from_jac_dev
    leg B  extract_displacement_field_dev(..., grads_ptr, weights_ptr), phasegradient2J_dev, props_from_jac_dev
Both legs are warmed up, then alternate A, B, A, B ... in one process; each repetition is timed by the host clock around the
sequence, which ends in one synchronisation of the plan's stream; profiling is off.  Median, quartiles and extremes per leg.
Leg A uses only entry points that exist without the one-sweep driver, so the same script measures a tree that lacks it
(leg B is skipped there).  The host-array plug-in call
    GPA.extract_displacement_field(img, ks, wfr_func=cuGPA.wfr2_grad_opt, return_gs=True)      (f64, host in / host out)
is timed as well, in both kinds of tree.

    python tools/onesweep_timing.py [--reps 100] [--host-reps 3] [--commit HASH] [--out profiles/onesweep_timing.txt]
"""
import argparse
import inspect
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(ts):
    a = np.sort(np.asarray(ts)) * 1e3
    q = lambda f: float(a[int(round(f * (len(a) - 1)))])   # noqa: E731
    return {'n': len(a), 'median_ms': q(0.5), 'q25_ms': q(0.25), 'q75_ms': q(0.75), 'min_ms': float(a[0]), 'max_ms': float(a[-1])}


def fmt(name, s):
    return '%-44s n=%-4d median %8.3f ms   quartiles %8.3f .. %8.3f   min %8.3f  max %8.3f' % (
        name, s['n'], s['median_ms'], s['q25_ms'], s['q75_ms'], s['min_ms'], s['max_ms'])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=4096)
    ap.add_argument('--reps', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--host-reps', type=int, default=3)
    ap.add_argument('--commit', default=None, help='what to call this tree in the report (default: git rev-parse HEAD)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'onesweep_timing.txt'))
    a = ap.parse_args()
    from pygpa_amd import _lib, cuGPA
    import pygpa_amd.geometric_phase_analysis as GPA
    from pygpa_amd.synthetic import hex_kvecs, explicit_klists, gaussian_bump_displacement, hex_moire
    commit = a.commit
    if commit is None:
        try:
            commit = subprocess.run(['git', '-C', ROOT, 'rev-parse', '--short', 'HEAD'], capture_output=True, text=True).stdout.strip()
        except OSError:
            commit = ''
        commit = commit or 'unknown'
    n, P, K, kmax, dt = a.n, 3, 16, 10, np.float32
    img64 = hex_moire((n, n), hex_kvecs(0.1, 7.0), gaussian_bump_displacement((n, n)), noise=0.1, seed=100, dtype=np.float64)
    img = (img64 - img64.mean()).astype(dt)
    s, npx = np.dtype(dt).itemsize, n * n
    plan = _lib.Plan((n, n), P * K, dt, device=0)
    sizes = dict(img=1, u=2, lock=2 * P, grad=2 * P, w=P, J=4, props=4)
    bufs = {k: _lib.DeviceBuffer(v * npx * s) for k, v in sizes.items()}
    bufs['img'].upload(img)
    ks, _ = GPA.extract_primary_ks_dev(plan, bufs['img'].ptr, pix_norm_range=(2, 0.2 * n))
    sigma = int(np.ceil(1 / np.linalg.norm(ks, axis=1).min()))
    kw = np.linalg.norm(ks, axis=1).mean() / 2.5
    klists = np.stack(explicit_klists(ks, kw, 4, 4))
    one_sweep = 'grads_ptr' in inspect.signature(plan.extract_displacement_field_dev).parameters

    def tail():
        plan.phasegradient2J_dev(ks, bufs['grad'].ptr, bufs['w'].ptr, 1.0, bufs['J'].ptr)
        plan.props_from_jac_dev(bufs['J'].ptr, bufs['props'].ptr, add_identity=True)
        plan.sync()

    def leg_a():
        plan.extract_displacement_field_dev(bufs['img'].ptr, ks, klists, sigma, 2 * sigma, kmax, bufs['u'].ptr)
        for p in range(P):
            plan.sweep_grad_dev(bufs['img'].ptr, ks[p], klists[p], sigma, bufs['lock'].ptr + p * 2 * npx * s,
                                bufs['grad'].ptr + p * 2 * npx * s)
        plan.lockin_weights_dev(bufs['lock'].ptr, P, bufs['w'].ptr)
        tail()

    def leg_b():
        plan.extract_displacement_field_dev(bufs['img'].ptr, ks, klists, sigma, 2 * sigma, kmax, bufs['u'].ptr,
                                            grads_ptr=bufs['grad'].ptr, weights_ptr=bufs['w'].ptr)
        tail()

    legs = [('A two sweeps', leg_a)] + ([('B one sweep', leg_b)] if one_sweep else [])
    for _ in range(a.warmup):
        for _, f in legs:
            f()
    times = {name: [] for name, _ in legs}
    for _ in range(a.reps):
        for name, f in legs:
            t = time.perf_counter()
            f()
            times[name].append(time.perf_counter() - t)
    props = {}
    for name, f in legs:       # what each leg leaves behind, for the record: the two routes give the same properties
        f()
        props[name] = bufs['props'].download((4, n, n), dt)
    plan.close()
    for b in bufs.values():
        b.free()
    lines = ['tree %s   %d^2 f32, %d x %d, kmax %d, sigma %d, resident' % (commit, n, P, K, kmax, sigma)]
    res = {name: stats(ts) for name, ts in times.items()}
    for name, _ in legs:
        lines.append(fmt('leg ' + name, res[name]))
    if one_sweep:
        ratio = res['B one sweep']['median_ms'] / res['A two sweeps']['median_ms']
        lines.append('median B / median A = %.3f' % ratio)
        pa, pb = props['A two sweeps'].astype(np.float64), props['B one sweep'].astype(np.float64)
        lines.append('properties, B against A: median |d kappa| %.2e, median |d alpha| %.2e'
                     % (np.median(np.abs(pa[3] - pb[3])), np.median(np.abs(pa[2] - pb[2]))))
    else:
        lines.append('leg B: this tree has no one-sweep driver')
    # host arrays in, host arrays out, f64: the reference's plug-in call with the per-peak results
    ts = []
    for i in range(a.host_reps + 1):
        t = time.perf_counter()
        u, gs = GPA.extract_displacement_field(img64, ks, wfr_func=cuGPA.wfr2_grad_opt, return_gs=True)
        if i:                   # (the first call builds the plan and its tables)
            ts.append(time.perf_counter() - t)
        del u, gs
    lines.append(fmt('host plug-in call, f64, return_gs', stats(ts)))
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'a') as f:
        f.write(text)


if __name__ == '__main__':
    main()
