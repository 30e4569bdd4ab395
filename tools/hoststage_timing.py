#!/usr/bin/env python
"""Timing of the host-pointer forms that stage through gpa_hoststage.h: image preparation, per-line medians, Kerelsky fits,
Jacobian / property maps.  The other timing tools measure the resident _dev forms; this one measures what a caller with host
arrays pays, copies and allocation included: the host clock around one call, which ends in a stream synchronise.

    python tools/hoststage_timing.py [--size 2048] [--reps 25] [--out profiles/hoststage_timing.txt]
    python tools/hoststage_timing.py --parent DIR ...    # DIR: a built tree of the parent commit (its pygpa_amd package)

With --parent the rows are measured three times in one session, each in a child process of its own: parent, this tree, parent
again.  The parent's run-to-run spread is the margin: a row passes when this tree is not above the parent's slower run by more
than that spread.  Inputs are those of prep_timing.py, axis_timing.py and kerelsky_timing.py; the Jacobian rows take uniform
random fields (the kernels' time does not depend on the values).
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = {'f32': np.float32, 'f64': np.float64}


def measure(fn, reps):
    fn()
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ts)), float(min(ts))


def child(tree, out, n, reps):
    sys.path.insert(0, tree)
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import pygpa_amd
    assert os.path.realpath(os.path.dirname(pygpa_amd.__file__)).startswith(os.path.realpath(tree)), pygpa_amd.__file__
    from pygpa_amd import _lib
    import pygpa_amd.imagetools as IT
    import prep_timing
    import axis_timing
    import kerelsky_timing
    rows = {}
    pimg, pmask = prep_timing.inputs(n)
    aimg, amask = axis_timing.inputs(n, 'smooth')
    rng = np.random.default_rng(1)
    J, A0, x0 = kerelsky_timing.tile_inputs('smooth')
    for name, dt in DTYPES.items():
        plan = _lib.Plan((n, n), 1, dt)
        try:
            x, ax = np.ascontiguousarray(pimg, dtype=dt), np.ascontiguousarray(aimg, dtype=dt)
            frames = rng.integers(100, 4000, size=(8, n, n)).astype(dt)
            frames[:, :n // 16, :] = 0
            rows['prep %s gauss_homogenize sigma 10, VV' % name] = measure(lambda: plan.gauss_homogenize(x, pmask, 10.0, want_vv=True), reps)
            rows['prep %s generate_mask 8 frames r 5' % name] = measure(lambda: IT.generate_mask(frames, 0.0, 5, dtype=dt), reps)
            rows['prep %s mask_bounds' % name] = measure(lambda: plan.mask_bounds(pmask), reps)
            rows['prep %s nan_trim_lims' % name] = measure(lambda: plan.nan_trim_lims(x), reps)
            rows['axis %s homogenize_per_axis sigma 50, mask, profiles' % name] = measure(
                lambda: plan.homogenize_per_axis(ax, 50.0, amask, want_profiles=True), reps)
            rows['axis %s line_nanmedian axis 0, mask' % name] = measure(lambda: plan.line_nanmedian(ax, 0, amask), reps)
        finally:
            plan.close()
        Jt = np.ascontiguousarray(J, dtype=dt)
        rows['kerelsky %s kerelsky_fit 1024^2' % name] = measure(lambda: _lib.kerelsky_fit(Jt, x0, a0=A0, dtype=dt), reps)
        u = rng.uniform(-1, 1, (2, n, n)).astype(dt)
        ph = rng.uniform(-3, 3, (3, n, n)).astype(dt)
        w = rng.uniform(0.1, 1, (3, n, n)).astype(dt)
        kv = np.array([[0.1, 0.02], [-0.03, 0.11], [0.07, -0.09]])
        jac = rng.uniform(-0.05, 0.05, (n, n, 2, 2)).astype(dt)
        rows['jac %s field_jacobian J + props' % name] = measure(lambda: _lib.field_jacobian(u, 0.5, want_J=True, want_props=True, dtype=dt), reps)
        rows['jac %s phases_jacobian J + props' % name] = measure(
            lambda: _lib.phases_jacobian(kv, ph, w, 0.5, want_J=True, want_props=True, dtype=dt), reps)
        rows['jac %s phys_props_from_jac' % name] = measure(lambda: _lib.phys_props_from_jac(jac, add_identity=True, dtype=dt), reps)
        rows['jac %s props_from_jac' % name] = measure(lambda: _lib.props_from_jac(jac, add_identity=True, dtype=dt), reps)
    with open(out, 'w') as f:
        json.dump(rows, f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent', default=None)
    ap.add_argument('--child', default=None, help='internal: measure the tree at this path and write --json')
    ap.add_argument('--json', default=None)
    ap.add_argument('--size', type=int, default=2048)
    ap.add_argument('--reps', type=int, default=25)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'hoststage_timing.txt'))
    a = ap.parse_args()
    if a.child:
        child(a.child, a.json, a.size, a.reps)
        return 0
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    runs = [('this tree', ROOT)]
    if a.parent:
        runs = [('parent, run 1', os.path.abspath(a.parent)), ('this tree', ROOT), ('parent, run 2', os.path.abspath(a.parent))]
    res = []
    for i, (label, tree) in enumerate(runs):
        js = os.path.join(tempfile.mkdtemp(), 'run_%d.json' % i)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', tree, '--json', js, '--size', str(a.size),
                            '--reps', str(a.reps)], timeout=280)
        if r.returncode != 0:
            print('child %s ended with %d: stopping' % (label, r.returncode))
            return 1
        res.append(json.load(open(js)))
        print(label, 'done', flush=True)
    lines = ['Host-pointer forms at %d^2 (Kerelsky: 1024^2), ms of one call by the host clock (the call ends in a stream synchronise): '
             'median of %d after two warm-up calls (minimum in brackets).' % (a.size, a.reps)]
    if not a.parent:
        lines += ['%-52s %8.2f (%7.2f)' % (k, v[0], v[1]) for k, v in res[0].items()]
        res = []
    else:
        lines += ['Three child processes in one session on one GPU, in this order: parent, this tree, parent again.',
                  'margin: the parent\'s slower run plus the spread of its two runs; ok: this tree is not above it.', '',
                  '%-52s %18s %18s %18s %9s  %s' % ('call', 'parent, run 1', 'parent, run 2', 'this tree', 'margin', '')]
    bad = 0
    for k in (res[0] if res else ()):
        p1, new, p2 = res[0][k], res[1][k], res[2][k]
        margin = max(p1[0], p2[0]) + abs(p1[0] - p2[0])
        ok = new[0] <= margin
        bad += not ok
        lines.append('%-52s %8.2f (%7.2f) %8.2f (%7.2f) %8.2f (%7.2f) %9.2f  %s'
                     % (k, p1[0], p1[1], p2[0], p2[1], new[0], new[1], margin, 'ok' if ok else 'SLOWER'))
    if res:
        lines += ['', '%d of %d rows above the margin' % (bad, len(res[0]))]
    text = '\n'.join(lines) + '\n'
    print(text)
    with open(a.out, 'w') as f:
        f.write(text)
    return 0


if __name__ == '__main__':
    sys.exit(main())
