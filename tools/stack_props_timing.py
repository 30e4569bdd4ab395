#!/usr/bin/env python
"""Property maps per frame of a stack, resident data, on one GPU: the stack driver with gradients followed by the one-pass
gradients -> properties kernel, against a loop over the single-image calls.

    python tools/stack_props_timing.py [--cases 512x16 1024x8 2048x2] [--reps 20] [--kernel-size 4096] [--out profiles/stack_props_timing.txt]

3 peaks x 16 candidates (4 x 4 lists), kmax = 10, f32 and f64; frames, u, gradients, weights and properties stay on the device.
  (a) stack : extract_displacement_field_grad_batch_dev (grads and |lock-in|) + gradients_jacobian_dev (properties only)
  (b) loop  : per frame extract_displacement_field_dev (grads and |lock-in|) + phasegradient2J_dev + props_from_jac_dev
Both run in this process on the same plan, alternating, after two warm-up rounds; a repetition is a host clock around the calls
and the synchronisation that ends them.  Reported: the median of --reps repetitions and max - min as the spread, per frame rate.
The outputs of (a) and (b) are compared once (the properties bit for bit).
Then the one-pass kernel alone against jacobian_kernel + props_kernel at --kernel-size squared (HIP events on the plan's stream),
beside its byte model: 3 P reals in and 4 out per pixel for the properties alone (+ 4 with J), against 3 P + 12 of the chain,
at the stream rate of 6300 GB/s.  There is no pass mark.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pygpa_amd import _lib                                                     # noqa: E402
import pygpa_amd.property_extract as pe                                        # noqa: E402
from pygpa_amd.geometric_phase_analysis import calc_diff_from_isotropic       # noqa: E402
from pygpa_amd.synthetic import explicit_klists, gaussian_bump_displacement, hex_kvecs, hex_moire   # noqa: E402

STREAM_GBS = 6300.0
DTYPES = {'f32': np.float32, 'f64': np.float64}
NM = 0.5
P = 3


def stats(ts):
    return float(np.median(ts)), float(np.max(ts) - np.min(ts))


def stack_case(n, B, name, reps, say):
    dt = DTYPES[name]
    item = np.dtype(dt).itemsize
    kvecs = hex_kvecs(0.1, 7.0)
    sigma = int(np.ceil(1 / np.linalg.norm(kvecs, axis=1).min()))
    kw = np.linalg.norm(kvecs, axis=1).mean() / 2.5
    klists = np.stack(explicit_klists(kvecs, kw, 4, 4))
    dks = calc_diff_from_isotropic(kvecs)
    _, theta_0, _ = pe.get_initial_props(kvecs)
    frames = np.stack([hex_moire((n, n), kvecs, (0.5 + 0.1 * i) * gaussian_bump_displacement((n, n)), noise=0.1, seed=1 + i, dtype=dt)
                       for i in range(B)])
    npx = n * n
    plan = _lib.Plan((n, n), P * 16, dt, device=0)
    sizes = dict(img=B * npx, u=2 * B * npx, g=2 * P * B * npx, w=P * B * npx, J=4 * npx, pa=4 * B * npx, pb=4 * B * npx)
    d = {k: _lib.DeviceBuffer(v * item) for k, v in sizes.items()}
    try:
        d['img'].upload(frames)

        def stack():
            plan.extract_displacement_field_grad_batch_dev(d['img'].ptr, B, kvecs, klists, sigma, 2 * sigma, 10, d['u'].ptr,
                                                           grads_ptr=d['g'].ptr, weights_ptr=d['w'].ptr, want_iters=False)
            pe.phasegradient2J_dev(kvecs, d['g'].ptr, d['w'].ptr, (B, P, n, n, 2), NM, props_ptr=d['pa'].ptr, refangle=theta_0,
                                   stream=plan.stream(), dtype=dt)
            plan.sync()

        def loop():
            for f in range(B):
                g, w = d['g'].ptr + f * 2 * P * npx * item, d['w'].ptr + f * P * npx * item
                plan.extract_displacement_field_dev(d['img'].ptr + f * npx * item, kvecs, klists, sigma, 2 * sigma, 10,
                                                    d['u'].ptr + f * 2 * npx * item, grads_ptr=g, weights_ptr=w)
                plan.phasegradient2J_dev(kvecs, g, w, NM, d['J'].ptr, dks=dks)
                plan.props_from_jac_dev(d['J'].ptr, d['pb'].ptr + f * 4 * npx * item, add_identity=True, refangle=theta_0)
            plan.sync()

        for _ in range(2):
            stack()
            loop()
        pa, pb = np.empty((B, 4, n, n), dtype=dt), np.empty((B, 4, n, n), dtype=dt)
        d['pa'].download_into(pa)
        d['pb'].download_into(pb)
        same = np.array_equal(pa, pb, equal_nan=True)
        ta, tb = [], []
        for _ in range(reps):
            for fn, ts in ((stack, ta), (loop, tb)):
                t0 = time.perf_counter()
                fn()
                ts.append((time.perf_counter() - t0) * 1e3)
        (ma, sa), (mb, sb) = stats(ta), stats(tb)
        say('%s %5d^2 x %2d  (a) stack %8.3f ms (spread %6.3f)  %6.0f Mpix/s   (b) loop %8.3f ms (spread %6.3f)  %6.0f Mpix/s   '
            'b - a = %7.3f ms, loop / stack = %.2f; properties %s'
            % (name, n, B, ma, sa, B * npx / ma / 1e3, mb, sb, B * npx / mb / 1e3, mb - ma, mb / ma,
               'equal bit for bit' if same else 'DIFFER: max |a - b| = %.3g' % float(np.nanmax(np.abs(pa - pb)))))
    finally:
        for b in d.values():
            b.free()
        plan.close()


def kernel_case(n, name, reps, say):
    dt = DTYPES[name]
    item = np.dtype(dt).itemsize
    kvecs = hex_kvecs(0.1, 7.0)
    dks = calc_diff_from_isotropic(kvecs)
    rng = np.random.default_rng(2)
    grads = rng.uniform(-np.pi, np.pi, size=(P, n, n, 2)).astype(dt)
    weights = (0.1 + rng.random((P, n, n))).astype(dt)
    plan = _lib.Plan((n, n), P, dt, device=0)
    npx = n * n
    d = {k: _lib.DeviceBuffer(v * item) for k, v in dict(g=2 * P * npx, w=P * npx, J=4 * npx, p=4 * npx).items()}
    try:
        d['g'].upload(grads)
        d['w'].upload(weights)

        def one_pass(want_J):
            pe.phasegradient2J_dev(kvecs, d['g'].ptr, d['w'].ptr, (P, n, n, 2), NM, J_ptr=d['J'].ptr if want_J else None,
                                   props_ptr=d['p'].ptr, stream=plan.stream(), dtype=dt)

        def chain():
            plan.phasegradient2J_dev(kvecs, d['g'].ptr, d['w'].ptr, NM, d['J'].ptr, dks=dks)
            plan.props_from_jac_dev(d['J'].ptr, d['p'].ptr, add_identity=True)

        runs = (('one pass, props', lambda: one_pass(False), 3 * P + 4), ('one pass, J + props', lambda: one_pass(True), 3 * P + 8),
                ('jacobian_kernel + props_kernel', chain, 3 * P + 12))
        for label, fn, reals in runs:
            fn()
            plan.sync()
            ts = []
            for _ in range(reps):
                plan.timer_start()
                fn()
                ts.append(plan.timer_stop())
            med, spread = stats(ts)
            mb = reals * npx * item / 1e6
            floor = mb / 1e3 / STREAM_GBS * 1e3
            say('%s %5d^2  %-31s %7.4f ms (spread %6.4f); byte model %2d reals = %5.0f MB = %6.4f ms: %4.1f %% of the stream rate'
                % (name, n, label, med, spread, reals, mb, floor, 100 * floor / med))
    finally:
        for b in d.values():
            b.free()
        plan.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', nargs='*', default=['512x16', '1024x8', '2048x2'])
    ap.add_argument('--dtypes', nargs='*', default=['f32', 'f64'])
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--kernel-size', type=int, default=4096)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'stack_props_timing.txt'))
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say('property maps per frame of a resident stack, 3 peaks x 16 candidates, kmax = 10; median of %d repetitions, spread = max - min'
        % args.reps)
    for name in args.dtypes:
        for case in args.cases:
            n, B = (int(v) for v in case.split('x'))
            stack_case(n, B, name, args.reps, say)
    say('the one-pass kernel alone (gpa_gradients_jacobian_dev, P = 3, iso_ref) against jacobian_kernel + props_kernel')
    for name in args.dtypes:
        kernel_case(args.kernel_size, name, args.reps, say)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
