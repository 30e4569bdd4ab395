"""Inputs of the y-spectral sweep tests (tests/test_gpu_yspec_sweep.py on the GPU, tests/test_yspec_host.py on the CPU): the
three k-list cases of DESIGN 2.1c on the two smallest shapes that reach every index path, with their oracle sweeps computed
once per process, and a mirror of the host's band-rotation arithmetic (gpa_api_tables.hip: shared_prepare)."""
import functools

import numpy as np

from oracle import gpa_oracle as orc
from pygpa_amd.synthetic import hex_kvecs, gaussian_bump_displacement, hex_moire, explicit_klists

SHAPES = [(64, 2048), (96, 4096)]
CASES = ['grid', 'wrap', 'shared']
SIGMA = 10


def band_rotation(klist, sigma, f32):
    """(s, blocks) of one peak's candidate list: the block of L / 16 bins its rotated Gaussian band starts in and the number
    of blocks it covers, as shared_prepare computes them"""
    fc = np.sqrt(np.log(1e9 if f32 else 1e17) / (2.0 * np.pi ** 2 * sigma ** 2))
    wy = np.asarray(klist)[:, 1]
    lo, width = -wy.max() - fc, (wy.max() - wy.min()) + 2 * fc
    flo = (lo - np.floor(lo)) * 16
    return int(np.floor(flo)) % 16, int(np.ceil((flo - np.floor(flo)) + width * 16 + 1e-9))


@functools.lru_cache(maxsize=None)
def case(name, shape):
    """(image, kvecs (P, 2), klists (P, K, 2)) -- 'grid': one peak of the hex lattice, 4 x 4 list; 'wrap': a reference vector
    almost along x, whose rotated band contains DC and so straddles blocks 15 -> 0; 'shared': two peaks with the same k_x (their
    lists share every x-plane) and k_y far apart (different bands, one of which does not wrap: a plane's live-block mask is a union)."""
    if name == 'grid':
        kv, peaks, seed = hex_kvecs(0.1, 7.0), [1], 5
    elif name == 'wrap':
        kv, peaks, seed = hex_kvecs(0.1, 2.0), [0], 6
    else:
        kv, peaks, seed = np.array([[0.08, 0.06], [0.08, -0.3]]), [0, 1], 7
    img = hex_moire(shape, kv, gaussian_bump_displacement(shape), noise=0.2, seed=seed)
    kw = orc.derive_params(hex_kvecs(0.1, 7.0))[0]
    klists = explicit_klists(kv, kw, 4, 4)
    return img, np.asarray(kv)[peaks], np.stack([klists[p] for p in peaks])


@functools.lru_cache(maxsize=None)
def oracle(name, shape):
    """per peak: the oracle's sweep (lock-in, kidx) and the amplitudes of all candidates"""
    img, kvecs, klists = case(name, shape)
    img0 = img - img.mean()
    out = []
    for kref, kl in zip(kvecs, klists):
        ref = orc.sweep(img0, SIGMA, kl, kref, workers=8)
        out.append((ref['lockin'], ref['kidx'], np.abs(orc.lockin_batch(img0, kl, SIGMA, workers=8))))
    return out


def near_ties(amps, rel=1e-5):
    """pixels whose two largest candidate amplitudes agree to `rel` of the larger"""
    top = np.sort(amps, axis=0)[-2:]
    return (top[1] - top[0]) <= rel * top[1]
