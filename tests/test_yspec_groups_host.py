"""Host side of the grouped y-spectral pass A, no GPU: yspec_groups of pygpa_amd/csrc/gpa_yspec.h cuts the
(plane, block) pairs of a staged list into groups of at most YSPEC_GROUP planes that read one block
(tests/host/yspec_groups_check.cpp: every band rotation, NBL = 6 and 8, one to three peaks that do and do not share planes, caps
1, 3, 4, 6, 12 and 16), and the groups of the benchmark's own lists (bench.py: hex lattice, 3 peaks x 4 x 4, sigma 10)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import yspec_cases as yc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_exe(directory):
    """tests/host/yspec_groups_check.cpp compiled into `directory` (None without g++)"""
    gxx = shutil.which('g++')
    if gxx is None:
        return None
    path = os.path.join(str(directory), 'yspec_groups_check')
    src = os.path.join(ROOT, 'tests', 'host', 'yspec_groups_check.cpp')
    subprocess.run([gxx, '-O2', '-std=c++17', '-I', os.path.join(ROOT, 'pygpa_amd', 'csrc'), src, '-o', path], check=True)
    return path


@pytest.fixture(scope='module')
def exe(tmp_path_factory):
    path = build_exe(tmp_path_factory.mktemp('yspec_groups'))
    if path is None:
        pytest.skip('g++ not available')
    return path


def test_groups_cover_every_pair_once(exe):
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:]
    assert out.stdout.strip().endswith('OK')


def _bench_rotations(f32):
    from pygpa_amd.synthetic import hex_kvecs, explicit_klists
    kvecs = hex_kvecs(0.1, 7.0)
    sigma = int(np.ceil(1 / np.linalg.norm(kvecs, axis=1).min()))
    kw = np.linalg.norm(kvecs, axis=1).mean() / 2.5
    return [yc.band_rotation(kl, sigma, f32)[0] for kl in explicit_klists(kvecs, kw, 4, 4)]


def groups_of(exe, nbl, cap, rotations, lg=12):
    """(entries, [(block, count)] in list order) of peaks with these band rotations on four x-planes each"""
    out = subprocess.run([exe, str(lg), str(nbl), str(cap), '4'] + [str(s) for s in rotations], capture_output=True, text=True,
                         timeout=60, check=True).stdout.split('\n')
    entries = int(out[0].split()[1])
    return entries, [tuple(int(v) for v in line.split()) for line in out[1:] if line.strip()]


def test_benchmark_lists(exe):
    """4096-point rows, three peaks on four x-planes each: f32 (6 live blocks per peak) reads 7 blocks by 12, 12, 4, 8, 12, 12, 12
    planes = 72 pairs; f64 (8 live blocks) 10 blocks and 96 pairs.  An uncapped list is one group per block; cap 4 cuts the f32
    list into 18 groups of four, cap 6 into eleven of six, one of four (block 2) and one of two (the rest of block 12)."""
    entries, groups = groups_of(exe, 6, 16, _bench_rotations(True))
    assert entries == 72
    assert [c for _, c in sorted(groups)] == [12, 12, 4, 8, 12, 12, 12]
    assert [b for b, _ in sorted(groups)] == [0, 1, 2, 12, 13, 14, 15]
    assert [c for _, c in groups] == sorted((c for _, c in groups), reverse=True)
    entries, groups = groups_of(exe, 6, 4, _bench_rotations(True))
    assert entries == 72 and [c for _, c in groups] == [4] * 18
    entries, groups = groups_of(exe, 6, 6, _bench_rotations(True))
    assert entries == 72 and [c for _, c in groups] == [6] * 11 + [4, 2]
    entries, groups = groups_of(exe, 8, 16, _bench_rotations(False))
    assert entries == 96
    assert [c for _, c in sorted(groups)] == [12, 12, 12, 8, 4, 4, 8, 12, 12, 12]
