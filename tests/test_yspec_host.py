"""Host side of the y-spectral sweep, no GPU: the block-shift formula and the live-block masks of
pygpa_amd/csrc/gpa_yspec.h against the transform's spec_index (tests/host/yspec_emulator.cpp: every band rotation s = 0 .. 15,
NBL = 6 and 8, 2048- and 4096-point rows), and the inputs of tests/test_gpu_yspec_sweep.py: their share of near-ties between
the two best candidates must stay below a tenth of what the comparison of the two f32 paths may excuse."""
import os
import shutil
import subprocess

import pytest

import yspec_cases as yc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_block_shift_and_masks(tmp_path):
    gxx = shutil.which('g++')
    if gxx is None:
        pytest.skip('g++ not available')
    exe = str(tmp_path / 'yspec_emulator')
    src = os.path.join(ROOT, 'tests', 'host', 'yspec_emulator.cpp')
    subprocess.run([gxx, '-O2', '-std=c++17', '-I', os.path.join(ROOT, 'pygpa_amd', 'csrc'), src, '-o', exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:]
    assert out.stdout.strip().endswith('OK')


@pytest.mark.parametrize('shape', yc.SHAPES)
@pytest.mark.parametrize('name', yc.CASES)
def test_inputs_have_few_near_ties(name, shape):
    """at most 1e-4 of the pixels (a tenth of the 0.1 % the GPU test may excuse) have their two largest candidate amplitudes
    within 1e-5 relative; the lists rotate their bands as the GPU test expects"""
    for p, (_, _, amps) in enumerate(yc.oracle(name, shape)):
        assert yc.near_ties(amps).mean() < 1e-4, (name, shape, p)
    for f32 in (True, False):
        for s, blocks in (yc.band_rotation(kl, yc.SIGMA, f32) for kl in yc.case(name, shape)[2]):
            assert 0 <= s < 16 and blocks <= (6 if f32 else 8)
