"""The launch plan of the temporal convolution (2s-agcn_amd/csrc/tconv_plan.h) against its definition, on the CPU:
tests/tconv_plan_check.cpp enumerates taps 1..9 x stride 1..9 x pad 0..(taps-1)/2 x T 1..40 and requires the
backward-data passes to cover exactly the (output frame, dy frame, tap) triples of the forward definition, every output
frame once, plus the literal launches of the 1- and 9-tap shapes the agcn_conv_* entry points cover.  The header is host
only, so the host C++ compiler builds the program; no GPU, no HIP."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tconv_plan_matches_definition(tmp_path):
    cxx = next((c for c in (os.environ.get('CXX'), 'c++', 'g++', 'clang++') if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip('no host C++ compiler')
    exe = str(tmp_path / 'tconv_plan_check')
    r = subprocess.run([cxx, '-std=c++17', '-Wall', '-Werror', '-O1', '-I', os.path.join(ROOT, '2s-agcn_amd', 'csrc'),
                        os.path.join(ROOT, 'tests', 'tconv_plan_check.cpp'), '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-4000:]
    assert '8370 cases, 0 failures' in r.stdout
