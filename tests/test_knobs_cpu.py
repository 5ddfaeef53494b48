"""The environment-switch table (2s-agcn_amd/csrc/knobs.h) on the CPU: tests/knobs_check.cpp holds every row's default
and its reading of "0", "1", "", "8" and "-1" against the values the hand-written reads it replaced gave (written out
per switch), and checks that a LATCHED switch keeps its first value after a setenv, a PER_CALL one follows it, and a
PROBE one gives its default to a dry run.  One child process per scenario.  The header is host only, so the host C++
compiler builds the program; no GPU, no HIP."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_knob_table_matches_the_reads_it_replaced(tmp_path):
    cxx = next((c for c in (os.environ.get('CXX'), 'c++', 'g++', 'clang++') if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip('no host C++ compiler')
    exe = str(tmp_path / 'knobs_check')
    r = subprocess.run([cxx, '-std=c++17', '-Wall', '-Werror', '-O1', '-I', os.path.join(ROOT, '2s-agcn_amd', 'csrc'),
                        os.path.join(ROOT, 'tests', 'knobs_check.cpp'), '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    env = {k: v for k, v in os.environ.items() if not k.startswith('AGCN_')}
    r = subprocess.run([exe], capture_output=True, text=True, env=env)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-4000:]
    assert '32 switches, 516 cases, 0 failures' in r.stdout
