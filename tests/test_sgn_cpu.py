"""CPU checks of the base SGN: the module's state_dict against the reference-generated fixtures, the tensor-code
composition against the reference's eval outputs and train-mode gradients (tests/golden/make_golden_sgn.py), the host
check of csrc/sgn_plan.h with its interval table against numpy, the numpy emulation of ``agcn_sgn_sample`` against the
reference's to_fix_length, and the C-ABI argument errors of the new entry points (returned before any HIP call)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import sgn_util as su

ROOT = su.ROOT


def _model(case):
    import agcn_amd  # noqa: F401
    from agcn_amd.model.sgn import SGN
    c = su.load_case(case)
    m = SGN(**su.model_args(c['meta']))
    m.load_state_dict(su.torch_state(c['state']))
    return c, m


def _err(got, ref):
    ref = np.asarray(ref, dtype=np.float64)
    return float(np.abs(np.asarray(got, dtype=np.float64) - ref).max() / max(1.0, float(np.abs(ref).max())))


@pytest.mark.parametrize('case', ['v15_seg20', 'v7_seg12_nobias'])
def test_state_dict_is_the_references(case):
    import agcn_amd  # noqa: F401
    from agcn_amd.model.sgn import SGN
    c = su.load_case(case)
    m = SGN(**su.model_args(c['meta']))               # constructs without a GPU
    sd = m.state_dict()
    assert list(sd.keys()) == c['keys']
    assert {k: tuple(v.shape) for k, v in sd.items()} == c['shapes']
    assert len(sd) == (70 if c['meta']['bias'] else 55)
    assert 'spa' not in sd and 'tem' not in sd
    assert m.spa.shape == (1, c['meta']['num_point'], c['meta']['num_point'], c['meta']['seg'])
    assert m.tem.shape == (1, c['meta']['seg'], c['meta']['num_point'], c['meta']['seg'])
    for gcn in (m.gcn1, m.gcn2, m.gcn3):              # the reference's zero initialisation of the g.x branch
        assert not gcn.w.cnn.weight.any()
    import model.sgn as shim
    assert shim.SGN is SGN


@pytest.mark.parametrize('case', su.CASES)
def test_composition_matches_reference_eval(case):
    c, m = _model(case)
    m.eval()
    with torch.no_grad():
        logits, g = m(torch.from_numpy(c['x']))
    assert tuple(g.shape) == c['g'].shape
    e_l, e_g = _err(logits.numpy(), c['logits']), _err(g.numpy(), c['g'])
    print(f'{case}: composition vs reference, eval: logits {e_l:.2e}, g {e_g:.2e}')
    assert e_l < 1e-4 and e_g < 1e-4


@pytest.mark.parametrize('case', su.TRAIN_CASES)
def test_composition_matches_reference_train(case):
    c, m = _model(case)
    rec = su.load_train(case)
    m.train()
    m.cnn.dropout.p = 0.0
    x = torch.from_numpy(c['x']).requires_grad_(True)
    logits, _ = m(x)
    (logits * torch.from_numpy(rec['c'])).sum().backward()
    worst = ('logits', _err(logits.detach().numpy(), rec['logits']))
    assert worst[1] < 1e-4, worst
    errs = {'x': _err(x.grad.numpy(), rec['grad_x'])}
    params = dict(m.named_parameters())
    assert set(params) == set(rec['grads'])
    for k, p in params.items():
        errs[k] = _err(p.grad.numpy(), rec['grads'][k])
    k = max(errs, key=errs.get)
    print(f'{case}: composition vs reference, train: logits {worst[1]:.2e}, worst gradient {k} {errs[k]:.2e}')
    assert errs[k] < 1e-4, (k, errs[k])


def test_sgn_plan_checker(tmp_path):
    cxx = next((c for c in (os.environ.get('CXX'), 'c++', 'g++', 'clang++') if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip('no host C++ compiler')
    exe, table = str(tmp_path / 'sgn_plan_check'), str(tmp_path / 'intervals.bin')
    r = subprocess.run([cxx, '-std=c++17', '-Wall', '-Werror', '-O1', '-I', os.path.join(ROOT, '2s-agcn_amd', 'csrc'),
                        os.path.join(ROOT, 'tests', 'sgn_plan_check.cpp'), '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe, table], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-4000:]
    assert ' cases, 0 failures' in r.stdout and int(r.stdout.split(' cases')[0].split()[-1]) > 400000
    got = np.fromfile(table, dtype=np.int32)
    want = np.concatenate([np.multiply(list(range(seg + 1)), L / seg).round().astype(int)
                           for seg in (20, 30, 64, 100) for L in range(seg, 4097)])
    assert np.array_equal(got, want)


@pytest.mark.parametrize('name', su.WINDOWS)
def test_sampler_emulation_matches_reference(name):
    f = su._npz('sgn_sample.npz')
    win, r = f[name + '.win'], f[name + '.r']
    out, L = su.sample_emulate(win[None], r[None], 20)
    assert int(L[0]) == int(f[name + '.L'])
    assert np.array_equal(out[0], f[name + '.out'])


def test_sampler_emulation_edges():
    f = su._npz('sgn_sample.npz')
    win = f['mixed.win']
    out, L = su.sample_emulate(np.zeros_like(win)[None], np.zeros((1, 5, 20), dtype=np.uint32), 20)
    assert not out.any() and int(L[0]) == 0
    out, L = su.sample_emulate(win[None], np.full((1, 5, 20), 0xFFFFFFFF, dtype=np.uint32), 20)
    rows = np.transpose(win, (1, 3, 2, 0)).reshape(-1, win.shape[2] * 3)
    assert all(any(np.array_equal(row, src) for src in rows) for row in out[0, 0])


def test_argument_errors_are_reported_not_thrown():
    import agcn_amd  # noqa: F401
    from agcn_amd import lib
    L = lib.load()
    p = ctypes.c_void_p(4096)          # never dereferenced: the checks come before any HIP call
    ARG = -1
    nf, nc = L.agcn_sgn_frames_weights(15), L.agcn_sgn_clip_weights(20, 60)
    assert nf == 12 * 15 + 2 * (192 + 64 + 4096 + 64) + 64 * 15 + 2 * (128 * 256 + 256) + 32768 + 128 + 65536 + 256 \
        + 131072 + 256
    assert nc == 20 * 256 + 3 * 65536 + 256 + 256 * 512 + 512 + 512 * 60 + 60
    assert L.agcn_sgn_frames_weights(33) == 0 and L.agcn_sgn_frames_weights(1) == 0
    assert L.agcn_sgn_frames(None, p, nf, p, p, 1, 20, 15, None) == ARG
    assert L.agcn_sgn_frames(p, None, nf, p, p, 1, 20, 15, None) == ARG
    assert L.agcn_sgn_frames(p, p, nf, None, p, 1, 20, 15, None) == ARG
    assert L.agcn_sgn_frames(p, p, nf, p, None, 1, 20, 33, None) == ARG           # V = 33
    assert L.agcn_sgn_frames(p, p, nf, p, None, 1, 0, 15, None) == ARG
    assert L.agcn_sgn_frames(p, p, nf - 1, p, None, 1, 20, 15, None) == ARG       # not the image of this V
    assert L.agcn_sgn_frames(p, p, nf, p, None, 1 << 30, 20, 15, None) == -3
    assert L.agcn_sgn_clip(None, p, nc, p, 1, 20, 60, None) == ARG
    assert L.agcn_sgn_clip(p, p, nc, None, 1, 20, 60, None) == ARG
    assert L.agcn_sgn_clip(p, p, nc + 1, p, 1, 20, 60, None) == ARG
    assert L.agcn_sgn_clip(p, p, nc, p, 1, 20, 5000, None) == -3
    assert L.agcn_sgn_sample(None, p, p, p, 1, 36, 15, 2, 5, 20, None) == ARG
    assert L.agcn_sgn_sample(p, None, p, p, 1, 36, 15, 2, 5, 20, None) == ARG
    assert L.agcn_sgn_sample(p, p, None, p, 1, 36, 15, 2, 5, 20, None) == ARG
    assert L.agcn_sgn_sample(p, p, p, None, 1, 36, 15, 2, 5, 20, None) == ARG
    assert L.agcn_sgn_sample(p, p, p, p, 1, 36, 15, 1, 5, 20, None) == ARG         # K = 1
    assert L.agcn_sgn_sample(p, p, p, p, 1, 36, 15, 3, 5, 20, None) == ARG
    assert L.agcn_sgn_sample(p, p, p, p, 1, 36, 33, 2, 5, 20, None) == ARG         # V = 33
    assert L.agcn_sgn_sample(p, p, p, p, 1, L.agcn_prenorm_max_frames() + 1, 15, 2, 5, 20, None) == ARG


def test_python_wrappers_refuse_other_body_counts():
    import agcn_amd  # noqa: F401
    from agcn_amd import ops
    from agcn_amd.online import ActionRecognition
    with pytest.raises(ValueError):
        ops.sgn_sample(torch.zeros(1, 3, 8, 15, 3), torch.zeros(1, 5, 20, dtype=torch.int32), 20)
    with pytest.raises(ValueError):
        ActionRecognition(torch.nn.Identity(), max_num_skeleton_true=1, sgn_preprocess=True, device='cpu')
