"""GPU parity of aagcn_v17 against the reference-generated fixtures of tests/golden/make_golden_v17.py (tv17_*), with the
encoder head on the HIP kernels (checked by ops.ENCODER_STATS), the same once more as tensor code (AGCN_ENCODER_HIP=0,
child process), the dropout path, and two optimiser steps.  ``-m gpu``.

Tolerances (the layer rule of test_gpu_tconv.py): y_eval, y and every attention matrix within 1e-4 of the tensor's own
max; dx and every parameter gradient within 2e-4 through golden_util.audit_grads.  AGCN_GEMM=bf16: 2e-2.
"""
import os
import subprocess
import sys

import pytest
import torch

from tests import golden_util as gu
from tests import v17_util as vu

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gpu():
    import agcn_amd  # noqa: F401
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device('cuda:0')


def _bf16():
    from agcn_amd import lib
    return lib.load().agcn_gemm_mode().decode() == 'bf16'


def trel(a, ref):
    a = a.detach().double().cpu()
    ref = torch.as_tensor(ref).double()
    return float((a - ref).abs().max() / max(float(ref.abs().max()), 1e-30))


def _model(name, dev, **over):
    from agcn_amd.model import aagcn_v17
    gold = vu.load(name)
    m = aagcn_v17.Model(**dict(vu.model_kwargs(name), **over))
    m.load_state_dict(vu.state(vu.shapes_of(gold), name), strict=True)
    return m.to(dev), gold


def _expect_route(layers):
    from agcn_amd import ops
    hip = ops.encoder_hip_enabled()
    assert ops.ENCODER_STATS['layers_hip'] == (layers if hip else 0), ops.ENCODER_STATS
    assert ops.ENCODER_STATS['layers_tensor'] == (0 if hip else layers), ops.ENCODER_STATS


@pytest.mark.parametrize('name', vu.NAMES)
def test_v17_vs_reference(name):
    from agcn_amd import ops
    dev = _gpu()
    m, gold = _model(name, dev)
    need_attn = bool(vu.model_kwargs(name).get('need_attn', False))
    tol_y, tol_g = (2e-2, 2e-2) if _bf16() else (1e-4, 2e-4)
    x = torch.from_numpy(gold['x']).to(dev)
    ops.ENCODER_STATS.update(layers_hip=0, layers_tensor=0)
    errs = {}
    m.eval()
    with torch.no_grad():
        y_eval, attn = m(x)
    errs['y_eval'] = trel(y_eval, gold['y_eval'])
    assert len(attn) == (2 if need_attn else 0)
    for i, a in enumerate(attn):
        errs[f'attn_eval.{i}'] = trel(a, gold[f'attn_eval.{i}'])
    m.train()
    xg = x.clone().requires_grad_(True)
    y, attn = m(xg)
    (y * torch.from_numpy(gold['r']).to(dev)).sum().backward()
    torch.cuda.synchronize()
    _expect_route(4)
    errs['y'] = trel(y, gold['y'])
    for i, a in enumerate(attn):
        assert not a.requires_grad
        errs[f'attn.{i}'] = trel(a, gold[f'attn.{i}'])
    print(name, {k: f'{v:.2e}' for k, v in errs.items()})
    for k, v in errs.items():
        assert gu.audit_value(name, k, v, tol_y), (k, v)
    e_dx = trel(xg.grad, gold['dx'])
    print(name, 'dx', f'{e_dx:.2e}', 'reference fp32 vs fp64', f"{trel(torch.from_numpy(gold['dx']), gold['dx64']):.2e}")
    assert gu.audit_value(name, 'dx', e_dx, tol_g), e_dx
    named = [(n, p.grad.detach().cpu().numpy()) for n, p in m.named_parameters()]
    assert all(('g.' + n + '.absmax') in gold for n, _ in named)
    bad, rec = gu.audit_grads(name, named, gold, tol_g)
    print(name, 'grads: worst err32', rec['worst_err32'], 'worst err64', rec['worst_err64'])
    assert not bad, bad


def test_v17_fixtures_as_tensor_code():
    """The five fixtures once more with AGCN_ENCODER_HIP=0 (read per call, but the counter check wants a clean process)."""
    _gpu()
    r = subprocess.run([sys.executable, '-m', 'pytest', os.path.join(ROOT, 'tests', 'test_gpu_v17.py'), '-q', '-x', '-m', 'gpu',
                        '-p', 'no:cacheprovider', '-k', 'test_v17_vs_reference'],
                       env=dict(os.environ, AGCN_ENCODER_HIP='0'), cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert '5 passed' in r.stdout and ' skipped' not in r.stdout, r.stdout[-2000:]


@pytest.mark.parametrize('mode', ['f32', 'bf16'])
def test_v17_other_gemm_modes_subprocess(mode):
    """AGCN_GEMM is read once per process: the fixtures and the dropout comparison once more with the backbone's
    contractions in AGCN_GEMM=<mode> (the encoder kernels are fp32 FMA in every mode)."""
    _gpu()
    r = subprocess.run([sys.executable, '-m', 'pytest', os.path.join(ROOT, 'tests', 'test_gpu_v17.py'), '-q', '-x', '-m', 'gpu',
                        '-p', 'no:cacheprovider', '-k', 'test_v17_vs_reference or test_v17_dropout'],
                       env=dict(os.environ, AGCN_GEMM=mode), cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert '6 passed' in r.stdout and ' skipped' not in r.stdout, r.stdout[-2000:]


def test_v17_dropout(monkeypatch):
    dev = _gpu()
    m, gold = _model('tv17_frame', dev, trans_dropout=0.2)
    m.train()
    x = torch.from_numpy(gold['x']).to(dev)
    r = torch.from_numpy(gold['r']).to(dev)

    def run():
        torch.manual_seed(77)
        xg = x.clone().requires_grad_(True)
        y, attn = m(xg)
        (y * r).sum().backward()
        return [y.detach(), xg.grad] + [a for a in attn]

    monkeypatch.setenv('AGCN_ENCODER_HIP', '1')
    a, b = run(), run()
    assert all(bool(torch.isfinite(t).all()) for t in a)
    for s, t in zip(a, b):
        assert torch.equal(s, t)
    # the returned attention is the dropped-out one: an entry of the mean over the 2 heads is zero where both heads
    # dropped it, 0.2^2 of the 2*21*21 entries of the unmasked first layer (standard deviation 0.0066)
    zeros = float((a[2] == 0).float().mean())
    assert 0.01 < zeros < 0.08, zeros
    monkeypatch.setenv('AGCN_ENCODER_HIP', '0')
    c = run()
    tol = 2e-2 if _bf16() else 1e-4          # (bf16: the backbone's backward amplifies the head's last-bit differences)
    for s, t in zip(a, c):
        assert trel(s, t.cpu()) < tol
    torch.manual_seed(78)                                  # another seed, another mask
    y2, _ = m(x)
    assert not torch.equal(y2.detach(), c[0])


def test_v17_train_steps():
    from agcn_amd.trainer import TrainEngine
    dev = _gpu()
    m, gold = _model('tv17_shipped', dev, trans_dropout=0.2)
    eng = TrainEngine(m, base_lr=0.05)
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    assert any(n.startswith('trans_enc.') for n in before) and 'cls_token' in before
    x = torch.from_numpy(gold['x']).to(dev)
    label = torch.tensor([3, 41], device=dev)
    for _ in range(2):
        loss = eng.train_step(x, label)
        assert bool(torch.isfinite(loss))
    same = [n for n, p in m.named_parameters() if torch.equal(p.detach(), before[n])]
    assert not same, same


def test_v17_strict_load_of_a_reference_style_checkpoint(tmp_path):
    dev = _gpu()
    m, gold = _model('tv17_forward', dev)
    path = str(tmp_path / 'v17.pt')
    torch.save({k: v.cpu() for k, v in m.state_dict().items()}, path)
    m2, _ = _model('tv17_forward', dev)
    with torch.no_grad():
        for p in m2.parameters():
            p.zero_()
    m2.load_state_dict(torch.load(path), strict=True)
    m.eval()
    m2.eval()
    x = torch.from_numpy(gold['x']).to(dev)
    with torch.no_grad():
        assert torch.equal(m(x)[0], m2(x)[0])
