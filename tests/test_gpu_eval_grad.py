"""Eval-mode (frozen BatchNorm statistics) forward + backward of the HIP units and small models against the fp64 oracle
run with the HIP forward's own ReLU patterns imposed -- the kink-free recipe of
test_gpu_parity.py::test_model_end_to_end_grads_with_pinned_relu_patterns.  GPU only.

Tolerances (tests/evalgrad_util.py): outputs 1e-4*max(1, max|ref|); dx and every parameter gradient 2e-4 of the
per-tensor max|g_ref|; single-scalar AAGCN parameters 5e-3; conv_a biases the absolute 1e-5 floor of the structurally
zero gradients; the WORST error of every tensor is asserted.  Under AGCN_GEMM=bf16 (subprocess repeat): the 2e-2 / 6e-2
bounds of tests/bf16_check.py, for the reason stated there."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import agcn_oracle as orc
from tests import evalgrad_util as eg
from tests import golden_util as gu

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gpu():
    import agcn_amd  # noqa: F401
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device('cuda:0')


def _mode():
    from agcn_amd import lib
    return lib.load().agcn_gemm_mode().decode()


def _out(y):
    return y[0] if isinstance(y, tuple) else y


def _gcn_pattern(unit, x):
    """ReLU pattern of a unit's GCN core at input x: the same kernels on the same input, attention gates off."""
    with torch.no_grad():
        g1 = unit.gcn1
        saved = [getattr(g1, a, None) for a in ('attn_s', 'attn_t', 'attn_c')]
        has = hasattr(g1, 'attn_s')
        if has:
            g1.attn_s = g1.attn_t = g1.attn_c = None
        g = g1(x.detach())
        if has:
            g1.attn_s, g1.attn_t, g1.attn_c = saved
    return (g > 0).double().cpu()


def _run_hip(name, dev, only_x=False):
    """Eval-mode forward + backward of the case on the HIP path.  Returns (module, y, dx, grads, masks)."""
    sd0, xn, rn = eg.state_and_inputs(name)
    m = eg.make_module(name)
    m.load_state_dict(sd0)
    m.to(dev).eval()
    if only_x:
        for p in m.parameters():
            p.requires_grad_(False)
    cap = {}
    ks = eg.layer_keys(name)
    hooks = []
    for k in ks:
        lay = getattr(m, f'l{k}')
        hooks.append(lay.register_forward_pre_hook(lambda mod, inp, k=k: cap.__setitem__(('x', k), inp[0].detach())))
        hooks.append(lay.register_forward_hook(lambda mod, inp, out, k=k: cap.__setitem__(('y', k), out.detach())))
    x = torch.from_numpy(xn).to(dev).requires_grad_(True)
    y = _out(m(x))
    (y * torch.from_numpy(rn).to(dev)).sum().backward()
    torch.cuda.synchronize()
    for h in hooks:
        h.remove()
    kind = eg.CASES[name]['kind']
    if kind == 'unit_tcn':
        masks = None
    elif kind.endswith('unit'):
        masks = (_gcn_pattern(m, x), (y.detach() > 0).double().cpu())
    else:
        masks = {k: (_gcn_pattern(getattr(m, f'l{k}'), cap[('x', k)]), (cap[('y', k)] > 0).double().cpu()) for k in ks}
    grads, seen = {}, set()
    for k, p in m.named_parameters():
        if id(p) in seen or p.grad is None:
            continue
        seen.add(id(p))
        grads[k] = p.grad.cpu().numpy()
    return m, y.detach().cpu().numpy(), x.grad.cpu().numpy(), grads, masks, (sd0, xn, rn)


_CACHE = {}


def _case(name, dev):
    """HIP results and the fp64 reference of a case, computed once and shared by the tests that need them."""
    if name not in _CACHE:
        m, y, dx, grads, masks, (sd0, xn, rn) = _run_hip(name, dev)
        ref = eg.oracle_run(name, sd0, xn, rn, masks, torch.float64)
        _CACHE[name] = (y, dx, grads, ref)
    return _CACHE[name]


def _check(name, dev):
    y, dx, grads, ref = _case(name, dev)
    bad, rec = eg.compare(name, y, dx, grads, ref, bf16=_mode() == 'bf16')
    worst = sorted(rec.items(), key=lambda kv: -kv[1])[:3]
    print(f'eval-grad {name} [{_mode()}]: {len(rec)} tensors, worst {worst}')
    assert not bad, bad[:8]
    # every parameter of the module got a gradient and was compared
    assert len(rec) == 2 + sum(not (_mode() == 'bf16' and eg.is_conv_a_bias(k)) for k in grads)
    return grads, ref


@pytest.mark.parametrize('name', eg.UNIT_CASES)
def test_unit_eval_grad(name):
    dev = _gpu()
    grads, ref = _check(name, dev)
    # the biases of the convolutions in front of the frozen BatchNorms: real, non-zero gradients equal to the oracle's
    # (compared above like every tensor); a port that keeps the train path's exact zeros fails here
    nz = [k for k in grads if eg.is_bn_conv_bias(k) or k == 'conv.bias']
    assert nz, list(grads)
    for k in nz:
        r = ref[2][gu.canonical_key(k)] if gu.canonical_key(k) in ref[2] else ref[2][k]
        assert float(r.abs().max()) > 1e-3 and float(np.abs(grads[k]).max()) > 0.5 * float(r.abs().max()), k
    assert len(nz) == N_BN_CONV_BIASES[name], nz


# conv_d.{0,1,2} + tcn1.conv [+ down.0] [+ residual.conv]; the stand-alone unit_tcn has its one convolution
N_BN_CONV_BIASES = {'agcn_unit_64_64_s1_v25': 4, 'agcn_unit_64_128_s2_v18_oddT': 6, 'agcn_unit_3_64_nores': 5,
                    'aagcn_unit_64_64_attn': 4, 'aagcn_unit_64_64_gbn2': 4, 'unit_tcn_k3s3p0': 1}


@pytest.mark.parametrize('name', eg.MODEL_CASES)
def test_model_eval_grad(name):
    if _mode() == 'bf16':
        pytest.skip("full-model gradients are not compared tensor by tensor in bf16 (tests/bf16_check.py)")
    _check(name, _gpu())


@pytest.mark.parametrize('name', ['agcn_unit_64_128_s2_v18_oddT', 'aagcn_unit_64_64_attn', 'unit_tcn_k3s3p0',
                                  'aagcn_model_l3_t32'])
def test_input_gradient_only_skips_the_sums(name):
    """requires_grad on x alone: every BatchNorm stage launches the want_sums=0 variant (y1 / y2 never read), no
    parameter receives a gradient, and dx has the bits of the full run's dx."""
    from agcn_amd import ops
    dev = _gpu()
    _, dx_full, _, _ = _case(name, dev)
    before = dict(ops.EVAL_BWD_STATS)
    m, y, dx, grads, _, _ = _run_hip(name, dev, only_x=True)
    delta = {k: ops.EVAL_BWD_STATS[k] - before[k] for k in before}
    assert delta['sums'] == 0 and delta['nosums'] >= 1, delta
    kind = eg.CASES[name]['kind']
    per_unit = 1 if kind == 'unit_tcn' else 2            # the GCN stage and the TCN stage
    units = max(1, len(eg.layer_keys(name)))
    assert delta['nosums'] == per_unit * units, delta
    assert not grads
    assert np.array_equal(dx, dx_full)
    # ... and the full run took the other variant
    before = dict(ops.EVAL_BWD_STATS)
    _run_hip(name, dev)
    delta = {k: ops.EVAL_BWD_STATS[k] - before[k] for k in before}
    assert delta == {'sums': per_unit * units, 'nosums': 0}, delta


def test_train_mode_after_eval_backward_still_matches_its_fixture():
    """No state leaks from the eval-mode backward: the train-mode forward + backward of the same unit, run afterwards,
    matches the reference fixture exactly as tests/test_gpu_parity.py::test_unit_golden asks."""
    if _mode() == 'bf16':
        pytest.skip("the fp32 fixture is not a bf16 criterion")
    dev = _gpu()
    from agcn_amd.model.agcn import TCN_GCN_unit
    fx = 'u_64_128_s2_v25'
    gold = gu.load(fx)
    cin, cout, stride, residual, t, v, seed = [int(i) for i in gold['meta']]
    unit = TCN_GCN_unit(cin, cout, gu.graph_A(v).numpy(), stride=stride, residual=bool(residual))
    sd = orc.randomized_state(orc.unit_param_shapes('', cin, cout, v, stride, bool(residual)), seed,
                              stress=float(gold['meta.stress']))
    unit.load_state_dict(sd)
    unit.to(dev)
    xn, rn = gu.unit_inputs(cin, cout, stride, t, v, seed)
    r = torch.from_numpy(rn).to(dev)

    def train_pass():
        unit.load_state_dict(sd)
        unit.train()
        unit.zero_grad(set_to_none=True)
        x = torch.from_numpy(xn).to(dev).requires_grad_(True)
        y = unit(x)
        (y * r).sum().backward()
        return y.detach(), x.grad, {k: p.grad.clone() for k, p in unit.named_parameters()}
    y0, dx0, g0 = train_pass()
    unit.load_state_dict(sd)
    unit.eval()
    unit.zero_grad(set_to_none=True)
    xe = torch.from_numpy(xn).to(dev).requires_grad_(True)
    ye = unit(xe)
    (ye * r).sum().backward()
    assert gu.rel_err(ye.detach().cpu().numpy(), gold['y_eval']) < 1e-4
    for k, b in unit.state_dict().items():            # eval mode leaves the running statistics alone
        if k.endswith(('running_mean', 'running_var')):
            assert torch.equal(b.cpu(), sd[k]), k
    assert any(float(p.grad.abs().max()) > 1e-3 for k, p in unit.named_parameters() if eg.is_bn_conv_bias(k))
    y1, dx1, g1 = train_pass()
    assert gu.rel_err(y1.cpu().numpy(), gold['y']) < 1e-4
    assert float(np.abs(dx1.cpu().numpy() - gold['dx']).max()) / max(1.0, float(np.abs(gold['dx']).max())) < 2e-4
    bad, _ = gu.audit_grads(fx + '(after an eval-mode backward)', [(k, g.cpu().numpy()) for k, g in g1.items()], gold,
                            2e-4)
    assert not bad, bad[:8]
    # bit for bit what the same pass gave before the eval-mode backward
    assert torch.equal(y1, y0) and torch.equal(dx1, dx0)
    for k in g0:
        assert torch.equal(g1[k], g0[k]), k


@pytest.mark.parametrize('mode', ['f32', 'bf16'])
def test_eval_grad_other_gemm_modes_subprocess(mode):
    """AGCN_GEMM is read once per process: the unit cases of this file once more in a process whose contractions run
    on the exact-f32 kernels, or on plain bf16 operands."""
    _gpu()
    if _mode() == mode:
        pytest.skip("already the mode of this process")
    r = subprocess.run([sys.executable, '-m', 'pytest', os.path.abspath(__file__), '-q', '-x', '-m', 'gpu', '-s',
                        '-p', 'no:cacheprovider', '-k', 'test_unit_eval_grad or test_input_gradient_only'],
                       env=dict(os.environ, AGCN_GEMM=mode), cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert ' passed' in r.stdout and ' skipped' not in r.stdout, r.stdout[-2000:]
    print('\n'.join(ln for ln in r.stdout.splitlines() if ln.startswith('eval-grad')))
