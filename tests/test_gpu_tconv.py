"""GPU parity of the temporal convolution with any kernel size, stride and padding (agcn_tconv_*): kernels against fp64
``torch.nn.functional.conv2d``, and the AAGCN TCNGCNUnit / BaseModel(102) / agcn.unit_tcn layers against the
reference-generated fixtures of tests/golden/make_golden_tconv.py.  ``-m gpu``.

Tolerance: 1e-4 of max(1, max|ref|) for the kernels (as test_gpu_kernels.py::test_conv_fwd_bwd); for the layers 1e-4
of the tensor's own max on outputs and 2e-4 on dx and every parameter gradient.  AGCN_GEMM is fixed per process, so two
tests run this file again in a process of its own: AGCN_GEMM=f32 (same tolerances) and AGCN_GEMM=bf16 (2e-2; the
layers' gradients there as a relative 2-norm, see _check_layer).
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')


def _gpu():
    import agcn_amd  # noqa: F401
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device('cuda:0')


def _mode():
    from agcn_amd import lib
    return lib.load().agcn_gemm_mode().decode()


def _tol(base):
    return 2e-2 if _mode() == 'bf16' else base


def rel(a, ref):
    a = a.detach().double().cpu()
    ref = ref.detach().double().cpu()
    return float((a - ref).abs().max() / max(1.0, float(ref.abs().max())))


def rnd(gen, *shape, scale=1.0):
    return torch.randn(*shape, generator=gen, dtype=torch.float64) * scale


KERNEL_CASES = [
    # N, Cin, Cout, T, V, taps, stride, pad
    (2, 3, 16, 30, 25, 3, 3, 0),        # windowed backbone layer 1
    (2, 16, 16, 30, 25, 3, 3, 0),       # windowed 16 -> 16
    (2, 16, 16, 31, 25, 3, 3, 0),       # trailing frame reached by no window
    (2, 16, 16, 30, 25, 1, 3, 0),       # its 1x1 stride-3 residual
    (2, 64, 64, 36, 25, 1, 9, 0),       # 1x1 stride-9 residual
    (2, 3, 64, 30, 25, 3, 3, 0),
    (2, 64, 64, 30, 25, 3, 3, 0),
    (2, 64, 64, 30, 25, 3, 3, 1),       # windowed with padding
    (2, 64, 64, 36, 25, 9, 9, 4),       # the heads' default
    (2, 64, 64, 23, 25, 3, 1, 1),
    (2, 64, 64, 22, 25, 5, 1, 0),
    (2, 256, 256, 15, 25, 3, 1, 1),     # 128-row blocks (conv_pc_kernel in the split modes)
    (2, 128, 128, 14, 25, 5, 1, 2),
    (2, 64, 128, 20, 25, 3, 1, 0),
    (2, 128, 128, 16, 25, 7, 1, 3),
    (2, 64, 128, 21, 25, 5, 2, 2),
    (2, 64, 64, 20, 18, 7, 1, 3),
    (2, 64, 64, 19, 25, 4, 1, 1),       # even taps
    (2, 32, 48, 17, 25, 6, 4, 2),
]


def expected_kernels(Cin, Cout, taps, stride, pad):
    """Kernels the forward, the backward-data and the weight gradient must have run (AGCN_NOTE_KERNEL)."""
    mode = _mode()
    if stride == 1 and taps in (3, 5, 7) and mode != 'f32':
        fwd = ('conv_pc_kernel<%d' % taps, 'conv_gemm_bf16_kernel<%d' % taps)
        bwd = fwd
    else:
        fwd = ('conv_gemm_kernel<%d, 0' % taps,)
        bwd = ('conv_gemm_kernel<',)          # one stride-1 problem per output-frame residue
    if (mode == 'bf16x6' and stride == 1 and taps in (3, 5, 7) and taps - pad <= 5 and Cout % 64 == 0
            and Cin % 64 == 0):
        wg = ('wgrad9_f16_kernel<',)         # the f16x3 weight gradient with the window shifted per tap
    else:
        wg = ('conv_wgrad_kernel<%d, 0' % taps,)
    return fwd, bwd, wg


@pytest.mark.parametrize('with_amax', [False, True])
@pytest.mark.parametrize('case', KERNEL_CASES)
def test_tconv_kernels_vs_fp64(case, with_amax):
    from agcn_amd import lib, ops
    dev = _gpu()
    L = lib.load()
    N, Cin, Cout, T, V, taps, stride, pad = case
    tol = _tol(1e-4)
    g = torch.Generator().manual_seed(hash(case) % 1000 + int(with_amax))
    x = rnd(g, N, Cin, T, V).requires_grad_(True)
    w = rnd(g, Cout, Cin, taps, 1, scale=1.0 / np.sqrt(Cin * taps)).requires_grad_(True)
    b = rnd(g, Cout, scale=0.1)
    y_ref = F.conv2d(x, w, b, stride=(stride, 1), padding=(pad, 0))
    dy = rnd(g, *y_ref.shape)
    y_ref.backward(dy)
    xg, wg, bg, dyg = x.detach().float().to(dev), w.detach().float().to(dev), b.float().to(dev), dy.float().to(dev)
    x_amax = xg.abs().max().reshape(1) if with_amax else None
    dy_amax = dyg.abs().max().reshape(1) if with_amax else None
    k_fwd, k_bwd, k_wg = expected_kernels(Cin, Cout, taps, stride, pad)
    y, stats = ops.conv_fwd(xg, wg, bg, stride, want_stats=True, x_amax=x_amax, pad=pad)
    torch.cuda.synchronize()
    kern = L.agcn_last_kernel().decode()
    assert kern.startswith(k_fwd), kern
    assert tuple(y.shape) == tuple(y_ref.shape)
    assert rel(y, y_ref) < tol
    s = stats.double().sum(0).cpu()
    assert rel(s[0], y_ref.detach().sum((0, 2, 3))) < tol * 10
    assert rel(s[1], (y_ref.detach() ** 2).sum((0, 2, 3))) < tol * 10
    dx = ops.conv_bwd_data(dyg, wg, tuple(x.shape), stride, dy_amax=dy_amax, pad=pad)
    kern = L.agcn_last_kernel().decode()
    assert kern.startswith(k_bwd), kern
    assert rel(dx, x.grad) < tol
    # accumulate + masked addends (the residual's backward-data writes into dx this way)
    base = rnd(g, *x.shape).float().to(dev)
    add = rnd(g, *x.shape).float().to(dev)
    mask = rnd(g, *x.shape).float().to(dev)
    out = base.clone()
    ops.conv_bwd_data(dyg, wg, tuple(x.shape), stride, out=out, accumulate=True, add1=add, mask1=mask, add2=add,
                      dy_amax=dy_amax, pad=pad)
    ref2 = x.grad + base.double().cpu() + (add.double().cpu() * (mask.cpu() > 0)) + add.double().cpu()
    assert rel(out, ref2) < tol
    dw = ops.conv_bwd_weight(dyg, xg, tuple(w.shape), stride, dy_amax, x_amax, pad=pad)
    kern = L.agcn_last_kernel().decode()
    assert kern.startswith(k_wg), kern
    assert rel(dw, w.grad) < tol


def test_unreached_frames_get_zero_gradient():
    from agcn_amd import ops
    dev = _gpu()
    g = torch.Generator().manual_seed(5)
    x = rnd(g, 2, 16, 32, 25).float().to(dev)
    w = rnd(g, 16, 16, 3, 1).float().to(dev)
    dy = rnd(g, 2, 16, 10, 25).float().to(dev)
    dx = ops.conv_bwd_data(dy, w, tuple(x.shape), 3, pad=0)
    assert float(dx[:, :, 30:].abs().max()) == 0.0
    assert float(dx[:, :, :30].abs().max()) > 0.0


@pytest.mark.parametrize('case', [KERNEL_CASES[1], KERNEL_CASES[9], KERNEL_CASES[11], KERNEL_CASES[8]])
def test_tconv_repeat_bit_identical(case):
    from agcn_amd import ops
    dev = _gpu()
    N, Cin, Cout, T, V, taps, stride, pad = case
    g = torch.Generator().manual_seed(11)
    x = rnd(g, N, Cin, T, V).float().to(dev)
    w = rnd(g, Cout, Cin, taps, 1, scale=0.1).float().to(dev)
    b = rnd(g, Cout).float().to(dev)
    outs = []
    for _ in range(2):
        y, st = ops.conv_fwd(x, w, b, stride, want_stats=True, pad=pad)
        dy = torch.sin(y)
        dx = ops.conv_bwd_data(dy, w, tuple(x.shape), stride, pad=pad)
        dw = ops.conv_bwd_weight(dy, x, tuple(w.shape), stride, pad=pad)
        outs.append((y, st, dx, dw))
    for a, b_ in zip(*outs):
        assert torch.equal(a, b_)


# ---- layers against the reference fixtures ----
UNIT_FIXTURES = ['tu_k3s3p0_3_16', 'tu_k3s3p0_16_16', 'tu_k3s3p0_16_16_oddT', 'tu_k9s9p4_64_64', 'tu_k3s1p1_64_64',
                 'tu_k5s2p2_64_128', 'tu_k7s1p3_64_64_v18', 'tu_k4s1p1_64_64']
TCN_FIXTURES = ['tt_k3s1_64_64', 'tt_k5s2_64_128']


def _gold(name):
    return dict(np.load(os.path.join(GOLDEN, name + '.npz')))


def _graph_A(v):
    return np.load(os.path.join(GOLDEN, 'graphs.npz'))[f'A_v{v}'].astype(np.float32)


def _state(gold, seed, stress):
    from oracle import agcn_oracle as orc
    shapes = {k[len('shape.'):]: tuple(int(d) for d in v) for k, v in gold.items() if k.startswith('shape.')}
    return orc.aagcn_randomized_state(shapes, seed, stress=stress)


def trel(a, ref):
    """max |a - ref| / max |ref|: the tensor's own scale."""
    a = a.detach().double().cpu()
    ref = ref.detach().double().cpu()
    return float((a - ref).abs().max() / max(float(ref.abs().max()), 1e-30))


def _grad_err(g, gold, name, bf16):
    """Error of a parameter gradient against the fixture: max-normalised by the tensor's max (fp32 modes) or as a
    relative 2-norm (bf16); tensors above the fixture's size limit are compared on its 256 stored samples, and their
    whole 2-norm against the stored one."""
    g = g.detach().double().cpu().numpy()
    if ('g.' + name) in gold:
        ref = gold['g.' + name].astype(np.float64)
        if bf16:
            return float(np.linalg.norm(g - ref) / max(np.linalg.norm(ref), 1e-30))
        return float(np.abs(g - ref).max() / max(float(gold['g.' + name + '.absmax']), 1e-30))
    idx = gold['g.' + name + '.idx']
    ref = gold['g.' + name + '.samples'].astype(np.float64)
    d = g.reshape(-1)[idx] - ref
    e = (np.linalg.norm(d) / max(np.linalg.norm(ref), 1e-30)) if bf16 else \
        float(np.abs(d).max() / max(float(gold['g.' + name + '.absmax']), 1e-30))
    norm_e = abs(np.linalg.norm(g) - float(gold['g.' + name + '.norm'])) / max(float(gold['g.' + name + '.norm']), 1e-30)
    return float(max(e, norm_e))


def _check_layer(m, gold, xin, dev, tol_y=1e-4, tol_g=2e-4):
    """Outputs (train and eval) and every gradient, each against its own max.  AGCN_GEMM=bf16: 2e-2 on the outputs and
    on the gradients as a relative 2-norm -- a 2^-9 forward error flips the ReLU pattern of a few elements, and a flipped
    element's gradient is off by its whole value in any bf16 implementation, so an element-wise max measures the flips
    (tests/bf16_check.py).  Even so the units' dx measures 2.2e-2 (k9/s9, whose convolution is the exact-f32 kernel in
    every mode) to 6.2e-2 (k3/s1, stress 3): the plain-bf16 graph convolution and attention in front of it, amplified
    by the flips, not the convolution under test, whose own kernel tests hold 2e-2 in this mode.  The layers'
    gradients are therefore bounded at 0.25 there: a wrong kernel or route gives O(1)."""
    from tests.golden_util import is_zero_grad_bias
    bf16 = _mode() == 'bf16'
    tol_y, tol_g = _tol(tol_y), (0.25 if bf16 else tol_g)
    m.to(dev)
    m.eval()
    with torch.no_grad():
        y_eval = m(xin)
    y_eval = y_eval[0] if isinstance(y_eval, tuple) else y_eval
    assert trel(y_eval, torch.from_numpy(gold['y_eval'])) < tol_y
    m.train()
    x = xin.clone().requires_grad_(True)
    y = m(x)
    y = y[0] if isinstance(y, tuple) else y
    assert trel(y, torch.from_numpy(gold['y'])) < tol_y
    (y * torch.from_numpy(gold['r']).to(dev)).sum().backward()
    dx_ref = torch.from_numpy(gold['dx']).double()
    if bf16:
        e = float((x.grad.double().cpu() - dx_ref).norm() / dx_ref.norm())
    else:
        e = trel(x.grad, dx_ref)
    assert e < tol_g, ('dx', e)
    bad = {}
    for name, p in m.named_parameters():
        assert ('g.' + name + '.absmax') in gold, f'{name} has no reference gradient in the fixture'
        if is_zero_grad_bias(name) or name == 'conv.bias':   # structurally zero (a BN follows the conv; the
            # softmax-invariant conv_a): compared absolutely
            if not float(p.grad.abs().max()) < 1e-5:
                bad[name] = float(p.grad.abs().max())
            continue
        if bf16 and p.numel() == 1:
            # (one-element parameters -- the attention biases, alpha -- are a single cancelling sum over the unit: in
            # plain bf16 their relative error says nothing about the convolution; the fp32 modes check them at 2e-4)
            continue
        e = _grad_err(p.grad, gold, name, bf16)
        if not e < tol_g:
            bad[name] = e
    assert not bad, bad


@pytest.mark.parametrize('name', UNIT_FIXTURES)
def test_tcngcn_unit_vs_reference(name):
    from agcn_amd.model import aagcn
    dev = _gpu()
    gold = _gold(name)
    cin, cout, k, s, pad, residual, t, v, seed, n = (int(a) for a in gold['meta'])
    unit = aagcn.TCNGCNUnit(cin, cout, _graph_A(v), kernel_size=k, stride=s, pad=bool(pad), residual=bool(residual))
    unit.load_state_dict(_state(gold, seed, float(gold['meta.stress'])))
    _check_layer(unit, gold, torch.from_numpy(gold['x']).to(dev), dev)


@pytest.mark.parametrize('name', TCN_FIXTURES)
def test_agcn_unit_tcn_vs_reference(name):
    from agcn_amd.model import agcn
    dev = _gpu()
    gold = _gold(name)
    cin, cout, k, s, t, v, seed, n = (int(a) for a in gold['meta'])
    m = agcn.unit_tcn(cin, cout, kernel_size=k, stride=s)
    m.load_state_dict(_state(gold, seed, 2.0))
    _check_layer(m, gold, torch.from_numpy(gold['x']).to(dev), dev)


def test_backbone_102_vs_reference():
    from agcn_amd.model import aagcn
    dev = _gpu()
    gold = _gold('tm_l102_k3s3_b2_t63')
    n, t, v, num_class, c, k, s, seed = (int(a) for a in gold['meta'])
    A = _graph_A(v)

    class Backbone(aagcn.BaseModel):
        def __init__(self):
            super().__init__(num_class=num_class, num_point=v, num_person=2, in_channels=3)

            def unit(_in, _out, stride=1, residual=True):
                return aagcn.TCNGCNUnit(_in, _out, A, kernel_size=k, stride=s, pad=False, residual=residual)
            self.init_model_backbone(model_layers=102, tcngcn_unit=unit, output_channel=c)
            self.init_fc(c, num_class)

    m = Backbone()
    m.load_state_dict(_state(gold, seed, float(gold['meta.stress'])))
    _check_layer(m, gold, torch.from_numpy(gold['x']).to(dev), dev)


def test_residual_frame_mismatch_is_a_clear_error():
    from agcn_amd.model import aagcn
    dev = _gpu()
    unit = aagcn.TCNGCNUnit(16, 16, _graph_A(25), kernel_size=3, stride=3, pad=False).to(dev)
    with pytest.raises(RuntimeError, match='residual has 22 frames'):
        unit(torch.randn(1, 16, 64, 25, device=dev))


@pytest.mark.parametrize('mode', ['f32', 'bf16'])
def test_tconv_other_gemm_modes_subprocess(mode):
    """AGCN_GEMM is read once per process: this file once more (its kernel, layer and model tests) in a process whose
    contractions run in AGCN_GEMM=<mode> -- the exact-f32 kernels everywhere, or plain bf16 operands on the split kernels."""
    _gpu()
    r = subprocess.run([sys.executable, '-m', 'pytest', os.path.join(ROOT, 'tests', 'test_gpu_tconv.py'), '-q', '-x',
                        '-m', 'gpu', '-p', 'no:cacheprovider', '-k', 'not other_gemm_modes and not repeat'],
                       env=dict(os.environ, AGCN_GEMM=mode), cwd=ROOT, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert ' passed' in r.stdout and ' skipped' not in r.stdout, r.stdout[-2000:]

