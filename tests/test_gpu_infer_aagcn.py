"""GPU tests of the folded AAGCN inference path: ``agcn_tconv_infer`` against fp64 ``conv2d`` on the explicitly gated
input, the eval outputs of every AAGCN fixture with the fold on and off, proof that the fused route (and not
``agcn_stc_apply``) ran, cache invalidation, and process-to-process determinism.  ``-m gpu``.

Tolerances are the ones the same fixtures / the same arithmetic already carry: 1e-4 (2e-2 under AGCN_GEMM=bf16) of the
output's own max for the kernels and the ``tu_*`` / ``tm_*`` fixtures (tests/test_gpu_tconv.py), 1e-4 of max(1, max|ref|)
for the ``au_*`` / ``am_*`` fixtures (tests/test_gpu_parity_aagcn.py), which like that file are checks of the
fp32-equivalent modes: plain AGCN_GEMM=bf16 misses 1e-4 there with the fold on and off alike (measured: up to 1.7e-1 on
the 7-layer model's logits either way)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import agcn_oracle as orc
from tests import golden_util as gu

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
TOL = 1e-4


def _gpu():
    import agcn_amd  # noqa: F401
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device('cuda:0')


def _mode():
    from agcn_amd import lib
    return lib.load().agcn_gemm_mode().decode()


def _tol(base=TOL):
    return 2e-2 if _mode() == 'bf16' else base


def trel(a, ref):
    """max |a - ref| / max |ref|: the tensor's own scale."""
    a = a.detach().double().cpu()
    ref = ref.detach().double().cpu()
    return float((a - ref).abs().max() / max(float(ref.abs().max()), 1e-30))


def rnd(gen, *shape, scale=1.0):
    return torch.randn(*shape, generator=gen, dtype=torch.float64) * scale


# ---- kernel level -----------------------------------------------------------------------------------------------------
KERNEL_CASES = [
    # N, Cin, Cout, T, V, taps, stride, pad, gates present ('s' joints, 't' frames, 'c' channels), residual
    (2, 64, 64, 23, 25, 9, 1, 4, 'stc', True),       # the default AAGCN layers: 64 / 128 / 256 rows, stride 1 and 2
    (2, 128, 128, 21, 25, 9, 1, 4, 'stc', True),
    (2, 256, 256, 15, 25, 9, 1, 4, 'stc', False),
    (2, 64, 128, 31, 25, 9, 2, 4, 'stc', True),
    (2, 128, 256, 20, 18, 9, 2, 4, 'st', True),
    (2, 64, 64, 23, 25, 9, 1, 4, '', False),         # no gates: the ungated kernels
    (2, 64, 64, 23, 25, 3, 1, 1, 'stc', True),       # stride-1 3/5/7 taps
    (2, 256, 256, 15, 25, 3, 1, 1, 'stc', True),
    (2, 64, 64, 21, 25, 3, 1, 0, 'c', False),
    (2, 128, 128, 17, 25, 5, 1, 2, 'stc', True),
    (2, 64, 128, 22, 25, 5, 1, 0, '', True),
    (2, 64, 64, 20, 18, 7, 1, 3, 'stc', True),
    (2, 128, 128, 16, 25, 7, 1, 0, 's', False),
    (2, 64, 64, 30, 25, 3, 3, 0, 'stc', True),       # everything else: the exact kernel
    (2, 64, 64, 31, 25, 3, 3, 1, 't', False),
    (2, 64, 64, 36, 25, 9, 9, 4, 'stc', True),
    (2, 64, 64, 27, 25, 9, 3, 4, 'stc', True),
    (2, 64, 64, 27, 25, 9, 1, 2, 'stc', True),
    (2, 64, 64, 36, 25, 1, 9, 0, 'stc', False),
    (2, 64, 128, 21, 25, 1, 2, 0, '', True),
    (2, 32, 48, 17, 25, 1, 1, 0, 'stc', True),
    (2, 48, 32, 19, 18, 2, 1, 0, 'stc', True),
    (2, 64, 64, 19, 25, 4, 1, 1, 'stc', True),
    (2, 64, 128, 21, 25, 5, 2, 2, 'stc', True),
    (2, 32, 48, 17, 25, 6, 4, 2, 'sc', False),
    (2, 64, 64, 25, 25, 8, 2, 3, 'tc', True),
    (2, 3, 16, 30, 25, 3, 3, 0, 'stc', False),
]


def _fast_route(taps, stride, pad):
    if _mode() == 'f32':
        return False
    return (taps == 9 and pad == 4 and stride in (1, 2)) or (stride == 1 and taps in (3, 5, 7))


def _gated_reference(x, w, b, gates, res, relu, stride, pad):
    a_s, a_t, a_c = gates
    xg = x
    if a_s is not None:
        xg = xg * a_s[:, None, None, :]
    if a_t is not None:
        xg = xg * a_t[:, None, :, None]
    if a_c is not None:
        xg = xg * a_c[:, :, None, None]
    y = F.conv2d(xg, w, b, stride=(stride, 1), padding=(pad, 0))
    if res is not None:
        y = y + res
    return torch.relu(y) if relu else y


def _run_kernel_case(case, relu, gate_lo=1.0, gate_span=1.0, spike=None, with_amax=False):
    from agcn_amd import lib, ops
    dev = _gpu()
    L = lib.load()
    N, Cin, Cout, T, V, taps, stride, pad, which, with_res = case
    g = torch.Generator().manual_seed(sum(int(v) * (i + 3) for i, v in enumerate(case[:8])) + len(which))
    x = rnd(g, N, Cin, T, V)
    if spike is not None:
        x[N - 1, Cin // 2, T // 2, V // 3] = spike
    w = rnd(g, Cout, Cin, taps, 1, scale=1.0 / np.sqrt(Cin * taps))
    b = rnd(g, Cout, scale=0.1)
    a_s = gate_lo + gate_span * torch.rand(N, V, generator=g, dtype=torch.float64) if 's' in which else None
    a_t = gate_lo + gate_span * torch.rand(N, T, generator=g, dtype=torch.float64) if 't' in which else None
    a_c = gate_lo + gate_span * torch.rand(N, Cin, generator=g, dtype=torch.float64) if 'c' in which else None
    To = (T + 2 * pad - taps) // stride + 1
    res = rnd(g, N, Cout, To, V) if with_res else None
    # the reference sees the fp32 values the kernel is given
    f32 = lambda t: None if t is None else t.float()                                       # noqa: E731
    xg, wg, bg, sg, tg, cg, rg = (f32(t) for t in (x, w, b, a_s, a_t, a_c, res))
    ref = _gated_reference(xg.double(), wg.double(), bg.double(), tuple(None if t is None else t.double()
                                                                         for t in (sg, tg, cg)),
                           None if rg is None else rg.double(), relu, stride, pad)
    d = lambda t: None if t is None else t.to(dev)                                         # noqa: E731
    x_amax = d(xg).abs().max().reshape(1) if with_amax else None
    y = ops.tconv_infer(d(xg), d(wg), d(bg), d(sg), d(tg), d(cg), res=d(rg), relu=relu, stride=stride, pad=pad,
                        x_amax=x_amax)
    torch.cuda.synchronize()
    assert y is not None
    kern = L.agcn_last_kernel().decode()
    if _fast_route(taps, stride, pad):
        assert kern.startswith(('conv_pc_kernel<%d' % taps, 'conv_gemm_bf16_kernel<%d' % taps)), kern
    else:
        assert kern.startswith('conv_gemm_kernel<%d, 0, ' % taps), kern
    # gates present: the launcher names the instantiation that multiplies the operand while it is staged
    assert kern.endswith('[gates on load]') == bool(which), kern
    assert tuple(y.shape) == tuple(ref.shape)
    assert bool(torch.isfinite(y).all())
    err = trel(y, ref)
    if spike is not None:
        # the spike sits in the last sample: the first sample's rows are O(1) everywhere and are measured against their
        # own max, so the small elements' bits under the tensor-wide scale are checked, not hidden behind the spike
        err = max(err, trel(y[0], ref[0]))
    print(f'tconv_infer {case} relu={relu}: {kern}  err {err:.2e}')
    return err


@pytest.mark.parametrize('case', KERNEL_CASES)
def test_tconv_infer_vs_fp64(case):
    assert _run_kernel_case(case, relu=True) < _tol()
    assert _run_kernel_case(case, relu=False, with_amax=True) < _tol()


@pytest.mark.parametrize('case', [KERNEL_CASES[0], KERNEL_CASES[1], KERNEL_CASES[3], KERNEL_CASES[6], KERNEL_CASES[7]])
def test_tconv_infer_range_scale_bound(case):
    """Gates near 2 and one element 1e4 times the rest: the f16x3 range scale has to cover the GATED operand (an
    ungated bound would push the element past fp16's range: Inf), and the small elements still keep their bits."""
    assert _run_kernel_case(case, relu=False, gate_lo=1.9, gate_span=0.1, spike=1.0e4) < _tol()
    assert _run_kernel_case(case, relu=False, gate_lo=1.9, gate_span=0.1, spike=-3.0e4, with_amax=True) < _tol()


def test_tconv_infer_repeat_bit_identical():
    from agcn_amd import ops
    dev = _gpu()
    g = torch.Generator().manual_seed(2)
    for (C, taps, stride, pad) in [(128, 9, 1, 4), (64, 3, 1, 1), (64, 3, 3, 0)]:
        x = rnd(g, 2, C, 22, 25).float().to(dev)
        w = rnd(g, C, C, taps, 1, scale=0.05).float().to(dev)
        b = rnd(g, C).float().to(dev)
        a_s, a_t, a_c = (1 + torch.rand(2, n, generator=g).to(dev) for n in (25, 22, C))
        ys = [ops.tconv_infer(x, w, b, a_s, a_t, a_c, relu=True, stride=stride, pad=pad) for _ in range(2)]
        assert torch.equal(ys[0], ys[1])


# ---- fixtures ---------------------------------------------------------------------------------------------------------
TU_FIXTURES = ['tu_k3s3p0_3_16', 'tu_k3s3p0_16_16', 'tu_k3s3p0_16_16_oddT', 'tu_k9s9p4_64_64', 'tu_k3s1p1_64_64',
               'tu_k5s2p2_64_128', 'tu_k7s1p3_64_64_v18', 'tu_k4s1p1_64_64']
AM_FIXTURES = ['am_ntu_b1_t64', 'am_ntu_l3_t32', 'am_ntu_l3_gbn2_t32', 'am_ntu_l6_t32', 'am_ntu_l7_t32']


def _counters():
    from agcn_amd import ops
    return dict(ops.INFER_STATS)


def _delta(before):
    from agcn_amd import ops
    return {k: ops.INFER_STATS[k] - before[k] for k in before}


def _fusable(cin):
    return cin >= 32 and _mode() != 'f32'


def _expect_route(delta, n_fusable, n_attention, n_attention_fusable, fold):
    """n_fusable: units with C >= 32 (0 in AGCN_GEMM=f32); n_attention: units with gates; n_attention_fusable: those of
    them with C >= 32.  fold on: every fusable unit ran folded end to end and launched no agcn_stc_apply -- only the
    unfused units' gate passes are counted.  fold off: neither -- nothing ran folded and every unit with gates
    launched its agcn_stc_apply."""
    if fold == '1':
        assert delta['aagcn_unit_fused'] == n_fusable, delta
        assert delta['stc_apply'] == n_attention - n_attention_fusable, delta
    else:
        assert delta['aagcn_unit_fused'] == 0 and delta['tconv_infer'] == 0, delta
        assert delta['stc_apply'] == n_attention, delta


def _au_unit(name, dev):
    from agcn_amd.model.aagcn import AdaptiveGCN, NonAdaptiveGCN, TCNGCNUnit
    gold = gu.load(name)
    cin, cout, stride, residual, t, v, seed, adaptive, attention = [int(i) for i in gold['meta']]
    gbn = gu.meta_int(gold, 'meta.gbn') or None
    unit = TCNGCNUnit(cin, cout, gu.graph_A(v).numpy(), stride=stride, residual=bool(residual),
                      adaptive=AdaptiveGCN if adaptive else NonAdaptiveGCN, attention=bool(attention), gbn_split=gbn)
    shapes = orc.aagcn_unit_param_shapes('', cin, cout, v, stride, bool(residual), bool(adaptive), bool(attention), gbn)
    unit.load_state_dict(orc.aagcn_randomized_state(shapes, seed, stress=float(gold['meta.stress'])))
    unit.to(dev)
    xn, _ = gu.unit_inputs(cin, cout, stride, t, v, seed, n=gu.meta_int(gold, 'meta.n', 2))
    return unit, gold, torch.from_numpy(xn).to(dev), cin, bool(attention)


@pytest.mark.parametrize('fold', ['1', '0'])
@pytest.mark.parametrize('name', gu.AAGCN_UNIT_NAMES)
def test_au_unit_eval(name, fold, monkeypatch):
    dev = _gpu()
    monkeypatch.setenv('AGCN_INFER_FOLD', fold)
    unit, gold, x, cin, attention = _au_unit(name, dev)
    unit.eval()                                  # (a training-mode module: GhostBatchNorm collates here)
    state = {k: v.clone() for k, v in unit.state_dict().items()}
    before = _counters()
    with torch.no_grad():
        ye = unit(x)
    err = gu.rel_err(ye.cpu().numpy(), gold['y_eval'])
    print(f'{name} fold={fold}: y_eval err {err:.2e}')
    assert err < TOL
    fus = _fusable(cin)
    _expect_route(_delta(before), int(fus), int(attention), int(attention and fus), fold)
    for k, v in unit.state_dict().items():       # neither path touches parameters or running statistics
        assert torch.equal(v, state[k]), k


def _tu_unit(name, dev):
    from agcn_amd.model import aagcn
    gold = dict(np.load(os.path.join(GOLDEN, name + '.npz')))
    cin, cout, k, s, pad, residual, t, v, seed, n = (int(a) for a in gold['meta'])
    A = np.load(os.path.join(GOLDEN, 'graphs.npz'))[f'A_v{v}'].astype(np.float32)
    unit = aagcn.TCNGCNUnit(cin, cout, A, kernel_size=k, stride=s, pad=bool(pad), residual=bool(residual))
    shapes = {kk[len('shape.'):]: tuple(int(d) for d in vv) for kk, vv in gold.items() if kk.startswith('shape.')}
    unit.load_state_dict(orc.aagcn_randomized_state(shapes, seed, stress=float(gold['meta.stress'])))
    return unit.to(dev), gold, cin


@pytest.mark.parametrize('fold', ['1', '0'])
@pytest.mark.parametrize('name', TU_FIXTURES)
def test_tu_unit_eval(name, fold, monkeypatch):
    dev = _gpu()
    monkeypatch.setenv('AGCN_INFER_FOLD', fold)
    unit, gold, cin = _tu_unit(name, dev)
    unit.eval()
    before = _counters()
    with torch.no_grad():
        ye = unit(torch.from_numpy(gold['x']).to(dev))
    err = trel(ye, torch.from_numpy(gold['y_eval']))
    print(f'{name} fold={fold}: y_eval err {err:.2e}')
    assert err < _tol()
    fus = _fusable(cin)
    _expect_route(_delta(before), int(fus), 1, int(fus), fold)


def _am_model(name, dev):
    from model.aagcn import Model
    gold = gu.load(name)
    n, v, num_class, seed, t = [int(i) for i in gold['meta']]
    layers, gbn = gu.meta_int(gold, 'meta.layers', 10), gu.meta_int(gold, 'meta.gbn') or None
    model = Model(num_class=num_class, num_point=v, num_person=2, graph='graph.ntu_rgb_d.Graph',
                  graph_args=dict(labeling_mode='spatial'), model_layers=layers, gbn_split=gbn)
    shapes = orc.aagcn_model_param_shapes(num_class, v, model_layers=layers, gbn_split=gbn)
    model.load_state_dict(orc.aagcn_randomized_state(shapes, seed, stress=float(gold['meta.stress'])))
    xn, _ = gu.model_inputs(n, v, num_class, seed, t)
    return model.to(dev), gold, torch.from_numpy(xn).to(dev), layers


@pytest.mark.parametrize('fold', ['1', '0'])
@pytest.mark.parametrize('name', AM_FIXTURES)
def test_am_model_eval(name, fold, monkeypatch):
    dev = _gpu()
    monkeypatch.setenv('AGCN_INFER_FOLD', fold)
    model, gold, x, layers = _am_model(name, dev)
    model.eval()
    before = _counters()
    with torch.no_grad():
        le, aux = model(x)
    assert aux is None
    err = gu.rel_err(le.cpu().numpy(), gold['logits_eval'])
    print(f'{name} fold={fold}: logits_eval err {err:.2e}')
    assert err < TOL
    # every layer but the 3-channel first one has C >= 32; the first one keeps its own gate pass
    nf = (layers - 1) if _mode() != 'f32' else 0
    _expect_route(_delta(before), nf, layers, nf, fold)


@pytest.mark.parametrize('fold', ['1', '0'])
def test_backbone_102_eval(fold, monkeypatch):
    from agcn_amd.model import aagcn
    dev = _gpu()
    monkeypatch.setenv('AGCN_INFER_FOLD', fold)
    gold = dict(np.load(os.path.join(GOLDEN, 'tm_l102_k3s3_b2_t63.npz')))
    n, t, v, num_class, c, k, s, seed = (int(a) for a in gold['meta'])
    A = np.load(os.path.join(GOLDEN, 'graphs.npz'))[f'A_v{v}'].astype(np.float32)

    class Backbone(aagcn.BaseModel):
        def __init__(self):
            super().__init__(num_class=num_class, num_point=v, num_person=2, in_channels=3)

            def unit(_in, _out, stride=1, residual=True):
                return aagcn.TCNGCNUnit(_in, _out, A, kernel_size=k, stride=s, pad=False, residual=residual)
            self.init_model_backbone(model_layers=102, tcngcn_unit=unit, output_channel=c)
            self.init_fc(c, num_class)

    m = Backbone()
    shapes = {kk[len('shape.'):]: tuple(int(d) for d in vv) for kk, vv in gold.items() if kk.startswith('shape.')}
    m.load_state_dict(orc.aagcn_randomized_state(shapes, seed, stress=float(gold['meta.stress'])))
    m.to(dev).eval()
    before = _counters()
    with torch.no_grad():
        le, _ = m(torch.from_numpy(gold['x']).to(dev))
    err = trel(le, torch.from_numpy(gold['y_eval']))
    print(f'tm_l102_k3s3_b2_t63 fold={fold}: logits_eval err {err:.2e}')
    assert err < _tol()
    nf = 1 if _fusable(c) else 0                 # l1 is the 3-channel layer, l2 has c channels
    _expect_route(_delta(before), nf, 2, nf, fold)


# ---- cache and statistics -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['au_64_128_s2_v25', 'au_64_64_s1_v25_gbn2'])
def test_folded_weights_follow_the_parameters(name, monkeypatch):
    """After a training step and train() -> eval() the folded weights are rebuilt: the output changes and matches the
    unfused passes on the same parameters; folding itself modifies no parameter or running statistic (bitwise)."""
    dev = _gpu()
    monkeypatch.setenv('AGCN_INFER_FOLD', '1')
    unit, gold, x, cin, _ = _au_unit(name, dev)
    fus = _fusable(cin)                          # (AGCN_GEMM=f32 has no folded route: the same checks on its passes)
    unit.eval()
    with torch.no_grad():
        y0 = unit(x)
    assert ('folded' in unit.__dict__['_infer_cache']) == fus
    unit.train()
    assert '_infer_cache' not in unit.__dict__
    opt = torch.optim.SGD(unit.parameters(), lr=0.05)
    unit(x).square().mean().backward()
    opt.step()
    unit.eval()
    state = {k: v.clone() for k, v in unit.state_dict().items()}
    before = _counters()
    with torch.no_grad():
        y1 = unit(x)
        y1_again = unit(x)                       # second call: served from the cache
    assert _delta(before)['aagcn_unit_fused'] == (2 if fus else 0)
    for k, v in unit.state_dict().items():
        assert torch.equal(v, state[k]), k
    assert torch.equal(y1, y1_again)
    monkeypatch.setenv('AGCN_INFER_FOLD', '0')
    with torch.no_grad():
        y1_unfused = unit(x)
    assert gu.rel_err(y1.cpu().numpy(), y1_unfused.cpu().numpy()) < TOL
    assert gu.rel_err(y1.cpu().numpy(), y0.cpu().numpy()) > 10 * TOL      # the step did move the output
    # in-place edit of one BatchNorm statistic in eval mode: seen through the tensor's version counter
    monkeypatch.setenv('AGCN_INFER_FOLD', '1')
    with torch.no_grad():
        unit.tcn1.bn.running_mean.add_(0.5)
        y2 = unit(x)
        monkeypatch.setenv('AGCN_INFER_FOLD', '0')
        y2_unfused = unit(x)
    assert gu.rel_err(y2.cpu().numpy(), y2_unfused.cpu().numpy()) < TOL
    assert not torch.equal(y2, y1)


# ---- the same driver under the AGCN unit -----------------------------------------------------------------------------------
AGCN_UNIT = (64, 128, 2, 2, 24, 25, 7)           # cin, cout, stride, n, t, v, seed


def _agcn_unit(dev):
    from agcn_amd.model.agcn import TCN_GCN_unit
    cin, cout, stride, n, t, v, seed = AGCN_UNIT
    unit = TCN_GCN_unit(cin, cout, gu.graph_A(v).numpy(), stride=stride)
    unit.load_state_dict(orc.randomized_state(orc.unit_param_shapes('', cin, cout, v, stride, True), seed, stress=4.0))
    xn, _ = gu.unit_inputs(cin, cout, stride, t, v, seed, n=n)
    return unit.to(dev).eval(), torch.from_numpy(xn).to(dev)


_UNFUSED_CHILD = r'''
import sys, numpy as np, torch
sys.path.insert(0, %(root)r)
import agcn_amd
from tests.test_gpu_infer_aagcn import _agcn_unit
from agcn_amd import ops
unit, x = _agcn_unit(torch.device('cuda:0'))
with torch.no_grad():
    y = unit(x)
torch.cuda.synchronize()
assert ops.INFER_STATS['aagcn_unit_fused'] == 0 and ops.INFER_STATS['tconv_infer'] == 0, ops.INFER_STATS
np.save(%(out)r, y.cpu().numpy())
'''


def test_agcn_unit_folded_route_cache_and_fold_off(tmp_path, monkeypatch):
    """An AGCN TCN_GCN_unit(64, 128, stride 2) in eval under no_grad runs folded end to end through ``ops.unit_infer``
    (9-tap temporal convolution on ``agcn_tconv_infer``), keeps its folded weights between calls, rebuilds them after
    ``note_params_changed`` and equals the unfused eval passes of a process with AGCN_INFER_FOLD=0."""
    from agcn_amd import ops
    dev = _gpu()
    monkeypatch.setenv('AGCN_INFER_FOLD', '1')
    fus = int(_fusable(AGCN_UNIT[0]))
    unit, x = _agcn_unit(dev)
    before = _counters()
    with torch.no_grad():
        y = unit(x)
    d = _delta(before)
    assert d['aagcn_unit_fused'] == fus and d['tconv_infer'] == fus and d['stc_apply'] == 0, d
    if fus:
        entry = unit.__dict__['_infer_cache']['folded']
        with torch.no_grad():
            y_again = unit(x)
        assert unit.__dict__['_infer_cache']['folded'] is entry           # served from the cache
        ops.note_params_changed()
        with torch.no_grad():
            y_rebuilt = unit(x)
        rebuilt = unit.__dict__['_infer_cache']['folded']
        assert rebuilt is not entry and rebuilt[0] != entry[0]
        assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(entry[1:], rebuilt[1:]))
        assert torch.equal(y, y_again) and torch.equal(y, y_rebuilt)
    out = str(tmp_path / 'y_unfused.npy')
    r = subprocess.run([sys.executable, '-c', _UNFUSED_CHILD % dict(root=ROOT, out=out)], cwd=ROOT,
                       env=dict(os.environ, AGCN_INFER_FOLD='0'), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    err = gu.rel_err(y.cpu().numpy(), np.load(out))
    print(f'AGCN unit folded vs unfused: {err:.2e}')
    assert err < TOL


# ---- determinism ---------------------------------------------------------------------------------------------------------
_CHILD = r'''
import hashlib, sys, torch
sys.path.insert(0, %(root)r)
import agcn_amd
from tests.test_gpu_infer_aagcn import _am_model
from agcn_amd import ops
model, gold, x, layers = _am_model('am_ntu_b1_t64', torch.device('cuda:0'))
model.eval()
with torch.no_grad():
    le, _ = model(x)
torch.cuda.synchronize()
print('FUSED', ops.INFER_STATS['aagcn_unit_fused'])
print('SHA', hashlib.sha256(le.cpu().numpy().tobytes()).hexdigest())
'''


def test_eval_logits_bit_identical_across_processes():
    _gpu()
    outs = []
    for _ in range(2):
        env = dict(os.environ, AGCN_INFER_FOLD='1')
        r = subprocess.run([sys.executable, '-c', _CHILD % dict(root=ROOT)], env=env, cwd=ROOT, capture_output=True,
                           text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        lines = dict(ln.split(' ', 1) for ln in r.stdout.splitlines() if ln.startswith(('SHA ', 'FUSED ')))
        outs.append(lines)
    assert outs[0]['SHA'] == outs[1]['SHA'], outs
    if _mode() != 'f32':
        assert int(outs[0]['FUSED']) == 9, outs

