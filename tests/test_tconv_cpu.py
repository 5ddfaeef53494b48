"""CPU checks of the temporal convolution with any kernel size, stride and padding: layer construction and state-dict
parity against the reference-generated fixtures (tests/golden/make_golden_tconv.py), output frame counts, the C-ABI
symbols and the host-side domain checks of the agcn_tconv_* entry points (no device call)."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')

UNIT_FIXTURES = ['tu_k3s3p0_3_16', 'tu_k3s3p0_16_16', 'tu_k3s3p0_16_16_oddT', 'tu_k9s9p4_64_64', 'tu_k3s1p1_64_64',
                 'tu_k5s2p2_64_128', 'tu_k7s1p3_64_64_v18', 'tu_k4s1p1_64_64']
TCN_FIXTURES = ['tt_k3s1_64_64', 'tt_k5s2_64_128']
NEW_SYMBOLS = ['agcn_tconv_workspace', 'agcn_tconv_stats_tiles', 'agcn_tconv_fwd', 'agcn_tconv_bwd_data',
               'agcn_tconv_bwd_weight_workspace', 'agcn_tconv_bwd_weight']
ERR_ARG, ERR_UNSUPPORTED = -1, -3


def _gold(name):
    return dict(np.load(os.path.join(GOLDEN, name + '.npz')))


def ref_shapes(gold):
    return {k[len('shape.'):]: tuple(int(d) for d in v) for k, v in gold.items() if k.startswith('shape.')}


def our_shapes(module):
    return {k: tuple(v.shape) for k, v in module.state_dict().items()}


def graph_A(v):
    g = np.load(os.path.join(GOLDEN, 'graphs.npz'))
    return g[f'A_v{v}'].astype(np.float32)


@pytest.mark.parametrize('name', UNIT_FIXTURES)
def test_tcngcn_unit_builds_with_reference_state_dict(name):
    from agcn_amd.model import aagcn
    gold = _gold(name)
    cin, cout, k, s, pad, residual, t, v = (int(a) for a in gold['meta'][:8])
    unit = aagcn.TCNGCNUnit(cin, cout, graph_A(v), kernel_size=k, stride=s, pad=bool(pad), residual=bool(residual))
    assert our_shapes(unit) == ref_shapes(gold)
    assert unit.tcn1.pad == ((k - 1) // 2 if pad else 0)
    assert unit.tcn1.conv.padding == (unit.tcn1.pad, 0) and unit.tcn1.conv.stride == (s, 1)


@pytest.mark.parametrize('name', TCN_FIXTURES)
def test_agcn_unit_tcn_builds_with_reference_state_dict(name):
    from agcn_amd.model import agcn
    gold = _gold(name)
    cin, cout, k, s = (int(a) for a in gold['meta'][:4])
    m = agcn.unit_tcn(cin, cout, kernel_size=k, stride=s)
    assert our_shapes(m) == ref_shapes(gold)
    assert m.pad == (k - 1) // 2


def test_backbone_102_builds_with_reference_state_dict():
    from agcn_amd.model import aagcn
    gold = _gold('tm_l102_k3s3_b2_t63')
    n, t, v, num_class, c, k, s = (int(a) for a in gold['meta'][:7])
    A = graph_A(v)

    class Backbone(aagcn.BaseModel):
        def __init__(self):
            super().__init__(num_class=num_class, num_point=v, num_person=2, in_channels=3)

            def unit(_in, _out, stride=1, residual=True):
                return aagcn.TCNGCNUnit(_in, _out, A, kernel_size=k, stride=s, pad=False, residual=residual)
            self.init_model_backbone(model_layers=102, tcngcn_unit=unit, output_channel=c)
            self.init_fc(c, num_class)

    assert our_shapes(Backbone()) == ref_shapes(gold)


@pytest.mark.parametrize('layers', [1002, 1003])
def test_backbone_1002_1003_pass_padding_to_the_factory(layers):
    from agcn_amd.model import aagcn
    calls = []

    def unit(_in, _out, stride=1, residual=True, padding=None):
        calls.append((_in, _out, stride, residual, padding))
        return torch.nn.Identity()
    m = aagcn.BaseModel()
    m.init_model_backbone(model_layers=layers, tcngcn_unit=unit, output_channel=16)
    expect = [(3, 16, 1, False, True), (16, 16, 1, True, None)] if layers == 1002 else \
             [(3, 16, 1, False, True), (16, 16, 1, True, True), (16, 16, 1, True, None)]
    assert calls == expect


@pytest.mark.parametrize('k', [0, 10, 11])
def test_kernel_size_outside_1_to_9_is_refused(k):
    from agcn_amd.model import aagcn, agcn
    with pytest.raises(NotImplementedError, match='1..9'):
        aagcn.TCNUnit(16, 16, kernel_size=k)
    with pytest.raises(NotImplementedError, match='1..9'):
        agcn.unit_tcn(16, 16, kernel_size=k)


@pytest.mark.parametrize('T,k,s,pad,expect', [
    (300, 3, 3, 0, 100), (300, 9, 9, 4, 34), (300, 9, 1, None, 300), (300, 9, 2, None, 150), (64, 3, 3, 0, 21),
    (22, 1, 3, 0, 8), (31, 3, 3, 0, 10), (16, 4, 1, 1, 15), (16, 5, 2, 2, 8), (75, 3, 1, 1, 75)])
def test_conv_out_frames_with_padding(T, k, s, pad, expect):
    from agcn_amd import ops
    assert ops.conv_out_frames(T, k, s, pad) == expect
    p = (k - 1) // 2 if pad is None else pad
    assert expect == (T + 2 * p - k) // s + 1


def test_new_symbols_in_header_binding_table_and_library():
    import agcn_amd  # noqa: F401
    from agcn_amd import lib
    text = open(os.path.join(ROOT, 'include', 'agcn_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    declared = set(re.findall(r'\b(agcn_[a-z0-9_]+)\s*\(', text))
    L = lib.load()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in lib.SIGNATURES, name
        assert hasattr(L, name), name


def test_domain_and_argument_checks_return_before_any_device_call():
    import agcn_amd  # noqa: F401
    from agcn_amd import lib
    L = lib.load()
    p = 16     # any non-null address: the checks must return before touching it
    fwd = lambda taps, stride, pad, T=30, N=2: L.agcn_tconv_fwd(p, p, None, p, None, p, 1 << 20, N, 16, 16, T, 25,  # noqa: E731
                                                                   taps, stride, pad, None, None)
    assert fwd(10, 1, 0) == ERR_UNSUPPORTED
    assert fwd(0, 1, 0) == ERR_UNSUPPORTED
    assert fwd(3, 0, 0) == ERR_UNSUPPORTED
    assert fwd(3, 10, 0) == ERR_UNSUPPORTED
    assert fwd(3, 1, 2) == ERR_UNSUPPORTED          # pad > (taps-1)//2
    assert fwd(4, 1, 2) == ERR_UNSUPPORTED
    assert fwd(3, 1, -1) == ERR_UNSUPPORTED
    assert fwd(9, 9, 0, T=8) == ERR_UNSUPPORTED     # not one whole window
    assert fwd(3, 3, 0, N=0) == ERR_ARG
    assert L.agcn_tconv_fwd(None, p, None, p, None, p, 1 << 20, 2, 16, 16, 30, 25, 3, 3, 0, None, None) == ERR_ARG
    bwd = lambda taps, stride, pad: L.agcn_tconv_bwd_data(p, p, p, 0, None, None, None, None, p, 1 << 20, 2, 16, 16, 30,  # noqa: E731
                                                          25, taps, stride, pad, None, None)
    assert bwd(10, 1, 0) == ERR_UNSUPPORTED and bwd(3, 0, 0) == ERR_UNSUPPORTED and bwd(3, 1, 2) == ERR_UNSUPPORTED
    wg = lambda taps, stride, pad: L.agcn_tconv_bwd_weight(p, p, p, p, 1 << 20, 2, 16, 16, 30, 25, taps, stride, pad,  # noqa: E731
                                                           None, None, None)
    assert wg(10, 1, 0) == ERR_UNSUPPORTED and wg(3, 0, 0) == ERR_UNSUPPORTED and wg(3, 1, 2) == ERR_UNSUPPORTED
    assert L.agcn_tconv_bwd_weight(None, p, p, p, 1 << 20, 2, 16, 16, 30, 25, 3, 3, 0, None, None, None) == ERR_ARG


def test_workspace_queries():
    import agcn_amd  # noqa: F401
    from agcn_amd import lib
    L = lib.load()
    # the shapes agcn_conv_* covers report the same workspaces as before
    for args in [(64, 64, 300, 25, 9, 1), (64, 128, 300, 25, 9, 2), (64, 128, 300, 25, 1, 2)]:
        pad = (args[4] - 1) // 2
        assert L.agcn_tconv_workspace(*args, pad) == L.agcn_conv_workspace(*args)
        assert L.agcn_tconv_stats_tiles(args[0], args[1], 150, args[3], args[4], args[5], pad) == \
            L.agcn_conv_stats_tiles(args[0], args[1], 150, args[3], args[4], args[5])
    assert L.agcn_tconv_bwd_weight_workspace(128, 64, 64, 300, 25, 9, 1, 4) == \
        L.agcn_conv_bwd_weight_workspace(128, 64, 64, 300, 25, 9, 1)
    assert L.agcn_tconv_workspace(16, 16, 300, 25, 3, 3, 0) > 0
    assert L.agcn_tconv_bwd_weight_workspace(128, 16, 16, 300, 25, 3, 3, 0) > 0
    assert L.agcn_tconv_stats_tiles(16, 16, 100, 25, 3, 3, 0) >= 10
