"""CPU checks of aagcn_v24: the module's state_dict against the reference-generated fixtures, its class paths, the
argument combinations it refuses, the C-ABI argument and domain errors of the new encoder entry points (returned before
any HIP call, so no GPU is needed), the plan checker tests/encoder_v24_plan_check.cpp, the tensor-code forms against
torch's own modules in fp64, and the mutants the fixtures store."""
import ctypes
import importlib
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import v24_util as vu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model(name, cfg=None, **over):
    from agcn_amd.model import aagcn_v24
    return aagcn_v24.Model(**dict(vu.model_kwargs(name, **(cfg or {})), **over))


@pytest.mark.parametrize('name', vu.NAMES)
def test_state_dict_matches_reference(name):
    import agcn_amd  # noqa: F401
    gold = vu.load(name)
    shapes = vu.shapes_of(gold)
    m = _model(name)
    mine = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert mine == shapes
    m.load_state_dict(vu.state(shapes, name), strict=True)
    params = dict(m.named_parameters())
    kw = vu.model_kwargs(name)
    assert ('s_pos_encoder.pe' in params) == (kw['pos_enc'] == 'True')
    assert ('s_pos_encoder.pe' in shapes) == (kw['pos_enc'] in ('True', 'cossin'))
    assert 'alpha' in params and 's_cls_token' in params
    pas = [k for k in params if k.endswith('.PA') and k.startswith('s_trans_enc_layers.')]
    assert len(pas) == (2 if vu.has_bias(name) else 0)
    for k in pas:
        assert shapes[k] == ((3, 51, 51) if kw['add_A'] == 'triple' else (51, 51))
        assert ('g.' + k + '.absmax') in gold
    assert ('g.alpha.absmax' in gold) == vu.has_bias(name)            # no bias: the reference leaves alpha without a gradient
    x, _ = vu.inputs(name)
    assert np.array_equal(x, gold['x']) and np.array_equal(vu.window_mask(x), gold['frame_mask'])
    assert list(gold['attn_seq']) == vu.attn_sequences(name)
    # sample 0 is null from frame 24 (window 8), sample 1 from frame 18 (window 6)
    want = np.zeros_like(gold['frame_mask'])
    want[0, 8:] = 1
    want[1, 6:] = 1
    assert np.array_equal(gold['frame_mask'], want)


def test_fresh_parameters_are_the_reference_initialisation():
    import agcn_amd  # noqa: F401
    from agcn_amd.model import aagcn_v24
    for name in ('tv24_shipped', 'tv24_triple'):
        m = _model(name)
        assert float(m.alpha.detach()) == 0.0
        for layer in m.s_trans_enc_layers:
            assert np.array_equal(layer.PA.detach().numpy(), vu.pa_init(name))
        assert m.s_trans_enc_layers[0].PA is not m.s_trans_enc_layers[1].PA            # deep copies
    m = _model('tv24_shipped')
    assert isinstance(m.s_pos_encoder, aagcn_v24.CosSinPositionalEncoding)
    assert torch.equal(m.s_pos_encoder.pe, vu.cossin_table((1, 100, 24)))
    assert _model('tv24_plain_kinetics').s_trans_enc_layers[0].PA is None


def test_both_class_paths_resolve():
    import agcn_amd  # noqa: F401
    from agcn_amd.model import aagcn_v24
    for path in ('model.aagcn_v24', 'model.architecture.aagcn.aagcn_v24'):
        mod = importlib.import_module(path)
        assert mod.Model is aagcn_v24.Model
        for n in ('PositionalEncoding', 'CosSinPositionalEncoding', 'TransformerEncoderLayerExt',
                  'TransformerEncoderLayerExtV2', 'TransformerEncoderExt', 'transformer_config_checker'):
            assert getattr(mod, n) is getattr(aagcn_v24, n)


def test_layer_is_a_transformer_encoder_layer():
    import agcn_amd  # noqa: F401
    from agcn_amd.model import aagcn_v17, aagcn_v24
    layer = aagcn_v24.TransformerEncoderLayerExt(8, 2, 16, 0.0, 'gelu', 1e-5, True, pre_norm=True, A=np.ones((5, 5)))
    assert isinstance(layer, torch.nn.TransformerEncoderLayer) and isinstance(layer, aagcn_v17.TransformerEncoderLayerExt)
    assert layer.pre_norm and isinstance(layer.PA, torch.nn.Parameter) and layer.PA.dtype == torch.float32
    stock = sorted(torch.nn.TransformerEncoderLayer(8, 2, 16, batch_first=True).state_dict())
    assert sorted(layer.state_dict()) == sorted(stock + ['PA'])
    cfg = dict(model_dim=8, num_heads=2, ffn_dim=16, dropout=0.0, activation='relu', layer_norm_eps=1e-5, batch_first=True,
               prenorm=False)
    v2 = aagcn_v24.TransformerEncoderLayerExtV2(cfg)
    assert v2.PA is None and sorted(v2.state_dict()) == stock and not v2.pre_norm
    enc = aagcn_v24.TransformerEncoderExt(v2, 2, need_attn=True)
    assert isinstance(enc, torch.nn.TransformerEncoder) and len(enc.layers) == 2
    aagcn_v24.transformer_config_checker(dict(cfg, num_layers=2))
    with pytest.raises(AssertionError, match='not in transformer config'):
        aagcn_v24.transformer_config_checker(dict(cfg, heads=2))
    with pytest.raises(ValueError, match='bias'):
        v2(torch.zeros(1, 5, 8), src_mask=torch.zeros(5, 5))


def test_refusals():
    import agcn_amd  # noqa: F401
    for ct in ('GAP', 'MAX', 'None'):
        with pytest.raises(ValueError, match='classifier_type'):
            _model('tv24_shipped', classifier_type=ct)
    kin = dict(num_point=18, graph='graph.kinetics.Graph')
    for add_A in ('single', 'triple'):
        with pytest.raises(ValueError, match='add_A.*num_point=25.*num_person=2'):
            _model('tv24_triple', add_A=add_A, **kin)
        with pytest.raises(ValueError, match='add_A.*num_point=25.*num_person=2'):
            _model('tv24_triple', add_A=add_A, num_person=1)
    _model('tv24_plain_kinetics', num_person=1)                        # without a bias any skeleton will do
    with pytest.raises(ValueError, match="triple.*num_heads=3"):
        _model('tv24_triple', cfg=dict(num_heads=2))
    _model('tv24_shipped', cfg=dict(num_heads=2))                      # a shared bias fits any head count
    with pytest.raises(ValueError, match='positional table'):
        _model('tv24_plain_kinetics', pos_enc='cossin', num_point=25, graph='graph.ntu_rgb_d.Graph', num_person=4)
    _model('tv24_plain_kinetics', pos_enc='False', num_point=25, graph='graph.ntu_rgb_d.Graph', num_person=4)
    with pytest.raises(NotImplementedError):
        from agcn_amd.model.aagcn import BaseModel
        BaseModel(data_norm='ln')


def test_v24_abi_errors_without_gpu():
    import agcn_amd  # noqa: F401
    from agcn_amd import lib
    L = lib.load()
    p = ctypes.c_void_p(4096)        # never dereferenced: every call below returns before its first HIP call
    ARG, WS, UNS = lib.ERR_ARG, lib.ERR_WORKSPACE, lib.ERR_UNSUPPORTED
    big = 1 << 40
    # spatial tokens: (x, cls, pe, pe_rows, tok, N, M, C, Tp, V)
    assert L.agcn_tokens_spatial_fwd(None, None, None, 0, p, 1, 1, 1, 1, 1, None) == ARG
    assert L.agcn_tokens_spatial_fwd(p, None, None, 0, None, 1, 1, 1, 1, 1, None) == ARG
    assert L.agcn_tokens_spatial_fwd(p, None, None, 0, p, 1, 1, 0, 1, 1, None) == ARG
    assert L.agcn_tokens_spatial_fwd(p, p, p, 50, p, 2, 2, 24, 10, 25, None) == ARG            # 51 tokens, 50 table rows
    assert L.agcn_tokens_spatial_fwd(p, p, None, 0, p, 2, 2, 16, 10, 320, None) == UNS          # 641 tokens
    assert L.agcn_tokens_spatial_fwd(p, None, None, 0, p, 2, 2, 2049, 10, 1, None) == UNS        # C > 2048
    assert L.agcn_tokens_spatial_fwd(p, None, None, 0, p, 2, 2, 328, 10, 24, None) == UNS        # one frame > the tile
    assert L.agcn_tokens_spatial_fwd(p, None, None, 0, p, 2097121, 1, 1, 1, 1, None) == UNS      # sequences
    # (dtok, dx, dcls, dpe, has_cls, pe_rows, ws, ws_bytes, N, M, C, Tp, V)
    assert L.agcn_tokens_spatial_bwd(None, p, None, None, 0, 0, None, 0, 1, 1, 1, 1, 1, None) == ARG
    assert L.agcn_tokens_spatial_bwd(p, p, p, None, 0, 0, p, big, 1, 1, 1, 1, 1, None) == ARG     # dcls without a CLS token
    assert L.agcn_tokens_spatial_bwd(p, p, None, None, 2, 0, None, 0, 1, 1, 1, 1, 1, None) == ARG
    assert L.agcn_tokens_spatial_bwd(p, p, p, None, 1, 0, None, 0, 1, 1, 1, 1, 1, None) == ARG    # sums without a slab
    assert L.agcn_tokens_spatial_bwd(p, p, None, p, 1, 50, p, big, 2, 2, 24, 10, 25, None) == ARG
    assert L.agcn_tokens_spatial_bwd(p, p, None, None, 1, 0, None, 0, 2, 2, 16, 10, 320, None) == UNS
    need = L.agcn_tokens_spatial_bwd_workspace(2, 2, 24, 10, 25, 1)
    assert need == 1 * 51 * 24 * 4                                      # 20 sequences: one slot of 32
    assert L.agcn_tokens_spatial_bwd_workspace(64, 2, 144, 100, 25, 1) == 200 * 51 * 144 * 4
    assert L.agcn_tokens_spatial_bwd_workspace(2, 2, 16, 10, 320, 1) == 0
    assert L.agcn_tokens_spatial_bwd(p, p, p, None, 1, 0, p, need - 1, 2, 2, 24, 10, 25, None) == WS
    # attention with a bias: (qkv, bias, Hb, null_tok, causal, keep, keep_scale, ctx, prob, avg, N, L, H, dh)
    assert L.agcn_mha_bias_fwd(None, p, 1, None, 0, None, 1.0, p, None, None, 1, 2, 3, 1, None) == ARG
    assert L.agcn_mha_bias_fwd(p, None, 1, None, 0, None, 1.0, p, None, None, 1, 2, 3, 1, None) == ARG
    assert L.agcn_mha_bias_fwd(p, p, 1, None, 0, None, 1.0, None, None, None, 1, 2, 3, 1, None) == ARG
    for hb in (0, 2, 4, -1):
        assert L.agcn_mha_bias_fwd(p, p, hb, None, 0, None, 1.0, p, None, None, 1, 2, 3, 1, None) == ARG
    assert L.agcn_mha_bias_fwd(p, p, 1, None, 3, None, 1.0, p, None, None, 1, 2, 3, 1, None) == ARG
    assert L.agcn_mha_bias_fwd(p, p, 1, None, 0, None, 1.0, p, None, None, 1, 0, 3, 1, None) == ARG
    assert L.agcn_mha_bias_fwd(p, p, 1, None, 0, None, 1.0, p, None, None, 1, 641, 1, 8, None) == UNS
    assert L.agcn_mha_bias_fwd(p, p, 3, None, 0, None, 1.0, p, None, None, 1, 8, 3, 257, None) == UNS
    assert L.agcn_mha_bias_fwd(p, p, 9, None, 0, None, 1.0, p, None, None, 1, 8, 9, 256, None) == UNS
    # (ds, dbias, ws, ws_bytes, N, L, H, Hb)
    assert L.agcn_mha_bias_grad(None, p, p, big, 1, 2, 3, 1, None) == ARG
    assert L.agcn_mha_bias_grad(p, None, p, big, 1, 2, 3, 1, None) == ARG
    assert L.agcn_mha_bias_grad(p, p, None, big, 1, 2, 3, 1, None) == ARG
    assert L.agcn_mha_bias_grad(p, p, p, big, 0, 2, 3, 1, None) == ARG
    for hb in (0, 2, 4):
        assert L.agcn_mha_bias_grad(p, p, p, big, 1, 2, 3, hb, None) == ARG
        assert L.agcn_mha_bias_grad_workspace(1, 2, 3, hb) == 0
    assert L.agcn_mha_bias_grad(p, p, p, big, 1, 641, 3, 1, None) == UNS
    assert L.agcn_mha_bias_grad(p, p, p, big, 2097121, 2, 3, 1, None) == UNS
    assert L.agcn_mha_bias_grad_workspace(1, 641, 3, 1) == 0
    assert L.agcn_mha_bias_grad_workspace(6400, 51, 3, 1) == 200 * 51 * 51 * 4
    assert L.agcn_mha_bias_grad_workspace(33, 51, 3, 3) == 2 * 3 * 51 * 51 * 4
    assert L.agcn_mha_bias_grad(p, p, p, 2 * 3 * 51 * 51 * 4 - 1, 33, 51, 3, 3, None) == WS


def test_encoder_v24_plan_checker(tmp_path):
    cxx = next((c for c in (os.environ.get('CXX'), 'c++', 'g++', 'clang++') if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip('no host C++ compiler')
    exe = str(tmp_path / 'encoder_v24_plan_check')
    r = subprocess.run([cxx, '-std=c++17', '-Wall', '-Werror', '-O1', '-I', os.path.join(ROOT, '2s-agcn_amd', 'csrc'),
                        os.path.join(ROOT, 'tests', 'encoder_v24_plan_check.cpp'), '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-4000:]
    assert ' cases, 0 failures' in r.stdout and int(r.stdout.split(' cases')[0].split()[-1]) > 300000


def test_tensor_code_forms_agree_with_torch():
    """ops.tokens_spatial_ref against the reference's permute / reshape / cat expression (aagcn_v24.py:287-292) and
    ops.mha_ref(bias=...) against nn.MultiheadAttention with a float attn_mask, Hb = 1 and Hb = H, in fp64 on the CPU."""
    import agcn_amd  # noqa: F401
    from agcn_amd import ops
    g = torch.Generator().manual_seed(24)
    N, M, C, T, V = 2, 2, 6, 3, 5
    x = torch.randn(N * M, C, T, V, generator=g, dtype=torch.float64)
    cls = torch.randn(1, 1, C, generator=g, dtype=torch.float64)
    pe = torch.randn(1, 14, C, generator=g, dtype=torch.float64)
    s_x = x.view(N, M, C, T, V).permute(0, 3, 1, 4, 2).contiguous().reshape(N * T, M * V, C)
    assert torch.equal(ops.tokens_spatial_ref(x, None, None, M), s_x)
    want = torch.cat((cls.repeat(N * T, 1, 1), s_x), dim=1)
    assert torch.equal(ops.tokens_spatial_ref(x, cls, None, M), want)
    want = want + pe[:, :want.size(1), :]
    assert float((ops.tokens_spatial_ref(x, cls, pe, M) - want).abs().max()) < 1e-12
    with pytest.raises(ValueError, match='pe must be'):
        ops.tokens_spatial_ref(x, cls, pe[:, :10], M)
    Nq, L, H, dh = 3, 7, 3, 4
    D = H * dh
    mha = torch.nn.MultiheadAttention(D, H, batch_first=True).double()
    mha.requires_grad_(False)
    t = torch.randn(Nq, L, D, generator=g, dtype=torch.float64)
    qkv = torch.nn.functional.linear(t, mha.in_proj_weight, mha.in_proj_bias)
    for Hb in (1, H):
        bias = 2.0 * torch.randn(Hb, L, L, generator=g, dtype=torch.float64)
        mask = bias[0] if Hb == 1 else bias.repeat(Nq, 1, 1)          # (N*H, L, L): slice h for head h of every sequence
        want, wavg = mha(t, t, t, attn_mask=mask)
        ctx, avg = ops.mha_ref(qkv, H, need_avg=True, bias=bias)
        got = torch.nn.functional.linear(ctx, mha.out_proj.weight, mha.out_proj.bias)
        assert float((got - want).abs().max()) < 1e-12 and float((avg - wavg).abs().max()) < 1e-12
        plain, _ = ops.mha_ref(qkv, H)
        assert float((plain - ctx).abs().max()) > 1e-2                # the bias is not a no-op here
    with pytest.raises(ValueError, match='bias must be'):
        ops.mha_ref(qkv, H, bias=torch.zeros(2, L, L, dtype=torch.float64))


@pytest.mark.parametrize('name', [n for n in vu.NAMES if vu.has_bias(n)])
def test_stored_mutants_move_the_logits(name):
    gold = vu.load(name)
    y = gold['y_eval'].astype(np.float64)
    assert vu.mutants(name) and sorted(k[4:] for k in gold if k.startswith('mut.')) == sorted(vu.mutants(name))
    for mutant in vu.mutants(name):
        moved = float(np.abs(gold['mut.' + mutant] - y).max() / np.abs(y).max())
        print(name, mutant, f'{moved:.3e}')
        assert moved >= vu.MUTANT_MOVE, (mutant, moved)
    assert not any(k.startswith('mut.') for k in vu.load('tv24_plain_kinetics'))
