"""CPU checks of aagcn_v17: the module's state_dict against the reference-generated fixtures, its class paths, the
argument combinations it refuses, the host-side frame mask, the C-ABI argument and domain errors of the six encoder entry
points (returned before any HIP call, so no GPU is needed), and the plan checker tests/encoder_plan_check.cpp."""
import ctypes
import importlib
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import v17_util as vu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model(name, **over):
    from agcn_amd.model import aagcn_v17
    return aagcn_v17.Model(**dict(vu.model_kwargs(name), **over))


@pytest.mark.parametrize('name', vu.NAMES)
def test_state_dict_matches_reference(name):
    import agcn_amd  # noqa: F401
    gold = vu.load(name)
    shapes = vu.shapes_of(gold)
    m = _model(name)
    mine = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert mine == shapes
    m.load_state_dict(vu.state(shapes, name), strict=True)
    pe_is_param = 'pos_encoder.pe' in dict(m.named_parameters())
    assert pe_is_param == (vu.model_kwargs(name)['pos_enc'] == 'True')
    assert ('g.pos_encoder.pe.absmax' in gold) == pe_is_param
    assert ('cls_token' in shapes) == (vu.model_kwargs(name)['classifier_type'] == 'CLS')


def test_both_class_paths_resolve():
    import agcn_amd  # noqa: F401
    from agcn_amd.model import aagcn_v17
    for path in ('model.aagcn_v17', 'model.architecture.aagcn.aagcn_v17'):
        mod = importlib.import_module(path)
        assert mod.Model is aagcn_v17.Model
        for n in ('PositionalEncoding', 'CosSinPositionalEncoding', 'TransformerEncoderLayerExt',
                  'generate_square_subsequent_mask'):
            assert getattr(mod, n) is getattr(aagcn_v17, n)


def test_layer_is_a_transformer_encoder_layer():
    import agcn_amd  # noqa: F401
    from agcn_amd.model import aagcn_v17
    layer = aagcn_v17.TransformerEncoderLayerExt(8, 2, 16, 0.0, 'gelu', 1e-5, True, pre_norm=True)
    assert isinstance(layer, torch.nn.TransformerEncoderLayer) and layer.pre_norm
    assert sorted(layer.state_dict()) == sorted(torch.nn.TransformerEncoderLayer(8, 2, 16, batch_first=True).state_dict())
    m = aagcn_v17.generate_square_subsequent_mask(4, 'cpu')
    assert torch.equal(m == 0, torch.tril(torch.ones(4, 4)).bool()) and bool(torch.isinf(m[0, 1]))


@pytest.mark.parametrize('masking', ['True', 'frame', 'forward', 'backward'])
def test_masks_need_cls_and_one_windowing_layer(masking):
    import agcn_amd  # noqa: F401
    with pytest.raises(ValueError, match='attn_masking.*classifier_type.*model_layers'):
        _model('tv17_shipped', attn_masking=masking, classifier_type='GAP')
    with pytest.raises(ValueError, match='attn_masking.*classifier_type.*model_layers'):
        _model('tv17_shipped', attn_masking=masking, model_layers=102)
    m = _model('tv17_shipped', attn_masking=masking)
    with pytest.raises(ValueError, match='kernel_size'):
        m(torch.zeros(1, 3, 31, 25, 2))


def test_other_refusals():
    import agcn_amd  # noqa: F401
    with pytest.raises(NotImplementedError):
        _model('tv17_shipped', data_norm='ln')
    with pytest.raises(ValueError, match='classifier_type'):
        _model('tv17_shipped', classifier_type='MAX')
    m = _model('tv17_shipped')
    with pytest.raises(ValueError, match='null_tok'):
        m.trans_enc[0](torch.zeros(1, 21, 400), src_mask=torch.zeros(21, 21))


@pytest.mark.parametrize('name', vu.NAMES)
def test_frame_mask_matches_reference(name):
    import agcn_amd  # noqa: F401
    from agcn_amd.model import aagcn_v17
    gold = vu.load(name)
    x, _ = vu.inputs(name)
    assert np.array_equal(x, gold['x'])
    mask = aagcn_v17.frame_null_tokens(torch.from_numpy(x), 3)
    assert mask.dtype == torch.uint8 and np.array_equal(mask.numpy(), gold['frame_mask'])
    if name == 'tv17_frame':
        # sample 1 null from frame 18 (window 6) on, person 1 from frame 24 (window 8) on; position 1 + t*M + m
        want = np.zeros((2, 21), np.uint8)
        want[1, 1 + 6 * 2:] = 1
        want[0, [1 + 8 * 2 + 1, 1 + 9 * 2 + 1]] = 1
        assert np.array_equal(gold['frame_mask'], want)


def test_encoder_abi_errors_without_gpu():
    import agcn_amd  # noqa: F401
    from agcn_amd import lib
    L = lib.load()
    p = ctypes.c_void_p(4096)        # never dereferenced: every call below returns before its first HIP call
    ARG, WS, UNS = -1, -2, -3
    # tokens
    assert L.agcn_tokens_fwd(None, None, None, 0, p, 1, 1, 1, 1, 1, None) == ARG
    assert L.agcn_tokens_fwd(p, None, None, 0, p, 1, 1, 0, 1, 1, None) == ARG
    assert L.agcn_tokens_fwd(p, p, p, 20, p, 2, 2, 16, 10, 25, None) == ARG            # 21 tokens, 20 table rows
    assert L.agcn_tokens_fwd(p, p, None, 0, p, 2, 2, 16, 320, 25, None) == UNS          # 641 tokens
    assert L.agcn_tokens_fwd(p, None, None, 0, p, 2, 2, 128, 10, 25, None) == UNS        # D = 3200
    assert L.agcn_tokens_bwd(None, p, None, None, 0, 0, 1, 1, 1, 1, 1, None) == ARG
    assert L.agcn_tokens_bwd(p, p, p, None, 0, 0, 1, 1, 1, 1, 1, None) == ARG             # dcls without a CLS token
    assert L.agcn_tokens_bwd(p, p, None, p, 1, 20, 2, 2, 16, 10, 25, None) == ARG
    assert L.agcn_tokens_bwd(p, p, None, None, 1, 0, 2, 2, 16, 320, 25, None) == UNS
    # attention core
    assert L.agcn_mha_fwd(None, None, 0, None, 1.0, p, None, None, 1, 2, 1, 1, None) == ARG
    assert L.agcn_mha_fwd(p, None, 3, None, 1.0, p, None, None, 1, 2, 1, 1, None) == ARG
    assert L.agcn_mha_fwd(p, None, 0, None, 1.0, p, None, None, 1, 0, 1, 1, None) == ARG
    assert L.agcn_mha_fwd(p, None, 0, None, 1.0, p, None, None, 1, 641, 1, 8, None) == UNS
    assert L.agcn_mha_fwd(p, None, 0, None, 1.0, p, None, None, 1, 8, 1, 257, None) == UNS
    assert L.agcn_mha_fwd(p, None, 0, None, 1.0, p, None, None, 1, 8, 9, 256, None) == UNS
    assert L.agcn_mha_bwd(p, p, None, None, 1.0, p, p, 1 << 30, 1, 2, 1, 1, None) == ARG   # no probabilities
    assert L.agcn_mha_bwd(p, p, p, None, 1.0, p, None, 0, 1, 2, 1, 1, None) == ARG
    assert L.agcn_mha_bwd(p, p, p, None, 1.0, p, p, 1 << 30, 1, 641, 1, 8, None) == UNS
    assert L.agcn_mha_bwd(p, p, p, None, 1.0, p, p, 2 * 2 * 21 * 21 * 4 - 1, 2, 21, 2, 200, None) == WS
    # LayerNorm
    assert L.agcn_ln_fwd(p, None, None, p, 1e-5, p, p, p, 4, 8, None) == ARG
    assert L.agcn_ln_fwd(p, None, p, p, 1e-5, p, p, p, 0, 8, None) == ARG
    assert L.agcn_ln_fwd(p, None, p, p, -1.0, p, p, p, 4, 8, None) == ARG
    assert L.agcn_ln_fwd(p, None, p, p, 1e-5, p, p, p, 4, 2049, None) == UNS
    assert L.agcn_ln_bwd(p, p, None, p, p, p, p, p, None, p, 1 << 20, 4, 8, None) == ARG
    assert L.agcn_ln_bwd(p, p, None, p, p, p, p, p, p, p, 1 << 20, 4, 2049, None) == UNS
    assert L.agcn_ln_bwd(p, p, None, p, p, p, p, p, p, p, 4 * 2 * 8 * 4 - 1, 4, 8, None) == WS


def test_encoder_plan_checker(tmp_path):
    cxx = next((c for c in (os.environ.get('CXX'), 'c++', 'g++', 'clang++') if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip('no host C++ compiler')
    exe = str(tmp_path / 'encoder_plan_check')
    r = subprocess.run([cxx, '-std=c++17', '-Wall', '-Werror', '-O1', '-I', os.path.join(ROOT, '2s-agcn_amd', 'csrc'),
                        os.path.join(ROOT, 'tests', 'encoder_plan_check.cpp'), '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-4000:]
    assert ' cases, 0 failures' in r.stdout and int(r.stdout.split(' cases')[0].split()[-1]) > 400000


def test_tensor_code_forms_agree_with_torch():
    """ops.mha_ref / add_ln_ref / tokens_ref (the AGCN_ENCODER_HIP=0 path and the GPU tests' fp64 comparison) against
    torch's own MultiheadAttention, LayerNorm and the reference's permute, on the CPU."""
    import agcn_amd  # noqa: F401
    from agcn_amd import ops
    g = torch.Generator().manual_seed(3)
    N, L, H, dh = 2, 7, 2, 5
    D = H * dh
    mha = torch.nn.MultiheadAttention(D, H, batch_first=True).double()
    mha.requires_grad_(False)
    x = torch.randn(N, L, D, generator=g, dtype=torch.float64)
    qkv = torch.nn.functional.linear(x, mha.in_proj_weight, mha.in_proj_bias)
    for causal in (0, 1, 2):
        i = torch.arange(L)
        mask = None if causal == 0 else ((i[None] > i[:, None]) if causal == 1 else (i[None] < i[:, None]))
        want, wavg = mha(x, x, x, attn_mask=mask)
        ctx, avg = ops.mha_ref(qkv, H, None, causal, need_avg=True)
        got = torch.nn.functional.linear(ctx, mha.out_proj.weight, mha.out_proj.bias)
        assert float((got - want).abs().max()) < 1e-12 and float((avg - wavg).abs().max()) < 1e-12
    null = torch.zeros(N, L, dtype=torch.uint8)
    null[:, 1:] = 1
    ctx, avg = ops.mha_ref(qkv, H, null, 0, need_avg=True)
    assert float(avg[:, 1:, 1:].abs().max()) == 0.0 and float((avg[:, 1:, 0] - 1).abs().max()) < 1e-12
    null[:, 0] = 1                                       # fully masked rows: zeros, not NaN
    ctx, avg = ops.mha_ref(qkv, H, null, 0, need_avg=True)
    assert float(ctx.abs().max()) == 0.0 and float(avg.abs().max()) == 0.0
    a, b = torch.randn(3, 4, 6, generator=g), torch.randn(3, 4, 6, generator=g)
    ln = torch.nn.LayerNorm(6)
    assert torch.equal(ops.add_ln_ref(a, b, ln.weight, ln.bias, ln.eps), ln(a + b))
    xx = torch.randn(2 * 2, 3, 4, 5, generator=g)
    cls, pe = torch.randn(1, 1, 15, generator=g), torch.randn(1, 20, 15, generator=g)
    want = xx.view(2, 2, 3, 4, 5).permute(0, 1, 3, 4, 2).contiguous().view(2, 8, 15)
    want = torch.cat((cls.repeat(2, 1, 1), want), 1) + pe[:, :9]
    assert torch.equal(ops.tokens_ref(xx, cls, pe, 2), want)
