"""CPU checks of SGN v15 (2s-agcn_amd/model/sgn_v15.py, csrc/sgn_v15_plan.h): the class against the reference-generated
fixtures (tests/golden/make_golden_sgn_v15.py), the fold and the layout of the weight images through
``ops.sgn15_forward_ref``, the plan header with the host compiler, the entries' argument checks and the yaml / processor
surface.  Bound: 1e-4 relative to max(1, max|reference tensor|) per tensor."""
import ctypes
import math
import os
import shutil
import subprocess
import types

import numpy as np
import pytest
import torch

from tests import sgn_v15_util as vu

ROOT = vu.ROOT
_MODELS = {}


def _model(case):
    if case not in _MODELS:
        import agcn_amd  # noqa: F401
        from agcn_amd.model.sgn_v15 import SGN
        c = vu.load_case(case)
        m = SGN(**c['meta']['model_args'])
        m.load_state_dict(vu.torch_state(c['state']))
        with torch.no_grad():
            out = m.eval()._forward_tensor(torch.from_numpy(c['x']))
        _MODELS[case] = (c, m, out)
    return _MODELS[case]


def _err(got, ref):
    ref = np.asarray(ref.detach().numpy() if torch.is_tensor(ref) else ref, dtype=np.float64)
    got = np.asarray(got.detach().numpy() if torch.is_tensor(got) else got, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.abs(got - ref).max() / max(1.0, float(np.abs(ref).max())))


def _images(m):
    frames, clip = m._folded()
    return torch.cat([t.reshape(-1) for t in frames]), torch.cat([t.reshape(-1) for t in clip])


@pytest.mark.parametrize('case', list(vu.CASES))
def test_state_dict_is_the_references(case):
    c, m, _ = _model(case)
    sd = m.state_dict()
    assert list(sd.keys()) == c['keys']
    assert {k: tuple(v.shape) for k, v in sd.items()} == c['shapes']
    assert 'semantic_embedding.spa_onehot.onehot' in sd and 'semantic_embedding.tem_onehot.onehot' in sd
    assert 'feature_extractor.pos_embed.cnn1.block.conv.conv.weight' in sd and 'fc.weight' in sd
    for b in ('spatial', 'temporal'):
        p = f'{b}_mha.transformer.layers.l1.'
        assert {p + 'attn.norm.fn.running_mean', p + 'attn.fn.to_q.weight', p + 'attn.fn.to_out.linear.bias',
                p + 'ffn.norm.fn.weight', p + 'ffn.fn.net.linear1.weight', p + 'ffn.fn.residual.weight'} <= set(sd)
    assert 'fused_attention' not in sd and m.fused_attention is False and m.seg == m.num_segment
    # the recipe reproduces the stored checksums (load_case asserts it) and leaves the class's own one-hot buffers
    fresh = type(m)(**c['meta']['model_args']).state_dict()
    for k in sd:
        if k.endswith('onehot'):
            assert np.array_equal(c['state'][k], fresh[k].numpy()), k
    assert len(c['meta']['qk_scale']) == 2 and all(0.2 <= v <= 0.8 for v in c['meta']['rowmax'].values())


@pytest.mark.parametrize('case', list(vu.CASES))
def test_composition_matches_reference(case):
    c, m, (logits, aux, feat) = _model(case)
    N, V, seg = c['x'].shape[0], m.num_point, m.num_segment
    assert set(aux) == {'tem_emb', 'spa_emb', 'spatial_attn_list', 'temporal_attn_list', 'spatial_featuremap',
                        'temporal_featuremap'}
    assert tuple(aux['spatial_featuremap'].shape) == (N, 256, V, seg) and tuple(aux['temporal_featuremap'].shape) == (N, 512, 1, seg)
    assert tuple(aux['spa_emb'].shape) == (N, 64, V, seg) and tuple(aux['tem_emb'].shape) == (N, 256, V, seg)
    errs = dict(logits=_err(logits, c['logits']), feat=_err(feat[:, :, 0], c['feat']),
                spatial_attn=_err(aux['spatial_attn_list'][0], c['spatial_attn']),
                temporal_attn=_err(aux['temporal_attn_list'][0], c['temporal_attn']),
                spa_emb=_err(aux['spa_emb'][0, :, :, 0], c['spa_emb']), tem_emb=_err(aux['tem_emb'][0, :, 0, :], c['tem_emb']),
                pooled=_err(aux['temporal_featuremap'].amax((2, 3)), c['pooled']))
    print(f'{case}: composition vs reference: ' + ', '.join(f'{k} {v:.2e}' for k, v in errs.items()))
    assert all(v < 1e-4 for v in errs.values()), errs


@pytest.mark.parametrize('case', list(vu.CASES))
def test_images_match_the_size_queries_and_the_composition(case):
    from agcn_amd import lib, ops
    c, m, (logits, aux, feat) = _model(case)
    V, seg, (sp, tp) = m.num_point, m.num_segment, m._geometry()
    assert m._structure_fused()
    with torch.no_grad():
        wf, wc = _images(m)
    L = lib.load()
    assert wf.numel() == L.agcn_sgn15_frames_weights(V, *sp) and wc.numel() == L.agcn_sgn15_clip_weights(seg, 60, *tp)
    assert ops.sgn15_weights_floats(V, seg, 60, sp, tp) == (wf.numel(), wc.numel())
    for secs, img in zip(ops.sgn15_image_sections(V, seg, 60, sp, tp), (wf, wc)):
        end = 0
        for name, off, shape in secs:                 # the sections tile the image without gaps
            assert off == end, name
            end = off + math.prod(shape)
        assert end == img.numel()
    with torch.no_grad():
        rl, rfeat, rsa, rta = ops.sgn15_forward_ref(torch.from_numpy(c['x']), wf, wc, V, seg, 60, sp, tp)
        tem = wc[:seg * 256].view(seg, 256)
    errs = dict(logits=_err(rl, logits), feat=_err(rfeat + tem, feat[:, :, 0]), spatial_attn=_err(rsa, aux['spatial_attn_list'][0]),
                temporal_attn=_err(rta, aux['temporal_attn_list'][0]))
    print(f'{case}: forward_ref on the images vs composition: ' + ', '.join(f'{k} {v:.2e}' for k, v in errs.items()))
    assert all(v < 1e-4 for v in errs.values()), errs
    assert float((rfeat + tem < 0).float().mean()) >= 0.1     # a maximum with a ReLU's neutral element would fail here


def test_stale_cache_is_rebuilt():
    import agcn_amd  # noqa: F401
    from agcn_amd.model.sgn_v15 import SGN
    m = SGN(**vu.case_args('j3_seg2')).eval()
    with torch.no_grad():
        wf, wc, spa, tem = m._images()
        assert m._images()[0] is wf                   # cached
        assert spa.data_ptr() != tem.data_ptr() and tuple(spa.shape) == (3, 64) and tuple(tem.shape) == (2, 256)
        m.fc.bias.add_(1.0)                           # a parameter, in place
        wf2, wc2, _, _ = m._images()
        assert wf2 is not wf and torch.equal(wc2[-60:], wc[-60:] + 1.0) and torch.equal(wf2, wf)
        m.spatial_mha.transformer.layers['l1']['attn'].norm.fn.running_mean.add_(0.5)     # a running statistic
        wf3 = m._images()[0]
        assert wf3 is not wf2 and not torch.equal(wf3, wf2)


def test_plan_checker(tmp_path):
    cxx = next((c for c in (os.environ.get('CXX'), 'c++', 'g++', 'clang++') if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip('no host C++ compiler')
    exe = str(tmp_path / 'sgn_v15_plan_check')
    r = subprocess.run([cxx, '-std=c++17', '-Wall', '-Werror', '-O1', '-I', os.path.join(ROOT, '2s-agcn_amd', 'csrc'),
                        os.path.join(ROOT, 'tests', 'sgn_v15_plan_check.cpp'), '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-4000:]
    assert ' cases, 0 failures' in r.stdout and int(r.stdout.split(' cases')[0].split()[-1]) > 50000


def test_argument_errors_are_reported_not_thrown():
    import agcn_amd  # noqa: F401
    from agcn_amd import lib
    L = lib.load()
    p = ctypes.c_void_p(4096)          # never dereferenced: the checks come before any HIP call
    ARG = lib.ERR_ARG
    sp, tp = (8, 16, 128), (8, 32, 256)
    nf, nc = L.agcn_sgn15_frames_weights(15, *sp), L.agcn_sgn15_clip_weights(20, 60, *tp)
    base = 12 * 15 + 2 * (192 + 64 + 4096 + 64) + 64 * 15
    assert nf == base + 128 * 384 + 384 + 128 * 128 + 128 + 128 * 128 + 128 + 256 * 256 + 256
    assert nc == 20 * 256 + 256 * 768 + 768 + 256 * 256 + 256 + 256 * 256 + 256 + 512 * 512 + 512 + 512 * 60 + 60
    # size queries return 0 outside the domain
    assert L.agcn_sgn15_frames_weights(1, *sp) == 0 and L.agcn_sgn15_frames_weights(33, *sp) == 0
    assert L.agcn_sgn15_frames_weights(15, 16, 8, 128) == 0 and L.agcn_sgn15_frames_weights(15, 9, 128, 128) == 0     # d_head 8, inner 1152
    assert L.agcn_sgn15_frames_weights(15, 8, 16, 1152) == 0 and L.agcn_sgn15_frames_weights(15, 8, 16, 64) == 0
    assert L.agcn_sgn15_frames_weights(15, 8, 48, 128) == 0                     # 8 x 48 = 384: heads straddle a 128-column group
    assert L.agcn_sgn15_clip_weights(33, 60, *tp) == 0 and L.agcn_sgn15_clip_weights(0, 60, *tp) == 0
    assert L.agcn_sgn15_clip_weights(20, 60, 16, 8, 128) == 0 and L.agcn_sgn15_clip_weights(20, 60, 9, 128, 128) == 0
    # entries
    assert L.agcn_sgn15_frames(None, p, nf, p, p, 1, 20, 15, *sp, None) == ARG
    assert L.agcn_sgn15_frames(p, None, nf, p, p, 1, 20, 15, *sp, None) == ARG
    assert L.agcn_sgn15_frames(p, p, nf, None, p, 1, 20, 15, *sp, None) == ARG
    assert L.agcn_sgn15_frames(p, p, nf, p, None, 1, 20, 1, *sp, None) == ARG            # V = 1
    assert L.agcn_sgn15_frames(p, p, nf, p, None, 1, 20, 33, *sp, None) == ARG           # V = 33
    assert L.agcn_sgn15_frames(p, p, nf, p, None, 1, 20, 15, 16, 8, 128, None) == ARG    # d_head = 8
    assert L.agcn_sgn15_frames(p, p, nf, p, None, 1, 20, 15, 9, 128, 128, None) == ARG   # inner = 1152
    assert L.agcn_sgn15_frames(p, p, nf - 1, p, None, 1, 20, 15, *sp, None) == ARG       # not the image of this geometry
    assert L.agcn_sgn15_frames(p, p, nf, p, None, 0, 20, 15, *sp, None) == ARG
    assert L.agcn_sgn15_clip(None, p, nc, p, p, 1, 20, 60, *tp, None) == ARG
    assert L.agcn_sgn15_clip(p, None, nc, p, p, 1, 20, 60, *tp, None) == ARG
    assert L.agcn_sgn15_clip(p, p, nc, None, p, 1, 20, 60, *tp, None) == ARG
    assert L.agcn_sgn15_clip(p, p, nc, p, None, 1, 33, 60, *tp, None) == ARG             # seg = 33
    assert L.agcn_sgn15_clip(p, p, nc, p, None, 1, 20, 60, 16, 8, 128, None) == ARG
    assert L.agcn_sgn15_clip(p, p, nc, p, None, 1, 20, 60, 9, 128, 128, None) == ARG
    assert L.agcn_sgn15_clip(p, p, nc + 1, p, None, 1, 20, 60, *tp, None) == ARG


def _args(**over):
    kw = vu.case_args('j3_seg2')
    for k, v in over.items():
        if k in ('spatial', 'temporal'):
            kw[k + '_mha_kwargs'] = dict(kw[k + '_mha_kwargs'], **v)
        else:
            kw[k] = v
    return kw


@pytest.mark.parametrize('over, names', [
    (dict(input_position=2), 'input_position'), (dict(input_velocity=11), 'input_velocity'),
    (dict(semantic_joint=3), 'semantic_joint'), (dict(semantic_frame=101), 'semantic_frame'),
    (dict(semantic_class=1), 'semantic_class'), (dict(norm_type='ln'), 'norm_type'), (dict(act_type='gelu'), 'act_type'),
    (dict(spatial=dict(post_norm=True)), 'post_norm'), (dict(temporal=dict(norm='ln')), 'norm'),
    (dict(spatial=dict(activation='gelu')), 'activation'),
])
def test_unsupported_arguments_are_named(over, names):
    import agcn_amd  # noqa: F401
    from agcn_amd.model.sgn_v15 import SGN
    with pytest.raises(NotImplementedError, match=names):
        SGN(**_args(**over))


def test_encoder_layer_branch_is_refused():
    import agcn_amd  # noqa: F401
    from agcn_amd.model.sgn_v15 import SGN
    kw = _args()
    kw['temporal_mha_kwargs'] = {k: v for k, v in kw['temporal_mha_kwargs'].items() if k != 'norm'}
    with pytest.raises(NotImplementedError, match='TransformerEncoderLayer'):
        SGN(**kw)


@pytest.mark.parametrize('over', [
    dict(input_emb_fusion=0, spatial=dict(d_model=[256])), dict(temporal=dict(global_norm=True)),
    dict(spatial=dict(num_layers=2, d_model=[128, 256], nhead=[2, 2], d_head=[64, 64], dim_feedforward=[128, 128],
                      dim_feedforward_output=[256, 256])),
    dict(num_segment=40), dict(semantic_joint_fusion=1, spatial=dict(d_model=[64])), dict(input_velocity=0),
    dict(spatial_maxpool=0, temporal=dict(d_model=[3 * 256], dim_feedforward_output=[3 * 512])), dict(temporal_maxpool=0),
    dict(semantic_frame=0), dict(c_multiplier=[0.5, 0.5, 0.5, 0.5], spatial=dict(d_model=[64], dim_feedforward_output=[128]),
                                 temporal=dict(d_model=[128], dim_feedforward_output=[256])),
])
def test_supported_configurations_outside_the_fused_domain_run_on_the_composition(over):
    import agcn_amd  # noqa: F401
    from agcn_amd import ops
    from agcn_amd.model.sgn_v15 import SGN
    kw = _args(**over)
    m = SGN(**kw)
    seg, V = kw['num_segment'], kw['num_point']
    x = torch.from_numpy(np.random.default_rng(1).standard_normal((2, seg, 3 * V)).astype(np.float32))
    assert not m._structure_fused() or seg > 32
    before = ops.SGN_STATS['forward_tensor']
    m.eval()
    with torch.no_grad():
        logits, aux = m(x)
    assert ops.SGN_STATS['forward_tensor'] == before + 1
    assert tuple(logits.shape) == (2, 60) and bool(torch.isfinite(logits).all())
    assert len(aux['spatial_attn_list']) == kw['spatial_mha_kwargs']['num_layers']
    m.train()                                          # a complete nn.Module: autograd reaches every parameter
    logits, _ = m(x)
    logits.square().mean().backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m.parameters())


def test_input_gradient_on_the_cpu():
    c, m, (logits, _, _) = _model('j3_seg2')
    x = torch.from_numpy(c['x'])
    cot = torch.from_numpy(np.random.default_rng(2).standard_normal(logits.shape).astype(np.float32))
    lg, aux, dx = m.input_gradient(x, cot)
    eps, d = 1e-5, torch.from_numpy(np.random.default_rng(3).standard_normal(c['x'].shape).astype(np.float32))
    with torch.no_grad():
        fd = float((((m.double().forward_tensor(x.double() + eps * d.double())[0]
                      - m.forward_tensor(x.double() - eps * d.double())[0]) * cot.double()).sum()) / (2 * eps))
    m.float()
    assert torch.equal(lg, logits) and not dx.requires_grad and aux['spatial_attn_list'][0].requires_grad is False
    assert abs(float((dx * d).sum()) - fd) <= 1e-3 * max(1.0, abs(fd))
    with pytest.raises(ValueError):
        m.train().input_gradient(x, cot)
    m.eval()


def test_processor_accepts_both_sgn_classes_and_no_other(tmp_path):
    """The check in front of SGNProcessor's construction, without a GPU: the constructor is run up to the model check."""
    import agcn_amd  # noqa: F401
    from agcn_amd import sgn_processor as sp

    class Probe(sp.SGNProcessor):
        def load_model(self):
            raise StopIteration                       # past the model check

    def arg(model):
        return types.SimpleNamespace(model=model, device=[0], seed=1, work_dir=str(tmp_path), world_size=1)

    real = torch.cuda.set_device
    torch.cuda.set_device = lambda d: None
    try:
        for ok in ('model.sgn.SGN', 'model.sgn_v15.SGN'):
            with pytest.raises(StopIteration):
                Probe(arg(ok))
        for bad in ('model.agcn.Model', 'model.aagcn.Model'):
            with pytest.raises(ValueError, match='model.sgn_v15.SGN'):
                Probe(arg(bad))
    finally:
        torch.cuda.set_device = real


@pytest.mark.parametrize('name', ['train_sgn_v15.yaml', 'test_sgn_v15.yaml'])
def test_yamls_parse_and_construct(name):
    import yaml
    import agcn_amd  # noqa: F401
    from agcn_amd.processor import import_class, load_args
    path = os.path.join(ROOT, 'config', 'nturgbd-cross-view', name)
    with open(path) as f:
        cfg = yaml.safe_load(f)
    arg = load_args(['--config', path])
    assert arg.model == cfg['model'] == 'model.sgn_v15.SGN' and arg.use_sgn_dataloader
    m = import_class(arg.model)(**arg.model_args)
    assert m._structure_fused() and m._geometry() == ((1, 512, 512), (1, 1024, 1024)) and m.seg == 20
    assert m.num_point == 25 and m.num_class == 60
