"""GPU checks of the fused SGN v15 inference path (csrc/sgn_v15.hip) against the reference-generated fixtures
(tests/golden/make_golden_sgn_v15.py): logits, feat and both attention maps in every case, independence of the batch,
the routes that must take the composition, the input gradient, the online recogniser and one SGNProcessor run.

Bound: the project's fp32 rule, 1e-4 relative to max(1, max|reference tensor|) per tensor.  Every test prints the
measured worst error per tensor before it asserts."""
import os

import numpy as np
import pytest
import torch

from tests import sgn_v15_util as vu

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
V15_AXES = dict(zaxis=(8, 1), xaxis=(2, 5))
_MODELS = {}


def _model(case):
    """The case's fixture and its model on the GPU in eval mode (built once, never modified by a test)."""
    if case not in _MODELS:
        import agcn_amd  # noqa: F401
        from agcn_amd.model.sgn_v15 import SGN
        c = vu.load_case(case)
        m = SGN(**c['meta']['model_args'])
        m.load_state_dict(vu.torch_state(c['state']))
        _MODELS[case] = (c, m.to(DEV).eval())
    return _MODELS[case]


def _err(got, ref):
    ref = np.asarray(ref.detach().cpu().numpy() if torch.is_tensor(ref) else ref, dtype=np.float64)
    got = np.asarray(got.detach().cpu().numpy() if torch.is_tensor(got) else got, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.abs(got - ref).max() / max(1.0, float(np.abs(ref).max())))


def _tensor_count():
    from agcn_amd import ops
    return ops.SGN_STATS['forward_tensor']


def _fused(m, x, attention):
    from agcn_amd import ops
    before, launches = _tensor_count(), dict(ops.SGN15_STATS)
    m.fused_attention = attention
    try:
        with torch.no_grad():
            out = m(x)
    finally:
        m.fused_attention = False
    assert _tensor_count() == before, 'the fused call ran the composition'
    assert ops.SGN15_STATS == dict(frames_hip=launches['frames_hip'] + 1, clip_hip=launches['clip_hip'] + 1)
    return out


@pytest.mark.parametrize('case', list(vu.CASES))
def test_fused_eval_matches_reference(case):
    from agcn_amd import ops
    c, m = _model(case)
    x = torch.from_numpy(c['x']).to(DEV)
    logits, aux = _fused(m, x, True)
    N, seg, V = x.shape[0], m.num_segment, m.num_point
    assert set(aux) == {'tem_emb', 'spa_emb', 'spatial_attn_list', 'temporal_attn_list'}
    assert tuple(aux['spa_emb'].shape) == (N, 64, V, seg) and tuple(aux['tem_emb'].shape) == (N, 256, V, seg)
    wf, wc, _, tem = m._images()
    sp, _ = m._geometry()
    feat, _ = ops.sgn15_frames(x, wf, V, *sp)
    errs = dict(logits=_err(logits, c['logits']), feat=_err(feat + tem, c['feat']),
                spatial_attn=_err(aux['spatial_attn_list'][0], c['spatial_attn']),
                temporal_attn=_err(aux['temporal_attn_list'][0], c['temporal_attn']),
                spa_emb=_err(aux['spa_emb'][0, :, :, 0], c['spa_emb']), tem_emb=_err(aux['tem_emb'][0, :, 0, :], c['tem_emb']))
    print(f'{case}: fused vs reference, relative to max(1, max|ref|): ' + ', '.join(f'{k} {v:.2e}' for k, v in errs.items()))
    assert float((c['feat'] < 0).mean()) >= 0.1 and float((c['pooled'] < 0).mean()) >= 0.1     # a ReLU-neutral maximum fails
    assert all(v < 1e-4 for v in errs.values()), errs


@pytest.mark.parametrize('case', ['j3_seg2', 'j15_deployed', 'j25_yaml', 'j9_seg7_h2x256', 'j16_seg17_h16x16'])
def test_attention_flag_and_batch_do_not_change_the_bits(case):
    c, m = _model(case)
    x = torch.from_numpy(c['x']).to(DEV)
    on, aux_on = _fused(m, x, True)
    off, aux_off = _fused(m, x, False)
    assert aux_off['spatial_attn_list'] is None and aux_off['temporal_attn_list'] is None
    assert torch.equal(on, off)
    for n in range(x.shape[0]):
        alone, aux = _fused(m, x[n:n + 1].contiguous(), True)
        assert torch.equal(alone[0], on[n]), f'clip {n} alone differs from the batch'
        assert torch.equal(aux['temporal_attn_list'][0][0], aux_on['temporal_attn_list'][0][n])


@pytest.mark.parametrize('case', ['j32_seg32', 'j7_seg12_nobias'])
def test_fused_matches_composition(case):
    c, m = _model(case)
    rng = np.random.default_rng(5)
    x = torch.from_numpy(np.concatenate([c['x'], c['x'][::-1] + 0.05 * rng.standard_normal(c['x'].shape).astype(np.float32)])
                         [:3].copy()).to(DEV)
    logits, aux = _fused(m, x, True)
    with torch.no_grad():
        ref_l, ref = m.forward_tensor(x)
    errs = dict(logits=_err(logits, ref_l), spatial_attn=_err(aux['spatial_attn_list'][0], ref['spatial_attn_list'][0]),
                temporal_attn=_err(aux['temporal_attn_list'][0], ref['temporal_attn_list'][0]))
    print(f'{case}: fused vs composition on the GPU: ' + ', '.join(f'{k} {v:.2e}' for k, v in errs.items()))
    assert all(v < 1e-4 for v in errs.values()), errs


def test_routes_that_take_the_composition():
    c, m = _model('j3_seg2')
    _MODELS.pop('j3_seg2')                                       # this test modifies the model
    x = torch.from_numpy(c['x']).to(DEV)
    fused, _ = _fused(m, x, False)

    def tensor_route(fn):
        before = _tensor_count()
        out = fn()
        assert _tensor_count() == before + 1
        return out

    with torch.no_grad():
        wide = torch.zeros(x.shape[0], x.shape[1], 2 * x.shape[2], device=DEV)
        wide[:, :, ::2] = x
        nc, aux = tensor_route(lambda: m(wide[:, :, ::2]))
        assert set(aux) >= {'spatial_featuremap', 'temporal_featuremap'} and _err(nc, fused) < 1e-4
        d, _ = tensor_route(lambda: m.double()(x.double()))
        m.float()
        assert d.dtype == torch.float64 and _err(d, fused) < 1e-4
    g, _ = tensor_route(lambda: m(x))                            # grad mode
    assert g.requires_grad and _err(g, fused) < 1e-4
    m.train()
    try:
        with torch.no_grad():
            tensor_route(lambda: m(x))
    finally:
        m.eval()
    # the running statistics moved in train(): the cached images are stale and must be rebuilt
    after, _ = _fused(m, x, False)
    with torch.no_grad():
        ref, _ = m.forward_tensor(x)
    assert _err(after, ref) < 1e-4 and not torch.equal(after, fused)


def test_a_large_batch_is_fused_and_a_larger_one_is_chunked():
    """20000 clips of 2 frames: 40000 workgroups in the frames launch, more clips than an evaluation batch
    (test_batch_size 512 x multi_test 5 = 2560) or a recording (2000 windows) has.  Then the chunk walk above
    ops.SGN15_MAX_CLIPS, forced with a small limit: the same bits."""
    from agcn_amd import ops
    c, m = _model('j3_seg2')
    rng = np.random.default_rng(9)
    N = 20000
    x = torch.from_numpy(np.tile(c['x'], (N // c['x'].shape[0], 1, 1))
                         + 0.05 * rng.standard_normal((N, 2, 9)).astype(np.float32)).to(DEV)
    x[:5] = torch.from_numpy(c['x']).to(DEV)
    big, aux = _fused(m, x, True)
    small, _ = _fused(m, x[:5].contiguous(), False)
    assert tuple(big.shape) == (N, 60) and torch.equal(big[:5], small)
    assert tuple(aux['spatial_attn_list'][0].shape) == (2 * N, 2, 3, 3) and tuple(aux['temporal_attn_list'][0].shape) == (N, 4, 2, 2)
    with torch.no_grad():
        ref, raux = m.forward_tensor(x[-64:])
    e = dict(logits=_err(big[-64:], ref), spatial_attn=_err(aux['spatial_attn_list'][0][-128:], raux['spatial_attn_list'][0]),
             temporal_attn=_err(aux['temporal_attn_list'][0][-64:], raux['temporal_attn_list'][0]))
    print('the last 64 of 20000 clips, fused vs composition: ' + ', '.join(f'{k} {v:.2e}' for k, v in e.items()))
    assert all(v < 1e-4 for v in e.values()), e
    limit, launches = ops.SGN15_MAX_CLIPS, dict(ops.SGN15_STATS)
    ops.SGN15_MAX_CLIPS = 7
    try:
        m.fused_attention = True
        with torch.no_grad():
            chunked, caux = m(x[:20])
    finally:
        ops.SGN15_MAX_CLIPS, m.fused_attention = limit, False
    assert ops.SGN15_STATS == dict(frames_hip=launches['frames_hip'] + 3, clip_hip=launches['clip_hip'] + 3)
    assert torch.equal(chunked, big[:20]) and torch.equal(caux['spatial_attn_list'][0], aux['spatial_attn_list'][0][:40])
    assert torch.equal(caux['temporal_attn_list'][0], aux['temporal_attn_list'][0][:20])


@pytest.mark.parametrize('over', [dict(num_segment=40), dict(temporal=(8, 48, 128)), dict(temporal=(4, 48, 128))])
def test_sizes_outside_the_kernels_domain_take_the_composition_silently(over):
    """seg > 32 (more than one 32-row tile), a head width that straddles a 128-column group (8 x 48 = 384, a multiple of
    128) and an inner width that is no multiple of 128 (4 x 48)."""
    import agcn_amd  # noqa: F401
    from agcn_amd.model.sgn_v15 import SGN
    seg = over.get('num_segment', 12)
    m = SGN(**vu.model_args(7, seg, 1, (8, 16, 128), over.get('temporal', (8, 32, 256)))).to(DEV).eval()
    x = torch.randn(2, seg, 21, device=DEV)
    before = _tensor_count()
    with torch.no_grad():
        logits, aux = m(x)
    assert _tensor_count() == before + 1 and 'temporal_featuremap' in aux and bool(torch.isfinite(logits).all())


def test_input_gradient_matches_autograd():
    c, m = _model('j7_seg12_nobias')
    x = torch.from_numpy(c['x']).to(DEV)
    cot = torch.from_numpy(np.random.default_rng(3).standard_normal((x.shape[0], 60)).astype(np.float32)).to(DEV)
    logits, aux, dx = m.input_gradient(x, cot)
    xg = x.clone().requires_grad_(True)
    ref_l, _ = m.forward_tensor(xg)
    ref_dx, = torch.autograd.grad((ref_l * cot).sum(), xg)
    assert not logits.requires_grad and dx.shape == x.shape and bool(torch.isfinite(dx).all())
    e = _err(dx, ref_dx)
    print(f'input_gradient vs autograd of the composition: {e:.2e}')
    assert e < 1e-4 and float(dx.abs().max()) > 0


def test_online_recogniser_reproduces_the_reference():
    from agcn_amd.online import ActionRecognition
    c = vu.load_online()
    frames = vu._npz('sgn_online_v15.npz')['frames']
    meta = c['meta']
    ar = ActionRecognition(model='model.sgn_v15.SGN', model_args=meta['model_args'], max_frame=meta['window'],
                           max_num_skeleton=meta['max_person'], max_num_skeleton_true=meta['select'], num_joint=15,
                           device=DEV, sgn_preprocess=True, multi_test=meta['multi_test'], **V15_AXES)
    ar.model.load_state_dict(vu.torch_state(c['state']))
    assert ar.seg == 20 and not ar.model.training
    record = [int(i) for i in c['record']]
    for i, f in enumerate(frames):
        ar.append_data(f)
        if i not in record:
            continue
        k = record.index(i)
        before = _tensor_count()
        scores, label = ar.predict(draws=c['draws'][k])
        assert _tensor_count() == before, 'the recogniser ran the composition'
        e, e_s = _err(ar.logits[0], c['logits'][k]), _err(np.asarray(scores), c['scores'][k])
        print(f'online append {i}: mean logits vs reference {e:.2e}, scores {e_s:.2e}, label {label}')
        assert e < 1e-4 and e_s < 1e-4 and label == int(c['labels'][k])
    sal, classes = ar.explain()
    assert sal.shape == (1, meta['window'], 2, 15) and np.isfinite(sal).all() and sal.max() > 0
    assert int(classes[0]) == int(c['labels'][-1])


def test_processor_trains_and_scores_from_the_yaml(tmp_path):
    """The new train yaml shrunk to the synthetic feeder: batch 4, two epochs of two batches on the composition, a
    checkpoint, then the scores through the fused forward."""
    from agcn_amd import ops
    from agcn_amd.processor import load_args
    from agcn_amd.sgn_processor import SGNProcessor
    cfg = os.path.join(vu.ROOT, 'config', 'nturgbd-cross-view', 'train_sgn_v15.yaml')
    arg = load_args(['--config', cfg, '--work-dir', str(tmp_path), '--batch-size', '4', '--test-batch-size', '4',
                     '--num-epoch', '2', '--log-interval', '1', '--print-log', 'False', '--save-score', 'True'])
    assert arg.model == 'model.sgn_v15.SGN' and arg.use_sgn_dataloader and arg.optimizer == 'Adam'
    arg.train_feeder_args = dict(num_samples=8, num_point=25, window_size=32)
    arg.test_feeder_args = dict(num_samples=6, num_point=25, window_size=32, seed=1)
    arg.train_dataloader_args = dict(dataset='NTU60-CV', seg=20, multi_test=1, aug=1)
    arg.test_dataloader_args = dict(dataset='NTU60-CV', seg=20, multi_test=3)
    p = SGNProcessor(arg)
    init = {k: v.detach().clone() for k, v in p.model.named_parameters()}
    tensor = _tensor_count()
    p.start()
    assert os.listdir(tmp_path / 'weight') == ['SGN-2-4.pt'] and p.global_step == 4
    assert _tensor_count() >= tensor + 4, 'training runs on the composition'
    moved = sum(int(not torch.equal(v, init[k])) for k, v in p.model.named_parameters())
    assert moved > len(init) // 2 and all(bool(torch.isfinite(v).all()) for v in p.model.parameters())
    score = p.last_score
    assert score.shape == (6, 60) and np.isfinite(score).all()
    before, launches = _tensor_count(), dict(ops.SGN15_STATS)
    loss, acc = p.eval(1)
    assert _tensor_count() == before and ops.SGN15_STATS['clip_hip'] == launches['clip_hip'] + 2
    assert np.isfinite(loss) and np.array_equal(p.last_score, score)
