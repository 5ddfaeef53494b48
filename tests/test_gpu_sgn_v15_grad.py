"""GPU checks of the SGN v15 input gradient (csrc/sgn_v15_bwd.hip).

a. The two kernels, each ALONE, over the table of tests/sgn_v15_grad_util.py against fp64 autograd through the tensor
   reference on seeded weight images: ``ops.sgn15_clip_bwd`` on the reference's feat rounded to fp32 and a seeded
   d logits, ``ops.sgn15_frames_bwd`` on x and a seeded d feat.
b. The whole model against the reference class's gradient (tests/golden/sgn15_evalgrad.npz).
c. ``explain()`` of an online v15 recogniser.

Bound: the project's fp32 rule per tensor, 1e-4 relative to max(1, max|reference tensor|); every comparison prints its
ratio, a multiple of that bound, before it asserts.  What makes these inputs able to show an error, and keeps them away
from the switches of every ReLU and maximum, is asserted in tests/test_sgn_v15_grad_cpu.py."""
import copy

import numpy as np
import pytest
import torch

from tests import sgn_v15_domain_util as du
from tests import sgn_v15_grad_util as gu
from tests import sgn_v15_util as vu

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
CASE_IDS = list(range(len(gu.CASES)))


def _clip_args(d, n=slice(None)):
    return d['feat32'][n].contiguous().to(DEV), d['wc'].to(DEV), d['dlogits'][n].contiguous().to(DEV)


def _frames_args(d, n=slice(None)):
    return d['x'][n].contiguous().to(DEV), d['wf'].to(DEV), d['dfeat_in'][n].contiguous().to(DEV)


def _transposed(d):
    from agcn_amd import ops
    V, seg, sp, tp, num_class, _ = d['case']
    return ops.sgn15_transpose_images(d['wf'].to(DEV), d['wc'].to(DEV), V, seg, num_class, sp, tp)


@pytest.mark.parametrize('i', CASE_IDS, ids=gu.IDS)
def test_clip_bwd_kernel_alone(i):
    import agcn_amd  # noqa: F401
    from agcn_amd import ops
    V, seg, sp, tp, num_class, N = gu.CASES[i]
    d = gu.load(i)
    feat, wc, dlogits = _clip_args(d)
    _, wc_t = _transposed(d)
    dfeat = ops.sgn15_clip_bwd(feat, wc, wc_t, dlogits, *tp)
    assert tuple(dfeat.shape) == (N, seg, 256) and bool(torch.isfinite(dfeat).all())
    r = du.check(dfeat, d['dfeat64'])
    print(f'case {i} clip_bwd fused vs fp64 autograd, in bounds: dfeat {r:.3e}')
    assert r <= 1.0, r
    assert torch.equal(ops.sgn15_clip_bwd(feat, wc, wc_t, dlogits, *tp), dfeat)            # equal bits on a second call
    if N > 1:                                                                                 # a clip alone
        f1, _, d1 = _clip_args(d, slice(1, 2))
        assert torch.equal(ops.sgn15_clip_bwd(f1, wc, wc_t, d1, *tp)[0], dfeat[1])


@pytest.mark.parametrize('i', CASE_IDS, ids=gu.IDS)
def test_frames_bwd_kernel_alone(i):
    import agcn_amd  # noqa: F401
    from agcn_amd import ops
    V, seg, sp, tp, num_class, N = gu.CASES[i]
    d = gu.load(i)
    x, wf, dfeat = _frames_args(d)
    wf_t, _ = _transposed(d)
    dx = ops.sgn15_frames_bwd(x, wf, wf_t, dfeat, V, *sp)
    assert tuple(dx.shape) == (N, seg, 3 * V) and bool(torch.isfinite(dx).all())
    r = du.check(dx, d['dx64'])
    print(f'case {i} frames_bwd fused vs fp64 autograd, in bounds: dx {r:.3e}')
    assert r <= 1.0, r
    assert torch.equal(ops.sgn15_frames_bwd(x, wf, wf_t, dfeat, V, *sp), dx)               # equal bits on a second call
    if N > 1:                                                                                 # a clip alone
        x1, _, d1 = _frames_args(d, slice(1, 2))
        assert torch.equal(ops.sgn15_frames_bwd(x1, wf, wf_t, d1, V, *sp)[0], dx[1])


def test_bwd_entries_refuse_bad_sizes():
    """AGCN_ERR_ARG for a wrong wt_floats, a workspace size that differs from the query and d_head 48; no launch."""
    import agcn_amd  # noqa: F401
    from agcn_amd import lib, ops
    V, seg, sp, tp, num_class, N = gu.CASES[1]
    d = gu.load(1)
    x, wf, dfeat_in = _frames_args(d)
    feat, wc, dlogits = _clip_args(d)
    wf_t, wc_t = _transposed(d)
    dfeat, dx = torch.empty_like(feat), torch.empty_like(x)
    ws_bytes = lib.load().agcn_sgn15_frames_bwd_workspace(N, seg, V)
    assert ws_bytes == 2 * N * seg * V * 3 * 4
    ws = torch.empty(ws_bytes // 4, device=DEV)

    def clip(wt_floats=wc_t.numel(), geo=tp):
        return lib.status('agcn_sgn15_clip_bwd', feat, wc, wc.numel(), wc_t, wt_floats, dlogits, dfeat, N, seg, num_class, *geo)

    def frames(wt_floats=wf_t.numel(), ws_b=ws_bytes, geo=sp):
        return lib.status('agcn_sgn15_frames_bwd', x, wf, wf.numel(), wf_t, wt_floats, dfeat_in, dx, ws, ws_b, N, seg, V, *geo)

    assert clip() == 0 and frames() == 0
    assert clip(wt_floats=wc_t.numel() - 1) == lib.ERR_ARG and frames(wt_floats=wf_t.numel() + 1) == lib.ERR_ARG
    assert frames(ws_b=ws_bytes - 4) == lib.ERR_ARG and frames(ws_b=ws_bytes + 4) == lib.ERR_ARG
    assert clip(geo=(8, 48, 256)) == lib.ERR_ARG and frames(geo=(8, 48, 128)) == lib.ERR_ARG
    assert lib.load().agcn_sgn15_clip_bwd_weights(seg, num_class, 8, 48, 256) == 0
    assert lib.load().agcn_sgn15_frames_bwd_weights(V, 8, 48, 128) == 0
    assert ops.sgn15_bwd_weights_floats(V, seg, num_class, sp, tp) == (wf_t.numel(), wc_t.numel())
    torch.cuda.synchronize()


# ---- b. the whole model against the reference class's gradient ----
@pytest.mark.parametrize('case', gu.GRAD_CASES)
def test_fused_input_gradient_matches_the_reference(case):
    import agcn_amd  # noqa: F401
    from agcn_amd import ops
    from agcn_amd.model.sgn_v15 import SGN
    c = gu.load_grad_case(case)
    m = SGN(**c['meta']['model_args'])
    m.load_state_dict(vu.torch_state(c['state']))
    m = m.to(DEV).eval()
    x, cot = torch.from_numpy(c['x']).to(DEV), torch.from_numpy(c['cot']).to(DEV)
    m.fused_input_gradient = True
    tensor, fwd, bwd = ops.SGN_STATS['forward_tensor'], dict(ops.SGN15_STATS), dict(ops.SGN15_BWD_STATS)
    logits, aux, dx = m.input_gradient(x, cot)
    assert ops.SGN_STATS['forward_tensor'] == tensor, 'the fused gradient ran the composition'
    assert ops.SGN15_BWD_STATS == dict(clip_bwd=bwd['clip_bwd'] + 1, frames_bwd=bwd['frames_bwd'] + 1)
    assert ops.SGN15_STATS == dict(frames_hip=fwd['frames_hip'] + 1, clip_hip=fwd['clip_hip'] + 1)
    assert dx.shape == x.shape and not dx.requires_grad and not logits.requires_grad
    assert set(aux) == {'tem_emb', 'spa_emb', 'spatial_attn_list', 'temporal_attn_list'}
    # the call came with grad mode on: neither the cached images nor anything returned may carry a graph
    assert torch.is_grad_enabled()
    assert all(not t.requires_grad and t.grad_fn is None for t in m._infer_cache['images'][1:])
    assert all(not t.requires_grad for v in aux.values() if v is not None for t in (v if isinstance(v, list) else [v]))
    m.fused_attention = True
    try:
        _, aux_a, dx_a = m.input_gradient(x, cot)
    finally:
        m.fused_attention = False
    assert torch.equal(dx_a, dx) and all(not t.requires_grad for k in ('spatial_attn_list', 'temporal_attn_list')
                                         for t in aux_a[k])
    with torch.no_grad():
        _, aux_f = m(x)
    assert not aux_f['tem_emb'].requires_grad and not aux_f['spa_emb'].requires_grad
    twin = copy.deepcopy(m)
    assert torch.equal(twin.input_gradient(x, cot)[2], dx)
    r = dict(dx=du.check(dx, c['grad_x64']), logits=du.check(logits, c['logits']))
    print(f'{case} fused input gradient vs the reference in fp64, in bounds: ' + ' '.join(f'{k} {v:.3e}' for k, v in r.items()))
    assert all(v <= 1.0 for v in r.values()), r
    # the same bits in chunks of whole clips
    if x.shape[0] > 1:
        keep, ops.SGN15_MAX_CLIPS = ops.SGN15_MAX_CLIPS, 1
        try:
            l2, _, dx2 = m.input_gradient(x, cot)
        finally:
            ops.SGN15_MAX_CLIPS = keep
        assert torch.equal(dx2, dx) and torch.equal(l2, logits)
    # flag off: the composition, counted, and its result
    m.fused_input_gradient = False
    bwd = dict(ops.SGN15_BWD_STATS)
    l0, _, dx0 = m.input_gradient(x, cot)
    assert ops.SGN_STATS['forward_tensor'] == tensor + 1 and ops.SGN15_BWD_STATS == bwd
    xg = x.clone().requires_grad_(True)
    ref_l, _ = m.forward_tensor(xg)
    ref_dx, = torch.autograd.grad((ref_l * cot).sum(), xg)
    assert torch.equal(dx0, ref_dx) and torch.equal(l0, ref_l.detach())
    r0 = du.check(dx0, c['grad_x64'])
    print(f'{case} composition vs the reference in fp64, in bounds: dx {r0:.3e}; fused vs composition {du.check(dx, dx0):.3e}')
    assert r0 <= 1.0
    m.fused_input_gradient = True
    m.train()
    with pytest.raises(ValueError):
        m.input_gradient(x, cot)


# ---- c. the online recogniser ----
def test_online_explain_runs_the_hip_backward():
    import agcn_amd  # noqa: F401
    from agcn_amd import ops
    from agcn_amd.online import ActionRecognition
    c = gu.online_case()
    meta = c['meta']
    ar = ActionRecognition(model='model.sgn_v15.SGN', model_args=meta['model_args'], device=DEV, **meta['recogniser'])
    assert ar.model.fused_input_gradient is True and ar.seg == 4
    ar.model.load_state_dict(gu.online_model(meta).state_dict())
    for f in vu._npz(meta['frames'])['frames']:
        ar.append_data(f)
    ar.predict(draws=c['draws'])
    rows, _ = ops.sgn_sample(ar.window, ar.draws, ar.seg)
    assert torch.equal(rows.cpu().view(-1), torch.from_numpy(c['rows']).view(-1)), 'not the rows the margin was asserted on'
    tensor, bwd, grad = ops.SGN_STATS['forward_tensor'], dict(ops.SGN15_BWD_STATS), dict(ops.SGN_GRAD_STATS)
    sal, classes = ar.explain()
    assert ops.SGN_STATS['forward_tensor'] == tensor, 'explain ran the composition'
    assert ops.SGN15_BWD_STATS == dict(clip_bwd=bwd['clip_bwd'] + 1, frames_bwd=bwd['frames_bwd'] + 1)
    assert ops.SGN_GRAD_STATS['sample_bwd'] == grad['sample_bwd'] + 1
    S, seg = ar.multi_test, ar.seg
    assert sal.shape == (1, meta['recogniser']['max_frame'], 2, 15) and np.isfinite(sal).all() and sal.max() > 0
    assert int(classes[0]) == int(torch.argmax(ar.logits, 1)[0])
    # bit for bit ops.sgn_sample_bwd of model.input_gradient on the re-sampled rows
    cot = (torch.nn.functional.one_hot(torch.argmax(ar.logits, 1), ar.logits.shape[1]).float() / S).repeat_interleave(S, 0)
    _, _, dx = ar.model.input_gradient(rows.view(S, seg, -1), cot)
    dwin = ops.sgn_sample_bwd(ar.window, ar.draws, dx.view(1, S, seg, -1), seg)
    dwin2, _ = ar._explain_device()
    assert torch.equal(dwin2, dwin)
    assert np.array_equal(sal, dwin.square().sum(1).sqrt().permute(0, 1, 3, 2).cpu().numpy())
    # the composition's saliency (flag off) within the bound
    ar.model.fused_input_gradient = False
    try:
        sal0, classes0 = ar.explain()
        dwin0, _ = ar._explain_device()
    finally:
        ar.model.fused_input_gradient = True
    assert ops.SGN_STATS['forward_tensor'] == tensor + 2
    r = dict(saliency=du.check(sal, sal0), dwin=du.check(dwin, dwin0))
    print('online explain fused vs the composition, in bounds: ' + ' '.join(f'{k} {v:.3e}' for k, v in r.items()))
    assert all(v <= 1.0 for v in r.values()) and np.array_equal(classes, classes0)
    for k in (-1, ar.logits.shape[1], 1.5):
        with pytest.raises(ValueError):
            ar.explain(k)
