"""GPU checks of SGN's eval-mode input gradient on the fused path (csrc/sgn_bwd.hip): against the reference's gradients
(tests/golden/make_golden_sgn_grad.py), the routing of ``SGN.forward`` in grad mode, independence of the batch (bitwise),
the sampler's adjoint against its numpy emulation, and ``explain`` of the online recognisers."""
import json
import os

import numpy as np
import pytest
import torch

from tests import sgn_grad_util as gu
from tests import sgn_util as su

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
V15_AXES = dict(zaxis=(8, 1), xaxis=(2, 5))
ZERO = dict(clip_bwd=0, frames_bwd=0, sample_bwd=0)


def _sgn(meta, state):
    import agcn_amd  # noqa: F401
    from agcn_amd.model.sgn import SGN
    m = SGN(**su.model_args(meta))
    m.load_state_dict(su.torch_state(state))
    return m.to(DEV).eval()


def _err(got, ref):
    ref = np.asarray(ref, dtype=np.float64)
    return float(np.abs(np.asarray(got.detach().cpu().numpy() if torch.is_tensor(got) else got, dtype=np.float64)
                        - ref).max() / max(1.0, float(np.abs(ref).max())))


def _stats():
    from agcn_amd import ops
    return dict(ops.SGN_STATS), dict(ops.SGN_GRAD_STATS)


def _delta(before):
    now = _stats()
    return tuple({k: n[k] - b[k] for k in n} for n, b in zip(now, before))


@pytest.mark.parametrize('case', gu.stored_cases())
def test_fused_input_gradient_matches_reference(case):
    c = gu.load_grad_case(case)
    m = _sgn(c['meta'], c['state'])
    x, cot = torch.from_numpy(c['x']).to(DEV), torch.from_numpy(c['c']).to(DEV)
    before = _stats()
    logits, g, dx = m.input_gradient(x, cot)
    fwd, bwd = _delta(before)
    assert fwd == dict(frames_hip=1, clip_hip=1, sample_hip=0, forward_tensor=0)
    assert bwd == dict(clip_bwd=1, frames_bwd=1, sample_bwd=0)
    e_l = _err(logits, c['logits'])
    e_g = float(np.abs(g.cpu().numpy().astype(np.float64) - c['g']).max())
    e_x = _err(dx, c['grad_x'])
    rows = np.abs(dx.cpu().numpy().astype(np.float64) - c['grad_x']).reshape(-1, c['x'].shape[-1]).max(1)
    print(f"{case}: fused vs reference: logits {e_l:.2e}, g {e_g:.2e}, dx {e_x:.2e} relative to max(1, max|ref| = "
          f"{float(np.abs(c['grad_x']).max()):.1f}); the reference's own fp32 vs fp64 {_err(c['grad_x'], c['grad_x64']):.2e}; "
          f"margin {c['meta']['margin']:.2e}; absolute error per frame: median {np.median(rows):.2e}, max {rows.max():.2e}")
    assert tuple(dx.shape) == c['x'].shape and dx.dtype == torch.float32
    assert e_l < 1e-4 and e_g < 1e-4
    assert e_x < 1e-4


def test_grad_mode_routing():
    from agcn_amd import ops
    c = gu.load_grad_case('v15_seg6')
    m = _sgn(c['meta'], c['state'])
    x, cot = torch.from_numpy(c['x']).to(DEV), torch.from_numpy(c['c']).to(DEV)
    _, g_want, want = m.input_gradient(x, cot)
    # trainable parameters: the composition, as before
    before = _stats()
    xg = x.clone().requires_grad_(True)
    logits, _ = m(xg)
    (logits * cot).sum().backward()
    fwd, bwd = _delta(before)
    assert fwd == dict(frames_hip=0, clip_hip=0, sample_hip=0, forward_tensor=1) and bwd == ZERO
    assert _err(xg.grad, c['grad_x']) < 1e-4 and m.fc.weight.grad is not None
    # frozen parameters and x.requires_grad: the fused forward with the HIP backward behind autograd
    for p in m.parameters():
        p.requires_grad_(False)
    before = _stats()
    xg = x.clone().requires_grad_(True)
    logits, g = m(xg)
    assert logits.requires_grad and not g.requires_grad and torch.equal(g, g_want)
    (logits * cot).sum().backward()
    fwd, bwd = _delta(before)
    assert fwd == dict(frames_hip=1, clip_hip=1, sample_hip=0, forward_tensor=0)
    assert bwd == dict(clip_bwd=1, frames_bwd=1, sample_bwd=0)
    assert torch.equal(xg.grad, want)
    # frozen parameters, x does not ask: grad mode still runs the composition (nothing to differentiate fused)
    before = _stats()
    m(x)
    assert _delta(before)[0]['forward_tensor'] == 1
    # no_grad: the fused forward
    before = _stats()
    with torch.no_grad():
        m(xg)
    assert _delta(before) == (dict(frames_hip=1, clip_hip=1, sample_hip=0, forward_tensor=0), ZERO)
    # the switch turns both off
    os.environ['AGCN_SGN_HIP'] = '0'
    try:
        before = _stats()
        _, _, off = m.input_gradient(x, cot)
        assert _delta(before) == (dict(frames_hip=0, clip_hip=0, sample_hip=0, forward_tensor=1), ZERO)
    finally:
        del os.environ['AGCN_SGN_HIP']
    assert _err(off, c['grad_x']) < 1e-4
    assert ops.sgn_hip_enabled()


@pytest.mark.parametrize('case', ['v15_seg20', 'v25_seg20'])
def test_a_clips_gradient_does_not_depend_on_its_batch(case):
    c = su.load_case(case)
    m = _sgn(c['meta'], c['state'])
    x = torch.from_numpy(c['x']).to(DEV)
    keep = x.clone()
    bs = x.shape[0]
    cot = torch.from_numpy(np.random.default_rng(77).standard_normal((bs, c['meta']['num_class'])).astype(np.float32)).to(DEV)
    _, _, dx = m.input_gradient(x, cot)
    _, _, again = m.input_gradient(x, cot)
    assert torch.equal(dx, again) and torch.equal(x, keep)
    assert bool(torch.isfinite(dx).all()) and float(dx.abs().max()) > 0
    for n in range(bs):
        _, _, one = m.input_gradient(x[n:n + 1].contiguous(), cot[n:n + 1].contiguous())
        assert torch.equal(one[0], dx[n]), n
    if bs >= 5:
        # the clips in between change: the dif term at t = 0 / seg - 1 and the conv's padding must not see them
        y = x.clone()
        y[1] += 3.0
        y[3] = 0.0
        _, _, dy = m.input_gradient(y, cot)
        for n in (0, 2, 4):
            assert torch.equal(dy[n], dx[n]), n
        assert not torch.equal(dy[1], dx[1])


@pytest.mark.parametrize('name', su.WINDOWS)
def test_sample_bwd_matches_emulation(name):
    import agcn_amd  # noqa: F401
    from agcn_amd import ops
    f = su._npz('sgn_sample.npz')
    win, r = f[name + '.win'][None], f[name + '.r'][None]
    d = np.random.default_rng(9).standard_normal((1, 5, 20, win.shape[3] * 3)).astype(np.float32)
    tw, tr, td = torch.from_numpy(win).to(DEV), torch.from_numpy(r.view(np.int32)).to(DEV), torch.from_numpy(d).to(DEV)
    kw, kr, kd = tw.clone(), tr.clone(), td.clone()
    before = _stats()
    dwin = ops.sgn_sample_bwd(tw, tr, td, 20)
    assert _delta(before)[1] == dict(clip_bwd=0, frames_bwd=0, sample_bwd=1)
    assert np.array_equal(dwin.cpu().numpy(), gu.sample_bwd_emulate(win, r, d, 20))
    assert torch.equal(tw, kw) and torch.equal(tr, kr) and torch.equal(td, kd)


def test_sample_bwd_edges():
    import agcn_amd  # noqa: F401
    from agcn_amd import ops
    f = su._npz('sgn_sample.npz')
    mixed = f['mixed.win']
    wins = np.stack([mixed, np.zeros_like(mixed), mixed[:, ::-1].copy()])
    r = np.stack([f['mixed.r'], f['mixed.r'], np.full_like(f['mixed.r'], 0xFFFFFFFF)])
    d = np.random.default_rng(10).standard_normal((3, 5, 20, 45)).astype(np.float32)
    dwin = ops.sgn_sample_bwd(torch.from_numpy(wins).to(DEV), torch.from_numpy(r.view(np.int32)).to(DEV),
                              torch.from_numpy(d).to(DEV), 20)
    want = gu.sample_bwd_emulate(wins, r, d, 20)
    assert np.array_equal(dwin.cpu().numpy(), want)
    assert not dwin[1].any() and bool(dwin[0].any()) and bool(dwin[2].any())


@pytest.fixture(scope='module')
def online():
    f = su._npz('sgn_online_v15.npz')
    meta = json.loads(str(f['meta']))
    shapes = {str(k): tuple(int(d) for d in str(s).split('x') if d) for k, s in zip(f['keys'], f['shapes'])}
    state = su.sgn_state(shapes, meta['seed'])
    assert np.array_equal(su.checksums(state), f['checksums'])
    return f, meta, _sgn(meta, state)


def test_explain_with_sgn(online):
    from agcn_amd import ops
    from agcn_amd.online import ActionRecognition
    f, meta, m = online
    ar = ActionRecognition(m, max_frame=meta['window'], max_num_skeleton=meta['max_person'],
                           max_num_skeleton_true=meta['select'], num_joint=15, sgn_preprocess=True,
                           multi_test=meta['multi_test'], **V15_AXES)
    with pytest.raises(RuntimeError):
        ar.explain()
    last = int(f['record'][1])
    for frame in f['frames'][:last + 1]:
        ar.append_data(frame)
    _, label = ar.predict(draws=f['draws'][1])
    before = _stats()
    sal, classes = ar.explain()
    fwd, bwd = _delta(before)
    assert fwd == dict(frames_hip=1, clip_hip=1, sample_hip=1, forward_tensor=0)
    assert bwd == dict(clip_bwd=1, frames_bwd=1, sample_bwd=1)
    T, S, seg = meta['window'], meta['multi_test'], meta['seg']
    assert sal.shape == (1, T, 2, 15) and sal.dtype == np.float32 and classes.tolist() == [label]
    # the chain by hand
    rows, _ = ops.sgn_sample(ar.window, ar.draws, seg)
    cot = torch.zeros(S, meta['num_class'], device=DEV)
    cot[:, label] = 1.0 / S
    _, _, dx = m.input_gradient(rows.view(S, seg, -1), cot)
    dwin = ops.sgn_sample_bwd(ar.window, ar.draws, dx.view(1, S, seg, -1), seg)
    want = dwin.square().sum(1).sqrt().permute(0, 1, 3, 2).cpu().numpy()
    assert np.array_equal(sal, want) and float(sal.max()) > 0
    # rows no draw picked: the pick table of the emulation on an all-ones cotangent
    picked = gu.sample_bwd_emulate(ar.window.cpu().numpy(), ar.draws.cpu().numpy().view(np.uint32),
                                   np.ones((1, S, seg, 45), dtype=np.float32), seg)
    hit = picked[0, 0, :, 0, :] > 0                                          # (T, body)
    assert 0 < hit.sum() <= S * seg and not sal[0][~hit].any()
    # another class
    other = (label + 1) % meta['num_class']
    sal2, classes2 = ar.explain(other)
    assert classes2.tolist() == [other] and sal2.shape == sal.shape and not np.array_equal(sal2, sal)
    assert not sal2[0][~hit].any()


def test_explain_with_agcn():
    import agcn_amd  # noqa: F401
    from agcn_amd.model.aagcn import Model
    from agcn_amd.online import ActionRecognition
    from oracle import agcn_oracle as orc
    fx = np.load(os.path.join(su.GOLDEN, 'online_model_v15.npz'))
    v, window, tracked, chosen, classes, seed = (int(x) for x in fx['meta'])
    model = Model(num_class=classes, num_point=v, num_person=chosen, graph='graph.openpose_b25_j15.Graph',
                  graph_args=dict(labeling_mode='spatial'), model_layers=10)
    model.load_state_dict(orc.aagcn_randomized_state(orc.aagcn_model_param_shapes(classes, v), seed,
                                                     stress=float(fx['stress'])))
    ar = ActionRecognition(model, max_frame=window, max_num_skeleton=tracked, max_num_skeleton_true=chosen, num_joint=v,
                           **V15_AXES)
    with pytest.raises(RuntimeError):
        ar.explain()
    for frame in fx['frames'][:int(fx['record'][0]) + 1]:
        ar.append_data(frame)
    _, label = ar.predict()
    sal, cls = ar.explain()
    assert sal.shape == (1, window, chosen, v) and cls.tolist() == [label]
    assert all(p.requires_grad for p in ar.model.parameters())          # left as they were
    for p in ar.model.parameters():
        p.requires_grad_(False)
    x = ar.window.detach().clone().requires_grad_(True)
    out = ar.model(x)
    out = out[0] if isinstance(out, tuple) else out
    out[:, label].sum().backward()
    want = x.grad.square().sum(1).sqrt().permute(0, 1, 3, 2).cpu().numpy()
    assert float(want.max()) > 0 and np.array_equal(sal, want)
