"""GPU checks of the fused SGN inference path (csrc/sgn.hip) against the reference-generated fixtures
(tests/golden/make_golden_sgn.py): the eval forward, the three ways padded joint rows could leak, independence of the
batch, the fold cache, the sampler, and the online recognisers with ``sgn_preprocess``."""
import json

import numpy as np
import pytest
import torch

from tests import sgn_util as su

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
V15_AXES = dict(zaxis=(8, 1), xaxis=(2, 5))


def _model(case):
    import agcn_amd  # noqa: F401
    from agcn_amd.model.sgn import SGN
    c = su.load_case(case)
    m = SGN(**su.model_args(c['meta']))
    m.load_state_dict(su.torch_state(c['state']))
    return c, m.to(DEV).eval()


def _err(got, ref):
    ref = np.asarray(ref, dtype=np.float64)
    return float(np.abs(np.asarray(got.detach().cpu().numpy() if torch.is_tensor(got) else got, dtype=np.float64)
                        - ref).max() / max(1.0, float(np.abs(ref).max())))


def _stats():
    from agcn_amd import ops
    return dict(ops.SGN_STATS)


def _delta(before):
    now = _stats()
    return {k: now[k] - before[k] for k in now}


@pytest.mark.parametrize('case', su.CASES)
def test_fused_eval_matches_reference(case):
    c, m = _model(case)
    x = torch.from_numpy(c['x']).to(DEV)
    before = _stats()
    with torch.no_grad():
        logits, g = m(x)
    assert _delta(before) == dict(frames_hip=1, clip_hip=1, sample_hip=0, forward_tensor=0)
    e_l = _err(logits, c['logits'])
    e_g = float(np.abs(g.cpu().numpy().astype(np.float64) - c['g']).max())
    print(f'{case}: fused vs reference: logits {e_l:.2e} (relative to max(1, max|ref|)), g {e_g:.2e} (absolute)')
    assert tuple(g.shape) == c['g'].shape
    assert e_l < 1e-4 and e_g < 1e-4


def test_padded_rows_stay_out_of_the_maximum():
    """Padded joint rows hold relu(folded bias).  With a large positive gcn3 bias and every input of one joint negative
    the fused path must still equal the composition."""
    c, m = _model('v15_seg20')
    with torch.no_grad():
        m.gcn3.bn.bias.fill_(4.0)
        m.gcn3.bn.running_mean.zero_()
    x = c['x'].reshape(5, 20, 15, 3).copy()
    x[:, :, 3, :] = -np.abs(x[:, :, 3, :]) - 0.5
    x = torch.from_numpy(x.reshape(5, 20, 45)).to(DEV)
    with torch.no_grad():
        logits, g = m(x)
        ref_l, ref_g = m.forward_tensor(x)
    assert float(m._images()[0][-256:].min()) > 1.0     # the folded gcn3 bias, the last region of the image
    e_l, e_g = _err(logits, ref_l.cpu().numpy()), _err(g, ref_g.cpu().numpy())
    print(f'padding guard: fused vs composition: logits {e_l:.2e}, g {e_g:.2e}')
    assert e_l < 1e-4 and e_g < 1e-4


def test_a_clip_does_not_depend_on_its_batch():
    c, m = _model('v15_seg20')
    x = torch.from_numpy(c['x']).to(DEV)
    with torch.no_grad():
        logits, g = m(x)
        for n in range(x.shape[0]):
            l1, g1 = m(x[n:n + 1].contiguous())
            assert torch.equal(l1[0], logits[n]) and torch.equal(g1[0], g[n]), n
        # the clip in front changes: dif at t = 0 and the temporal conv at t = 0 / seg - 1 must not see it
        y = x.clone()
        y[1] += 3.0
        y[3] = 0.0
        l2, g2 = m(y)
    for n in (0, 2, 4):
        assert torch.equal(l2[n], logits[n]) and torch.equal(g2[n], g[n]), n
    assert not torch.equal(l2[1], logits[1])


def test_fold_cache_follows_the_parameters():
    c, m = _model('v15_seg20')
    x = torch.from_numpy(c['x']).to(DEV)
    with torch.no_grad():
        first, _ = m(x)
        again, _ = m(x)
        assert torch.equal(first, again)
        m.gcn2.bn.weight.add_(0.5)
        changed, _ = m(x)
        ref, _ = m.forward_tensor(x)
        assert not torch.equal(changed, first)
        assert _err(changed, ref.cpu().numpy()) < 1e-4
        m.load_state_dict(su.torch_state(c['state']))
        back, _ = m(x)
    assert torch.equal(back, first)


def test_env_switch_and_grad_mode_run_the_composition(monkeypatch):
    c, m = _model('v7_seg12_nobias')
    x = torch.from_numpy(c['x']).to(DEV)
    before = _stats()
    logits, _ = m(x)                                   # grad mode
    monkeypatch.setenv('AGCN_SGN_HIP', '0')
    with torch.no_grad():
        off, _ = m(x)
    assert _delta(before) == dict(frames_hip=0, clip_hip=0, sample_hip=0, forward_tensor=2)
    assert _err(logits, c['logits']) < 1e-4 and _err(off, c['logits']) < 1e-4


@pytest.mark.parametrize('name', su.WINDOWS)
def test_sampler_matches_reference(name):
    import agcn_amd  # noqa: F401
    from agcn_amd import ops
    f = su._npz('sgn_sample.npz')
    win = torch.from_numpy(f[name + '.win'][None]).to(DEV)
    keep = win.clone()
    r = torch.from_numpy(f[name + '.r'].view(np.int32)[None]).to(DEV)
    before = _stats()
    out, L = ops.sgn_sample(win, r, 20)
    assert _delta(before)['sample_hip'] == 1
    assert int(L[0]) == int(f[name + '.L'])
    assert np.array_equal(out[0].cpu().numpy(), f[name + '.out'])
    assert torch.equal(win, keep)


def test_sampler_edges_and_batches():
    import agcn_amd  # noqa: F401
    from agcn_amd import ops
    f = su._npz('sgn_sample.npz')
    mixed = f['mixed.win']
    wins = np.stack([mixed, np.zeros_like(mixed), mixed[:, ::-1].copy()])
    r = np.stack([f['mixed.r'], f['mixed.r'], f['mixed.r'][::-1].copy()])
    want, want_L = su.sample_emulate(wins, r, 20)
    out, L = ops.sgn_sample(torch.from_numpy(wins).to(DEV), torch.from_numpy(r.view(np.int32)).to(DEV), 20)
    assert np.array_equal(L.cpu().numpy(), want_L) and int(L[1]) == 0
    assert np.array_equal(out.cpu().numpy(), want) and not out[1].any()
    # any draw stays inside the window: all-ones patterns still return rows of the source
    ones = torch.full((1, 5, 20), -1, dtype=torch.int32, device=DEV)
    out, L = ops.sgn_sample(torch.from_numpy(mixed[None]).to(DEV), ones, 20)
    want, _ = su.sample_emulate(mixed[None], np.full((1, 5, 20), 0xFFFFFFFF, dtype=np.uint32), 20)
    assert np.array_equal(out.cpu().numpy(), want)
    rows = np.transpose(mixed, (1, 3, 2, 0)).reshape(-1, 45)
    assert all(any(np.array_equal(row, src) for src in rows) for row in out[0, 0].cpu().numpy())
    # seg = 30 (another interval plan), uint32 input
    r30 = np.random.default_rng(5).integers(0, 1 << 32, (1, 2, 30), dtype=np.uint64).astype(np.uint32)
    want, want_L = su.sample_emulate(f['full.win'][None], r30, 30)
    out, L = ops.sgn_sample(torch.from_numpy(f['full.win'][None]).to(DEV), torch.from_numpy(r30.view(np.int32)).to(DEV), 30)
    assert np.array_equal(out.cpu().numpy(), want) and int(L[0]) == 600


@pytest.fixture(scope='module')
def online():
    import agcn_amd  # noqa: F401
    from agcn_amd.model.sgn import SGN
    f = su._npz('sgn_online_v15.npz')
    meta = json.loads(str(f['meta']))
    shapes = {str(k): tuple(int(d) for d in str(s).split('x') if d) for k, s in zip(f['keys'], f['shapes'])}
    state = su.sgn_state(shapes, meta['seed'])
    assert np.array_equal(su.checksums(state), f['checksums'])
    m = SGN(**su.model_args(meta))
    m.load_state_dict(su.torch_state(state))
    return f, meta, m


def _recogniser(cls, online, **kw):
    f, meta, m = online
    return cls(m, max_frame=meta['window'], max_num_skeleton=meta['max_person'], max_num_skeleton_true=meta['select'],
               num_joint=15, sgn_preprocess=True, multi_test=meta['multi_test'], **V15_AXES, **kw)


def test_action_recognition_with_sgn_preprocess(online):
    from agcn_amd.online import ActionRecognition
    f, meta, _ = online
    ar = _recogniser(ActionRecognition, online)
    record = f['record'].tolist()
    for i, frame in enumerate(f['frames']):
        ar.append_data(frame)
        if i not in record:
            continue
        k = record.index(i)
        before = _stats()
        scores, label = ar.predict(draws=f['draws'][k])
        assert _delta(before) == dict(frames_hip=1, clip_hip=1, sample_hip=1, forward_tensor=0)
        e = float(np.abs(np.asarray(scores, dtype=np.float64) - f['scores'][k]).max())
        e_l = _err(ar.logits[0], f['logits'][k])
        print(f'append {i}: mean scores {e:.2e}, mean logits {e_l:.2e}, label {label}')
        assert e < 1e-4 and label == int(f['labels'][k])
        assert torch.equal(ar.draws.cpu(), torch.from_numpy(f['draws'][k].view(np.int32))[None])
    scores, label = ar.predict()                       # draws of its own: still a prediction
    assert len(scores) == meta['num_class'] and ar.draws.shape == (1, meta['multi_test'], meta['seg'])


def test_labelling_equals_the_frame_by_frame_loop(online):
    """The kernels give a window the same bits alone and in a batch; the mean over the draws and the softmax behind them
    are torch reductions whose order may depend on the batch, so scores are compared at 1e-6 (a few fp32 ulps of 1)."""
    from agcn_amd.online import ActionRecognition, RecordingRecognition
    f, meta, _ = online
    frames = f['frames'][:40]
    draws = np.random.default_rng(11).integers(0, 1 << 32, (40, meta['multi_test'], meta['seg']),
                                               dtype=np.uint64).astype(np.uint32)
    rr = _recogniser(RecordingRecognition, online, batch=16)
    scores, labels, ends = rr.label(frames, draws=draws)
    assert ends.tolist() == list(range(40))
    ar = _recogniser(ActionRecognition, online)
    for i, frame in enumerate(frames):
        ar.append_data(frame)
        s, lb = ar.predict(draws=draws[i])
        assert lb == int(labels[i]), i
        assert float(np.abs(np.asarray(s, dtype=np.float32) - scores[i]).max()) <= 1e-6, i
