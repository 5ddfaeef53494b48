"""GPU tests of the online-recognition path against fixtures computed by the reference on the CPU
(tests/golden/make_online_golden.py): ``preprocess.pre_normalization`` (agcn_prenorm), the device ring with its moving
average (agcn_skel_append) and ``online.ActionRecognition`` end to end.

Bound of the normalised data: max|out - ref| <= 5e-6 * max(1, max|ref|).  A numpy emulation of the kernel's arithmetic
(rotation matrices in fp64, their product applied once in fp32, the same index plan) was within 3.9e-7 of the reference
over 40 such cases; the bound leaves ~13x for FMA contraction and the GPU's own rounding.  What the reference leaves
null must be exactly zero."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
PRENORM_TOL = 5e-6
GROUPS = ['base_v15', 'base_v25', 'base_v18', 'firstframe_v25', 'nopad_v18', 'noz_v15', 'zaxis2_v25']
# T = 150, V = 25: more frames than one 64-frame chunk of the padding plan's prefix sum (leading nulls across a chunk
# boundary) and more (frame, joint) pairs than the workgroup has threads
LONG_GROUPS = ['long_v25']
V15_AXES = dict(zaxis=(8, 1), xaxis=(2, 5))


def _dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def cases():
    both = dict(np.load(os.path.join(GOLDEN, 'prenorm_cases.npz')))
    long_ = np.load(os.path.join(GOLDEN, 'prenorm_long.npz'))
    assert long_['groups'].tolist() == LONG_GROUPS
    both.update({k: long_[k] for k in long_.files if k != 'groups'})
    return both


@pytest.fixture(scope='module')
def stream():
    return np.load(os.path.join(GOLDEN, 'online_stream_v15.npz'))


def _check_normalised(out, ref, what):
    scale = max(1.0, float(np.abs(ref).max()))
    err = float(np.abs(out - ref).max())
    print(f'{what}: max|out - ref| = {err:.3e} (bound {PRENORM_TOL * scale:.3e})')
    assert err <= PRENORM_TOL * scale, (what, err)
    assert not out[ref == 0].any(), f'{what}: a null frame or joint of the reference is not exactly zero'


def test_fixture_groups_are_all_listed(cases):
    assert sorted(cases['groups'].tolist()) == sorted(GROUPS)


@pytest.mark.parametrize('group', GROUPS + LONG_GROUPS)
def test_pre_normalization_matches_reference(cases, group):
    import agcn_amd  # noqa: F401
    from agcn_amd import preprocess
    raw, ref = cases[group + '.raw'], cases[group + '.ref']             # (N, M, T, V, 3), (N, 3, T, V, M)
    kinds, opts = cases[group + '.kinds'].tolist(), json.loads(str(cases[group + '.opts']))
    assert raw.shape[0] > 1
    data = torch.from_numpy(np.ascontiguousarray(np.transpose(raw, [0, 4, 2, 3, 1]))).to(_dev())
    before = data.clone()
    out = preprocess.pre_normalization(data, **opts)
    assert out.shape == data.shape and torch.equal(data, before)
    out = out.cpu().numpy()
    for i, kind in enumerate(kinds):
        _check_normalised(out[i], ref[i], f'{group}[{kind}]')
        if kind == 'zero':
            assert not out[i].any()


def _recogniser(model=None, window=24, moving_avg=1):
    import agcn_amd  # noqa: F401
    from agcn_amd.online import ActionRecognition
    return ActionRecognition(model if model is not None else torch.nn.Identity(), max_frame=window, max_num_skeleton=4,
                             max_num_skeleton_true=2, num_joint=15, moving_avg=moving_avg, **V15_AXES)


@pytest.mark.parametrize('moving_avg', [1, 3])
def test_stream_matches_reference_after_every_append(stream, moving_avg):
    """Fill phase, leading null frames, the interior gap of body 3, the wrap-around (29 frames into a ring of 24) and the
    recursive moving average."""
    frames, wins, sels = stream['frames'], stream[f'win_ma{moving_avg}'], stream[f'sel_ma{moving_avg}']
    assert frames.shape == (29, 4, 1, 15, 3) and wins.shape == (29, 1, 3, 24, 15, 2)
    ar = _recogniser(moving_avg=moving_avg)
    for i, f in enumerate(frames):
        ar.append_data(f)
        out = ar.normalize().cpu().numpy()
        assert ar.selected.cpu().numpy().tolist() == [sels[i].tolist()], (i, ar.energy.cpu().numpy())
        _check_normalised(out, wins[i], f'moving_avg={moving_avg} append {i}')


def test_ring_equals_a_plain_window(stream):
    """After the stream has wrapped, a fresh recogniser fed only the last 24 frames holds the same window in slots
    0..23 with origin 0: the normalised windows must be bitwise identical."""
    frames = stream['frames']
    ar = _recogniser()
    for f in frames:
        ar.append_data(f)
    assert ar.counter == 24 and ar.head == (29 - 24) % 24 != 0
    fresh = _recogniser()
    for f in frames[-24:]:
        fresh.append_data(torch.from_numpy(f))           # tensors are taken as well as arrays
    assert fresh.head == 0
    a, b = ar.normalize(), fresh.normalize()
    assert torch.equal(a, b) and torch.equal(ar.selected, fresh.selected) and torch.equal(ar.energy, fresh.energy)
    ar.reset()
    assert ar.counter == 0 and not ar.ring.any()
    with pytest.raises(ValueError):
        ar.append_data(frames[0][:3])                    # fewer bodies than the ring tracks


def test_full_size_ring_equals_a_plain_window():
    """The deployment shape (window 300, 4 tracked bodies, 25 joints), wrapped by 37 frames, against the same 300 frames
    handed to ``ops.prenorm`` as a plain tensor: bitwise identical, and the two active bodies are the ones selected."""
    import agcn_amd  # noqa: F401
    from agcn_amd import ops
    from agcn_amd.online import ActionRecognition
    rng = np.random.default_rng(5)
    frames = np.zeros((337, 4, 1, 25, 3), dtype=np.float32)
    frames[:, 2, 0] = rng.standard_normal((337, 25, 3)) * 0.2 + (0.3, 2.5, 0.9)
    frames[40:, 0, 0] = rng.standard_normal((297, 25, 3)) * 0.4 + (1.0, 2.2, 0.8)
    frames[100:130, 0] = 0
    ar = ActionRecognition(torch.nn.Identity(), max_frame=300, max_num_skeleton=4, max_num_skeleton_true=2, num_joint=25)
    for f in frames:
        ar.append_data(f)
    assert ar.head == 37
    win = ar.normalize()
    assert ar.selected.cpu().tolist() == [[0, 2]]
    plain = torch.from_numpy(np.ascontiguousarray(frames[37:, :, 0].transpose(1, 0, 2, 3))).to(_dev())[None]
    out, sel, energy = ops.prenorm(plain, num_select=2)
    assert torch.equal(out, win) and torch.equal(sel, ar.selected) and torch.equal(energy, ar.energy)
    assert torch.isfinite(out).all() and float(out.abs().max()) < 10.0
    # body 0 (selected first) starts with null frames: they are compacted away, so its frame 0 is centred on joint 1
    assert not out[0, :, 0, 1, 0].any() and out[0, :, 0, 0, 0].any()


@pytest.fixture(scope='module')
def model_run():
    """online_model_v15.npz through ActionRecognition, raw frames in: what predict() returned and left on the device at
    the recorded appends, the folded-path counters around the first prediction, and a repeated prediction."""
    import agcn_amd  # noqa: F401
    from agcn_amd import ops
    from agcn_amd.model.aagcn import Model
    from oracle import agcn_oracle as orc
    fx = np.load(os.path.join(GOLDEN, 'online_model_v15.npz'))
    v, window, tracked, chosen, classes, seed = (int(x) for x in fx['meta'])
    model = Model(num_class=classes, num_point=v, num_person=chosen, graph='graph.openpose_b25_j15.Graph',
                  graph_args=dict(labeling_mode='spatial'), model_layers=10)
    model.load_state_dict(orc.aagcn_randomized_state(orc.aagcn_model_param_shapes(classes, v), seed,
                                                     stress=float(fx['stress'])))
    ar = _recogniser(model, window=window)
    got, stats = [], None
    for i, f in enumerate(fx['frames']):
        ar.append_data(f)
        if i in fx['record'].tolist():
            before = dict(ops.INFER_STATS)
            scores, label = ar.predict()
            if stats is None:
                stats = {k: ops.INFER_STATS[k] - before[k] for k in before}
            got.append((ar.logits[0].cpu().numpy(), np.asarray(scores, dtype=np.float32), label))
    again = ar.predict()
    return fx, got, stats, again


def test_model_logits_scores_and_labels(model_run):
    """Logits within the project's forward tolerance 1e-4 * max(1, max|ref|), scores within 1e-5, labels equal, at an
    append while the window fills, at the one that fills it and after the ring has wrapped.  (The seeded parameter
    recipe gives logits of ~1e6, as in the other eval-mode model fixtures, so the scores are one-hot.)"""
    fx, got, _, _ = model_run
    assert len(got) == 3
    for (logits, scores, label), ref_l, ref_s, i in zip(got, fx['logits'], fx['scores'], fx['record']):
        scale = max(1.0, float(np.abs(ref_l).max()))
        err_l, err_s = float(np.abs(logits - ref_l).max()), float(np.abs(scores - ref_s).max())
        print(f'append {i}: logits err {err_l:.3e} (bound {1e-4 * scale:.3e}), scores err {err_s:.3e}')
        assert err_l <= 1e-4 * scale, (i, err_l, scale)
        assert err_s <= 1e-5, (i, err_s)
        assert label == int(ref_l.argmax()) == int(ref_s.argmax())
        assert len(scores) == ref_s.shape[0]


def test_model_ran_on_the_folded_path(model_run):
    from agcn_amd import lib
    _, _, stats, _ = model_run
    # every unit but the 3-channel first one runs folded (none under AGCN_GEMM=f32, which has no folded kernels); the
    # units that do not keep their own gate pass
    nf = 9 if lib.load().agcn_gemm_mode() != b'f32' else 0
    assert stats['aagcn_unit_fused'] == nf and stats['tconv_infer'] >= nf, stats
    assert stats['stc_apply'] == 10 - nf, stats


def test_prediction_is_repeatable(model_run):
    _, got, _, again = model_run
    scores, label = again
    assert np.array_equal(np.asarray(scores, dtype=np.float32), got[-1][1]) and label == got[-1][2]
