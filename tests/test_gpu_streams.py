"""GPU checks of the bone / motion input streams (csrc/streams.hip): the forward bit for bit against the files the
reference's dataset scripts wrote and against the tensor-code form, the backward against the same formula in fp64 within
the bound its fixed summation order gives, a bone model through ``prepare_batch``, the two-stream online recogniser, and
the host refusals."""
import os
import pickle

import numpy as np
import pytest
import torch

from tests import streams_util as su
from tests.test_gpu_parity import GTOL, TOL      # the project's parity tolerances, imported, not copied

pytestmark = pytest.mark.gpu

# (N, C, T, V, M): T = 1 (the motions are all zero), T = 2, M = 1 and M = 3 (odd: element by element), M = 4 (16-byte
# vectors), V = 15 / 18 / 25, N = 1, C = 2, one full-size clip pair (more than one workgroup), and more than 2048
# workgroups of items (the grid-stride loop)
SHAPES = [(2, 3, 1, 25, 2), (2, 3, 2, 25, 2), (2, 3, 5, 25, 1), (2, 3, 5, 18, 3), (2, 3, 5, 25, 4), (2, 3, 4, 15, 2),
          (2, 3, 4, 18, 2), (1, 3, 5, 25, 2), (2, 2, 5, 25, 2), (2, 3, 300, 25, 2), (24, 3, 300, 25, 2)]


def _dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _ops():
    import agcn_amd  # noqa: F401
    from agcn_amd import ops
    assert ops.stream_hip_enabled()
    return ops


def _x(shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g).to(_dev())


def _guarded(shape, misalign=0):
    """A tensor of `shape` inside a NaN-filled buffer with one guard row of shape[1:] (plus `misalign` floats) in front and
    one behind -> (tensor, buffer, slice of the tensor in the flat buffer)."""
    n = int(np.prod(shape))
    row = n // shape[0]
    buf = torch.full((n + 2 * row + misalign,), float('nan'), device=_dev())
    lo = row + misalign
    return buf[lo:lo + n].view(shape), buf, slice(lo, lo + n)


def _guards_untouched(buf, sl):
    return bool(torch.isnan(buf[:sl.start]).all()) and bool(torch.isnan(buf[sl.stop:]).all())


def _run_guarded(ops, x, parent, want, misalign=0):
    outs, bufs = {}, {}
    for s in want:
        outs[s], buf, sl = _guarded(tuple(x.shape), misalign)
        bufs[s] = (buf, sl)
    with torch.no_grad():
        got = ops.skeleton_streams(x, parent, want, out=outs)
    torch.cuda.synchronize()
    for s in want:
        assert got[s].data_ptr() == outs[s].data_ptr()
        assert _guards_untouched(*bufs[s]), f'{s}: a guard row was written'
        assert not torch.isnan(got[s]).any(), f'{s}: an element was not written'
    return got


# ---- forward ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,V', [('ntu', 25), ('kinetics', 18)])
def test_forward_equals_the_reference_files_bit_for_bit(name, V):
    ops, f = _ops(), su.fixture(name)
    x = torch.from_numpy(f['x'].copy()).to(_dev())
    parent = su.graph_parents(V)
    for want in su.SUBSETS:                                  # every non-empty subset of outputs, one launch each
        got = _run_guarded(ops, x, parent, want)
        assert tuple(got) == want
        for s in want:
            assert np.array_equal(got[s].cpu().numpy(), f[s]), (want, s)
    got = ops.skeleton_streams(x, parent, su.DERIVED)        # outputs allocated by the call
    for s in su.DERIVED:
        assert np.array_equal(got[s].cpu().numpy(), f[s]), s


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_forward_equals_tensor_code_bit_for_bit(shape):
    ops = _ops()
    x = _x(shape, seed=sum(shape))
    x[-1, :, shape[2] // 2:] = 0                             # the dataset's zero padding
    parent = su.graph_parents(shape[3])
    ref = ops.streams_ref(x, parent, su.DERIVED)
    got = _run_guarded(ops, x, parent, su.DERIVED)
    for s in su.DERIVED:
        assert torch.equal(got[s], ref[s]), s
    if shape[2] == 1:
        assert not got['joint_motion'].any() and not got['bone_motion'].any()
    own = [v for v, p in enumerate(parent) if p == v]
    assert own and not got['bone'][:, :, :, own].any()       # a joint that is its own parent: exactly 0
    for want in (('bone',), ('joint_motion',), ('bone_motion',), ('joint_motion', 'bone')):
        one = _run_guarded(ops, x, parent, want)
        assert all(torch.equal(one[s], ref[s]) for s in want), want
    if shape[4] in (2, 4):
        # outputs aligned to 4 bytes only: the same tensor goes element by element, same bits
        got = _run_guarded(ops, x, parent, su.DERIVED, misalign=1)
        assert all(torch.equal(got[s], ref[s]) for s in su.DERIVED)


# ---- backward --------------------------------------------------------------------------------------------------------------
def _check_backward(ops, cot, parent, what):
    got = ops.streams_bwd(cot, parent, su.WEIGHTS)
    want, mag, cnt = su.backward64({k: v.cpu().numpy() for k, v in cot.items()}, parent)
    err = np.abs(got.cpu().numpy().astype(np.float64) - want)
    bound = su.backward_bound(mag, cnt)
    ratio = float((err / np.where(bound > 0, bound, 1.0)).max())
    print(f'{what}: max err {float(err.max()):.3e}, max err / bound {ratio:.3f}, most addends {int(cnt.max())}')
    assert (err <= bound).all(), (what, float(err.max()), ratio)
    return got


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_backward_within_the_bound_of_its_summation_order(shape):
    ops = _ops()
    parent = su.graph_parents(shape[3])
    cot = {s: _x(shape, seed=100 + i) for i, s in enumerate(su.STREAMS)}
    dx = _check_backward(ops, cot, parent, f'{shape} all four')
    for s in su.STREAMS:
        _check_backward(ops, {s: cot[s]}, parent, f'{shape} {s} alone')
    assert torch.equal(ops.streams_bwd(cot, parent, su.WEIGHTS), dx)          # fixed order: the same bits again
    if shape[2] == 1:
        assert not ops.streams_bwd({'joint_motion': cot['joint_motion'], 'bone_motion': cot['bone_motion']}, parent).any()


def test_autograd_node_makes_the_same_gradient():
    ops = _ops()
    shape = (2, 3, 6, 25, 2)
    parent = su.graph_parents(25)
    x = _x(shape, 7).requires_grad_(True)
    out = ops.skeleton_streams(x, parent, su.DERIVED)
    cot = {s: _x(shape, 200 + i) for i, s in enumerate(su.DERIVED)}
    dx, = torch.autograd.grad([out[s] for s in su.DERIVED], x, [cot[s] for s in su.DERIVED])
    assert torch.equal(dx, ops.streams_bwd(cot, parent))
    only, = torch.autograd.grad(ops.skeleton_streams(x, parent, su.DERIVED)['bone_motion'].sum(), x)
    assert torch.equal(only, ops.streams_bwd({'bone_motion': torch.ones_like(x)}, parent))


# ---- host refusals ---------------------------------------------------------------------------------------------------------
def test_ops_refuses_before_any_launch(monkeypatch):
    ops = _ops()
    x = _x((2, 3, 4, 25, 2))
    parent = su.graph_parents(25)

    def reached(*a, **k):
        raise AssertionError('a refused call reached the library')
    monkeypatch.setattr(ops._lib, 'call', reached)
    monkeypatch.setattr(ops._lib, 'status', reached)
    with pytest.raises(ValueError, match='contiguous'):
        ops.skeleton_streams(x.transpose(1, 2), parent)
    with pytest.raises(ValueError, match='contiguous'):
        ops.skeleton_streams(x[:, :, ::2], parent)
    with pytest.raises(ValueError, match='float32'):
        ops.skeleton_streams(x.double(), parent)
    with pytest.raises(ValueError, match='float32'):
        ops.skeleton_streams(x.half(), parent)
    with pytest.raises(ValueError, match='24 entries for 25 joints'):
        ops.skeleton_streams(x, parent[:-1])
    with pytest.raises(ValueError, match='26 entries for 25 joints'):
        ops.skeleton_streams(x, parent + [0])
    with pytest.raises(ValueError, match='parent'):
        ops.skeleton_streams(x, [25] + parent[1:])
    with pytest.raises(ValueError, match='at most 32 joints'):
        ops.skeleton_streams(_x((1, 3, 2, 33, 2)), list(range(33)))
    with pytest.raises(ValueError, match='out'):
        ops.skeleton_streams(x, parent, ('bone',), out={'bone': torch.empty_like(x).cpu()})
    with pytest.raises(ValueError, match='alias'):
        ops.skeleton_streams(x, parent, ('bone',), out={'bone': x})
    with pytest.raises(ValueError, match='d_bone'):
        ops.streams_bwd({'joint': x, 'bone': x[:1].contiguous()}, parent)
    with pytest.raises(ValueError, match='contiguous'):
        ops.streams_bwd({'bone': x.transpose(1, 2)}, parent)


# ---- a bone model ----------------------------------------------------------------------------------------------------------
def test_bone_model_through_prepare_batch_equals_precomputed_bone_input():
    """model.agcn.Model, one training forward + backward at (2, 3, 20, 25, 2): stream='bone' through prepare_batch against the
    same model fed the bone tensor computed on the host with the reference script's statement."""
    _ops()
    from agcn_amd.model.agcn import Model
    from agcn_amd.processor import prepare_batch
    torch.manual_seed(3)
    model = Model(num_class=11, num_point=25, num_person=2, graph='graph.ntu_rgb_d.Graph').to(_dev()).train()
    parent = model.graph.bone_parents
    xn = np.random.default_rng(3).standard_normal((2, 3, 20, 25, 2)).astype(np.float32)
    xn[1, :, 14:] = 0
    bone = xn.copy()
    for v1, v2 in enumerate(parent):
        bone[:, :, :, v1, :] = xn[:, :, :, v1, :] - xn[:, :, :, v2, :]
    label = torch.tensor([3, 7], device=_dev())

    def run(inp):
        state = {k: v.clone() for k, v in model.state_dict().items()}      # the same running statistics for both runs
        model.zero_grad(set_to_none=True)
        out = model(inp)
        out = out[0] if isinstance(out, tuple) else out
        torch.nn.functional.cross_entropy(out, label).backward()
        grads = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
        model.load_state_dict(state)
        return out.detach(), grads

    x = torch.from_numpy(xn).to(_dev()).requires_grad_(True)
    b = torch.from_numpy(bone).to(_dev()).requires_grad_(True)
    ref_out, ref_g = run(b)
    out, g = run(prepare_batch(x, None, 'bone', parent))
    scale = max(1.0, float(ref_out.abs().max()))
    err = float((out - ref_out).abs().max())
    assert err <= TOL * scale, (err, scale)
    assert set(g) == set(ref_g) and len(g) > 50
    worst = 0.0
    for n in ref_g:
        e = float((g[n] - ref_g[n]).abs().max()) / max(float(ref_g[n].abs().max()), 1e-30)
        worst = max(worst, e)
        assert e <= GTOL, (n, e)
    equal = torch.equal(out, ref_out) and all(torch.equal(g[n], ref_g[n]) for n in ref_g)
    print(f'bone model: logits err {err:.3e} (bound {TOL * scale:.1e}), worst gradient err {worst:.3e} (bound {GTOL:.1e}), '
          f'bits equal: {equal}')
    # the gradient reaches the joint data through the transpose of the bone stream
    want, mag, cnt = su.backward64({'bone': b.grad.cpu().numpy()}, parent, (0.0, 1.0, 0.0, 0.0))
    assert (np.abs(x.grad.cpu().numpy() - want) <= su.backward_bound(mag, cnt)).all()


def test_bone_yamls_train_score_and_fuse(tmp_path):
    """train_bone.yaml and test_bone.yaml on joint clips alone: two training steps, the checkpoint scored with save_score,
    and ensemble.py on the joint and bone score files."""
    _ops()
    import ensemble
    from agcn_amd.processor import Processor, load_args
    cfgdir = os.path.join(su.ROOT, 'config', 'nturgbd-cross-view')
    small = ['--batch-size', '4', '--test-batch-size', '4', '--print-log', 'False', '--model-saved-name', '']
    scores = {}
    for stream, cfg in (('joint', 'train_joint.yaml'), ('bone', 'train_bone.yaml')):
        work = tmp_path / stream
        arg = load_args(['--config', os.path.join(cfgdir, cfg), '--work-dir', str(work), '--num-epoch', '1',
                         '--max-steps-per-epoch', '2', '--eval-interval', '100', '--save-score', 'True'] + small)
        arg.train_feeder_args = dict(num_samples=8, window_size=32)
        arg.test_feeder_args = dict(num_samples=6, window_size=32, seed=1)
        assert arg.stream == stream
        p = Processor(arg)
        assert p.stream == stream and (p.stream_parents == tuple(p.model.graph.bone_parents)) == (stream == 'bone')
        p.start()
        scores[stream] = str(work / 'score' / 'epoch1_test.pkl')
        assert os.path.exists(scores[stream])
        labels = p.datasets['test'].label
    ckpt = str(tmp_path / 'bone' / 'weight' / 'Model-1-2.pt')
    arg = load_args(['--config', os.path.join(cfgdir, 'test_bone.yaml'), '--work-dir', str(tmp_path / 'scored'),
                     '--weights', ckpt] + small)
    arg.test_feeder_args = dict(num_samples=6, window_size=32, seed=1)
    assert arg.stream == 'bone' and arg.phase == 'test' and arg.save_score
    p = Processor(arg)
    p.start()
    with open(tmp_path / 'scored' / 'score' / 'epoch1_test.pkl', 'rb') as f:
        again = pickle.load(f)
    with open(scores['bone'], 'rb') as f:
        first = pickle.load(f)
    assert sorted(again) == sorted(first) == list(range(6))
    assert all(np.allclose(again[i], first[i], atol=1e-5) for i in range(6))        # the bone model, scored on bone input
    with open(scores['joint'], 'rb') as f:
        joint = pickle.load(f)
    assert not all(np.allclose(joint[i], first[i], atol=1e-3) for i in range(6))
    with open(tmp_path / 'labels.pkl', 'wb') as f:
        pickle.dump((list(range(6)), [int(v) for v in labels]), f)
    acc = ensemble.main(['--joint-score', scores['joint'], '--bone-score', str(tmp_path / 'scored' / 'score' / 'epoch1_test.pkl'),
                         '--label', str(tmp_path / 'labels.pkl'), '--alpha', '1.0'])
    assert 0.0 <= acc[1] <= acc[5] <= 1.0


# ---- online ----------------------------------------------------------------------------------------------------------------
WINDOW, ALPHA = 20, (1.0, 0.7)


def _models():
    from agcn_amd.model.agcn import Model
    nets = []
    for seed in (11, 12):
        torch.manual_seed(seed)
        nets.append(Model(num_class=9, num_point=25, num_person=2, graph='graph.ntu_rgb_d.Graph'))
    return nets


def _frames(n):
    rng = np.random.default_rng(21)
    frames = np.zeros((n, 4, 1, 25, 3), dtype=np.float32)
    frames[:, 1, 0] = rng.standard_normal((n, 25, 3)) * 0.3 + (0.2, 2.4, 0.9)
    frames[3:, 3, 0] = rng.standard_normal((n - 3, 25, 3)) * 0.4 + (1.0, 2.1, 0.8)
    return frames


def _recogniser(cls=None, **kw):
    from agcn_amd.online import ActionRecognition
    return (cls or ActionRecognition)(max_frame=WINDOW, max_num_skeleton=4, max_num_skeleton_true=2, num_joint=25, **kw)


@pytest.fixture(scope='module')
def online():
    """One two-stream recogniser and the two single-stream ones on the same 27 frames (a ring of 20, wrapped)."""
    ops = _ops()
    joint, bone = _models()
    two = _recogniser(streams=[('joint', joint), ('bone', bone)], alpha=ALPHA)
    rj, rb = _recogniser(model=joint), _recogniser(model=bone)
    for f in _frames(WINDOW + 7):
        for r in (two, rj):
            r.append_data(f)
    scores, label = two.predict()
    sj, lj = rj.predict()
    assert torch.equal(two.window, rj.window)
    bone_window = ops.streams_ref(rj.window, joint.graph.bone_parents, ('bone',))['bone']       # precomputed, tensor code
    rb.window = bone_window
    rb.forward(bone_window)
    return two, rj, rb, scores, label


def test_two_stream_logits_are_the_weighted_sum(online):
    two, rj, rb, scores, label = online
    want = rj.logits + ALPHA[1] * rb.logits
    scale = max(1.0, float(want.abs().max()))
    err = float((two.logits - want).abs().max())
    print(f'two-stream logits: err {err:.3e} (bound {TOL * scale:.1e}), bits equal: {torch.equal(two.logits, want)}')
    assert err <= TOL * scale
    assert len(two.stream_logits) == 2
    assert float((two.stream_logits[0] - rj.logits).abs().max()) <= TOL * scale
    assert float((two.stream_logits[1] - rb.logits).abs().max()) <= TOL * scale
    want_scores = torch.softmax(want, 1)[0].cpu().numpy()
    assert np.abs(np.asarray(scores, dtype=np.float32) - want_scores).max() <= 1e-5 and label == int(want_scores.argmax())
    assert two.stream_parents == tuple(two.models[0].graph.bone_parents) and two.model is two.models[0]


def test_two_stream_explain_folds_the_gradients_into_the_joint_window(online):
    two, rj, rb, _, _ = online
    k = 4
    dwin, classes = two._explain_device(k)
    dj, cj = rj._explain_device(k)
    db, cb = rb._explain_device(k)
    assert classes.tolist() == cj.tolist() == cb.tolist() == [k]
    weights = (1.0, float(np.float32(ALPHA[1])), 0.0, 0.0)        # the weights reach the kernel as C floats
    want, mag, cnt = su.backward64({'joint': dj.cpu().numpy(), 'bone': db.cpu().numpy()}, two.stream_parents, weights)
    err = np.abs(dwin.cpu().numpy().astype(np.float64) - want)
    bound = su.backward_bound(mag, cnt)
    print(f'two-stream explain: max err {float(err.max()):.3e}, max err / bound '
          f'{float((err / np.where(bound > 0, bound, 1.0)).max()):.3f}')
    assert (err <= bound).all() and float(np.abs(want).max()) > 0
    sal, cls = two.explain(k)
    assert sal.shape == (1, WINDOW, 2, 25) and cls.tolist() == [k] and np.isfinite(sal).all() and sal.any()


def test_streams_with_sgn_preprocess_and_other_misuse_raise():
    _ops()
    joint, bone = _models()
    with pytest.raises(ValueError, match='sgn_preprocess'):
        _recogniser(streams=[('joint', joint), ('bone', bone)], sgn_preprocess=True)
    with pytest.raises(ValueError, match='alpha'):
        _recogniser(streams=[('joint', joint), ('bone', bone)], alpha=[1.0])
    with pytest.raises(ValueError, match='streams'):
        _recogniser(streams=[('joint', joint), ('limb', bone)])
    with pytest.raises(ValueError, match='streams'):
        _recogniser(streams=[('bone', joint), ('bone', bone)])
    with pytest.raises(ValueError, match='model'):
        _recogniser(model=joint, streams=[('bone', bone)])
    with pytest.raises(ValueError, match='alpha'):
        _recogniser(model=joint, alpha=[1.0])
    with pytest.raises(ValueError, match='model'):
        _recogniser()


def test_shared_base_serves_the_other_recognisers():
    """RecordingRecognition and MultiStreamRecognition get the streams through the base class: the same fused logits as
    ActionRecognition for the same frames."""
    _ops()
    from agcn_amd.online import MultiStreamRecognition, RecordingRecognition
    joint, bone = _models()
    frames = _frames(WINDOW + 3)
    streams = [('joint', joint), ('bone', bone)]
    ar = _recogniser(streams=streams, alpha=ALPHA)
    for f in frames:
        ar.append_data(f)
    ar.predict()
    rec = _recogniser(RecordingRecognition, streams=streams, alpha=ALPHA)
    rec.label(frames, ends=[len(frames) - 1])
    scale = max(1.0, float(ar.logits.abs().max()))
    assert float((rec.logits - ar.logits).abs().max()) <= TOL * scale
    many = _recogniser(lambda **kw: MultiStreamRecognition(None, 2, **kw), streams=streams, alpha=ALPHA)
    for f in frames:
        many.append_data(np.stack((f, f)))
    many.predict()
    assert many.logits.shape[0] == 2 and float((many.logits - ar.logits).abs().max()) <= TOL * scale
    dwin, _ = many._explain_device(1)
    assert tuple(dwin.shape) == (2, 3, WINDOW, 25, 2)


def test_recogniser_without_streams_is_unchanged():
    """No ``streams``: one window through the recogniser gives the bits of the unchanged code path, the model called on
    the normalised window in eval mode under no_grad."""
    _ops()
    joint, _ = _models()
    ar = _recogniser(model=joint)
    for f in _frames(WINDOW):
        ar.append_data(f)
    scores, label = ar.predict()
    assert ar.models is None and ar.stream_logits is None and ar.stream_names is None
    with torch.no_grad():
        out = ar.model(ar.window)
        out = out[0] if isinstance(out, tuple) else out
        want = torch.softmax(out, 1)
    assert torch.equal(ar.logits, out)
    assert np.array_equal(np.asarray(scores, dtype=np.float32), want[0].cpu().numpy()) and label == int(want.argmax())
    # and its explanation is the plain input gradient
    dwin, _ = ar._explain_device(2)
    onehot = torch.nn.functional.one_hot(torch.tensor([2], device=_dev()), out.shape[1]).float()
    assert torch.equal(dwin, ar._input_gradient(ar.model, ar.window, onehot))
