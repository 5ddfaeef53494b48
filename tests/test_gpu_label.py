"""GPU tests of batched window normalisation: ``ops.prenorm_windows`` / ``ops.skel_smooth`` / ``ops.skel_append_many``
(csrc/prenorm.hip) and ``online.RecordingRecognition`` / ``online.MultiStreamRecognition``, against the reference's
fixtures (tests/golden/make_online_golden.py) and against the frame-by-frame path (``online.ActionRecognition``).

Bounds.  Normalised windows: the rule of tests/test_gpu_online.py, max|out - ref| <= 5e-6 * max(1, max|ref|), and what
the reference leaves null exactly zero.  Against the frame-by-frame path the windows, selections and energies are
compared bit for bit: the batched kernel is a second instantiation of the same code with the same order of sums.
Logits: the project's forward rule, 1e-4 * max(1, max|ref|).  They cannot be bit-equal to the batch-1 path: the f16x3
range scale of the folded forward is taken over the whole batch tensor, so a window's logits depend, within that rule,
on which other windows share its batch."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
PRENORM_TOL = 5e-6
FORWARD_TOL = 1e-4
GROUPS = ['base_v15', 'base_v25', 'base_v18', 'firstframe_v25', 'nopad_v18', 'noz_v15', 'zaxis2_v25', 'long_v25']
V15_AXES = dict(zaxis=(8, 1), xaxis=(2, 5))


def _dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _i32(values):
    return torch.tensor(np.asarray(values, dtype=np.int32), device=_dev())


def _check_normalised(out, ref, what):
    scale = max(1.0, float(np.abs(ref).max()))
    err = float(np.abs(out - ref).max())
    print(f'{what}: max|out - ref| = {err:.3e} (bound {PRENORM_TOL * scale:.3e})')
    assert err <= PRENORM_TOL * scale, (what, err)
    assert not out[ref == 0].any(), f'{what}: a null frame or joint of the reference is not exactly zero'


def _recogniser(model=None, window=24, moving_avg=1, cls=None, **kw):
    import agcn_amd  # noqa: F401
    from agcn_amd import online
    cls = cls or online.ActionRecognition
    return cls(model if model is not None else torch.nn.Identity(), max_frame=window, max_num_skeleton=4,
               max_num_skeleton_true=2, num_joint=15, moving_avg=moving_avg, **V15_AXES, **kw)


@pytest.fixture(scope='module')
def stream():
    return np.load(os.path.join(GOLDEN, 'online_stream_v15.npz'))


@pytest.fixture(scope='module')
def batched(stream):
    """moving_avg -> (smoothed recording (4, 29, 15, 3), windows (29, 3, 24, 15, 2), selections, energies) of the
    stream fixture, every window ending at 0..28 in ONE launch; computed once per moving average and left unchanged."""
    import agcn_amd  # noqa: F401
    from agcn_amd import ops
    from agcn_amd.online import window_plan
    raw = torch.from_numpy(np.ascontiguousarray(stream['frames'][:, :, 0])).to(_dev())
    start, length = window_plan(29, 24, range(29))
    cache = {}

    def get(k):
        if k not in cache:
            sm = ops.skel_smooth(raw, k)
            cache[k] = (sm,) + ops.prenorm_windows(sm[None], _i32(start), _i32(length), frames=24, num_select=2,
                                                   **V15_AXES)
        return cache[k]
    return get


# ---- 1. against the reference, the whole recording in one launch ---------------------------------------------------------
@pytest.mark.parametrize('moving_avg', [1, 3])
def test_recording_matches_reference_in_one_launch(stream, batched, moving_avg):
    """Fill phase, leading nulls, the interior gap of body 3 and the null rule: window i holds i + 1 frames and the
    frames behind it in the buffer are the recording's future."""
    wins, sels = stream[f'win_ma{moving_avg}'], stream[f'sel_ma{moving_avg}']
    sm, out, sel, energy = batched(moving_avg)
    assert sm.shape == (4, 29, 15, 3) and out.shape == (29, 3, 24, 15, 2) and energy.shape == (29, 4)
    assert sel.cpu().numpy().tolist() == sels.tolist()
    out = out.cpu().numpy()
    for i in range(29):
        _check_normalised(out[i], wins[i, 0], f'moving_avg={moving_avg} window {i}')


def test_a_window_does_not_see_the_frames_behind_it(stream, batched):
    """Window 5 (frames 0..5) of the full recording against the same window of a recording whose frames 6..28 are
    zero: bit-identical."""
    from agcn_amd import ops
    sm, out, sel, energy = batched(1)
    cut = sm.clone()
    cut[:, 6:] = 0
    o, s, e = ops.prenorm_windows(cut[None], _i32([0]), _i32([6]), frames=24, num_select=2, **V15_AXES)
    assert sm[:, 6:].any()
    assert torch.equal(o[0], out[5]) and torch.equal(s[0], sel[5]) and torch.equal(e[0], energy[5])


# ---- 2. bit-equality with the frame-by-frame path ------------------------------------------------------------------------
@pytest.mark.parametrize('moving_avg', [1, 3, 5])
def test_bit_equal_to_frame_by_frame(stream, batched, moving_avg):
    sm, out, sel, energy = batched(moving_avg)
    ar = _recogniser(moving_avg=moving_avg)
    for i, f in enumerate(stream['frames']):
        ar.append_data(f)
        win = ar.normalize()
        assert torch.equal(win[0], out[i]), i
        assert torch.equal(ar.selected[0], sel[i]) and torch.equal(ar.energy[0], energy[i]), i
    for f in range(29 - 24, 29):                         # the ring holds frame f in slot f mod 24
        assert torch.equal(ar.ring[:, f % 24], sm[:, f]), f


@pytest.mark.parametrize('k', [33, 34, 40])
def test_smoothing_beyond_the_on_chip_history(k):
    """k = 33 is the longest average whose history stays on chip, 34 the first that reads its own stores back: a ring of
    48 slots after 60 appends against the smoothed recording, bit for bit."""
    from agcn_amd import ops
    frames = np.random.default_rng(k).standard_normal((60, 4, 1, 15, 3)).astype(np.float32)
    ar = _recogniser(window=48, moving_avg=k)
    for f in frames:
        ar.append_data(f)
    sm = ops.skel_smooth(torch.from_numpy(frames[:, :, 0].copy()).to(_dev()), k)
    for f in range(60 - 48, 60):
        assert torch.equal(ar.ring[:, f % 48], sm[:, f]), f


# ---- 3. every option path ------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def cases():
    both = dict(np.load(os.path.join(GOLDEN, 'prenorm_cases.npz')))
    long_ = np.load(os.path.join(GOLDEN, 'prenorm_long.npz'))
    both.update({k: long_[k] for k in long_.files if k != 'groups'})
    return both


@pytest.mark.parametrize('group', GROUPS)
def test_every_option_path(cases, group):
    """start = 0, len = T on the fixtures' plain tensors (block n = sample n): bit-identical to ``ops.prenorm`` and
    within the window bound of the reference.  long_v25 has three 64-frame chunks and 3750 (t, v) pairs."""
    import agcn_amd  # noqa: F401
    from agcn_amd import ops
    raw, ref = cases[group + '.raw'], cases[group + '.ref']              # (N, M, T, V, 3), (N, 3, T, V, M)
    opts = json.loads(str(cases[group + '.opts']))
    n, _, t = raw.shape[:3]
    x = torch.from_numpy(raw).to(_dev())
    want, wsel, _ = ops.prenorm(x, **opts)
    got, gsel, energy = ops.prenorm_windows(x, _i32([0] * n), _i32([t] * n), block=_i32(range(n)), **opts)
    assert energy is None and torch.equal(got, want) and torch.equal(gsel, wsel)
    got = got.cpu().numpy()
    for i, kind in enumerate(cases[group + '.kinds'].tolist()):
        _check_normalised(got[i], ref[i], f'{group}[{kind}]')


# ---- 4. plan handling ----------------------------------------------------------------------------------------------------
def _windows(pool, start, length, block=None):
    from agcn_amd import ops
    return ops.prenorm_windows(pool, _i32(start), _i32(length), block=None if block is None else _i32(block), frames=24,
                               num_select=2, **V15_AXES)


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize('ends', [[7, 28, 0, 7, 15, 7], [12], (np.arange(300) * 7 % 29).tolist()],
                         ids=['unsorted_repeated', 'one', 'n300'])
def test_plans_in_any_order_and_number(batched, ends):
    """Unsorted and repeated windows, a single one, and 300 of them (more workgroups than the chip has CUs)."""
    from agcn_amd.online import window_plan
    sm, out, sel, energy = batched(1)
    got = _windows(sm[None], *window_plan(29, 24, ends))
    idx = torch.tensor(ends, device=_dev())
    assert _same(got, (out[idx], sel[idx], energy[idx]))


def test_two_block_pool(batched):
    sm, out, sel, energy = batched(1)
    other = (sm.flip(1) * 1.5).contiguous()                          # the recording played backwards, scaled
    start, length, block = [0, 3, 5, 0, 5], [10, 24, 24, 29, 24], [1, 0, 1, 1, 0]
    got = _windows(torch.stack((sm, other)), start, length, block)
    for i, b in enumerate(block):
        want = _windows((other if b else sm)[None], start[i:i + 1], length[i:i + 1])
        assert _same([g[i:i + 1] for g in got], want), i
    assert torch.equal(got[0][4], out[28])                            # start 5, 24 frames of block 0 = the window ending at 28
    assert not torch.equal(got[0][2], got[0][4])


def test_out_of_range_plans_are_clamped(batched):
    """block into [0, nblocks), start into [0, Tmax), len into [0, T]: the result is the clamped plan's, and finite.
    (start 28 with 24 frames also wraps round the end of the block.)"""
    sm = batched(1)[0]
    pool = torch.stack((sm, (sm * 0.5).contiguous()))
    wild = _windows(pool, [-7, 1000, 3, 2 ** 31 - 1], [-2, 99, 24, -2 ** 31], [-3, 5, 2 ** 31 - 1, -2 ** 31])
    tame = _windows(pool, [0, 28, 3, 28], [0, 24, 24, 0], [0, 1, 1, 0])
    assert _same(wild, tame)
    assert torch.isfinite(wild[0]).all() and torch.isfinite(wild[2]).all()
    assert not wild[0][0].any() and wild[0][1].any()                  # no frames: an all-null window


# ---- 5. the deployment shape ---------------------------------------------------------------------------------------------
def test_deployment_shape_equals_plain_slices():
    """Window 300, 25 joints, a recording of 337 frames (the recipe of test_full_size_ring_equals_a_plain_window):
    windows ending while the window fills, as it fills and after, against ``ops.prenorm`` on the zero-padded slices."""
    import agcn_amd  # noqa: F401
    from agcn_amd import ops
    from agcn_amd.online import window_plan
    rng = np.random.default_rng(5)
    frames = np.zeros((337, 4, 25, 3), dtype=np.float32)
    frames[:, 2] = rng.standard_normal((337, 25, 3)) * 0.2 + (0.3, 2.5, 0.9)
    frames[40:, 0] = rng.standard_normal((297, 25, 3)) * 0.4 + (1.0, 2.2, 0.8)
    frames[100:130, 0] = 0
    ends = [0, 150, 299, 300, 336]
    start, length = window_plan(337, 300, ends)
    assert start.tolist() == [0, 0, 0, 1, 37] and length.tolist() == [1, 151, 300, 300, 300]
    sm = ops.skel_smooth(torch.from_numpy(frames).to(_dev()), 1)
    got = ops.prenorm_windows(sm[None], _i32(start), _i32(length), frames=300, num_select=2)
    plain = np.zeros((5, 4, 300, 25, 3), dtype=np.float32)
    for i, (s, n) in enumerate(zip(start, length)):
        plain[i, :, :n] = frames[s:s + n].transpose(1, 0, 2, 3)
    want = ops.prenorm(torch.from_numpy(plain).to(_dev()), num_select=2)
    assert _same(got, want)
    assert torch.isfinite(got[0]).all() and got[1][4].tolist() == [0, 2]


# ---- 6..8. the model -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def model_fx():
    import agcn_amd  # noqa: F401
    from agcn_amd.model.aagcn import Model
    from oracle import agcn_oracle as orc
    fx = np.load(os.path.join(GOLDEN, 'online_model_v15.npz'))
    v, window, tracked, chosen, classes, seed = (int(x) for x in fx['meta'])
    assert (v, window, tracked, chosen) == (15, 36, 4, 2) and fx['frames'].shape[0] == 44
    model = Model(num_class=classes, num_point=v, num_person=chosen, graph='graph.openpose_b25_j15.Graph',
                  graph_args=dict(labeling_mode='spatial'), model_layers=10)
    model.load_state_dict(orc.aagcn_randomized_state(orc.aagcn_model_param_shapes(classes, v), seed,
                                                     stress=float(fx['stress'])))
    return fx, model.to(_dev()).eval()


def test_model_against_reference(model_fx):
    """``label`` at the recorded appends (while the window fills, as it fills, after it has wrapped): logits within the
    forward rule of the reference's, scores within 1e-5, labels equal, and the fold ran."""
    from agcn_amd import lib, ops, online
    fx, model = model_fx
    rr = _recogniser(model, window=36, cls=online.RecordingRecognition, batch=64)
    before = dict(ops.INFER_STATS)
    scores, labels, ends = rr.label(fx['frames'], ends=fx['record'])
    stats = {k: ops.INFER_STATS[k] - before[k] for k in before}
    assert ends.tolist() == fx['record'].tolist() == [19, 35, 43] and scores.shape == fx['scores'].shape
    logits = rr.logits.cpu().numpy()
    for i, end in enumerate(ends):
        ref_l, ref_s = fx['logits'][i], fx['scores'][i]
        scale = max(1.0, float(np.abs(ref_l).max()))
        err_l, err_s = float(np.abs(logits[i] - ref_l).max()), float(np.abs(scores[i] - ref_s).max())
        print(f'window ending at {end}: logits err {err_l:.3e} (bound {FORWARD_TOL * scale:.3e}), scores err {err_s:.3e}')
        assert err_l <= FORWARD_TOL * scale, (end, err_l, scale)
        assert err_s <= 1e-5, (end, err_s)
        assert labels[i] == int(ref_l.argmax()) == int(ref_s.argmax())
    # one batched forward: every unit but the 3-channel first one folded (none under AGCN_GEMM=f32)
    nf = 9 if lib.load().agcn_gemm_mode() != b'f32' else 0
    assert stats['aagcn_unit_fused'] == nf and stats['tconv_infer'] >= nf, stats
    assert stats['stc_apply'] == 10 - nf, stats


def test_whole_recording_in_ragged_batches(model_fx):
    """All 44 windows in batches of 16, 16 and 12 against ``ActionRecognition.predict()`` after every append: logits
    within the forward rule for every window; labels where the frame-by-frame logits' top-two gap exceeds twice the
    bound, which must be the case for at least 90 % of the windows; a second call returns the same bits."""
    from agcn_amd import online
    fx, model = model_fx
    frames = fx['frames']
    ar = _recogniser(model, window=36)
    ref_logits, ref_labels = [], []
    for f in frames:
        ar.append_data(f)
        _, label = ar.predict()
        ref_logits.append(ar.logits[0].cpu().numpy())
        ref_labels.append(label)
    rr = _recogniser(model, window=36, cls=online.RecordingRecognition, batch=16)
    scores, labels, ends = rr.label(frames)
    logits = rr.logits.cpu().numpy()
    assert ends.tolist() == list(range(44)) and logits.shape == (44, 60) and scores.shape == (44, 60)
    comparable = 0
    for i in range(44):
        bound = FORWARD_TOL * max(1.0, float(np.abs(ref_logits[i]).max()))
        err = float(np.abs(logits[i] - ref_logits[i]).max())
        top = np.sort(ref_logits[i])[-2:]
        print(f'window {i}: logits err {err:.3e} (bound {bound:.3e}), top-two gap {top[1] - top[0]:.3e}')
        assert err <= bound, (i, err, bound)
        if top[1] - top[0] > 2 * bound:
            comparable += 1
            assert labels[i] == ref_labels[i], i
    print(f'{comparable} of 44 windows have a comparable label')
    assert comparable >= 0.9 * 44, comparable
    again = rr.label(torch.from_numpy(frames[:, :, 0].copy()))        # (L, M, V, 3) tensors are taken as well
    assert np.array_equal(again[0], scores) and np.array_equal(again[1], labels)
    assert torch.equal(rr.logits, torch.from_numpy(logits).to(_dev()))


@pytest.mark.parametrize('moving_avg', [1, 3])
def test_many_streams(model_fx, moving_avg):
    """Three streams on the model fixture's frames, one as it is, one starting 5 ticks late, one missing ticks 7 and 8,
    against three independent ``ActionRecognition`` at every tick: windows, selections and energies bit for bit; logits
    within the forward rule while filling, when stream 0 is just full and after all three have wrapped."""
    from agcn_amd import online
    fx, model = model_fx
    frames = fx['frames']
    ms = online.MultiStreamRecognition(model, 3, max_frame=36, max_num_skeleton=4, max_num_skeleton_true=2, num_joint=15,
                                       moving_avg=moving_avg, **V15_AXES)
    singles = [_recogniser(model, window=36, moving_avg=moving_avg) for _ in range(3)]
    assert ms.predict()[0].shape[0] == 0 and ms.streams == []          # nothing appended yet
    for tick in range(44):
        present = np.array([True, tick >= 5, tick not in (7, 8)])
        tick_frames = np.stack((frames[tick], frames[max(tick - 5, 0)], frames[tick]))
        ms.append_data(tick_frames, present)
        for s in range(3):
            if present[s]:
                singles[s].append_data(tick_frames[s])
        win = ms.normalize()
        assert ms.streams == ([0, 2] if tick < 5 else [0, 1, 2]), tick  # a stream without frames is left out
        for row, s in enumerate(ms.streams):
            want = singles[s].normalize()
            assert torch.equal(win[row], want[0]), (tick, s)
            assert torch.equal(ms.selected[row], singles[s].selected[0]), (tick, s)
            assert torch.equal(ms.energy[row], singles[s].energy[0]), (tick, s)
        if tick in (2, 10, 35, 43):
            scores, labels, streams = ms.predict()
            assert streams.tolist() == ms.streams and scores.shape == (len(streams), 60)
            got = ms.logits.cpu().numpy()
            for row, s in enumerate(streams):
                singles[s].predict()
                ref = singles[s].logits[0].cpu().numpy()
                bound = FORWARD_TOL * max(1.0, float(np.abs(ref).max()))
                err = float(np.abs(got[row] - ref).max())
                print(f'tick {tick} stream {s}: logits err {err:.3e} (bound {bound:.3e})')
                assert err <= bound, (tick, s, err, bound)
    assert ms.counter.tolist() == [36, 36, 36] and ms.head.tolist() == [8, 3, 6]
    only, _, which = ms.predict(streams=[2])
    assert which.tolist() == [2] and only.shape == (1, 60)
    for s in range(3):
        assert torch.equal(ms.rings[s], singles[s].ring), s
