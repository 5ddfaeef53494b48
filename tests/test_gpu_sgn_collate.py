"""GPU checks of the SGN collate (csrc/sgn.hip::sgn_collate_kernel) against the reference-generated fixture
(tests/golden/make_golden_sgn_collate.py) and its specification ``ops.sgn_collate_ref``, and of the SGN route through the
processor (``sgn_processor.SGNProcessor``) end to end on synthetic clips."""
import os
import pickle

import numpy as np
import pytest
import torch

from tests import test_sgn_collate_cpu as cc

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


def _ops():
    import agcn_amd  # noqa: F401
    from agcn_amd import ops
    return ops


def _draws(shape, seed):
    g = np.random.default_rng(seed)
    return torch.from_numpy(g.integers(0, 1 << 32, size=shape, dtype=np.uint64).astype(np.uint32).view(np.int32))


def _both(pool, r, seg, index=None, angles=None):
    """(kernel results, emulation results), each (x, L, s) as numpy."""
    ops = _ops()
    before = dict(ops.SGN_COLLATE_STATS)
    got = ops.sgn_collate(pool.to(DEV), r.to(DEV), seg, index=None if index is None else index.to(DEV),
                          angles=None if angles is None else angles.to(DEV), want_subject=True)
    assert ops.SGN_COLLATE_STATS['collate_hip'] == before['collate_hip'] + 1
    ref = ops.sgn_collate_ref(pool, r, seg, index=index, angles=angles, want_subject=True)
    assert all(t.device.type == 'cuda' for t in got)
    return [t.cpu().numpy() for t in got], [t.numpy() for t in ref]


def _same(got, ref, rotated):
    assert np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2])
    if not rotated:
        assert np.array_equal(got[0], ref[0])
        return 0.0
    err = cc.rel_err(got[0], ref[0])
    assert err < cc.BOUND
    assert not got[0][np.abs(ref[0]).max(-1) == 0].any()            # padding rows stay exactly zero
    return err


@pytest.mark.parametrize('mode', cc.MODES)
@pytest.mark.parametrize('group', cc.GROUPS)
def test_kernel_matches_reference(group, mode):
    ops = _ops()
    err = cc.check_collate(cc.fixture(), group, mode, ops.sgn_collate, device=DEV)
    print(f'{group} {mode}: kernel vs reference: rotated x {err:.2e}')


@pytest.mark.parametrize('group', cc.GROUPS)
def test_kernel_matches_emulation_and_sampler(group):
    ops = _ops()
    f = cc.fixture()
    pool, seg = torch.from_numpy(f[group + '.data']), int(f[group + '.seg'])
    r = torch.from_numpy(f[f'{group}.test.r'].astype(np.int64)).to(torch.int32)
    got, ref = _both(pool, r, seg)                                  # index=None, angles=None
    _same(got, ref, False)
    out, L = ops.sgn_sample(pool.to(DEV), r.to(DEV), seg)
    assert np.array_equal(got[0], out.cpu().numpy()) and np.array_equal(got[1], L.cpu().numpy())
    # without the subject flags the same values
    x, L2, s = ops.sgn_collate(pool.to(DEV), r.to(DEV), seg)
    assert s is None and torch.equal(x, out) and torch.equal(L2, L)


def _pool7():
    f = cc.fixture()
    g = np.random.default_rng(77)
    extra = g.standard_normal((2, 3, 64, 15, 2)).astype(np.float32)
    extra[0] = 0                                                    # sample 5: all null
    return torch.from_numpy(np.concatenate([f['v15.data'], extra]))


def test_index_gather_with_repeats():
    pool = _pool7()
    index = torch.tensor([6, 2, 2, 0, 5, 3, 3, 1, 4], dtype=torch.int64)
    r = _draws((9, 2, 12), 1)
    r[2] = r[1]                                                     # the same sample with the same draws: the same clip
    got, ref = _both(pool, r, 12, index=index)
    _same(got, ref, False)
    assert got[1].tolist() == [128, 106, 106, 128, 0, 12, 12, 64, 18]
    assert np.array_equal(got[0][1], got[0][2]) and not np.array_equal(got[0][0], got[0][3])
    angles = _ops().sgn_rotation_angles(9, 0.5, 'cpu')
    got, ref = _both(pool, r, 12, index=index, angles=angles)
    print(f'gather with rotation, kernel vs emulation: {_same(got, ref, True):.2e}')


def test_bad_index_and_empty_sample():
    pool = _pool7()
    index = torch.tensor([-1, 7, 5, 3, -(1 << 40), 1 << 40], dtype=torch.int64)
    angles = torch.full((6, 3), 0.3)
    for a in (None, angles):
        got, ref = _both(pool, _draws((6, 3, 12), 2), 12, index=index, angles=a)
        _same(got, ref, a is not None)
        assert got[1].tolist() == [0, 0, 0, 12, 0, 0]
        for n in (0, 1, 2, 4, 5):
            assert not got[0][n].any() and not got[2][n].any()
        assert got[0][3].any()


def test_domain_edge():
    """T = 2048 (every thread compacts a full chunk of rows), V = 2."""
    g = np.random.default_rng(5)
    pool = g.standard_normal((3, 3, 2048, 2, 2)).astype(np.float32)
    pool[0, :, 100:1900, :, 1] = 0
    pool[1, :, 2047] = 0
    pool[2, :, 3:] = 0                                               # 6 kept rows: padding
    pool = torch.from_numpy(pool)
    r = _draws((3, 2, 20), 3)
    got, ref = _both(pool, r, 20)
    _same(got, ref, False)
    assert got[1].tolist() == [4096 - 1800, 4094, 20]
    got, ref = _both(pool, r, 20, index=torch.tensor([2, 1, 0]), angles=torch.tensor([[0.5, -0.5, 0.25]] * 3))
    _same(got, ref, True)


def test_draws_of_a_sample_share_its_rotation():
    ops = _ops()
    f = cc.fixture()
    pool, seg = torch.from_numpy(f['v25.data']), 20
    r = torch.from_numpy(f['v25.test.r'].astype(np.int64)).to(torch.int32)
    angles = ops.sgn_rotation_angles(5, 0.5, 'cpu')
    got, ref = _both(pool, r, seg, angles=angles)
    _same(got, ref, True)
    plain, _ = _both(pool, r, seg)
    R = ops.sgn_rotation_ref(angles).astype(np.float64)                                       # (5, 3, 3)
    p = plain[0].astype(np.float64).reshape(5, 5, seg, 25, 3)
    want = np.einsum('nij,nskvj->nskvi', R, p).reshape(5, 5, seg, 75)
    err = cc.rel_err(got[0], want)
    print(f'S = 5, one rotation per sample, kernel vs fp64: {err:.2e}')
    assert err < cc.BOUND
    assert not np.array_equal(got[0][0, 0], got[0][0, 1])                                     # the draws differ


def test_sgn_processor_end_to_end(tmp_path):
    """2 epochs of Adam with the label-smoothing loss on synthetic clips, checkpoint, eval at multi_test = 3 on the fused
    forward, score pickle, reload."""
    import agcn_amd  # noqa: F401
    from agcn_amd import ops
    from agcn_amd.processor import Processor, load_args
    from agcn_amd.sgn_processor import SGNProcessor
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = os.path.join(root, 'config', 'nturgbd-cross-view', 'train_sgn.yaml')
    argv = ['--config', cfg, '--work-dir', str(tmp_path), '--batch-size', '4', '--test-batch-size', '4', '--num-epoch', '2',
            '--log-interval', '1', '--print-log', 'False', '--save-score', 'True']
    arg = load_args(argv)
    assert arg.use_sgn_dataloader and arg.optimizer == 'Adam' and arg.label_smoothing == 0.1 and arg.base_lr == 1e-3
    assert arg.step == [60, 90, 110] and arg.num_epoch == 2 and arg.weight_decay == 1e-4

    def shrink(a):
        a.train_feeder_args = dict(num_samples=8, num_point=25, window_size=32)
        a.test_feeder_args = dict(num_samples=6, num_point=25, window_size=32, seed=1)
        a.train_dataloader_args = dict(dataset='NTU60-CV', seg=20, multi_test=1, aug=1)
        a.test_dataloader_args = dict(dataset='NTU60-CV', seg=20, multi_test=3)
        return a
    p = SGNProcessor(shrink(arg))
    assert isinstance(p.optimizer, torch.optim.Adam)
    init = {k: v.detach().clone() for k, v in p.model.named_parameters()}
    p.start()
    assert os.listdir(tmp_path / 'weight') == ['SGN-2-4.pt'] and p.global_step == 4
    assert set(p.last_timer) == {'dataloader', 'model', 'statistics'} and p.last_timer['model'] > 0
    moved = 0
    for k, v in p.model.named_parameters():
        assert torch.isfinite(v).all(), k
        moved += int(not torch.equal(v, init[k]))
    assert moved > len(init) // 2
    tracked = {k: int(v) for k, v in p.model.state_dict().items() if k.endswith('num_batches_tracked')}
    assert tracked and set(tracked.values()) == {4}, tracked

    # the eval scores: the mean over the recorded draws of the fused forward
    score = p.last_score
    assert score.shape == (6, 60) and len(p.eval_draws) == 2 and p.eval_draws[0].shape == (4, 3, 20)
    before = dict(ops.SGN_STATS)
    loss, acc = p.eval(1)
    assert ops.SGN_STATS['forward_tensor'] == before['forward_tensor']
    assert ops.SGN_STATS['frames_hip'] == before['frames_hip'] + 2 and np.isfinite(loss) and 0.0 <= acc[1] <= 1.0
    assert np.array_equal(p.last_score, score)                       # seeded per epoch
    pool = torch.from_numpy(p.datasets['test'].data).to(DEV)
    want = []
    p.model.eval()
    with torch.no_grad():
        for k, r in enumerate(p.eval_draws):
            index = torch.arange(4 * k, min(4 * k + 4, 6), device=DEV)
            x, _, _ = ops.sgn_collate(pool, r, 20, index=index)
            logits, _ = p.model(x.view(-1, 20, 75))
            want.append(logits.view(-1, 3, 60).mean(1))
    assert np.abs(torch.cat(want).cpu().numpy() - score).max() < 1e-5
    with open(tmp_path / 'score' / 'epoch2_test.pkl', 'rb') as f:
        sc = pickle.load(f)
    assert len(sc) == 6 and np.array_equal(np.stack([sc[i] for i in range(6)]), score)

    # --phase test --weights reloads the same state
    arg2 = shrink(load_args(argv + ['--phase', 'test', '--weights', str(tmp_path / 'weight' / 'SGN-2-4.pt')]))
    p2 = SGNProcessor(arg2)
    assert p2.global_step == 4
    for k, v in p.model.state_dict().items():
        assert torch.equal(v.cpu(), p2.model.state_dict()[k].cpu()), k
    p2.eval(1)
    assert np.abs(p2.last_score - score).max() < 1e-5
    # the plain Processor still refuses Adam; the SGN route refuses other models and more than one process
    with pytest.raises(ValueError):
        Processor(load_args(argv + ['--use-sgn-dataloader', 'False']))
    with pytest.raises(ValueError):
        SGNProcessor(shrink(load_args(argv + ['--model', 'model.agcn.Model'])))
    with pytest.raises(ValueError):
        SGNProcessor(shrink(load_args(argv + ['--world-size', '2'])))
