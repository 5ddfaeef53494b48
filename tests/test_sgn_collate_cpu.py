"""CPU checks of the SGN training / evaluation input side: ``ops.sgn_collate_ref`` (the specification of
``agcn_sgn_collate``) against the reference's three collates (tests/golden/make_golden_sgn_collate.py), the host check of
the collate part of csrc/sgn_plan.h with its rotation against the reference's matrices, the label-smoothing loss against
the reference's, ``SGNBatches`` on CPU tensors, the SGN pickle branch of ``Feeder`` and the C-ABI argument errors of
``agcn_sgn_collate`` (returned before any HIP call)."""
import os
import pickle
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import sgn_util as su

ROOT = su.ROOT
GROUPS = ('v25', 'v15')
MODES = ('train_cv', 'train_cs', 'val', 'test')
THETA = dict(train_cv=0.5, train_cs=0.3)
# the project's fp32 bound, relative to max(1, max|ref|)
BOUND = 1e-4


def fixture():
    return su._npz('sgn_collate.npz')


def collate_case(f, group, mode, fn, device='cpu'):
    """The reference's batch ``group.mode`` through ``fn`` (ops.sgn_collate or ops.sgn_collate_ref) after applying the
    reference's batch permutation idx -> (x (B*S, seg, 3V), L (B,) of the samples in dataset order, s, the fixture's
    prefix)."""
    p = f'{group}.{mode}.'
    seg, S = int(f[group + '.seg']), int(f[p + 'S'])
    pool = torch.from_numpy(f[group + '.data']).to(device)
    B = pool.shape[0]
    idx = f[p + 'idx']
    r = torch.from_numpy(f[p + 'r'].astype(np.int64)).to(torch.int32)
    angles = None
    if mode in THETA:                                   # S = 1: the permutation acts on the samples
        index = torch.from_numpy(idx.copy())
        r = r[index]
        angles = torch.from_numpy(f[p + 'angles']).to(device)
    else:
        assert np.array_equal(idx, np.arange(B * S))
        index = torch.arange(B)
    x, L, s = fn(pool, r.contiguous().to(device), seg, index=index.to(device), angles=angles, want_subject=True)
    Ls = np.zeros(B, dtype=np.int32)
    Ls[index.numpy()] = L.cpu().numpy()
    return x.reshape(B * S, seg, -1).cpu().numpy(), Ls, s.reshape(B * S, seg, 1).cpu().numpy(), p


def rel_err(got, ref):
    ref = np.asarray(ref, dtype=np.float64)
    return float(np.abs(np.asarray(got, dtype=np.float64) - ref).max() / max(1.0, float(np.abs(ref).max())))


def check_collate(f, group, mode, fn, device='cpu'):
    """-> the rotated case's error.  Unrotated x, s and L exactly; rotated x within BOUND."""
    x, L, s, p = collate_case(f, group, mode, fn, device)
    assert np.array_equal(L, f[p + 'valid_frames'])
    assert np.array_equal(s, f[p + 's'])
    if mode not in THETA:
        assert np.array_equal(x, f[p + 'x'])
        return 0.0
    assert float(np.abs(f[p + 'angles']).max()) <= THETA[mode]
    err = rel_err(x, f[p + 'x'])
    print(f'{group} {mode}: rotated x vs reference: {err:.2e}')
    assert err < BOUND
    # padding rows stay exactly zero under the rotation
    pad = np.abs(f[p + 'x_unrotated']).max(-1) == 0
    assert pad.any() and not x[pad].any() and not s[pad].any()
    return err


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('group', GROUPS)
def test_collate_ref_matches_reference(group, mode):
    import agcn_amd  # noqa: F401
    from agcn_amd import ops
    check_collate(fixture(), group, mode, ops.sgn_collate_ref)


@pytest.mark.parametrize('group', GROUPS)
def test_collate_ref_unrotated_train_is_exact(group):
    """The training collate without its angles is the reference's sorted, unrotated batch, bit for bit."""
    import agcn_amd  # noqa: F401
    from agcn_amd import ops
    f = fixture()
    for mode in THETA:
        p = f'{group}.{mode}.'
        index = torch.from_numpy(f[p + 'idx'].copy())
        r = torch.from_numpy(f[p + 'r'].astype(np.int64)).to(torch.int32)[index].contiguous()
        x, _, _ = ops.sgn_collate_ref(torch.from_numpy(f[group + '.data']), r, int(f[group + '.seg']), index=index)
        assert np.array_equal(x[:, 0].numpy(), f[p + 'x_unrotated'])


def test_collate_ref_bad_index_and_checks():
    import agcn_amd  # noqa: F401
    from agcn_amd import ops
    f = fixture()
    pool = torch.from_numpy(f['v15.data'])
    r = torch.zeros((3, 2, 12), dtype=torch.int32)
    x, L, s = ops.sgn_collate_ref(pool, r, 12, index=torch.tensor([-1, 5, 1]), want_subject=True)
    assert not x[:2].any() and x[2].any() and L.tolist() == [0, 0, 64] and not s[:2].any()
    with pytest.raises(ValueError):
        ops.sgn_collate_ref(pool, torch.zeros((6, 1, 12), dtype=torch.int32), 12)          # no index: N <= P
    with pytest.raises(ValueError):
        ops.sgn_collate_ref(pool, r, 12, index=torch.tensor([0, 1, 2], dtype=torch.int32))
    with pytest.raises(ValueError):
        ops.sgn_collate_ref(pool, r, 12, angles=torch.zeros((3, 2)))
    with pytest.raises(ValueError):
        ops.sgn_collate_ref(pool[..., :1], r, 12)
    a = ops.sgn_rotation_angles(1000, 0.3, 'cpu')
    assert a.shape == (1000, 3) and a.dtype == torch.float32 and float(a.min()) >= -0.3 and float(a.max()) < 0.3
    assert float(a.std()) > 0.1


def test_collate_plan_checker_and_rotation(tmp_path):
    """The SGN_HD rotation the kernel builds, compiled for the host, against the matrices of the reference's _rot."""
    import agcn_amd  # noqa: F401
    from agcn_amd import ops
    cxx = next((c for c in (os.environ.get('CXX'), 'c++', 'g++', 'clang++') if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip('no host C++ compiler')
    f = fixture()
    keys = [f'{g}.{m}.' for g in GROUPS for m in THETA]
    angles = np.concatenate([f[k + 'angles'] for k in keys]).astype(np.float32)
    want = np.concatenate([f[k + 'rot'] for k in keys])
    exe, fin, fout = str(tmp_path / 'sgn_collate_plan_check'), str(tmp_path / 'angles.bin'), str(tmp_path / 'rot.bin')
    angles.tofile(fin)
    r = subprocess.run([cxx, '-std=c++17', '-Wall', '-Werror', '-O1', '-I', os.path.join(ROOT, '2s-agcn_amd', 'csrc'),
                        os.path.join(ROOT, 'tests', 'sgn_collate_plan_check.cpp'), '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-4000:]
    assert ' checks, 0 failures' in r.stdout and int(r.stdout.split(' checks')[0].split()[-1]) > 1000
    got = np.fromfile(fout, dtype=np.float32).reshape(-1, 3, 3)
    assert got.shape == want.shape
    # entries of at most 1 from at most two products of three cos / sin values, each within an ulp or two of fp32
    err = float(np.abs(got.astype(np.float64) - want).max())
    err_py = float(np.abs(ops.sgn_rotation_ref(angles).astype(np.float64) - want).max())
    print(f'rotation matrices vs reference _rot: host sgn_rotation {err:.2e}, ops.sgn_rotation_ref {err_py:.2e}')
    assert err < 1e-6 and err_py < 1e-6


def test_label_smoothing_loss_matches_reference():
    import agcn_amd  # noqa: F401
    from agcn_amd.sgn_processor import label_smoothing_loss
    f = fixture()
    for i in range(int(f['loss_cases'])):
        p = f'loss{i}.'
        logits = torch.from_numpy(f[p + 'logits']).requires_grad_(True)
        target, eps = torch.from_numpy(f[p + 'target']), float(f[p + 'eps'])
        val = label_smoothing_loss(logits, target, eps)
        val.backward()
        assert abs(float(val.detach()) - float(f[p + 'value'])) < 1e-5 * max(1.0, abs(float(f[p + 'value'])))
        assert rel_err(logits.grad.numpy(), f[p + 'grad']) < 1e-6
        if eps > 0 and logits.shape[1] > 2:      # it is not torch's label_smoothing, which spreads eps over all C classes
            other = torch.nn.functional.cross_entropy(logits.detach(), target, label_smoothing=eps)
            assert abs(float(other) - float(f[p + 'value'])) > 1e-4


class _Data:
    def __init__(self, n, t=9, v=3, seed=0):
        g = np.random.default_rng(seed)
        self.data = g.standard_normal((n, 3, t, v, 2)).astype(np.float32)
        self.label = g.integers(0, 60, size=(n,)).astype(np.int64)

    def __len__(self):
        return len(self.label)


def _epoch(b):
    out = []
    for x, label, index in b:
        out.append((x.clone(), label.clone(), index.clone(), b.last_draws.clone(),
                    None if b.last_angles is None else b.last_angles.clone(), b.last_L.clone()))
    return out


@pytest.mark.parametrize('resident', [True, False])
def test_sgn_batches_on_cpu(resident):
    import agcn_amd  # noqa: F401
    from agcn_amd import ops
    from agcn_amd.feeders.sgn import SGNBatches
    ds = _Data(11)
    kw = dict(device='cpu', resident=resident, seed=5)
    tr = SGNBatches(ds, 4, 6, multi_test=3, mode='train', dataset_name='NTU60-CV', **kw)
    assert tr.resident == resident and tr.S == 1 and tr.theta == 0.5 and len(tr) == 2
    e0 = _epoch(tr.set_epoch(0))
    assert len(e0) == 2                                               # drop_last in train
    seen = torch.cat([b[2] for b in e0]).tolist()
    assert len(set(seen)) == 8 and set(seen) <= set(range(11))
    for x, label, index, r, a, L in e0:
        assert x.shape == (4, 6, 9) and r.shape == (4, 1, 6) and a.shape == (4, 3) and float(a.abs().max()) <= 0.5
        assert np.array_equal(label.numpy(), ds.label[index.numpy()]) and L.tolist() == [18] * 4
        ref, _, _ = ops.sgn_collate_ref(torch.from_numpy(ds.data), r, 6, index=index, angles=a)
        assert torch.equal(x, ref.view(4, 6, 9))
    again = _epoch(SGNBatches(ds, 4, 6, mode='train', dataset_name='NTU60-CV', **kw).set_epoch(0))
    for a, b in zip(e0, again):                                       # the same seed: the same order, draws and angles
        assert all(torch.equal(p, q) for p, q in zip(a, b))
    e1 = _epoch(tr.set_epoch(1))
    assert not torch.equal(torch.cat([b[2] for b in e0]), torch.cat([b[2] for b in e1]))
    assert not torch.equal(e0[0][3], e1[0][3]) and not torch.equal(e0[0][4], e1[0][4])
    # an epoch of N = 12 in batches of 4 visits every index exactly once
    full = SGNBatches(_Data(12), 4, 6, mode='train', dataset_name='NTU120-XSet', aug=1, **kw)
    assert full.theta == 0.3 and sorted(torch.cat([b[2] for b in _epoch(full)]).tolist()) == list(range(12))

    for mode, S in (('val', 1), ('test', 3)):
        ev = SGNBatches(ds, 4, 6, multi_test=3, mode=mode, dataset_name='anything', **kw)
        assert ev.S == S and ev.theta is None and len(ev) == 3
        e = _epoch(ev)
        assert torch.cat([b[2] for b in e]).tolist() == list(range(11))          # in order, the partial batch kept
        assert [b[0].shape[0] for b in e] == [4 * S, 4 * S, 3 * S] and all(b[4] is None for b in e)
        assert all(b[3].shape == (len(b[2]), S, 6) for b in e)

    # injected draws and angles
    r0 = torch.arange(4 * 6, dtype=torch.int32).view(4, 1, 6)
    a0 = torch.full((4, 3), 0.25)
    inj = SGNBatches(ds, 4, 6, mode='train', dataset_name='NTU60-CS', draws=lambda k, B: r0[:B] + k,
                     angles=lambda k, B: a0[:B], **kw)
    e = _epoch(inj)
    assert torch.equal(e[1][3], r0 + 1) and torch.equal(e[1][4], a0)


def test_sgn_batches_theta_rule():
    import agcn_amd  # noqa: F401
    from agcn_amd.feeders.sgn import SGNBatches, rotation_theta
    assert rotation_theta('NTU60-CS') == 0.3 and rotation_theta('NTU60-CV') == 0.5 and rotation_theta('NTU120-CSet') == 0.3
    with pytest.raises(ValueError):
        rotation_theta('kinetics')
    ds = _Data(5)
    with pytest.raises(ValueError):
        SGNBatches(ds, 2, 6, mode='train', dataset_name='SYSU', aug=1, device='cpu')
    assert SGNBatches(ds, 2, 6, mode='train', dataset_name='SYSU', aug=0, device='cpu').theta is None
    with pytest.raises(ValueError):
        SGNBatches(ds, 2, 6, mode='bogus', device='cpu')


def test_feeder_sgn_pickle_branch(tmp_path):
    import agcn_amd  # noqa: F401
    from agcn_amd.feeders.feeder import Feeder
    g = np.random.default_rng(3)
    parts = {}
    for split, n in (('train', 5), ('val', 2), ('test', 3)):
        data = g.standard_normal((n, 8, 2 * 25 * 3)).astype(np.float32)
        label = g.integers(0, 60, size=(n,)).astype(np.int64)
        parts[split] = (data, label)
        with open(tmp_path / f'NTU_CV_{split}.pkl', 'wb') as f:
            pickle.dump(data, f)
        with open(tmp_path / f'NTU_CV_{split}_label.pkl', 'wb') as f:
            pickle.dump(label, f)

    def feeder(split, **kw):
        return Feeder(str(tmp_path / f'NTU_CV_{split}.pkl'), str(tmp_path / f'NTU_CV_{split}_label.pkl'),
                      dataset='NTU60-CV-SGN', **kw)
    tr = feeder('train')                                   # train joins its val sibling
    data = np.concatenate([parts['train'][0], parts['val'][0]])
    assert tr.data.shape == (7, 3, 8, 25, 2) and tr.data.dtype == np.float32 and len(tr) == 7
    assert np.array_equal(tr.label, np.concatenate([parts['train'][1], parts['val'][1]]))
    assert np.array_equal(tr.sample_name, np.arange(7))
    # (n, t, m, v, c) -> (n, c, t, v, m)
    assert np.array_equal(tr.data, data.reshape(7, 8, 2, 25, 3).transpose(0, 4, 1, 3, 2))
    clip, label, index = tr[6]
    assert np.array_equal(clip, tr.data[6]) and label == tr.label[6] and index == 6
    te = feeder('test')
    assert te.data.shape == (3, 3, 8, 25, 2) and np.array_equal(te.label, parts['test'][1])
    with pytest.raises(ValueError):
        feeder('test', joint_15=True)


def test_collate_cabi_argument_errors():
    import agcn_amd  # noqa: F401
    from agcn_amd import lib
    L = lib.load()
    one = 1                                                 # any non-null address: rejected before it is read
    ok = dict(P=7, N=3, T=40, V=25, K=2, S=1, seg=20)

    def call(pool=one, r=one, out=one, Lp=one, index=None, **kw):
        a = dict(ok, **kw)
        return L.agcn_sgn_collate(pool, index, r, None, out, None, Lp, a['P'], a['N'], a['T'], a['V'], a['K'], a['S'],
                                  a['seg'], None)
    for kw in (dict(pool=None), dict(r=None), dict(out=None), dict(Lp=None), dict(P=0), dict(N=0), dict(N=8), dict(T=0),
               dict(T=2049), dict(V=1), dict(V=33), dict(K=1), dict(S=0), dict(seg=0)):
        assert call(**kw) == -1, kw
