"""Generate the SGN collate fixture by running the REFERENCE on the CPU:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_sgn_collate.py

  sgn_collate.npz   two groups of samples (C, T, V, 2) -- V = 25, T = 40, seg = 20 and V = 15, T = 64, seg = 12 -- through
                    feeders/loader.py::NTUDataLoaders.collate_fn_fix_train (theta 0.5 and 0.3), _val and _test (S = 5):
                    inputs, labels, the recorded draws r = idx - low, the rotation angles and matrices, the reference's
                    batch permutation idx, and the outputs x, s, y and valid_frames.  Also a few (logits, target, eps)
                    cases with the value and gradient of utils/loss.py::LabelSmoothingLoss.

The samples of a group: both bodies throughout; the second body null throughout; the first body null in some frames
and both null in a tail (the dataset's zero padding); fewer kept rows than seg (zero padding rows, s = 0 there); 1.5 * seg
kept rows (half-integer interval bounds: 30 at seg = 20).

Needs the reference checkout.  Only data is stored.  np.random.randint is wrapped to record the draws
(make_golden_sgn.Draws); the angles are recorded by drawing them again under the same torch seed, and the recipe asserts
that they reproduce the reference's rotated output through its own _rot."""
import importlib
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

import make_golden as mg  # noqa: E402
import make_online_golden as mo  # noqa: E402
from make_golden_sgn import Draws, LIMIT  # noqa: E402

GROUPS = [('v25', 25, 40, 20, 1500), ('v15', 15, 64, 12, 1510)]
S_TEST = 5
TRAIN = [('train_cv', 'NTU60-CV', 0.5), ('train_cs', 'NTU60-CS', 0.3)]


def load_reference():
    sys.path.insert(0, mg.REF)
    for k in [k for k in sys.modules if k.split('.')[0] in ('feeders', 'utils')]:
        del sys.modules[k]
    loader = importlib.import_module('feeders.loader')
    tools = importlib.import_module('feeders.tools')
    assert loader.__file__.startswith(mg.REF) and tools.__file__.startswith(mg.REF)
    spec = importlib.util.spec_from_file_location('ref_loss', os.path.join(mg.REF, 'utils/loss.py'))
    loss = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(loss)
    return loader, tools, loss


def samples(rng, t, v, seg):
    """(5, 3, T, V, 2) and the kept rows each sample must give."""
    out, want = [], []
    for kind in ('both', 'single', 'mixed', 'short', 'half'):
        s = np.stack([mo.body(rng, t, v, np.zeros(3)), mo.body(rng, t, v, np.array([0.8, 0.3, 0.0]))]) - mo.CENTRE
        if kind == 'both':
            kept = 2 * t
        elif kind == 'single':
            s[1] = 0
            kept = t
        elif kind == 'mixed':
            s[0, 3:9] = 0                      # only body 1
            s[1, 12:14] = 0                    # only body 0
            s[:, t - 7:] = 0                   # the dataset's zero padding
            kept = 2 * (t - 7) - 6 - 2
        elif kind == 'short':
            s[0, 4:] = 0
            s[1, 3:] = 0
            kept = 7
        else:
            s[1] = 0
            s[0, seg * 3 // 2:] = 0
            kept = seg * 3 // 2
        mo.check_null_tests(s, kind)
        out.append(np.transpose(s.astype(np.float32), (3, 1, 2, 0)))        # (3, T, V, M)
        want.append(max(kept, seg))
    return np.ascontiguousarray(np.stack(out)), want


def run(fn, batch, seed):
    np.random.seed(seed)
    torch.manual_seed(seed)
    with Draws() as d:
        (x, s), y, valid = fn(batch)
    return x.numpy(), s.numpy(), np.asarray(y), np.asarray(valid, dtype=np.int32), d.r()


def make_group(loader, tools, name, v, t, seg, seed, out):
    data, want = samples(np.random.default_rng(seed), t, v, seg)
    B = len(data)
    labels = np.arange(B, dtype=np.int64) * 7 % 60
    batch = [(data[i], int(labels[i]), i) for i in range(B)]
    out[f'{name}.data'], out[f'{name}.label'], out[f'{name}.seg'] = data, labels, np.int64(seg)

    def store(mode, x, s, y, valid, r, S, idx, angles=None, rot=None):
        assert x.dtype == np.float32 and x.shape == (B * S, seg, v * 3) and s.shape == (B * S, seg, 1), (x.shape, s.shape)
        assert list(valid) == want, (mode, valid, want)
        p = f'{name}.{mode}.'
        out[p + 'x'], out[p + 's'], out[p + 'y'], out[p + 'valid_frames'] = x, s.astype(np.float32), y, valid
        out[p + 'r'], out[p + 'idx'], out[p + 'S'] = r.reshape(B, S, seg), np.asarray(idx, dtype=np.int64), np.int64(S)
        if angles is not None:
            out[p + 'angles'], out[p + 'rot'] = angles, rot
        print(f'{name} {mode}: x {x.shape}, valid {list(valid)}, |x|max {float(np.abs(x).max()):.3f}')

    for mi, (mode, dataset, theta) in enumerate(TRAIN):
        dl = loader.NTUDataLoaders(dataset=dataset, aug=1, seg=seg, multi_test=S_TEST)
        x, s, y, valid, r = run(dl.collate_fn_fix_train, batch, seed + 1 + mi)
        # the same draws without the rotation, the sort's permutation, and the angles under the same torch seed
        x0, s0, y0, _, r0 = run(lambda b: dl.collate_fn_fix(b, sampling_frequency=1, sort_data=True), batch, seed + 1 + mi)
        assert np.array_equal(r, r0) and np.array_equal(s, s0) and np.array_equal(y, y0)
        idx = np.array([seg] * B, dtype=int).argsort()[::-1]
        assert np.array_equal(y, labels[idx])
        torch.manual_seed(seed + 1 + mi)
        angles = torch.empty(B, 3).uniform_(-theta, theta)
        rot = tools._rot(angles.repeat(1, seg).view(-1, seg, 3))                                   # (B, seg, 3, 3)
        p = torch.from_numpy(x0).view(B, seg, v, 3)
        again = torch.matmul(rot, p.transpose(2, 3)).transpose(2, 3).contiguous().view(B, seg, v * 3)
        assert np.array_equal(again.numpy(), x), 'the re-drawn angles do not reproduce the rotated output'
        assert float(angles.abs().max()) <= theta and rot.dtype == torch.float32
        out[f'{name}.{mode}.x_unrotated'] = x0
        store(mode, x, s, y, valid, r, 1, idx, angles.numpy(), rot[:, 0].numpy())
    dl = loader.NTUDataLoaders(dataset='NTU60-CV', aug=1, seg=seg, multi_test=S_TEST)
    store('val', *run(dl.collate_fn_fix_val, batch, seed + 5), 1, np.arange(B))
    store('test', *run(dl.collate_fn_fix_test, batch, seed + 6), S_TEST, np.arange(B * S_TEST))


def make_loss(loss, out):
    cases = [(4, 60, 0.1, 1601), (3, 7, 0.3, 1602), (5, 2, 0.1, 1603), (2, 60, 0.0, 1604)]
    for i, (b, c, eps, seed) in enumerate(cases):
        rng = np.random.default_rng(seed)
        logits = torch.from_numpy((3.0 * rng.standard_normal((b, c))).astype(np.float32)).requires_grad_(True)
        target = torch.from_numpy(rng.integers(0, c, size=(b,)).astype(np.int64))
        val = loss.LabelSmoothingLoss(classes=c, smoothing=eps)(logits, target)
        val.backward()
        p = f'loss{i}.'
        out[p + 'logits'], out[p + 'target'], out[p + 'eps'] = logits.detach().numpy(), target.numpy(), np.float64(eps)
        out[p + 'value'], out[p + 'grad'] = val.detach().numpy(), logits.grad.numpy()
        print(f'loss{i}: C {c}, eps {eps}, value {float(val):.6f}')
    out['loss_cases'] = np.int64(len(cases))


if __name__ == '__main__':
    torch.set_num_threads(1)
    loader, tools, loss = load_reference()
    out = {'groups': np.array([g[0] for g in GROUPS]), 'train_modes': np.array([m[0] for m in TRAIN])}
    for name, v, t, seg, seed in GROUPS:
        make_group(loader, tools, name, v, t, seg, seed, out)
    make_loss(loss, out)
    path = os.path.join(HERE, 'sgn_collate.npz')
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < LIMIT, os.path.getsize(path)
    print(path, os.path.getsize(path))
