"""Shared by the SGN tests and tests/golden/make_golden_sgn.py: the seeded parameter recipe (the fixtures store the seed,
the key list and a checksum per tensor, not the 2.7 MB of parameters), the fixture loaders and a numpy emulation of
``agcn_sgn_sample`` that pins its specification without a GPU."""
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')

CASES = ('v15_seg20', 'v25_seg20', 'v15_sharp', 'v7_seg12_nobias')
TRAIN_CASES = ('v15_seg20', 'v7_seg12_nobias')
WINDOWS = ('mixed', 'short', 'full', 'v25')


def sgn_state(shapes, seed, gscale=1.0):
    """{key: numpy array} for the (key, shape) pairs of an SGN state_dict.  Every tensor has its own generator, seeded by
    (seed, position of the key in the sorted key list): BatchNorm weights and running variances uniform in [0.5, 1.5],
    running means and every bias 0.2 / 0.1 * normal, weights normal with std sqrt(2 / fan_in) -- the gcn*.w weights too,
    which the reference initialises to zero (the g.x branch would be dead).  ``gscale`` multiplies the weights and biases
    of compute_g1.g1 / g2, so the logits of the adjacency softmax scale with its square."""
    out = {}
    for i, key in enumerate(sorted(shapes)):
        shape = tuple(shapes[key])
        rng = np.random.default_rng([int(seed), i])
        leaf = key.rsplit('.', 1)[-1]
        is_bn = any(part.startswith('bn') for part in key.split('.')[:-1])
        if leaf == 'num_batches_tracked':
            v = np.zeros(shape, dtype=np.int64)
        elif leaf == 'running_var' or (is_bn and leaf == 'weight'):
            v = rng.uniform(0.5, 1.5, shape).astype(np.float32)
        elif leaf == 'running_mean':
            v = (0.2 * rng.standard_normal(shape)).astype(np.float32)
        elif leaf == 'bias':
            v = (0.1 * rng.standard_normal(shape)).astype(np.float32)
        else:
            fan_in = int(np.prod(shape[1:]))
            v = (np.sqrt(2.0 / fan_in) * rng.standard_normal(shape)).astype(np.float32)
        if key.startswith('compute_g1.') and gscale != 1.0:
            v = (v * np.float32(gscale)).astype(np.float32)
        out[key] = v
    return out


def checksums(state):
    """fp64 (sum, sum of squares) per tensor, in sorted key order."""
    return np.array([[np.asarray(state[k], dtype=np.float64).sum(), np.square(np.asarray(state[k], dtype=np.float64)).sum()]
                     for k in sorted(state)])


_FILES = {}


def _npz(name):
    if name not in _FILES:
        with np.load(os.path.join(GOLDEN, name)) as f:
            _FILES[name] = {k: f[k] for k in f.files}
    return _FILES[name]


def load_case(case):
    """-> dict(meta, keys, shapes, state (regenerated and checked against the stored checksums), x, logits, g)."""
    f = _npz('sgn_model.npz')
    meta = json.loads(str(f[case + '.meta']))
    keys = [str(k) for k in f[case + '.keys']]
    shapes = {k: tuple(int(d) for d in s.split('x') if d) for k, s in zip(keys, (str(s) for s in f[case + '.shapes']))}
    state = sgn_state(shapes, meta['seed'], meta['gscale'])
    assert np.array_equal(checksums(state), f[case + '.checksums']), 'the seeded recipe no longer reproduces the fixture'
    return dict(meta=meta, keys=keys, shapes=shapes, state=state, x=f[case + '.x'], logits=f[case + '.logits'],
                g=f[case + '.g'])


def load_train(case):
    """The train-mode record of a case: dict(c, logits, grad_x, grads {key: array}); the gradients are spread over files
    of less than 1 MiB each."""
    head = _npz(f'sgn_train_{case}_p0.npz')
    grads = {}
    for p in range(int(head['parts'])):
        part = _npz(f'sgn_train_{case}_p{p}.npz')
        grads.update({k[5:]: v for k, v in part.items() if k.startswith('grad.')})
    return dict(c=head['c'], logits=head['logits'], grad_x=head['grad_x'], grads=grads)


def model_args(meta):
    return dict(num_class=meta['num_class'], num_point=meta['num_point'], in_channels=3, seg=meta['seg'], bias=meta['bias'])


def torch_state(state):
    import torch
    return {k: torch.from_numpy(np.array(v)) for k, v in state.items()}


# ---- agcn_sgn_sample in numpy ------------------------------------------------------------------------------------------
def sample_intervals(L, seg):
    """b_k = rint(k * (L / seg)) in fp64, k = 0..seg (round half to even, as numpy's round)."""
    return np.array([int(np.rint(float(k) * (float(L) / float(seg)))) for k in range(seg + 1)], dtype=np.int64)


def sample_emulate(win, r, seg):
    """win (N, 3, T, V, 2) normalised windows, r (N, S, seg) uint32 -> (out (N, S, seg, V*3) fp32, L (N,) int32):
    row (t, m) is kept iff body m's frame t is not all zero, rows ordered by (t, m); fewer than seg rows are followed by
    zero rows up to seg; idx_k = b_k + r % (b_{k+1} - b_k)."""
    N, C, T, V, K = win.shape
    assert C == 3 and K == 2
    S = r.shape[1]
    out = np.zeros((N, S, seg, V * 3), dtype=np.float32)
    Ls = np.zeros(N, dtype=np.int32)
    for n in range(N):
        rows = np.transpose(win[n], (1, 3, 2, 0)).reshape(T * 2, V * 3)          # (t, m) major, (v, c) minor
        kept = rows[(rows != 0).any(1)]
        if len(kept) == 0:
            continue
        if len(kept) < seg:
            kept = np.concatenate([kept, np.zeros((seg - len(kept), V * 3), dtype=np.float32)])
        L = len(kept)
        b = sample_intervals(L, seg)
        for s in range(S):
            idx = b[:-1] + (r[n, s].astype(np.int64) % (b[1:] - b[:-1]))
            out[n, s] = kept[idx]
        Ls[n] = L
    return out, Ls
