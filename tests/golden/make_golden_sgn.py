"""Generate the SGN fixtures by running the REFERENCE on the CPU:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_sgn.py

  sgn_model.npz            four cases: key list, shapes and checksums of the state_dict (the parameters themselves come
                           from the seeded recipe tests/sgn_util.py::sgn_state), x, and the eval logits and g of the
                           reference model/architecture/sgn/archiv/sgn.py::SGN
  sgn_train_<case>_p*.npz  train-mode record of two cases (dropout p = 0): logits and the gradient of sum(logits * c)
                           w.r.t. x and every parameter, spread over files below the size limit of a committed file
  sgn_sample.npz           four windows in prenorm's output layout through feeders/loader.py::NTUDataLoaders.to_fix_length
                           (equal-interval branch, S = 5): output, row count and the recorded draws r = idx - low
  sgn_online_v15.npz       raw frames -> DataPreprocessorV2 (aagcn_normalize + sgn_preprocess, window 36) -> SGN -> mean
                           logits, scores and label, with the recorded draws

Needs the reference checkout.  Only data is stored.  sgn.py is imported by path with torch.Tensor.cuda patched to the
identity (its constructor calls .cuda()); np.random.randint is wrapped to record the draws."""
import importlib
import importlib.util
import json
import os
import sys
from functools import partial

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

import make_golden as mg  # noqa: E402
import make_online_golden as mo  # noqa: E402

sys.path.insert(0, mg.ROOT)
from tests import sgn_util as su  # noqa: E402

LIMIT = 1 << 20
GAP = 1e-3


def load_reference_sgn():
    ref, pre, dp, gen = mo.load_reference_online()
    spec = importlib.util.spec_from_file_location('ref_sgn', os.path.join(mg.REF, 'model/architecture/sgn/archiv/sgn.py'))
    mod = importlib.util.module_from_spec(spec)
    cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        spec.loader.exec_module(mod)
    finally:
        torch.Tensor.cuda = cuda
    for k in [k for k in sys.modules if k.split('.')[0] == 'feeders']:
        del sys.modules[k]
    loader = importlib.import_module('feeders.loader')
    assert loader.__file__.startswith(mg.REF)
    return mod, loader, pre, dp, gen


def build(mod, **kw):
    cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        return mod.SGN(**kw)
    finally:
        torch.Tensor.cuda = cuda


class Draws:
    """np.random.randint wrapped: every call with array bounds is recorded as (low, result)."""

    def __enter__(self):
        self.calls = []
        self.orig = np.random.randint

        def spy(*a, **k):
            out = self.orig(*a, **k)
            if 'low' in k and np.ndim(k['low']) == 1:
                self.calls.append((np.asarray(k['low']).copy(), np.asarray(out).copy()))
            return out
        np.random.randint = spy
        return self

    def __exit__(self, *exc):
        np.random.randint = self.orig

    def r(self):
        return np.stack([out - low for low, out in self.calls]).astype(np.uint32)


# ---- sgn_model.npz, sgn_train_* ----------------------------------------------------------------------------------------
MODEL_CASES = [
    # name, V, seg, bs, bias, seed, sharp
    ('v15_seg20', 15, 20, 5, True, 1201, False),
    ('v25_seg20', 25, 20, 3, True, 1202, False),
    ('v15_sharp', 15, 20, 1, True, 1203, True),
    ('v7_seg12_nobias', 7, 12, 2, False, 1204, False),
]
NUM_CLASS = 60


def clip(rng, bs, seg, v):
    """(bs, seg, V*3): a pose per clip that drifts, as rows of a normalised window look."""
    pose = 0.5 * rng.standard_normal((bs, 1, v, 3))
    drift = np.cumsum(0.05 * rng.standard_normal((bs, seg, 1, 3)), axis=1)
    return (pose + drift + 0.03 * rng.standard_normal((bs, seg, v, 3))).astype(np.float32).reshape(bs, seg, v * 3)


def g3_max(model, x):
    seen = []
    h = model.compute_g1.softmax.register_forward_hook(lambda m, i, o: seen.append(float(i[0].abs().max())))
    with torch.no_grad():
        model(x)
    h.remove()
    return seen[0]


def make_models(mod):
    out = {}
    for name, v, seg, bs, bias, seed, sharp in MODEL_CASES:
        kw = dict(num_class=NUM_CLASS, num_point=v, in_channels=3, seg=seg, bias=bias)
        model = build(mod, **kw)
        sd = model.state_dict()
        assert 'spa' not in sd and 'tem' not in sd and len(sd) == (70 if bias else 55), len(sd)
        shapes = {k: tuple(t.shape) for k, t in sd.items()}
        x = torch.from_numpy(clip(np.random.default_rng(seed), bs, seg, v))
        gscale = 1.0
        model.load_state_dict(su.torch_state(su.sgn_state(shapes, seed)))
        model.eval()
        if sharp:
            gscale = float(np.sqrt(30.0 / g3_max(model, x)))
            model.load_state_dict(su.torch_state(su.sgn_state(shapes, seed, gscale)))
            m = g3_max(model, x)
            assert 25.0 < m < 35.0, m
            print(f'{name}: gscale {gscale:.4f}, max|g3| {m:.2f}')
        state = su.sgn_state(shapes, seed, gscale)
        with torch.no_grad():
            logits, g = model(x)
        assert g.shape == (bs, seg, v, v)
        if name == 'v15_seg20':            # the five clips as the five draws of one prediction
            top = torch.sort(torch.softmax(logits.mean(0), 0), descending=True).values
            assert float(top[0] - top[1]) >= GAP, f'{name}: top-1 minus top-2 mean score {float(top[0] - top[1]):.2e}'
            print(f'{name}: top-1 minus top-2 mean score {float(top[0] - top[1]):.2e}')
        keys = list(sd.keys())
        meta = dict(kw, seed=seed, gscale=gscale, bs=bs)
        out[name + '.meta'] = np.array(json.dumps(meta))
        out[name + '.keys'] = np.array(keys)
        out[name + '.shapes'] = np.array(['x'.join(str(d) for d in shapes[k]) for k in keys])
        out[name + '.checksums'] = su.checksums(state)
        out[name + '.x'] = x.numpy()
        out[name + '.logits'] = logits.numpy()
        out[name + '.g'] = g.numpy()
        print(f'{name}: {len(keys)} keys, |logits|max {float(logits.abs().max()):.3f}')
        if name in su.TRAIN_CASES:
            make_train(name, model, x, seed)
    path = os.path.join(HERE, 'sgn_model.npz')
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < LIMIT


def make_train(name, model, x, seed):
    model.train()
    model.cnn.dropout.p = 0.0
    c = torch.from_numpy(np.random.default_rng(seed + 50).standard_normal((x.shape[0], NUM_CLASS)).astype(np.float32))
    xg = x.clone().requires_grad_(True)
    logits, _ = model(xg)
    (logits * c).sum().backward()
    grads = {k: p.grad.numpy() for k, p in model.named_parameters()}
    assert all(g is not None for g in grads.values())
    parts, size = [dict()], 0
    for k in sorted(grads):                    # greedy packing below the limit (random floats do not compress)
        n = grads[k].nbytes + 512
        if size + n > LIMIT - (64 << 10):
            parts.append(dict())
            size = 0
        parts[-1]['grad.' + k] = grads[k]
        size += n
    parts[0].update(c=c.numpy(), logits=logits.detach().numpy(), grad_x=xg.grad.numpy(), parts=np.int64(len(parts)))
    for p, d in enumerate(parts):
        path = os.path.join(HERE, f'sgn_train_{name}_p{p}.npz')
        np.savez_compressed(path, **d)
        assert os.path.getsize(path) < LIMIT, (path, os.path.getsize(path))
    print(f'{name} train: {len(parts)} files, |dx|max {float(xg.grad.abs().max()):.3e}')


# ---- sgn_sample.npz ----------------------------------------------------------------------------------------------------
def window(rng, t, v, kind):
    """(3, T, V, 2) in prenorm's output layout."""
    s = np.stack([mo.body(rng, t, v, np.zeros(3)), mo.body(rng, t, v, np.array([0.8, 0.3, 0.0]))]) - mo.CENTRE    # M, T, V, 3
    if kind == 'mixed':
        s[:, 5] = 0                  # a null frame
        s[1, 10:15] = 0              # only body 0
        s[0, 20:26] = 0              # only body 1
    elif kind == 'short':
        s[0, 4:] = 0
        s[1, 3:] = 0
    return np.ascontiguousarray(np.transpose(s.astype(np.float32), (3, 1, 2, 0)))


SAMPLE_WINDOWS = [('mixed', 37, 15, 61), ('short', 20, 15, 20), ('full', 300, 15, 600), ('v25', 64, 25, 128)]


def to_fix_length(loader, win, seg, S):
    """win (N, 3, T, V, 2) -> reference (N*S, seg, V*3), valid frames, r (N*S, seg)."""
    data = np.transpose(win, [0, 2, 4, 3, 1])
    data = data.reshape((*data.shape[0:2], -1))
    fn = loader.NTUDataLoaders(dataset='NTU60', seg=seg, multi_test=S).to_fix_length
    with Draws() as d:
        seqs, _, _, valid = fn(data, labels=None, sampling_frequency=S)
    return np.array(seqs, dtype=seqs[0].dtype), np.array(valid, dtype=np.int32), d.r()


def make_sample(loader):
    out = {}
    for gi, (name, t, v, want) in enumerate(SAMPLE_WINDOWS):
        win = window(np.random.default_rng(1300 + gi), t, v, name)[None]
        mo.check_null_tests(np.transpose(win, [0, 4, 2, 3, 1]), name)
        ref, valid, r = to_fix_length(loader, win, 20, 5)
        assert ref.dtype == np.float32 and ref.shape == (5, 20, v * 3) and int(valid[0]) == want, (ref.shape, valid)
        emu, L = su.sample_emulate(win, r.reshape(1, 5, 20), 20)
        assert np.array_equal(emu[0], ref) and int(L[0]) == want
        out[name + '.win'], out[name + '.out'], out[name + '.L'], out[name + '.r'] = win[0], ref, valid[0], r
        print(f'{name}: window {win.shape[1:]}, L {int(valid[0])}')
    np.savez_compressed(os.path.join(HERE, 'sgn_sample.npz'), **out)
    assert os.path.getsize(os.path.join(HERE, 'sgn_sample.npz')) < LIMIT


# ---- sgn_online_v15.npz ------------------------------------------------------------------------------------------------
ONLINE_SEED = 1401


def make_online(mod, loader, pre, dp, gen):
    v, window_len, n, seg, S = 15, 36, 44, 20, 5
    record = (19, 35, 43)
    frames = mo.stream_frames(np.random.default_rng(1400), n, v, starts={0: 0, 2: 3}, gaps={2: (12,)})
    kw = dict(num_class=NUM_CLASS, num_point=v, in_channels=3, seg=seg, bias=True)
    model = build(mod, **kw)
    shapes = {k: tuple(t.shape) for k, t in model.state_dict().items()}
    state = su.sgn_state(shapes, ONLINE_SEED)
    model.load_state_dict(su.torch_state(state))
    model.eval()
    norm = partial(pre.pre_normalization, **mo.AXES[v], verbose=False, tqdm=False)
    fix = partial(loader.NTUDataLoaders(dataset='NTU60', seg=seg, multi_test=S).to_fix_length, labels=None,
                  sampling_frequency=S)
    proc = dp.DataPreprocessorV2(num_joint=v, max_seq_length=window_len, max_person=4, moving_avg=1,
                                 aagcn_normalize_fn=norm, sgn_preprocess_fn=fix)
    draws, logits, scores, labels = [], [], [], []
    for i, f in enumerate(frames):
        proc.append_data(f)
        if i not in record:
            continue
        energy = np.array([gen.get_nonzero_std(x) for x in proc.data])
        mo.check_energies(energy, f'sgn stream append {i}')
        chosen = proc.data[energy.argsort()[::-1][0:2]][None]
        mo.normalize_checked(pre, np.ascontiguousarray(np.transpose(chosen, [0, 4, 2, 3, 1])), f'sgn stream append {i}',
                             **mo.AXES[v])
        with Draws() as d:
            data = proc.select_skeletons_and_normalize_data(2, aagcn_normalize=True, sgn_preprocess=True)
        assert data.shape == (S, seg, v * 3) and data.dtype == np.float32, (data.shape, data.dtype)
        with torch.no_grad():
            lg, _ = model(torch.from_numpy(data))
            lg = lg.view((-1, S, lg.size(1))).mean(1)
            sc = torch.softmax(lg, 1)
        top = torch.sort(sc[0], descending=True).values
        assert float(top[0] - top[1]) >= GAP, f'append {i}: top-1 minus top-2 mean score {float(top[0] - top[1]):.2e}'
        print(f'online append {i}: label {int(sc[0].argmax())}, gap {float(top[0] - top[1]):.2e}')
        draws.append(d.r())
        logits.append(lg[0].numpy())
        scores.append(sc[0].numpy())
        labels.append(int(sc[0].argmax()))
    out = dict(frames=frames, record=np.array(record, dtype=np.int64), draws=np.stack(draws), logits=np.stack(logits),
               scores=np.stack(scores), labels=np.array(labels, dtype=np.int64), checksums=su.checksums(state),
               keys=np.array(list(shapes)), shapes=np.array(['x'.join(str(d) for d in shapes[k]) for k in shapes]),
               meta=np.array(json.dumps(dict(kw, seed=ONLINE_SEED, gscale=1.0, window=window_len, max_person=4, select=2,
                                             multi_test=S))))
    np.savez_compressed(os.path.join(HERE, 'sgn_online_v15.npz'), **out)
    assert os.path.getsize(os.path.join(HERE, 'sgn_online_v15.npz')) < LIMIT


if __name__ == '__main__':
    torch.manual_seed(0)
    np.random.seed(0)
    torch.set_num_threads(8)
    mod, loader, pre, dp, gen = load_reference_sgn()
    make_sample(loader)
    make_models(mod)
    make_online(mod, loader, pre, dp, gen)
