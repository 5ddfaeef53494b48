"""Generate the SGN v15 fixtures by running the REFERENCE class (model/architecture/sgn/sgn_v15.py::SGN) on the CPU:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_sgn_v15.py

  sgn15_<case>.npz   one file per case of tests/sgn_v15_util.py::CASES: key list, shapes and checksums of the state_dict
                     (the parameters themselves come from the seeded recipe sgn_v15_util.sgn15_state), x, the eval logits,
                     both attention maps, spa_emb[0, :, :, 0], tem_emb[0, :, 0, :] and the two pooled maxima
  sgn15_online.npz   the raw frames of sgn_online_v15.npz -> DataPreprocessorV2 (window 36) -> the v15 model in the
                     j15_deployed configuration -> mean logits, scores and label, with the recorded draws

Needs the reference checkout and einops.  Only data is stored.  The reference's packages model, model.architecture and
model.architecture.sgn are registered as bare modules carrying __path__, so that their __init__s (which import torchinfo)
do not run; torchinfo itself is a stub.

Three conditions are asserted per case, a seed is searched for if one fails, and the measured values go into the meta:
  1. in both blocks the median over rows of the largest attention probability lies in [0.2, 0.8] (a one-hot map hides
     every error in the scores);
  2. at least 10 % of the pooled maxima of each pooling are negative (a ReLU-neutral maximum must fail);
  3. the reference's own fp32-vs-fp64 distance of every stored tensor is at most a quarter of the tests' bound."""
import importlib
import json
import os
import sys
import types
from functools import partial

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

import make_golden as mg  # noqa: E402
import make_online_golden as mo  # noqa: E402
import make_golden_sgn as ms  # noqa: E402

sys.path.insert(0, mg.ROOT)
from tests import sgn_v15_util as vu  # noqa: E402

LIMIT = 1 << 20
GAP = 1e-3


def load_reference_v15():
    _, pre, dp, gen = mo.load_reference_online()
    for k in [k for k in sys.modules if k.split('.')[0] in ('model', 'feeders')]:
        del sys.modules[k]
    ti = types.ModuleType('torchinfo')
    ti.summary = lambda *a, **k: None
    sys.modules['torchinfo'] = ti
    for name in ('model', 'model.architecture', 'model.architecture.sgn'):
        m = types.ModuleType(name)
        m.__path__ = [os.path.join(mg.REF, *name.split('.'))]
        sys.modules[name] = m
    mod = importlib.import_module('model.architecture.sgn.sgn_v15')
    loader = importlib.import_module('feeders.loader')
    assert mod.__file__.startswith(mg.REF) and loader.__file__.startswith(mg.REF)
    return mod, loader, pre, dp, gen


def run(model, x):
    """-> the stored tensors of one eval forward, in x's dtype."""
    seen = {}
    hooks = [model.smp.register_forward_hook(lambda m, i, o: seen.__setitem__('feat', o)),
             model.tmp.register_forward_hook(lambda m, i, o: seen.__setitem__('pooled', o))]
    with torch.no_grad():
        logits, aux = model(x)
    for h in hooks:
        h.remove()
    assert len(aux['spatial_attn_list']) == 1 and len(aux['temporal_attn_list']) == 1
    return dict(logits=logits, spatial_attn=aux['spatial_attn_list'][0], temporal_attn=aux['temporal_attn_list'][0],
                spa_emb=aux['spa_emb'][0, :, :, 0], tem_emb=aux['tem_emb'][0, :, 0, :],
                feat=seen['feat'][:, :, 0, :].transpose(1, 2).contiguous(), pooled=seen['pooled'].flatten(1))


def measure(mod, kw, state, x):
    model = mod.SGN(**kw)
    model.load_state_dict(vu.torch_state(state))
    model.eval()
    out = run(model, x)
    out64 = run(model.double(), x.double())
    dist = {k: float((out[k].double() - out64[k]).abs().max()) for k in out}
    out = {k: v.numpy() for k, v in out.items()}
    rowmax = {k: float(np.median(out[k].max(-1))) for k in ('spatial_attn', 'temporal_attn')}
    neg = {k: float((out[k] < 0).mean()) for k in ('feat', 'pooled')}
    ok = (all(0.2 <= v <= 0.8 for v in rowmax.values()) and all(v >= 0.10 for v in neg.values())
          and all(dist[k] <= 0.25 * vu.bound(out[k]) for k in out))
    return ok, out, dict(rowmax=rowmax, negative=neg, fp32_vs_fp64=dist)


def make_cases(mod):
    for ci, (case, (V, seg, bs, bias, spatial, temporal)) in enumerate(vu.CASES.items()):
        kw = vu.case_args(case)
        sd = mod.SGN(**kw).state_dict()
        keys = list(sd.keys())
        shapes = {k: tuple(t.shape) for k, t in sd.items()}
        for seed in range(11 + 100 * ci, 11 + 100 * ci + 8):
            x = torch.from_numpy(ms.clip(np.random.default_rng(seed), bs, seg, V))
            scale = list(vu.QK_SCALE)
            for _ in range(12):                              # a block's scale moves until its map is neither one-hot nor flat
                state = vu.sgn15_state(shapes, seed, tuple(scale))
                ok, out, measured = measure(mod, kw, state, x)
                if ok:
                    break
                moved = False
                for b, k in enumerate(('spatial_attn', 'temporal_attn')):
                    r = measured['rowmax'][k]
                    if r < 0.25 or r > 0.75:
                        scale[b] = scale[b] * 1.5 if r < 0.25 else scale[b] / 1.5
                        moved = True
                if not moved:
                    break
            for k in keys:                                   # the recipe's one-hot buffers are the class's own
                if k.endswith('onehot'):
                    assert np.array_equal(state[k], sd[k].numpy()), k
            if ok:
                break
            print(f'{case}: seed {seed} rejected at scales {scale}: {measured}')
        else:
            raise SystemExit(f'{case}: no seed meets the three conditions')
        meta = dict(case=case, seed=seed, bs=bs, model_args=kw, qk_scale=scale, **measured)
        rec = dict(meta=np.array(json.dumps(meta)), x=x.numpy(), **out)
        vu.pack_state(rec, state, keys)
        path = os.path.join(HERE, f'sgn15_{case}.npz')
        np.savez_compressed(path, **rec)
        assert os.path.getsize(path) < LIMIT, (path, os.path.getsize(path))
        print(f'{case}: seed {seed}, {len(keys)} keys, {os.path.getsize(path) >> 10} KiB, {measured}')


ONLINE_SEED = 1511


def make_online(mod, loader, pre, dp, gen):
    with np.load(os.path.join(HERE, 'sgn_online_v15.npz')) as f:
        frames, record = f['frames'], tuple(int(i) for i in f['record'])
    v, window_len, seg, S = 15, 36, 20, 5
    kw = vu.case_args('j15_deployed')
    model = mod.SGN(**kw)
    sd = model.state_dict()
    keys = list(sd.keys())
    scale = json.loads(str(np.load(os.path.join(HERE, 'sgn15_j15_deployed.npz'))['meta']))['qk_scale']
    state = vu.sgn15_state({k: tuple(t.shape) for k, t in sd.items()}, ONLINE_SEED, tuple(scale))
    model.load_state_dict(vu.torch_state(state))
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
        with ms.Draws() as d:
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
    out = dict(record=np.array(record, dtype=np.int64), draws=np.stack(draws), logits=np.stack(logits),
               scores=np.stack(scores), labels=np.array(labels, dtype=np.int64),
               meta=np.array(json.dumps(dict(seed=ONLINE_SEED, qk_scale=scale, model_args=kw, window=window_len, max_person=4, select=2,
                                             multi_test=S, frames='sgn_online_v15.npz'))))
    vu.pack_state(out, state, keys)
    np.savez_compressed(os.path.join(HERE, 'sgn15_online.npz'), **out)
    assert os.path.getsize(os.path.join(HERE, 'sgn15_online.npz')) < LIMIT


if __name__ == '__main__':
    torch.manual_seed(0)
    np.random.seed(0)
    torch.set_num_threads(8)
    mod, loader, pre, dp, gen = load_reference_v15()
    make_cases(mod)
    make_online(mod, loader, pre, dp, gen)
