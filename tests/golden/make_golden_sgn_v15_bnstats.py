"""Generate the batch-statistics fixture of SGN v15 by running the REFERENCE class
(model/architecture/sgn/sgn_v15.py::SGN) on the CPU:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_sgn_v15_bnstats.py

  sgn15_bnstats.npz  five cases on the geometries of the eval fixtures (tests/sgn_v15_bnstats_util.py::CASES).  Per case
                     ONE train() forward of the whole x as one batch with every dropout probability 0: the batch mean and
                     biased variance each of the six BatchNorms saw (forward pre-hooks, reduced in fp64 from the fp32
                     activations), the train-mode logits, the running statistics after that forward from
                     reset_running_stats() with momentum None and with 0.1, the eval logits after the momentum-None one,
                     and per tensor the distance of the fp32 reference from the same reference in fp64 (its own noise
                     floor, relative to max(1, max|fp64|)).  Parameters come from the seeded recipe
                     sgn_v15_util.sgn15_state; the file stores x, the key list, shapes and checksums.

Needs the reference checkout and einops.  Only data is stored.  Conditions asserted, all on the reference alone:
  1. every tensor's fp32-vs-fp64 floor is below half the tests' bound;
  2. under BATCH statistics the median over rows of the largest attention probability of both maps lies in [0.2, 0.8]
     (n_a now normalises to unit variance, so the scales of the eval fixtures need not hold: the to_q / to_k scales move
     as in make_golden_sgn_v15.py and are recorded);
  3. at least 10 % of both pooled maxima are negative.
No minimum variance is asserted: the spa columns of the spatial tile are the same in every frame, and a column whose
ReLU is dead for every joint has variance exactly 0.  The number of such channels is recorded per case and at least one
case must have some."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

import make_golden as mg  # noqa: E402
import make_golden_sgn_v15 as mv  # noqa: E402

sys.path.insert(0, mg.ROOT)
from tests import sgn_v15_util as vu  # noqa: E402
from tests import sgn_v15_bnstats_util as bu  # noqa: E402

LIMIT = 1 << 20
CONSTANT = 1e-12
SEEDS = 16


def clip(rng, bs, seg, v):
    """(bs, seg, V*3): ONE skeleton for every clip, a centre per clip, a drift per frame common to the joints and a little
    noise per joint.  make_golden_sgn.py::clip draws a pose per clip AND joint; in train mode the DataNorms then normalise
    every joint's coordinates over the batch on their own, the joints of a frame come out uncorrelated, and the maximum
    over 15 or 25 such joints is negative in only 3 - 7 % of the columns (measured on the reference), short of condition
    3.  Joints that move together, as the joints of a body do, leave 9 - 15 %."""
    skeleton = 0.5 * rng.standard_normal((1, 1, v, 3))
    centre = 0.3 * rng.standard_normal((bs, 1, 1, 3))
    drift = np.cumsum(0.05 * rng.standard_normal((bs, seg, 1, 3)), axis=1)
    return (skeleton + centre + drift + 0.01 * rng.standard_normal((bs, seg, v, 3))).astype(np.float32).reshape(bs, seg, v * 3)


def one_forward(model, x, momentum):
    """reset_running_stats, one train-mode forward with every dropout probability 0 -> (stats {name: (mean, var)} in
    fp64, logits, running {name: (running_mean, running_var)}, the two attention maps, the two pooled maxima)."""
    model.train()
    for m in model.modules():
        if isinstance(m, torch.nn.modules.dropout._DropoutNd):
            m.p = 0.0
    seen, extra, hooks = {}, {}, []
    for name in bu.BN_NAMES:
        bn = model.get_submodule(name)
        bn.reset_running_stats()
        bn.momentum = momentum

        def hook(_m, args, name=name):
            a = args[0].detach().double()
            dims = [d for d in range(a.dim()) if d != 1]
            seen[name] = (a.mean(dims).numpy(), a.var(dims, unbiased=False).numpy())
        hooks.append(bn.register_forward_pre_hook(hook))
    hooks += [model.smp.register_forward_hook(lambda m, i, o: extra.__setitem__('feat', o.detach().numpy())),
              model.tmp.register_forward_hook(lambda m, i, o: extra.__setitem__('pooled', o.detach().numpy()))]
    with torch.no_grad():
        logits, aux = model(x)
    for h in hooks:
        h.remove()
    assert tuple(seen) == bu.BN_NAMES, 'the BatchNorms ran in another order'
    extra['spatial_attn'] = aux['spatial_attn_list'][0].detach().numpy()
    extra['temporal_attn'] = aux['temporal_attn_list'][0].detach().numpy()
    running = {n: (model.get_submodule(n).running_mean.detach().clone().numpy(),
                   model.get_submodule(n).running_var.detach().clone().numpy()) for n in bu.BN_NAMES}
    for n in bu.BN_NAMES:
        assert int(model.get_submodule(n).num_batches_tracked) == 1
    return seen, logits.detach().numpy(), running, extra


def record(mod, kw, state, x):
    """-> ({key: fp32 array} of one case, its floors, the measured conditions)."""
    out, measured = {}, {}
    for dtype in (torch.float32, torch.float64):
        model = mod.SGN(**kw)
        model.load_state_dict(vu.torch_state(state))
        model = model.to(dtype)
        xt = torch.from_numpy(x).to(dtype)
        r = {}
        stats, r['logits'], run_none, extra = one_forward(model, xt, None)
        if dtype == torch.float32:
            measured['rowmax'] = {k: float(np.median(extra[k].max(-1))) for k in ('spatial_attn', 'temporal_attn')}
            measured['negative'] = {k: float((extra[k] < 0).mean()) for k in ('feat', 'pooled')}
        model.eval()
        with torch.no_grad():
            r['eval_logits'] = model(xt)[0].numpy()
        _, _, run_01, _ = one_forward(model, xt, 0.1)
        for n in bu.BN_NAMES:
            r['mean.' + n], r['var.' + n] = stats[n]
            r['rm_none.' + n], r['rv_none.' + n] = run_none[n]
            r['rm_01.' + n], r['rv_01.' + n] = run_01[n]
        out[dtype] = r
    r32, r64 = out[torch.float32], out[torch.float64]
    floors = {k: float(np.abs(r32[k].astype(np.float64) - r64[k]).max() / max(1.0, float(np.abs(r64[k]).max())))
              for k in r32}
    measured['constant_channels'] = {n: int((r64['var.' + n] < CONSTANT).sum()) for n in bu.BN_NAMES}
    return {k: np.asarray(v, dtype=np.float32) for k, v in r32.items()}, floors, measured


def conditions(floors, measured):
    return (all(v < 0.5 * bu.BOUND for v in floors.values()) and all(0.2 <= v <= 0.8 for v in measured['rowmax'].values())
            and all(v >= 0.10 for v in measured['negative'].values()))


def main():
    torch.manual_seed(0)
    np.random.seed(0)
    torch.set_num_threads(8)
    mod = mv.load_reference_v15()[0]
    out, constant = {}, 0
    for case, (bs, seed0) in bu.CASES.items():
        V, seg, _, bias, spatial, temporal = vu.CASES[case]
        kw = vu.case_args(case)
        sd = mod.SGN(**kw).state_dict()
        keys = list(sd.keys())
        shapes = {k: tuple(t.shape) for k, t in sd.items()}
        for seed in range(seed0, seed0 + SEEDS):
            x = clip(np.random.default_rng(seed), bs, seg, V)
            scale = list(vu.QK_SCALE)
            for _ in range(12):                              # a block's scale moves until its map is neither one-hot nor flat
                state = vu.sgn15_state(shapes, seed, tuple(scale))
                rec, floors, measured = record(mod, kw, state, x)
                ok = conditions(floors, measured)
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
            if ok:
                break
            print(f'{case}: seed {seed} rejected at scales {scale}: {measured}, worst floor {max(floors.values()):.2e}')
        else:
            raise SystemExit(f'{case}: no seed meets the conditions')
        worst = max(floors, key=floors.get)
        n_const = sum(measured['constant_channels'].values())
        constant += n_const
        print(f'{case}: seed {seed}, scales {scale}, {measured}, worst noise floor {worst} {floors[worst]:.2e}, '
              f'|logits|max {float(np.abs(rec["logits"]).max()):.3f}')
        out[case + '.meta'] = np.array(json.dumps(dict(case=case, seed=seed, bs=bs, model_args=kw, qk_scale=scale, **measured)))
        out[case + '.keys'] = np.array(keys)
        out[case + '.shapes'] = np.array(['x'.join(str(d) for d in shapes[k]) for k in keys])
        out[case + '.checksums'] = vu.checksums(state)
        out[case + '.x'] = x
        for k, v in rec.items():
            out[f'{case}.{k}'] = v
        out[case + '.floor'] = np.array(json.dumps(floors))
    assert constant > 0, 'no case has a constant channel'
    path = os.path.join(HERE, 'sgn15_bnstats.npz')
    np.savez_compressed(path, **out)
    print(f'{path}: {os.path.getsize(path)} bytes')
    assert os.path.getsize(path) < LIMIT


if __name__ == '__main__':
    main()
