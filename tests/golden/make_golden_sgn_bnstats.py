"""Generate the batch-statistics fixture of SGN by running the REFERENCE on the CPU:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_sgn_bnstats.py

  sgn_bnstats.npz   five cases.  Per case ONE train-mode forward of the whole x as one batch with cnn.dropout.p = 0 (the
                    convention of make_golden_sgn.py::make_train) of the reference
                    model/architecture/sgn/archiv/sgn.py::SGN: the batch mean and biased variance each of the seven
                    BatchNorms saw (forward pre-hooks, reduced in fp64 from the fp32 activations), the train-mode logits
                    and g, the running statistics after that forward from reset_running_stats() with momentum None and
                    with 0.1, the eval logits after the momentum-None one, and per tensor the distance of the fp32
                    reference from the same reference in fp64 (its own noise floor, relative to max(1, max|fp64|)).
                    The three cases taken from sgn_model.npz store no state and no x (tests/sgn_util.py::load_case has
                    them); the two new ones store x, the key list, shapes and checksums in that file's format.

Needs the reference checkout.  Only data is stored."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

import make_golden as mg  # noqa: E402
import make_golden_sgn as ms  # noqa: E402

sys.path.insert(0, mg.ROOT)
from tests import sgn_util as su  # noqa: E402
from tests import sgn_bnstats_util as bu  # noqa: E402

LIMIT = 1 << 20
BOUND = 1e-4            # the tests' bound, relative to max(1, max|ref|)
MIN_VAR = 1e-3

# name, V, seg, bs, bias, seed: the cases that sgn_model.npz does not have.  The seeds were chosen on the reference alone:
# with 1212 the nine-clip case has a noise floor of 4.8e-5 in g (a sharp adjacency softmax), just under half the bound;
# 1217 has 1.9e-5.
NEW_CASES = [('v3_seg34', 3, 34, 3, True, 1211), ('v15_seg20_b9', 15, 20, 9, True, 1217)]


def one_forward(model, x, momentum):
    """reset_running_stats, one train-mode forward -> (stats {name: (mean, var)} in fp64, logits, g, running {name:
    (running_mean, running_var)})."""
    model.train()
    model.cnn.dropout.p = 0.0
    seen, hooks = {}, []
    for name in bu.BN_NAMES:
        bn = model.get_submodule(name)
        bn.reset_running_stats()
        bn.momentum = momentum

        def hook(_m, args, name=name):
            a = args[0].detach().double()
            dims = [d for d in range(a.dim()) if d != 1]
            seen[name] = (a.mean(dims).numpy(), a.var(dims, unbiased=False).numpy())
        hooks.append(bn.register_forward_pre_hook(hook))
    with torch.no_grad():
        logits, g = model(x)
    for h in hooks:
        h.remove()
    running = {n: (model.get_submodule(n).running_mean.detach().clone().numpy(),
                   model.get_submodule(n).running_var.detach().clone().numpy()) for n in bu.BN_NAMES}
    for n in bu.BN_NAMES:
        assert int(model.get_submodule(n).num_batches_tracked) == 1
    return seen, logits.detach().numpy(), g.detach().numpy(), running


def record(mod, kw, state, x):
    """-> {key: array} of one case, and its floors."""
    out = {}
    for dtype in (torch.float32, torch.float64):
        model = ms.build(mod, **kw)
        model.load_state_dict(su.torch_state(state))
        model = model.to(dtype)
        if dtype == torch.float64:          # the reference keeps its one-hot inputs as plain attributes
            model.spa, model.tem = model.spa.double(), model.tem.double()
        xt = torch.from_numpy(x).to(dtype)
        r = {}
        stats, r['logits'], r['g'], run_none = one_forward(model, xt, None)
        model.eval()
        with torch.no_grad():
            r['eval_logits'] = model(xt)[0].numpy()
        _, _, _, run_01 = one_forward(model, xt, 0.1)
        for n in bu.BN_NAMES:
            r['mean.' + n], r['var.' + n] = stats[n]
            r['rm_none.' + n], r['rv_none.' + n] = run_none[n]
            r['rm_01.' + n], r['rv_01.' + n] = run_01[n]
        out[dtype] = r
    r32, r64 = out[torch.float32], out[torch.float64]
    floors = {k: float(np.abs(r32[k].astype(np.float64) - r64[k]).max() / max(1.0, float(np.abs(r64[k]).max())))
              for k in r32}
    return {k: np.asarray(v, dtype=np.float32) for k, v in r32.items()}, floors


def main():
    torch.manual_seed(0)
    np.random.seed(0)
    torch.set_num_threads(8)
    mod = ms.load_reference_sgn()[0]
    out = {}
    for case in bu.CASES:
        new = {c[0]: c for c in NEW_CASES}.get(case)
        if new is None:
            c = su.load_case(case)
            kw, state, x = su.model_args(c['meta']), c['state'], c['x'][:bu.BATCH[case]]
        else:
            _, v, seg, bs, bias, seed = new
            kw = dict(num_class=ms.NUM_CLASS, num_point=v, in_channels=3, seg=seg, bias=bias)
            sd = ms.build(mod, **kw).state_dict()
            shapes = {k: tuple(t.shape) for k, t in sd.items()}
            state = su.sgn_state(shapes, seed)
            x = ms.clip(np.random.default_rng(seed), bs, seg, v)
            keys = list(sd.keys())
            out[case + '.meta'] = np.array(json.dumps(dict(kw, seed=seed, gscale=1.0, bs=bs)))
            out[case + '.keys'] = np.array(keys)
            out[case + '.shapes'] = np.array(['x'.join(str(d) for d in shapes[k]) for k in keys])
            out[case + '.checksums'] = su.checksums(state)
            out[case + '.x'] = x
        assert x.shape[0] == bu.BATCH[case], (case, x.shape)
        rec, floors = record(mod, kw, state, x)
        min_var = min(float(rec['var.' + n].min()) for n in bu.BN_NAMES)
        worst = max(floors, key=floors.get)
        print(f'{case}: minimum batch variance {min_var:.2e}, worst noise floor {worst} {floors[worst]:.2e}, '
              f'|logits|max {float(np.abs(rec["logits"]).max()):.3f}')
        assert min_var >= MIN_VAR, (case, min_var)
        assert floors[worst] < 0.5 * BOUND, (case, worst, floors[worst])
        if case in su.TRAIN_CASES:          # the same convention as the stored train-mode record
            d = float(np.abs(rec['logits'] - su.load_train(case)['logits']).max())
            print(f'{case}: train-mode logits vs sgn_train_{case}: {d:.2e}')
            assert d < 1e-5, d
        for k, v in rec.items():
            out[f'{case}.{k}'] = v
        out[case + '.floor'] = np.array(json.dumps(floors))
    path = os.path.join(HERE, 'sgn_bnstats.npz')
    np.savez_compressed(path, **out)
    print(f'{path}: {os.path.getsize(path)} bytes')
    assert os.path.getsize(path) < LIMIT


if __name__ == '__main__':
    main()
