"""Generate tests/golden/sgn_evalgrad.npz by running the REFERENCE SGN (model/architecture/sgn/archiv/sgn.py) on the CPU
in eval mode:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_sgn_grad.py

Per case: meta, the key list, shapes and checksums of the state_dict (the parameters come from the seeded recipe
tests/sgn_util.py::sgn_state), x, a cotangent c ~ N(0, 1), the eval logits and g, and the gradient of sum(logits * c) with
respect to x from the reference in fp32 (grad_x) and in fp64 (grad_x64).  The gap between the two is the reference's own
noise floor.  Only data is stored.

The margin condition.  A gradient is discontinuous where a ReLU or a maximum switches: one flipped unit moves dx by far
more than any tolerance.  So the seed of every case is searched: seeds SEED0, SEED0 + 1, ... (at most SEEDS of them), the
first whose fp64 forward keeps every ReLU pre-activation at least MARGIN away from 0 and, in both maxima (over the joints,
over the frames), the top-1 minus top-2 gap at least MARGIN wherever top-1 > 0.  The margin found is stored and asserted.
MARGIN is a condition on the fixture, not a tolerance of any comparison.

Needs the reference checkout."""
import json
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

import make_golden as mg  # noqa: E402
import make_golden_sgn as ms  # noqa: E402

sys.path.insert(0, mg.ROOT)
from tests import sgn_grad_util as gu  # noqa: E402
from tests import sgn_util as su  # noqa: E402

MARGIN = 2e-5
SEED0, SEEDS = 3000, 150
NUM_CLASS = 60
MAX_SITES = 175_000          # ReLU sites that depend on x (the search gets hopeless beyond)

CASES = [
    # name, V, seg, bs, bias, kind
    ('v25_seg2', 25, 2, 1, True, 'plain'),           # odd V: Kg = 26, 25 real rows of 32
    ('v15_seg6', 15, 6, 1, True, 'plain'),           # the deployed skeleton
    ('v7_seg12_nobias', 7, 12, 2, False, 'plain'),   # no bias; a clip boundary for the dif term
    ('v2_seg40', 2, 40, 1, True, 'plain'),           # two tiles and a halo in the clip kernel
    ('v3_seg34', 3, 34, 1, True, 'plain'),           # a second tile of two frames
    ('v15_seg3_guard', 15, 3, 1, True, 'guard'),     # padded joint rows hold large positive values
    ('v15_seg4_sharp', 15, 4, 1, True, 'sharp'),     # softmax logits near 30
]
assert tuple(c[0] for c in CASES) == gu.GRAD_CASES + gu.OPTIONAL_GRAD_CASES


def to_double(model):
    model.double()
    model.spa, model.tem = model.spa.double(), model.tem.double()       # plain attributes in the reference
    return model


class Margins:
    """Forward hooks on every nn.ReLU (minimum |pre-activation|) and on the inputs of both maxima (minimum top-1 minus
    top-2 gap over the pooled positions, where top-1 > 0)."""

    def __init__(self, model):
        self.relu, self.gap, self.sites, self.handles = np.inf, np.inf, 0, []
        for name, m in model.named_modules():
            if isinstance(m, nn.ReLU):
                m.counted = not name.startswith(('tem_embed', 'spa_embed'))     # input independent: checked, not counted
                self.handles.append(m.register_forward_hook(self.on_relu))
        # the maximum over the joints is judged on gcn3's output (bs, C, V, seg): local.maxpool sees it shifted by tem1
        # (sgn.py:89), the same for every joint, so where all joints are dead (0) its input ties at tem1 > 0 -- a tie at
        # which nothing flows.  The maximum over the frames (bs, C, 1, seg) -> (1, 1) is judged on its own input.
        self.handles.append(model.gcn3.register_forward_hook(lambda m, i, o: self.on_max(o.detach().permute(0, 1, 3, 2))))
        self.handles.append(model.maxpool.register_forward_hook(lambda m, i, o: self.on_max(i[0].detach().flatten(2))))

    def on_relu(self, m, inp, out):
        self.relu = min(self.relu, float(inp[0].detach().abs().min()))
        self.sites += inp[0].numel() if m.counted else 0

    def on_max(self, pooled):
        if pooled.shape[-1] < 2:
            return
        top = torch.topk(pooled, 2, dim=-1).values
        gap = (top[..., 0] - top[..., 1])[top[..., 0] > 0]
        if gap.numel():
            self.gap = min(self.gap, float(gap.min()))

    def close(self):
        for h in self.handles:
            h.remove()
        return min(self.relu, self.gap)


def candidate(mod, name, v, seg, bs, bias, kind, seed):
    """-> (margin, sites, model fp32 in eval mode, x, meta, state, shapes, keys) of one seed."""
    kw = dict(num_class=NUM_CLASS, num_point=v, in_channels=3, seg=seg, bias=bias)
    model = ms.build(mod, **kw)
    sd = model.state_dict()
    keys = list(sd.keys())
    shapes = {k: tuple(t.shape) for k, t in sd.items()}
    x = ms.clip(np.random.default_rng(seed), bs, seg, v)
    gscale = 1.0
    if kind == 'sharp':
        model.load_state_dict(su.torch_state(su.sgn_state(shapes, seed)))
        model.eval()
        gscale = float(np.sqrt(30.0 / ms.g3_max(model, torch.from_numpy(x))))
    meta = dict(kw, seed=seed, gscale=gscale, bs=bs, kind=kind)
    state = su.sgn_state(shapes, seed, gscale)
    x = gu.case_input(x, meta)
    model.load_state_dict(su.torch_state(gu.case_state(state, meta)))
    model.eval()
    if kind == 'sharp':
        m = ms.g3_max(model, torch.from_numpy(x))
        assert 25.0 < m < 35.0, m
    hooks = Margins(to_double(model))
    with torch.no_grad():
        model(torch.from_numpy(x).double())
    margin = hooks.close()
    model.float()
    model.spa, model.tem = model.spa.float(), model.tem.float()
    return margin, hooks.sites, model, x, meta, state, shapes, keys


def gradient(model, x, c):
    xg = x.clone().requires_grad_(True)
    logits, g = model(xg)
    (logits * c).sum().backward()
    return logits.detach(), g.detach(), xg.grad


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    mod = ms.load_reference_sgn()[0]
    out = {}
    for name, v, seg, bs, bias, kind in CASES:
        found = None
        for seed in range(SEED0, SEED0 + SEEDS):
            margin, sites, model, x, meta, state, shapes, keys = candidate(mod, name, v, seg, bs, bias, kind, seed)
            assert sites <= MAX_SITES, (name, sites)
            if margin >= MARGIN:
                found = seed
                break
        if found is None:
            assert name in gu.OPTIONAL_GRAD_CASES, f'{name}: no seed in [{SEED0}, {SEED0 + SEEDS}) reaches the margin'
            print(f'{name}: no seed in [{SEED0}, {SEED0 + SEEDS}) reaches the margin; left out')
            continue
        assert margin >= MARGIN
        c = np.random.default_rng(found + 50).standard_normal((bs, NUM_CLASS)).astype(np.float32)
        xt, ct = torch.from_numpy(x), torch.from_numpy(c)
        logits, g, grad = gradient(model, xt, ct)
        _, _, grad64 = gradient(to_double(model), xt.double(), ct.double())
        floor = float((grad.double() - grad64).abs().max() / max(1.0, float(grad64.abs().max())))
        meta.update(margin=margin, sites=sites)
        out[name + '.meta'] = np.array(json.dumps(meta))
        out[name + '.keys'] = np.array(keys)
        out[name + '.shapes'] = np.array(['x'.join(str(d) for d in shapes[k]) for k in keys])
        out[name + '.checksums'] = su.checksums(state)
        out[name + '.x'], out[name + '.c'] = x, c
        out[name + '.logits'], out[name + '.g'] = logits.numpy(), g.numpy()
        out[name + '.grad_x'], out[name + '.grad_x64'] = grad.numpy(), grad64.numpy()
        print(f'{name}: seed {found}, {sites} sites, margin {margin:.2e}, max|dx| {float(grad64.abs().max()):.1f}, '
              f'fp32 vs fp64 reference {floor:.2e}')
    path = os.path.join(HERE, 'sgn_evalgrad.npz')
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < ms.LIMIT
    print(f'{path}: {os.path.getsize(path)} bytes')


if __name__ == '__main__':
    main()
