"""Generate tests/golden/sgn15_evalgrad.npz by running the REFERENCE class (model/architecture/sgn/sgn_v15.py::SGN) on the
CPU: the eval-mode input gradient of the whole v15 model,

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_sgn_v15_grad.py

Per case of CASES: x, a cotangent ~ N(0, 1), the eval logits, grad_x = d sum(logits * cot) / dx by torch autograd in fp32
and in fp64, the key list, shapes and checksums of the state_dict (the parameters come from the seeded recipe
tests/sgn_v15_util.py::sgn15_state) and the meta.  Needs the reference checkout and einops.  Only data is stored.

A gradient is discontinuous where a ReLU or a maximum switches, so a seed is searched per case until, in fp64,
  (a) every x-dependent ReLU pre-activation of the model (found by hooks: a ReLU whose input moves with x) is at least
      MARGIN away from 0, and
  (b) every pooled column's top-1 minus top-2 gap, in both poolings, is at least MARGIN,
with MARGIN = max(2e-5, 4 x the reference's own fp32-vs-fp64 distance on that tensor), next to the three conditions of
make_golden_sgn_v15.py (attention maps neither one-hot nor flat -- the q/k scale moves the same way --, negative maxima,
fp32 headroom).  The distances, the margins found and the site count go into the meta."""
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
import make_golden_sgn_v15 as m15  # noqa: E402

sys.path.insert(0, mg.ROOT)
from tests import sgn_v15_util as vu  # noqa: E402

MARGIN_FLOOR = 2e-5
MAX_SITES = 60000
SEEDS = 100
# name: V, seg, bs, bias, spatial (heads, d_head, ff), temporal (heads, d_head, ff)
CASES = {
    'j15_seg4_deployed': (15, 4, 1, 1, (8, 16, 128), (8, 32, 256)),
    'j7_seg3_nobias': (7, 3, 2, 0, (4, 32, 128), (4, 64, 256)),
    'j5_seg3_sliced': (5, 3, 1, 1, (1, 256, 256), (1, 512, 512)),
    'j25_seg2_yaml': (25, 2, 1, 1, (1, 512, 512), (1, 1024, 1024)),            # the yaml's own heads
}


def switches(model, x):
    """-> {name: tensor}: the input of every ReLU module and of the two poolings in one eval forward."""
    seen, hooks = {}, []
    for name, m in model.named_modules():
        if isinstance(m, torch.nn.ReLU):
            hooks.append(m.register_forward_pre_hook(lambda mod, i, name=name: seen.__setitem__('relu:' + name, i[0])))
    hooks.append(model.smp.register_forward_pre_hook(lambda mod, i: seen.__setitem__('pool:smp', i[0])))
    hooks.append(model.tmp.register_forward_pre_hook(lambda mod, i: seen.__setitem__('pool:tmp', i[0])))
    with torch.no_grad():
        model(x)
    for h in hooks:
        h.remove()
    return seen


def margin(mod, kw, state, x):
    """-> (ok, {tensor: [required, found, fp32-vs-fp64 distance]}, x-dependent ReLU sites)."""
    model = mod.SGN(**kw)
    model.load_state_dict(vu.torch_state(state))
    model.eval()
    s32 = switches(model, x)
    other = switches(model, x.flip(1) * 1.5 + 0.25)                 # a ReLU whose input does not move is input independent
    model.double()
    s64 = switches(model, x.double())
    out, sites, ok = {}, 0, True
    for name, v in s64.items():
        if name.startswith('relu:'):
            if torch.equal(s32[name], other[name]):
                continue
            sites += v.numel()
            found = float(v.abs().min())
        else:                                                        # (bs, C, V, seg): smp pools V, tmp pools seg
            dim = 2 if name == 'pool:smp' else 3
            if v.shape[dim] < 2:
                continue
            top = v.topk(2, dim=dim).values
            found = float((top.select(dim, 0) - top.select(dim, 1)).min())
        dist = float((s32[name].double() - v).abs().max())
        need = max(MARGIN_FLOOR, 4 * dist)
        out[name] = [need, found, dist]
        ok = ok and found >= need
    return ok, out, sites


def gradient(mod, kw, state, x, cot, double):
    model = mod.SGN(**kw)
    model.load_state_dict(vu.torch_state(state))
    model.eval()
    if double:
        model, x, cot = model.double(), x.double(), cot.double()
    xg = x.clone().requires_grad_(True)
    logits, _ = model(xg)
    g, = torch.autograd.grad((logits * cot).sum(), xg)
    return logits.detach(), g


def main():
    mod = m15.load_reference_v15()[0]
    rec = {}
    for ci, (case, (V, seg, bs, bias, spatial, temporal)) in enumerate(CASES.items()):
        kw = vu.model_args(V, seg, bias, spatial, temporal)
        sd = mod.SGN(**kw).state_dict()
        keys = list(sd.keys())
        shapes = {k: tuple(t.shape) for k, t in sd.items()}
        for seed in range(21 + 100 * ci, 21 + 100 * ci + SEEDS):
            x = torch.from_numpy(ms.clip(np.random.default_rng(seed), bs, seg, V))
            scale = list(vu.QK_SCALE)
            for _ in range(12):                              # as the forward maker: a block's scale moves with its map
                state = vu.sgn15_state(shapes, seed, tuple(scale))
                ok, out, measured = m15.measure(mod, kw, state, x)
                moved = False
                for b, k in enumerate(('spatial_attn', 'temporal_attn')):
                    r = measured['rowmax'][k]
                    if not ok and (r < 0.25 or r > 0.75):
                        scale[b] = scale[b] * 1.5 if r < 0.25 else scale[b] / 1.5
                        moved = True
                if ok or not moved:
                    break
            if ok:
                ok, margins, sites = margin(mod, kw, state, x)
            if ok:
                break
            print(f'{case}: seed {seed} rejected', flush=True)
        else:
            raise SystemExit(f'{case}: no seed of {SEEDS} meets the conditions')
        assert sites <= MAX_SITES, (case, sites)
        cot = torch.from_numpy(np.random.default_rng([seed, 7]).standard_normal((bs, vu.NUM_CLASS)).astype(np.float32))
        logits, g32 = gradient(mod, kw, state, x, cot, False)
        _, g64 = gradient(mod, kw, state, x, cot, True)
        fp32 = float((g32.double() - g64).abs().max()) / vu.bound(g64.numpy())
        meta = dict(case=case, seed=seed, bs=bs, model_args=kw, qk_scale=scale, sites=sites, margins=margins,
                    margin=min(v[1] for v in margins.values()), grad_fp32_in_bounds=fp32, **measured)
        one = dict(meta=np.array(json.dumps(meta)), x=x.numpy(), cot=cot.numpy(), logits=logits.numpy(),
                   grad_x=g32.numpy(), grad_x64=g64.numpy())
        vu.pack_state(one, state, keys)
        rec.update({f'{case}.{k}': v for k, v in one.items()})
        print(f'{case}: seed {seed}, scales {scale}, {sites} sites, smallest distance to a switch {meta["margin"]:.2e}, '
              f'fp32 autograd at {fp32:.3f} of the bound', flush=True)
    path = os.path.join(HERE, 'sgn15_evalgrad.npz')
    np.savez_compressed(path, **rec)
    assert os.path.getsize(path) < m15.LIMIT, os.path.getsize(path)
    print(f'{path}: {os.path.getsize(path) >> 10} KiB')


if __name__ == '__main__':
    torch.manual_seed(0)
    main()
