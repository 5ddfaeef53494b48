"""Generate tests/golden/sgn15_paramgrad_<case>.npz by running the REFERENCE class (model/architecture/sgn/sgn_v15.py::SGN)
on the CPU in eval mode:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_sgn_v15_paramgrad.py

The cases are the four GRAD_CASES of sgn15_evalgrad.npz exactly as tests/sgn_v15_grad_util.py::load_grad_case rebuilds them
(same seeds, x, cotangent and state; their ReLU / maximum margins are established by make_golden_sgn_v15_grad.py).  Per
case the reference's logits are asserted to equal the stored ones, and sum(logits * cot) is backpropagated to every
parameter in fp32 and in fp64.

Stored per parameter tensor, in the scheme of make_golden_sgn_paramgrad.py (only data; one file per case, each below
1 MiB), from the fp64 gradient (entries rounded to fp32 for storage):
  full.<key>   the gradient, for tensors of at most FULL elements
  samp.<key>   SAMPLES entries of the flat gradient at the indices tests/sgn_wgrad_util.py::sample_index draws from the
               stored seed, plus rows.<key> / cols.<key>: the fp64 row and column sums of its (shape[0], -1) view
  max.<key>    max |gradient| in fp64;  floor.<key>  max |fp32 - fp64| / max(1, max |fp64|), the reference's own noise
The generator asserts floor < FLOOR_LIMIT (half the tests' bound) for every tensor: a condition on the fixture.

Needs the reference checkout and einops."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

import make_golden as mg  # noqa: E402
import make_golden_sgn_v15 as m15  # noqa: E402

sys.path.insert(0, mg.ROOT)
from tests import sgn_v15_grad_util as gu  # noqa: E402
from tests import sgn_v15_util as vu  # noqa: E402
from tests import sgn_v15_wgrad_util as wg  # noqa: E402
from tests import sgn_wgrad_util as wu  # noqa: E402


def gradients(mod, kw, state, x, cot, double):
    model = mod.SGN(**kw)
    model.load_state_dict(vu.torch_state(state))
    model.eval()
    if double:
        model, x, cot = model.double(), x.double(), cot.double()
    logits, _ = model(x)
    (logits * cot).sum().backward()
    return logits.detach(), {k: p.grad.detach().clone() for k, p in model.named_parameters()}


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    mod = m15.load_reference_v15()[0]
    for case in gu.GRAD_CASES:
        d = gu.load_grad_case(case)
        kw = d['meta']['model_args']
        x, cot = torch.from_numpy(d['x']), torch.from_numpy(d['cot'])
        logits, g32 = gradients(mod, kw, d['state'], x, cot, False)
        assert np.array_equal(logits.numpy(), d['logits']), f'{case}: the reference no longer reproduces the stored logits'
        _, g64 = gradients(mod, kw, d['state'], x, cot, True)
        out = {'meta': np.array(json.dumps(dict(d['meta'], index_seed=wg.INDEX_SEED))), 'keys': np.array(sorted(g32))}
        worst = (0.0, '')
        for k in sorted(g32):
            a, b = g32[k].numpy(), g64[k].numpy()
            scale = max(1.0, float(np.abs(b).max()))
            floor = float(np.abs(a.astype(np.float64) - b).max() / scale)
            assert floor < wu.FLOOR_LIMIT, (case, k, floor)
            worst = max(worst, (floor, k))
            out['max.' + k], out['floor.' + k] = np.float64(np.abs(b).max()), np.float64(floor)
            if b.size <= wg.FULL:
                out['full.' + k] = b.astype(np.float32)
            else:
                out['samp.' + k] = b.reshape(-1)[wg.sample_index(k, b.size, wg.INDEX_SEED)].astype(np.float32)
                m = b.reshape(b.shape[0], -1)
                out['rows.' + k], out['cols.' + k] = m.sum(1), m.sum(0)
        path = os.path.join(HERE, wg.fixture_name(case))
        np.savez_compressed(path, **out)
        assert os.path.getsize(path) < m15.LIMIT, (path, os.path.getsize(path))
        print(f'{case}: {len(g32)} tensors, largest |grad| {max(float(out["max." + k]) for k in g32):.1f}, '
              f'worst fp32 vs fp64 {worst[0]:.2e} ({worst[1]}), {os.path.getsize(path)} bytes')


if __name__ == '__main__':
    main()
