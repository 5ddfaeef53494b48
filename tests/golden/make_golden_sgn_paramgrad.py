"""Generate tests/golden/sgn_paramgrad_<case>.npz by running the REFERENCE SGN (model/architecture/sgn/archiv/sgn.py) on
the CPU in eval mode:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_sgn_paramgrad.py

The cases are those of sgn_evalgrad.npz exactly as tests/sgn_grad_util.py::load_grad_case rebuilds them (same seeds, x,
cotangent c and state; their ReLU / maximum margins are established there).  Per case the reference's logits are asserted
to equal the stored ones, and sum(logits * c) is backpropagated to every parameter in fp32 and in fp64.

Stored per parameter tensor (only data; one file per case, each below 1 MiB):
  full.<key>   the fp32 gradient, for tensors of at most FULL elements
  samp.<key>   SAMPLES entries of the flat fp32 gradient at the indices tests/sgn_wgrad_util.py::sample_index draws from
               the stored seed, plus rows.<key> / cols.<key>: the fp64 row and column sums of its (shape[0], -1) view
  max.<key>    max |gradient| in fp64;  floor.<key>  max |fp32 - fp64| / max(1, max |fp64|), the reference's own noise
The generator asserts floor < FLOOR_LIMIT for every tensor: a condition on the fixture (half the tests' bound).

Needs the reference checkout."""
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
import make_golden_sgn_grad as mgg  # noqa: E402

sys.path.insert(0, mg.ROOT)
from tests import sgn_grad_util as gu  # noqa: E402
from tests import sgn_util as su  # noqa: E402
from tests import sgn_wgrad_util as wu  # noqa: E402


def gradients(model, x, c):
    model.zero_grad(set_to_none=True)
    logits, _ = model(x)
    (logits * c).sum().backward()
    return logits.detach(), {k: p.grad.detach().clone() for k, p in model.named_parameters()}


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    mod = ms.load_reference_sgn()[0]
    for case in gu.stored_cases():
        d = gu.load_grad_case(case)
        model = ms.build(mod, **su.model_args(d['meta']))
        model.load_state_dict(su.torch_state(d['state']))
        model.eval()
        x, c = torch.from_numpy(d['x']), torch.from_numpy(d['c'])
        logits, g32 = gradients(model, x, c)
        assert np.array_equal(logits.numpy(), d['logits']), f'{case}: the reference no longer reproduces the stored logits'
        _, g64 = gradients(mgg.to_double(model), x.double(), c.double())
        out = {'meta': np.array(json.dumps(dict(d['meta'], index_seed=wu.INDEX_SEED))), 'keys': np.array(sorted(g32))}
        worst = (0.0, '')
        for k in sorted(g32):
            a, b = g32[k].numpy(), g64[k].numpy()
            scale = max(1.0, float(np.abs(b).max()))
            floor = float(np.abs(a.astype(np.float64) - b).max() / scale)
            assert floor < wu.FLOOR_LIMIT, (case, k, floor)
            worst = max(worst, (floor, k))
            out['max.' + k], out['floor.' + k] = np.float64(np.abs(b).max()), np.float64(floor)
            if a.size <= wu.FULL:
                out['full.' + k] = a
            else:
                out['samp.' + k] = a.reshape(-1)[wu.sample_index(k, a.size)]
                m = a.reshape(a.shape[0], -1).astype(np.float64)
                out['rows.' + k], out['cols.' + k] = m.sum(1), m.sum(0)
        path = os.path.join(HERE, f'sgn_paramgrad_{case}.npz')
        np.savez_compressed(path, **out)
        assert os.path.getsize(path) < ms.LIMIT, (path, os.path.getsize(path))
        print(f'{case}: {len(g32)} tensors, largest |grad| {max(float(out["max." + k]) for k in g32):.1f}, '
              f'worst fp32 vs fp64 {worst[0]:.2e} ({worst[1]}), {os.path.getsize(path)} bytes')


if __name__ == '__main__':
    main()
