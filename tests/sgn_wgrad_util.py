"""Shared by the SGN parameter-gradient tests and tests/golden/make_golden_sgn_paramgrad.py: the fixture format, its
loader, and the comparison of a {name: gradient} dict against a fixture.

The bound is the project's SGN bound: 1e-4 relative to max(1, max |reference tensor|), per tensor (``BOUND``).  Tensors of
more than ``FULL`` elements are stored as ``SAMPLES`` sampled entries (compared at that bound on the tensor's own scale)
plus the row and column sums of their (shape[0], -1) view.  A sum of n entries that are each within b of the reference is
within n * b of the reference's sum (triangle inequality), so that is the bound of a sum over n entries: it follows from
the per-entry bound and asks nothing the per-entry bound does not imply, yet sees a single wrong entry outside the sample
once it is off by more than n * b."""
import json
import zlib

import numpy as np

from tests import sgn_grad_util as gu
from tests import sgn_util as su

BOUND = 1e-4
FLOOR_LIMIT = 5e-5           # the reference's own fp32-vs-fp64 distance, asserted by the generator for every tensor
FULL = 4096
SAMPLES = 4096
INDEX_SEED = 7100


def sample_index(key, numel, seed=INDEX_SEED):
    """The flat indices of the stored samples of tensor ``key`` (with replacement; a function of the seed and the name)."""
    return np.random.default_rng([seed, zlib.crc32(key.encode())]).integers(0, numel, SAMPLES)


def fixture_name(case):
    return f'sgn_paramgrad_{case}.npz'


def load_paramgrad(case):
    """-> dict(meta, keys, full {key: array}, samp / rows / cols {key: array}, max {key: float}, floor {key: float})."""
    f = su._npz(fixture_name(case))
    meta = json.loads(str(f['meta']))
    keys = [str(k) for k in f['keys']]
    pick = lambda p: {k: f[p + k] for k in keys if p + k in f}  # noqa: E731
    return dict(meta=meta, keys=keys, full=pick('full.'), samp=pick('samp.'), rows=pick('rows.'), cols=pick('cols.'),
                max={k: float(v) for k, v in pick('max.').items()}, floor={k: float(v) for k, v in pick('floor.').items()})


def build_model(case, device=None):
    """-> (model in eval mode with the case's state, x, c as torch tensors, the evalgrad case dict)."""
    import torch
    from agcn_amd.model.sgn import SGN
    d = gu.load_grad_case(case)
    model = SGN(**su.model_args(d['meta']))
    model.load_state_dict(su.torch_state(d['state']))
    model.eval()
    x, c = torch.from_numpy(d['x']), torch.from_numpy(d['c'])
    if device is not None:
        model, x, c = model.to(device), x.to(device), c.to(device)
    return model, x, c, d


def compare(grads, fix, what=''):
    """grads {name: tensor or array} against a loaded fixture -> (worst relative error, its name, the floor of that
    tensor); asserts that every parameter of the fixture is present with its shape and within the bound.  Relative =
    divided by max(1, max |reference tensor|) (and by n for a sum over n entries, see the module docstring)."""
    assert sorted(grads) == sorted(fix['keys']), (sorted(set(grads) ^ set(fix['keys'])), what)
    worst = (0.0, '', 0.0)
    for k in fix['keys']:
        a = np.asarray(grads[k].detach().cpu() if hasattr(grads[k], 'detach') else grads[k])
        scale = max(1.0, fix['max'][k])
        errs = []
        if k in fix['full']:
            assert a.shape == fix['full'][k].shape, (k, a.shape, what)
            errs.append(np.abs(a.astype(np.float64) - fix['full'][k]).max() / scale)
        else:
            m = a.reshape(a.shape[0], -1).astype(np.float64)
            assert m.shape == (fix['rows'][k].size, fix['cols'][k].size), (k, a.shape, what)
            errs.append(np.abs(a.reshape(-1)[sample_index(k, a.size, fix['meta']['index_seed'])] - fix['samp'][k]).max() / scale)
            errs.append(np.abs(m.sum(1) - fix['rows'][k]).max() / (scale * m.shape[1]))
            errs.append(np.abs(m.sum(0) - fix['cols'][k]).max() / (scale * m.shape[0]))
        err = float(max(errs))
        assert np.isfinite(a).all(), (k, what)
        worst = max(worst, (err, k, fix['floor'][k]))
        assert err < BOUND, f'{what} {k}: {err:.2e} relative to max(1, {fix["max"][k]:.3g}) (reference floor {fix["floor"][k]:.1e})'
    return worst
