"""GPU checks of the two SGN v15 kernels (csrc/sgn_v15.hip), each ALONE, over the domain table of
tests/sgn_v15_domain_util.py against the fp64 tensor reference on seeded weight images: no model, no fixture.

  frames kernel   ``ops.sgn15_frames`` on x            vs the reference's feat and spatial map
  clip kernel     ``ops.sgn15_clip`` on the REFERENCE's feat rounded to fp32
                                                       vs the reference's logits and temporal map from that same input

so the clip kernel's verdict holds no frames-side error.  Bound: the project's fp32 rule per tensor, 1e-4 relative to
max(1, max|reference tensor|); the printed ratios are multiples of that bound (measured on MI355X:
profiles/sgn_v15_domain.txt).  What makes these inputs able to show an error is asserted in
tests/test_sgn_v15_domain_cpu.py."""
import pytest
import torch

from tests import sgn_v15_domain_util as du

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
CASE_IDS = list(range(len(du.CASES)))


def _maps(name, attn, ref, shape):
    """The checks every stored map gets; -> its ratio."""
    assert tuple(attn.shape) == tuple(ref.shape) == shape, (name, tuple(attn.shape), shape)      # real rows only: no padded entries exist
    assert bool(torch.isfinite(attn).all()), name
    rowsum = float((attn.double().sum(-1) - 1).abs().max())
    assert rowsum <= 1e-5, (name, rowsum)
    return du.check(attn, ref)


@pytest.mark.parametrize('i', CASE_IDS, ids=du.IDS)
def test_frames_kernel_alone(i):
    import agcn_amd  # noqa: F401
    from agcn_amd import ops
    V, seg, sp, _, _ = du.CASES[i]
    d = du.load(i)
    N = d['x'].shape[0]
    x, wf = d['x'].to(DEV), d['wf'].to(DEV)
    feat, attn = ops.sgn15_frames(x, wf, V, *sp, want_attn=True)
    assert tuple(feat.shape) == (N, seg, 256) and bool(torch.isfinite(feat).all())
    r = dict(feat=du.check(feat, d['feat']), spatial_attn=_maps('spatial_attn', attn, d['spatial_attn'], (N * seg, sp[0], V, V)))
    print(f'case {i} frames fused vs fp64, in bounds: ' + ' '.join(f'{k} {v:.3e}' for k, v in r.items()))
    assert all(v <= 1.0 for v in r.values()), r
    # the same bits without the maps, and for clip 1 alone
    quiet, none = ops.sgn15_frames(x, wf, V, *sp, want_attn=False)
    assert none is None and torch.equal(quiet, feat)
    alone, alone_attn = ops.sgn15_frames(x[1:2].contiguous(), wf, V, *sp, want_attn=True)
    assert torch.equal(alone[0], feat[1]) and torch.equal(alone_attn, attn[seg:2 * seg])


@pytest.mark.parametrize('i', CASE_IDS, ids=du.IDS)
def test_clip_kernel_alone(i):
    import agcn_amd  # noqa: F401
    from agcn_amd import ops
    _, seg, _, tp, num_class = du.CASES[i]
    d = du.load(i)
    N = d['feat32'].shape[0]
    feat, wc = d['feat32'].to(DEV), d['wc'].to(DEV)
    logits, attn = ops.sgn15_clip(feat, wc, num_class, *tp, want_attn=True)
    assert tuple(logits.shape) == (N, num_class) and bool(torch.isfinite(logits).all())
    r = dict(logits=du.check(logits, d['clip']['logits']),
             temporal_attn=_maps('temporal_attn', attn, d['clip']['attn'], (N, tp[0], seg, seg)))
    print(f'case {i} clip fused vs fp64, in bounds: ' + ' '.join(f'{k} {v:.3e}' for k, v in r.items()))
    assert all(v <= 1.0 for v in r.values()), r
    if seg == 1:
        assert bool((attn == 1.0).all())                 # a single frame attends to itself, exactly
    quiet, none = ops.sgn15_clip(feat, wc, num_class, *tp, want_attn=False)
    assert none is None and torch.equal(quiet, logits)
    alone, alone_attn = ops.sgn15_clip(feat[1:2].contiguous(), wc, num_class, *tp, want_attn=True)
    assert torch.equal(alone[0], logits[1]) and torch.equal(alone_attn[0], attn[1])
