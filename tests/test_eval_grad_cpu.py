"""CPU side of the eval-mode (frozen BatchNorm statistics) backward:
* header, binding table and library exports carry the new entry points, and reject bad arguments on the host;
* the oracle's eval-mode gradients reproduce fixtures generated from the REFERENCE in ``.eval()`` with gradients
  enabled (tests/golden/make_golden_evalgrad.py): outputs at 2e-5, gradients at 1e-4, as test_oracle_golden.py does;
* the seeds of the GPU cases (tests/evalgrad_util.py): the oracle run in fp32 with its ReLU patterns pinned stays inside
  the stated tolerances of its own fp64 run, so a correct fp32 implementation can pass them."""
import ctypes
import re

import numpy as np
import pytest
import torch

from oracle import agcn_oracle as orc
from tests import evalgrad_util as eg
from tests import golden_util as gu
from tests.test_cabi import ROOT, header_symbols

NEW = ('agcn_bn_bwd_eval', 'agcn_bn_bwd_eval_finalize', 'agcn_bn_eval_coeff_ex')
TOL = 2e-5


def test_new_entry_points_in_header_binding_and_library():
    import agcn_amd  # noqa: F401
    from agcn_amd import lib
    handle = ctypes.CDLL(lib.LIB_PATH)
    for name in NEW:
        assert name in header_symbols(), name
        assert name in lib.SIGNATURES, name
        assert hasattr(handle, name), name
    src = open(ROOT + '/2s-agcn_amd/ops.py').read()
    assert not re.search(r'\b_need_train\b', src)


def test_argument_errors():
    """Null or non-positive arguments are rejected on the host before any launch (no device needed)."""
    import agcn_amd  # noqa: F401
    from agcn_amd import lib
    L = lib.load()
    p = ctypes.addressof(ctypes.create_string_buffer(64))       # any non-null address: never dereferenced on an error
    ERR = -1
    ok = dict(dout=p, mask=None, bits=0, y1=p, s1=p, y2=None, s2=None, sums=1, part=p, dy1=p, dy2=None, amax=None,
              N=1, C=1, P=1)

    def call(**kw):
        a = dict(ok, **kw)
        return L.agcn_bn_bwd_eval(a['dout'], a['mask'], a['bits'], a['y1'], a['s1'], a['y2'], a['s2'], a['sums'],
                                  a['part'], a['dy1'], a['dy2'], a['amax'], a['N'], a['C'], a['P'], None)
    for kw in (dict(dout=None), dict(s1=None), dict(dy1=None), dict(N=0), dict(C=0), dict(P=-3),
               dict(y1=None), dict(part=None),                  # the sums need y1 and the slab
               dict(s2=p), dict(s2=p, dy2=p)):                  # branch 2 needs dy2, and y2 for the sums
        assert call(**kw) == ERR, kw
    fin = [p, 1, 1, p, p, p, None, None, None, p, p, None, None, None, None, None]
    for i, bad in ((0, None), (1, 0), (2, 0), (3, None), (4, None), (5, None), (9, None), (10, None)):
        a = list(fin)
        a[i] = bad
        assert L.agcn_bn_bwd_eval_finalize(*a) == ERR, i
    a = list(fin)
    a[6] = p                                                    # branch 2 without its statistics / outputs
    assert L.agcn_bn_bwd_eval_finalize(*a) == ERR
    co = [p, p, p, p, 1e-5, 1, p, p, p, p, None]
    for i in (0, 1, 2, 3, 6, 7, 8, 9):
        a = list(co)
        a[i] = None
        assert L.agcn_bn_eval_coeff_ex(*a) == ERR, i
    a = list(co)
    a[5] = 0
    assert L.agcn_bn_eval_coeff_ex(*a) == ERR


EG_FIXTURES = ['eg_u_64_64_s1_v25', 'eg_u_64_128_s2_v18_oddT', 'eg_au_64_64_s1_v25']


@pytest.mark.parametrize('name', EG_FIXTURES)
def test_oracle_eval_backward_matches_reference(name):
    gold = dict(np.load(f'{gu.GOLDEN}/{name}.npz'))
    cin, cout, stride, residual, t, v, seed, n = [int(i) for i in gold['meta']]
    aagcn = name.startswith('eg_au')
    if aagcn:
        shapes = orc.aagcn_unit_param_shapes('', cin, cout, v, stride, bool(residual), True, True, None)
        sd0 = orc.aagcn_randomized_state(shapes, seed, stress=float(gold['meta.stress']))
    else:
        sd0 = orc.randomized_state(orc.unit_param_shapes('', cin, cout, v, stride, bool(residual)), seed,
                                   stress=float(gold['meta.stress']))
    A = gu.graph_A(v)
    xn, rn = gu.unit_inputs(cin, cout, stride, t, v, seed, n=n)
    for dtype, sfx, pfx in ((torch.float32, '', 'g.'), (torch.float64, '64', 'g64.')):
        sd = orc.with_grad({k: (v_.to(dtype) if v_.is_floating_point() else v_) for k, v_ in sd0.items()})
        for k in list(sd):
            if gu.is_alias_key(k):
                sd[k] = sd[gu.canonical_key(k)]
        x = torch.from_numpy(xn).to(dtype).requires_grad_(True)
        if aagcn:
            y = orc.aagcn_unit_forward(x, sd, '', None, stride, bool(residual), training=False)
        else:
            y = orc.tcn_gcn_unit_forward(x, sd, '', A.to(dtype), stride, bool(residual), training=False)
        (y * torch.from_numpy(rn).to(dtype)).sum().backward()
        assert gu.rel_err(y.detach().numpy(), gold['y_eval' + sfx]) < TOL, (name, sfx)
        assert gu.rel_err(x.grad.numpy(), gold['dx' + sfx]) < TOL * max(1.0, np.abs(gold['dx' + sfx]).max()), (name, sfx)
        nonzero_bias = 0
        for k, p in sd.items():
            if orc.is_buffer(k) or gu.is_alias_key(k):
                continue
            if eg.is_conv_a_bias(k):          # structurally zero in either mode (the softmax cancels it)
                assert float(p.grad.abs().max()) < 1e-4 * max(1.0, float(np.abs(gold['dx']).max())), k
                continue
            assert gu.grad_err(p.grad.numpy(), gold, k, prefix=pfx) < 1e-4, (k, sfx)
            if eg.is_bn_conv_bias(k):         # NOT zero in eval mode, in the reference either
                assert float(gold[pfx + k + '.absmax']) > 1e-2 and float(p.grad.abs().max()) > 1e-2, k
                nonzero_bias += 1
        assert nonzero_bias >= 4, nonzero_bias


@pytest.mark.parametrize('name', list(eg.CASES))
def test_seeds_leave_room_for_fp32(name):
    """The oracle in fp32, with the ReLU patterns of its fp64 run pinned, against that fp64 run, on the criteria the
    GPU tests assert: if this failed, no fp32 implementation could be expected to pass the case."""
    torch.set_num_threads(min(8, torch.get_num_threads()))
    sd0, xn, rn = eg.state_and_inputs(name)
    masks = eg.oracle_own_masks(name, sd0, xn)
    ref = eg.oracle_run(name, sd0, xn, rn, masks, torch.float64)
    y, dx, grads = eg.oracle_run(name, sd0, xn, rn, masks, torch.float32)
    bad, rec = eg.compare(name, y.numpy(), dx.numpy(), {k: g.numpy() for k, g in grads.items()}, ref)
    print(name, 'worst', max(rec.items(), key=lambda kv: kv[1]))
    assert not bad, bad[:6]
    # the conv biases in front of the frozen BatchNorms have real gradients
    nz = [k for k in ref[2] if eg.is_bn_conv_bias(k) or k == 'conv.bias']
    assert nz and all(float(ref[2][k].abs().max()) > 1e-3 for k in nz), nz
