"""Kernel-level parity of the eval-mode (frozen statistics) BatchNorm backward -- ``agcn_bn_bwd_eval`` and
``agcn_bn_bwd_eval_finalize`` through ``ops.bn_bwd_eval`` -- against plain fp64 tensor maths.  GPU only.

Criterion: the one ``tests/test_gpu_kernels.py::test_bn_act_fwd_bwd`` applies to ``agcn_bn_bwd`` at these sizes:
max|a-ref| / max(1, max|ref|) < 1e-4 for the activation-sized gradients and < 5e-4 for the per-channel vectors (the
bias-gradient vectors are per-channel vectors of the same kind as dbeta)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
TOL = 1e-4
EPS = 1e-5

# (T, V): P = 75 (P % 4 != 0, misaligned rows), 18, 1125 (more than one sweep of the workgroup, P % 4 = 1), 1024
ROWS = [(3, 25), (1, 18), (45, 25), (32, 32)]
SHAPES = [(N, C, T, V) for N in (1, 3) for C in (1, 5, 64) for (T, V) in ROWS]


def _gpu():
    import agcn_amd  # noqa: F401
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device('cuda:0')


def rel(a, ref):
    a = a.detach().double().cpu()
    ref = ref.detach().double().cpu()
    return float((a - ref).abs().max() / max(1.0, float(ref.abs().max())))


def _case(shape, two, seed):
    """fp64 inputs and the fp64 reference of one stage out = relu(bn1(y1) [+ bn2(y2)]) at frozen statistics."""
    N, C, T, V = shape
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    d = dict(y1=r(N, C, T, V) * 1.5 + 0.3, y2=r(N, C, T, V), dout=r(N, C, T, V))
    for k in ('1', '2'):       # running statistics away from (0, 1)
        d['g' + k], d['b' + k] = r(C) * 0.3 + 1, r(C) * 0.1
        d['rm' + k], d['rv' + k] = r(C) * 0.5, torch.rand(C, generator=g, dtype=torch.float64) * 1.5 + 0.25
    # the values the kernels see are the fp32 roundings
    d = {k: v.float().double() for k, v in d.items()}
    d['two'] = two
    return d


def _reference(d, masked):
    """Autograd in fp64 through the explicit conv-bias form z = g*(y + cb - rm)*invstd + b with cb = 0, so that the
    gradient of the bias of the convolution in front of each BatchNorm comes out of the same graph."""
    leaves = {k: d[k].clone().requires_grad_(True) for k in ('y1', 'y2', 'g1', 'b1', 'g2', 'b2')}
    C = d['g1'].numel()
    cb1 = torch.zeros(C, dtype=torch.float64, requires_grad=True)
    cb2 = torch.zeros(C, dtype=torch.float64, requires_grad=True)
    v = lambda t: t.view(1, -1, 1, 1)  # noqa: E731
    z = v(leaves['g1']) * (leaves['y1'] + v(cb1) - v(d['rm1'])) / torch.sqrt(v(d['rv1']) + EPS) + v(leaves['b1'])
    if d['two']:
        z = z + v(leaves['g2']) * (leaves['y2'] + v(cb2) - v(d['rm2'])) / torch.sqrt(v(d['rv2']) + EPS) + v(leaves['b2'])
    out = torch.relu(z) if masked else z
    out.backward(d['dout'])
    ref = {k: t.grad for k, t in leaves.items()}
    ref['cb1'], ref['cb2'] = cb1.grad, cb2.grad
    return out.detach(), ref


def _device_side(d, dev):
    from agcn_amd import ops
    f = lambda t: t.float().to(dev).contiguous()  # noqa: E731
    st1 = ops.bn_eval_coeffs(f(d['g1']), f(d['b1']), f(d['rm1']), f(d['rv1']))
    st2 = ops.bn_eval_coeffs(f(d['g2']), f(d['b2']), f(d['rm2']), f(d['rv2'])) if d['two'] else None
    return f(d['y1']), f(d['y2']) if d['two'] else None, f(d['dout']), st1, st2


def _bits_of(out):
    """Sign bit words of a tensor, packed on the host exactly as agcn_bn_act_fwd packs them (bit e of word w <->
    element 32*w + e is positive); any element count: the last word is zero padded."""
    flat = (out.flatten() > 0).cpu().numpy()
    pad = (-flat.size) % 32
    by = np.packbits(np.concatenate([flat, np.zeros(pad, dtype=bool)]), bitorder='little')
    return torch.from_numpy(by.view(np.int32).copy())


@pytest.mark.parametrize('two', [False, True], ids=['one_branch', 'two_branches'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_bn_bwd_eval_against_fp64(shape, two):
    from agcn_amd import ops
    dev = _gpu()
    N, C, T, V = shape
    d = _case(shape, two, 11 + N + 7 * C + T * V + int(two))
    y1, y2, dout, st1, st2 = _device_side(d, dev)
    straddles = (N * C * T * V) % 32 != 0 or (T * V) % 32 != 0
    for kind in ('fp32', 'bits', 'none'):
        out_ref, ref = _reference(d, masked=kind != 'none')
        mask = {'fp32': out_ref.float().to(dev), 'bits': _bits_of(out_ref).to(dev), 'none': None}[kind]
        amax = torch.full((1,), -1.0, device=dev)
        res = ops.bn_bwd_eval(dout, mask, y1, st1, y2, st2, want_sums=True, amax_out=amax)
        dy1, dg1, db1, dc1, dy2, dg2, db2, dc2 = res
        what = (shape, two, kind, straddles)
        assert rel(dy1, ref['y1']) < TOL, what
        assert rel(dg1, ref['g1']) < 5 * TOL and rel(db1, ref['b1']) < 5 * TOL, what
        assert rel(dc1, ref['cb1']) < 5 * TOL, what
        # a port that keeps the train path's zero bias gradients fails here: the reference is not zero
        assert float(ref['cb1'].abs().max()) > 1e-3 and float(dc1.abs().max()) > 1e-3, what
        if two:
            assert rel(dy2, ref['y2']) < TOL, what
            assert rel(dg2, ref['g2']) < 5 * TOL and rel(db2, ref['b2']) < 5 * TOL, what
            assert rel(dc2, ref['cb2']) < 5 * TOL, what
        else:
            assert dy2 is None and dg2 is None and db2 is None and dc2 is None
        # the device scalar is bit-equal to max |dy1| of the tensor that came back
        assert torch.equal(amax, dy1.abs().max().reshape(1)), what
        # a second call gives the same bits (fixed-order sums, no float atomics)
        again = ops.bn_bwd_eval(dout, mask, y1, st1, y2, st2, want_sums=True, amax_out=amax)
        for a_, b_ in zip(again, res):
            assert (a_ is None and b_ is None) or torch.equal(a_, b_), what
        # without the sums y1 / y2 are not read at all (NULL pointers) and dy is unchanged
        amax0 = torch.full((1,), -1.0, device=dev)
        lean = ops.bn_bwd_eval(dout, mask, None, st1, None, st2, want_sums=False, amax_out=amax0)
        assert torch.equal(lean[0], dy1) and torch.equal(amax0, amax), what
        assert (lean[4] is None) if not two else torch.equal(lean[4], dy2), what
        assert all(lean[i] is None for i in (1, 2, 3, 5, 6, 7)), what


def test_bits_straddle_words_and_rows_are_misaligned():
    """The case list really holds what it is meant to: rows whose mask nibbles straddle two words (N*C*P and P no
    multiples of 32) and rows that start 4-byte aligned only."""
    assert any((N * C * T * V) % 32 and (T * V) % 4 for N, C, T, V in SHAPES)
    assert any((T * V) > 1024 for _, _, T, V in SHAPES) and any((T * V) < 1024 for _, _, T, V in SHAPES)


def test_bn_bwd_dispatches_eval_states():
    """ops.bn_bwd with eval-mode states takes the one-pass route and hands out the conv-bias gradients."""
    from agcn_amd import ops
    dev = _gpu()
    d = _case((3, 5, 3, 25), True, 5)
    y1, y2, dout, st1, st2 = _device_side(d, dev)
    out_ref, ref = _reference(d, masked=True)
    before = dict(ops.EVAL_BWD_STATS)
    bias = []
    dy1, dg1, db1, dy2, dg2, db2 = ops.bn_bwd(dout, out_ref.float().to(dev), y1, None, st1, y2, None, st2,
                                              bias_out=bias)
    assert ops.EVAL_BWD_STATS['sums'] == before['sums'] + 1 and ops.EVAL_BWD_STATS['nosums'] == before['nosums']
    assert rel(dy1, ref['y1']) < TOL and rel(dy2, ref['y2']) < TOL
    assert rel(dg1, ref['g1']) < 5 * TOL and rel(dg2, ref['g2']) < 5 * TOL
    assert rel(bias[0], ref['cb1']) < 5 * TOL and rel(bias[1], ref['cb2']) < 5 * TOL
