"""GPU checks of aagcn_v24: the spatial-token kernels, the attention core with an additive bias and the bias gradient
against the fp64 tensor-code composition of the same maths on the CPU (ops.tokens_spatial_ref / mha_ref(bias=...), held
against torch's own modules by tests/test_v24_cpu.py), the new C entries on buffers of exactly the queried sizes, the
adjacency-gradient partials of the backbone at the fixtures' width (22 to 63 channels) against fp64, and the model against the reference-generated fixtures of tests/golden/make_golden_v24.py (tv24_*) on the HIP route (checked by
ops.ENCODER_STATS), once more as tensor code (AGCN_ENCODER_HIP=0, child process), with dropout, through two optimiser
steps and through a checkpoint.  ``-m gpu``.

Tolerances: kernels within TOL = 1e-4 of max(1, max|ref|) of the fp64 result (test_gpu_encoder.py's rule; avg on its own
maximum); the token forward is a gather plus one add and is also compared bit for bit with its fp32 tensor-code form.
Model: y_eval, y and every attention matrix within 1e-4 of the tensor's own max, dx and every parameter gradient within
2e-4 through golden_util.audit_grads (test_gpu_v17.py's rule; AGCN_GEMM=bf16: 2e-2).
"""
import os
import subprocess
import sys

import pytest
import torch

from tests import golden_util as gu
from tests import v24_util as vu

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-4


def _gpu():
    import agcn_amd  # noqa: F401
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device('cuda:0')


def _bf16():
    from agcn_amd import lib
    return lib.load().agcn_gemm_mode().decode() == 'bf16'


def rel(a, ref):
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    return float((a - ref).abs().max() / max(1.0, float(ref.abs().max())))


def own(a, ref):
    a, ref = a.detach().double().cpu(), torch.as_tensor(ref).detach().double().cpu()
    return float((a - ref).abs().max() / max(float(ref.abs().max()), 1e-30))


# ---------------------------------------------------------------------------------------------------------------------
# spatial tokens
# ---------------------------------------------------------------------------------------------------------------------
def _tokens_case(N, M, C, Tp, V, with_cls, with_pe, seed=0):
    from agcn_amd import ops
    L = M * V + with_cls
    g = torch.Generator().manual_seed(seed + 100 * C + 10 * Tp + V)
    x = torch.randn(N * M, C, Tp, V, generator=g).float()
    cls = torch.randn(1, 1, C, generator=g).float() if with_cls else None
    pe = torch.randn(1, L + 3, C, generator=g).float() if with_pe else None
    r = torch.randn(N * Tp, L, C, generator=g).float()
    ts64 = [t if t is None else t.double().requires_grad_(True) for t in (x, cls, pe)]
    ref = ops.tokens_spatial_ref(*ts64, M)
    (ref * r.double()).sum().backward()
    return (x, cls, pe), r, ts64, ref.detach(), L


def _run_tokens(ts, r, M, dev):
    from agcn_amd import ops
    leaves = [t if t is None else t.to(dev).requires_grad_(True) for t in ts]
    tok = ops.SpatialTokensFunction.apply(*leaves, M)
    (tok * r.to(dev)).sum().backward()
    torch.cuda.synchronize()
    return tok, leaves


@pytest.mark.parametrize('with_pe', [False, True])
@pytest.mark.parametrize('with_cls', [False, True])
@pytest.mark.parametrize('dims', [(3, 1, 18), (24, 10, 25), (25, 3, 25)])
def test_spatial_tokens_vs_fp64(dims, with_cls, with_pe):
    """(C, T', V): the smallest clip of the Kinetics skeleton; the fixtures' shape (6 frames per tile, 10 = 6 + 4); an
    odd width whose 3 frames share one tile."""
    from agcn_amd import lib, ops
    dev = _gpu()
    C, Tp, V = dims
    N, M = 2, 2
    ts, r, ts64, ref, L = _tokens_case(N, M, C, Tp, V, with_cls, with_pe)
    tok, leaves = _run_tokens(ts, r, M, dev)
    assert lib.load().agcn_last_kernel().decode().startswith("stokens_kernel<fwd> C=%d T'=%d V=%d" % (C, Tp, V))
    assert tuple(tok.shape) == (N * Tp, L, C)
    errs = {'tok': rel(tok, ref)}
    assert torch.equal(tok.detach().cpu(), ops.tokens_spatial_ref(*ts, M))          # bit for bit
    for name, a, b in zip(('dx', 'dcls', 'dpe'), leaves, ts64):
        if a is not None:
            errs[name] = rel(a.grad, b.grad)
    print(dims, with_cls, with_pe, errs)
    assert all(e < TOL for e in errs.values()), errs
    if with_pe:
        assert float(leaves[2].grad[:, L:].abs().max()) == 0.0                      # rows no token reads
        assert float(leaves[2].grad[:, :L].abs().max()) > 0.0


@pytest.mark.parametrize('seqs', [(1, 1), (3, 1), (1, 3), (11, 3), (4, 16)])
def test_spatial_token_sums_over_sequences(seqs):
    """dcls / dpe over N*T' = 1, 3, 33 (one over the 32 sequences of a slab slot) and 64 (two full slots) sequences,
    and the same bits on a second run."""
    dev = _gpu()
    N, Tp = seqs
    ts, r, ts64, _, L = _tokens_case(N, 2, 3, Tp, 18, True, True, seed=5)
    _, a = _run_tokens(ts, r, 2, dev)
    _, b = _run_tokens(ts, r, 2, dev)
    errs = {'dcls': rel(a[1].grad, ts64[1].grad), 'dpe': rel(a[2].grad, ts64[2].grad), 'dx': rel(a[0].grad, ts64[0].grad)}
    print(seqs, errs)
    assert all(e < TOL for e in errs.values()), errs
    for s, t in zip(a, b):
        assert torch.equal(s.grad, t.grad)
    assert torch.equal(a[1].grad.reshape(-1), a[2].grad[0, 0])                       # dcls is row 0 of dpe: the same additions


# ---------------------------------------------------------------------------------------------------------------------
# attention core with a bias
# ---------------------------------------------------------------------------------------------------------------------
BIAS_SHAPES = [
    # N, L, H, dh
    (3, 51, 3, 8),         # the fixtures' head: 4 row blocks, the last with 3 rows
    (2, 51, 3, 48),        # the shipped head width
    (5, 37, 1, 25),        # Kinetics token count, one head, dh not a multiple of 4
    (1, 1, 2, 4),          # smallest
    (300, 51, 3, 8),       # ten slab slots, the last with 12 sequences
]
BIAS_CASES = [(s, hb) for s in BIAS_SHAPES for hb in sorted({1, s[2]})]


def _bias_case(shape, Hb, p_drop=0.0, null=False, big=False, seed=0):
    """Inputs and the fp64 reference: ctx, avg, dqkv, dbias for the loss sum(ctx * r)."""
    from agcn_amd import ops
    N, L, H, dh = shape
    g = torch.Generator().manual_seed(1000 * seed + 7 * L + dh + 31 * Hb)
    qkv = torch.randn(N, L, 3 * H * dh, generator=g).float()
    qkv[..., :H * dh] *= 1.5                             # logits q.k/sqrt(dh) ~ 1.5 N(0, 1): a peaked softmax
    bias = torch.randn(Hb, L, L, generator=g).float()
    if big:
        # scores up to 70 and bias entries of +-30, one +30 on the largest score: the sum passes 88.7, where expf
        # overflows unless the row maximum is taken AFTER the bias is added
        q, k = (qkv[..., i * H * dh:(i + 1) * H * dh].reshape(N, L, H, dh).double() for i in (0, 1))
        s = torch.einsum('nihd,njhd->nhij', q, k) / dh ** 0.5
        qkv[..., :H * dh] *= float(70.0 / s.max())
        s = s * (70.0 / s.max())
        pick = torch.rand(Hb, L, L, generator=g)
        bias[pick < 0.1] = 30.0
        bias[pick > 0.9] = -30.0
        top = (s == s.max()).nonzero()[0]
        bias[int(top[1]) if Hb > 1 else 0, int(top[2]), int(top[3])] = 30.0
        assert float(s.max()) < 88.0 and float((s + bias.double()[None]).max()) > 89.0
    r = torch.randn(N, L, H * dh, generator=g).float()
    null_tok = None
    if null:
        null_tok = (torch.rand(N, L, generator=g) < 0.5).to(torch.uint8)
        null_tok[:, 0] = 0
    keep, scale = None, 1.0
    if p_drop > 0:
        keep = (torch.rand(N, H, L, L, generator=g) >= p_drop).to(torch.uint8)
        scale = 1.0 / (1.0 - p_drop)
    q64, b64 = qkv.double().requires_grad_(True), bias.double().requires_grad_(True)
    ctx, avg = ops.mha_ref(q64, H, null_tok, 0, keep, scale, need_avg=True, bias=b64)
    (ctx * r.double()).sum().backward()
    return dict(qkv=qkv, bias=bias, r=r, null=null_tok, keep=keep, scale=scale, ctx=ctx.detach(), avg=avg.detach(),
                dqkv=q64.grad, dbias=b64.grad)


def _run_bias(c, H, dev, with_bias=True):
    from agcn_amd import ops
    dv = lambda t: None if t is None else t.to(dev)      # noqa: E731
    qkv = c['qkv'].to(dev).requires_grad_(True)
    bias = c['bias'].to(dev).requires_grad_(True) if with_bias else None
    ctx, avg = ops.MHABiasFunction.apply(qkv, H, bias, dv(c['null']), 0, dv(c['keep']), c['scale'], True)
    (ctx * c['r'].to(dev)).sum().backward()
    torch.cuda.synchronize()
    return ctx, avg, qkv.grad, None if bias is None else bias.grad


def _errs(out, c):
    ctx, avg, dq, db = out
    return dict(ctx=rel(ctx, c['ctx']), avg=own(avg, c['avg']), dqkv=rel(dq, c['dqkv']), dbias=rel(db, c['dbias']))


@pytest.mark.parametrize('shape,Hb', BIAS_CASES)
def test_mha_bias_vs_fp64(shape, Hb):
    from agcn_amd import lib
    dev = _gpu()
    N, L, H, dh = shape
    c = _bias_case(shape, Hb)
    out = _run_bias(c, H, dev)
    assert tuple(out[3].shape) == (Hb, L, L) and tuple(out[1].shape) == (N, L, L) and not out[1].requires_grad
    errs = _errs(out, c)
    print(shape, Hb, errs, 'max|dbias|', float(c['dbias'].abs().max()))
    assert all(e < TOL for e in errs.values()), errs
    assert float(c['dbias'].abs().max()) > 0 or L == 1                 # (one key: the softmax is 1 whatever the bias)
    # the bias is not a no-op: without it the context moves by far more than the tolerance
    if L > 1:
        plain = _run_bias(c, H, dev, with_bias=False)
        assert rel(plain[0], c['ctx']) > 100 * TOL
    assert lib.load().agcn_last_kernel() is not None


@pytest.mark.parametrize('Hb', [1, 3])
@pytest.mark.parametrize('what', ['keep', 'null', 'big'])
def test_mha_bias_with_keep_mask_null_tokens_and_large_bias(what, Hb):
    dev = _gpu()
    shape = (3, 51, 3, 8)
    c = _bias_case(shape, Hb, p_drop=0.2 if what == 'keep' else 0.0, null=what == 'null', big=what == 'big', seed=3)
    out = _run_bias(c, shape[2], dev)
    assert all(bool(torch.isfinite(t).all()) for t in out)
    errs = _errs(out, c)
    print(what, Hb, errs)
    assert all(e < TOL for e in errs.values()), errs


def test_mha_bias_grad_of_300_sequences_is_the_ordered_sum_and_repeats():
    """dbias over 300 sequences (x 3 heads for the shared slice) against the fp64 sum in the kernel's order, n ascending
    and h ascending inside n, which in fp64 is the sum in any order to 1e-13; and the same bits on a second run."""
    from agcn_amd import ops
    dev = _gpu()
    shape = (300, 51, 3, 8)
    for Hb in (1, 3):
        c = _bias_case(shape, Hb)
        # dS of every (n, h) in fp64, from the autograd of the tensor-code form with one bias slice per (n, h)
        q64 = c['qkv'].double()
        full = c['bias'].double().expand(3, 51, 51).unsqueeze(0).repeat(300, 1, 1, 1).requires_grad_(True)
        N, L, D3 = q64.shape
        q, k, v = (t.reshape(N, L, 3, 8).transpose(1, 2) for t in q64.split(D3 // 3, dim=-1))
        p = torch.softmax(q @ k.transpose(-1, -2) / 8 ** 0.5 + full, dim=-1)
        ((p @ v).transpose(1, 2).reshape(N, L, 24) * c['r'].double()).sum().backward()
        ds = full.grad                                               # (300, 3, 51, 51)
        ordered = torch.zeros(Hb, L, L, dtype=torch.float64)
        for n in range(300):
            for h in range(3):
                ordered[h if Hb == 3 else 0] += ds[n, h]
        assert float((ordered - c['dbias']).abs().max()) < 1e-10
        a = _run_bias(c, 3, dev)
        b = _run_bias(c, 3, dev)
        err = rel(a[3], ordered)
        print(Hb, 'dbias', err, 'max', float(ordered.abs().max()))
        assert err < TOL
        for s, t in zip(a, b):
            assert torch.equal(s, t)
    assert ops.MHABiasFunction is not ops.MHAFunction


@pytest.mark.parametrize('shape', [(3, 51, 3, 8), (5, 37, 1, 25)])
def test_without_a_bias_the_result_is_mha_functions(shape):
    from agcn_amd import ops
    dev = _gpu()
    N, L, H, dh = shape
    c = _bias_case(shape, 1, p_drop=0.2, null=True, seed=9)
    outs = []
    for fn, extra in ((ops.MHAFunction, ()), (ops.MHABiasFunction, (None,))):
        qkv = c['qkv'].to(dev).requires_grad_(True)
        ctx, avg = fn.apply(qkv, H, *extra, c['null'].to(dev), 0, c['keep'].to(dev), c['scale'], True)
        (ctx * c['r'].to(dev)).sum().backward()
        outs.append((ctx.detach(), avg, qkv.grad))
    torch.cuda.synchronize()
    for s, t in zip(*outs):
        assert torch.equal(s, t)
    # a zero bias adds 0.0f to every logit: the same values through the other instantiation
    qkv = c['qkv'].to(dev)
    ctx0, _ = ops.MHABiasFunction.apply(qkv, H, torch.zeros(1, L, L, device=dev), c['null'].to(dev), 0, c['keep'].to(dev),
                                        c['scale'], False)
    assert rel(ctx0, outs[0][0]) < 1e-6


def test_python_side_checks():
    from agcn_amd import ops
    dev = _gpu()
    qkv = torch.zeros(2, 5, 3 * 6, device=dev)
    for bad in (torch.zeros(2, 5, 5), torch.zeros(5, 5), torch.zeros(1, 5, 4), torch.zeros(3, 4, 5)):
        with pytest.raises(ValueError, match='bias must be'):
            ops.MHABiasFunction.apply(qkv, 3, bad.to(dev), None, 0, None, 1.0, False)
    with pytest.raises(ValueError, match='qkv must be'):
        ops.MHABiasFunction.apply(torch.zeros(2, 5, 20, device=dev), 3, None, None, 0, None, 1.0, False)
    with pytest.raises(ValueError, match='null_tok must be'):
        ops.MHABiasFunction.apply(qkv, 3, None, torch.zeros(2, 4, dtype=torch.uint8, device=dev), 0, None, 1.0, False)
    with pytest.raises(ValueError, match='keep must be'):
        ops.MHABiasFunction.apply(qkv, 3, None, None, 0, torch.zeros(2, 3, 5, 4, dtype=torch.uint8, device=dev), 1.25, False)
    with pytest.raises(RuntimeError, match='GPU tensor'):
        ops.MHABiasFunction.apply(qkv, 3, torch.zeros(1, 5, 5), None, 0, None, 1.0, False)       # a bias on the CPU
    # a transposed (non-contiguous) bias is made contiguous, not misread
    b = torch.randn(1, 5, 5, device=dev)
    q = torch.randn(2, 5, 18, device=dev)
    a1, _ = ops.MHABiasFunction.apply(q, 3, b.transpose(1, 2), None, 0, None, 1.0, False)
    a2, _ = ops.MHABiasFunction.apply(q, 3, b.transpose(1, 2).contiguous(), None, 0, None, 1.0, False)
    assert torch.equal(a1, a2)
    x = torch.zeros(4, 3, 2, 5, device=dev)
    with pytest.raises(ValueError, match='x must be'):
        ops.SpatialTokensFunction.apply(x, None, None, 3)
    with pytest.raises(ValueError, match='cls must be'):
        ops.SpatialTokensFunction.apply(x, torch.zeros(1, 1, 4, device=dev), None, 2)
    with pytest.raises(ValueError, match='pe must be'):
        ops.SpatialTokensFunction.apply(x, None, torch.zeros(1, 9, 3, device=dev), 2)


# ---------------------------------------------------------------------------------------------------------------------
# the C entries on buffers of exactly the queried sizes
# ---------------------------------------------------------------------------------------------------------------------
SENTINEL = -7.5e30
GUARD = 64


def _guarded(n, dev):
    buf = torch.full((n + GUARD,), SENTINEL, device=dev)
    return buf, buf[:n]


def _intact(buf, n):
    return bool((buf[n:] == SENTINEL).all()) and not bool((buf[:n] == SENTINEL).any())


def test_c_entries_on_exact_buffers():
    """agcn_tokens_spatial_fwd / _bwd, agcn_mha_bias_fwd and agcn_mha_bias_grad write every element of their outputs and
    nothing behind them: outputs and workspaces of exactly the documented / queried sizes, sentinel floats behind."""
    from agcn_amd import lib, ops
    dev = _gpu()
    Lb = lib.load()
    g = torch.Generator().manual_seed(12)
    N, M, C, Tp, V = 11, 2, 5, 3, 18                      # 33 sequences: two slab slots
    L, S = M * V + 1, N * Tp
    x = torch.randn(N * M, C, Tp, V, generator=g).to(dev)
    cls, pe = torch.randn(C, generator=g).to(dev), torch.randn(L + 2, C, generator=g).to(dev)
    tok_b, tok = _guarded(S * L * C, dev)
    lib.call("agcn_tokens_spatial_fwd", x, cls, pe, L + 2, tok, N, M, C, Tp, V)
    torch.cuda.synchronize()
    assert _intact(tok_b, S * L * C)
    want = ops.tokens_spatial_ref(x, cls.view(1, 1, C), pe.view(1, L + 2, C), M)
    assert torch.equal(tok.view(S, L, C), want)
    dtok = torch.randn(S, L, C, generator=g).to(dev)
    nbytes = Lb.agcn_tokens_spatial_bwd_workspace(N, M, C, Tp, V, 1)
    assert nbytes == 2 * L * C * 4
    (dx_b, dx), (dc_b, dc), (dp_b, dp), (ws_b, ws) = (_guarded(n, dev) for n in (x.numel(), C, (L + 2) * C, nbytes // 4))
    lib.call("agcn_tokens_spatial_bwd", dtok, dx, dc, dp, 1, L + 2, ws, nbytes, N, M, C, Tp, V)
    torch.cuda.synchronize()
    assert _intact(dx_b, x.numel()) and _intact(dc_b, C) and _intact(dp_b, (L + 2) * C)
    assert bool((ws_b[nbytes // 4:] == SENTINEL).all())
    assert rel(dp.view(L + 2, C)[:L], dtok.double().sum(0)) < TOL and float(dp.view(L + 2, C)[L:].abs().max()) == 0.0
    assert torch.equal(dc, dp[:C])
    # attention with a bias, and its bias gradient
    Nq, Lq, H, dh = 33, 37, 3, 5
    D = H * dh
    qkv = torch.randn(Nq, Lq, 3 * D, generator=g).to(dev)
    for Hb in (1, H):
        bias = torch.randn(Hb, Lq, Lq, generator=g).to(dev)
        (c_b, ctx), (p_b, prob), (a_b, avg) = (_guarded(n, dev) for n in (Nq * Lq * D, Nq * H * Lq * Lq, Nq * Lq * Lq))
        lib.call("agcn_mha_bias_fwd", qkv, bias, Hb, None, 0, None, 1.0, ctx, prob, avg, Nq, Lq, H, dh)
        torch.cuda.synchronize()
        assert _intact(c_b, Nq * Lq * D) and _intact(p_b, Nq * H * Lq * Lq) and _intact(a_b, Nq * Lq * Lq)
        wctx, wavg = ops.mha_ref(qkv.double().cpu(), H, need_avg=True, bias=bias.double().cpu())
        assert rel(ctx.view(Nq, Lq, D), wctx) < TOL and own(avg.view(Nq, Lq, Lq), wavg) < TOL
        ds = torch.randn(Nq, H, Lq, Lq, generator=g).to(dev)
        nbytes = Lb.agcn_mha_bias_grad_workspace(Nq, Lq, H, Hb)
        assert nbytes == 2 * Hb * Lq * Lq * 4
        (d_b, dbias), (w_b, ws) = (_guarded(n, dev) for n in (Hb * Lq * Lq, nbytes // 4))
        lib.call("agcn_mha_bias_grad", ds, dbias, ws, nbytes, Nq, Lq, H, Hb)
        torch.cuda.synchronize()
        assert _intact(d_b, Hb * Lq * Lq) and _intact(w_b, nbytes // 4)
        wsum = ds.double().sum(0) if Hb == H else ds.double().sum((0, 1)).unsqueeze(0)
        assert rel(dbias.view(Hb, Lq, Lq), wsum) < TOL
        assert lib.status("agcn_mha_bias_grad", ds, dbias, ws, nbytes - 1, Nq, Lq, H, Hb) == lib.ERR_WORKSPACE


# ---------------------------------------------------------------------------------------------------------------------
# the backbone at the fixtures' width
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dims', [(24, 24, 9, 25), (24, 24, 3, 18), (43, 24, 5, 25), (63, 16, 7, 25), (21, 24, 9, 25)])
def test_adjacency_gradient_partials_at_widths_between_22_and_63(dims):
    """agcn_gcn_dadj at (C, Cout, T, V) with 64 < 3C < 192, the second unit of tv24_two_windows among them: the rows of a
    subset straddle two 64-row blocks of the exact kernel, which used to share one slot (C = 21: the widest that fits
    one block).  sum over the slots of dadj_part against fp64: dadj_i[u, v] = sum_{c,t} x[c,t,u] (Wd_i^T dy)[c,t,v]."""
    from agcn_amd import lib, ops
    dev = _gpu()
    C, Cout, T, V = dims
    N = 2
    g = torch.Generator().manual_seed(C + T)
    x = torch.randn(N, C, T, V, generator=g).float()
    dy = torch.randn(N, Cout, T, V, generator=g).float()
    w = (torch.randn(Cout, 3 * C, generator=g) / Cout ** 0.5).float()
    ref = torch.einsum('nctu,oic,notv->niuv', x.double(), w.double().view(Cout, 3, C), dy.double())
    L = lib.load()
    nslots = L.agcn_dadj_num_slots(C, V, T)
    assert nslots > 0
    buf, dpart = _guarded(N * 3 * nslots * V * V, dev)
    xg, dyg, wg = x.to(dev), dy.to(dev), w.to(dev)
    ws, nb = ops._gcn_ws(C, Cout, T, V, xg)
    lib.call("agcn_gcn_dadj_ex", dyg, wg, xg, dpart, ws, nb, N, C, Cout, T, V, None, None)
    torch.cuda.synchronize()
    assert _intact(buf, dpart.numel())
    err = rel(dpart.view(N, 3, nslots, V, V).sum(2), ref)
    print(dims, 'slots', nslots, 'err', err, lib.load().agcn_last_kernel().decode())
    assert err < TOL


# ---------------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------------
def _model(name, dev, cfg=None, **over):
    from agcn_amd.model import aagcn_v24
    gold = vu.load(name)
    m = aagcn_v24.Model(**dict(vu.model_kwargs(name, **(cfg or {})), **over))
    m.load_state_dict(vu.state(vu.shapes_of(gold), name), strict=True)
    return m.to(dev), gold


def _expect_route(layers):
    from agcn_amd import ops
    hip = ops.encoder_hip_enabled()
    assert ops.ENCODER_STATS['layers_hip'] == (layers if hip else 0), ops.ENCODER_STATS
    assert ops.ENCODER_STATS['layers_tensor'] == (0 if hip else layers), ops.ENCODER_STATS


@pytest.mark.parametrize('name', vu.NAMES)
def test_v24_vs_reference(name):
    from agcn_amd import ops
    dev = _gpu()
    m, gold = _model(name, dev, need_attn=True)
    tol_y, tol_g = (2e-2, 2e-2) if _bf16() else (1e-4, 2e-4)
    x = torch.from_numpy(gold['x']).to(dev)
    seqs = [int(s) for s in gold['attn_seq']]
    windows = vu.windows(name)
    L = 1 + vu.M * vu.model_kwargs(name)['num_point']
    ops.ENCODER_STATS.update(layers_hip=0, layers_tensor=0)
    errs = {}
    m.eval()
    with torch.no_grad():
        y_eval, attn = m(x)
    errs['y_eval'] = own(y_eval, gold['y_eval'])
    assert len(attn) == 2
    for i, a in enumerate(attn):
        assert tuple(a.shape) == (vu.N * windows, L, L)
        errs[f'attn_eval.{i}'] = own(a[seqs], gold[f'attn_eval.{i}'])
    m.train()
    xg = x.clone().requires_grad_(True)
    y, attn = m(xg)
    (y * torch.from_numpy(gold['r']).to(dev)).sum().backward()
    torch.cuda.synchronize()
    _expect_route(4)
    errs['y'] = own(y, gold['y'])
    for i, a in enumerate(attn):
        assert not a.requires_grad
        errs[f'attn.{i}'] = own(a[seqs], gold[f'attn.{i}'])
    print(name, {k: f'{v:.2e}' for k, v in errs.items()})
    for k, v in errs.items():
        assert gu.audit_value(name, k, v, tol_y), (k, v)
    e_dx = own(xg.grad, gold['dx'])
    print(name, 'dx', f'{e_dx:.2e}')
    assert gu.audit_value(name, 'dx', e_dx, tol_g), e_dx
    named = [(n, p.grad.detach().cpu().numpy()) for n, p in m.named_parameters() if p.grad is not None]
    none = [n for n, p in m.named_parameters() if p.grad is None]
    assert none == ([] if vu.has_bias(name) else ['alpha']), none           # without a bias alpha gets no gradient
    assert all(('g.' + n + '.absmax') not in gold for n in none)
    assert all(('g.' + n + '.absmax') in gold for n, _ in named)
    got = {n for n, _ in named}
    assert {'s_cls_token'} <= got and (('alpha' in got) == vu.has_bias(name))
    assert sum(n.endswith('.PA') and n.startswith('s_trans_enc_layers.') for n in got) == (2 if vu.has_bias(name) else 0)
    bad, rec = gu.audit_grads(name, named, gold, tol_g)
    print(name, 'grads: worst err32', rec['worst_err32'], 'worst err64', rec['worst_err64'])
    assert not bad, bad


def test_v24_fixtures_as_tensor_code():
    """The four fixtures once more with AGCN_ENCODER_HIP=0 (read per call, but the counter check wants a clean process)."""
    _gpu()
    r = subprocess.run([sys.executable, '-m', 'pytest', os.path.join(ROOT, 'tests', 'test_gpu_v24.py'), '-q', '-x', '-m', 'gpu',
                        '-p', 'no:cacheprovider', '-k', 'test_v24_vs_reference'],
                       env=dict(os.environ, AGCN_ENCODER_HIP='0'), cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert '4 passed' in r.stdout and ' skipped' not in r.stdout, r.stdout[-2000:]


def test_v24_dropout(monkeypatch):
    dev = _gpu()
    m, gold = _model('tv24_triple', dev, cfg=dict(dropout=0.2), need_attn=True)
    m.train()
    x = torch.from_numpy(gold['x']).to(dev)
    r = torch.from_numpy(gold['r']).to(dev)

    def run():
        torch.manual_seed(77)
        m.zero_grad(set_to_none=True)
        xg = x.clone().requires_grad_(True)
        y, attn = m(xg)
        (y * r).sum().backward()
        pas = [layer.PA.grad.clone() for layer in m.s_trans_enc_layers]
        return [y.detach(), xg.grad, m.alpha.grad.clone()] + pas + [a for a in attn]

    monkeypatch.setenv('AGCN_ENCODER_HIP', '1')
    a, b = run(), run()
    assert all(bool(torch.isfinite(t).all()) for t in a)
    for s, t in zip(a, b):
        assert torch.equal(s, t)
    # the returned attention is the dropped-out one: an entry of the mean over the 3 heads is zero where all three heads
    # dropped it, 0.2^3 of the 20*51*51 entries of the first layer (standard deviation 0.0004)
    zeros = float((a[5] == 0).float().mean())
    assert 0.004 < zeros < 0.012, zeros
    monkeypatch.setenv('AGCN_ENCODER_HIP', '0')
    c = run()
    tol = 2e-2 if _bf16() else 1e-4          # (bf16: the backbone's backward amplifies the head's last-bit differences)
    for s, t in zip(a, c):
        assert own(s, t) < tol
    torch.manual_seed(78)                                  # another seed, another mask
    y2, _ = m(x)
    assert not torch.equal(y2.detach(), c[0])


def test_v24_train_steps():
    from agcn_amd.trainer import TrainEngine
    dev = _gpu()
    m, gold = _model('tv24_shipped', dev, cfg=dict(dropout=0.2))
    eng = TrainEngine(m, base_lr=0.05)
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    assert {'alpha', 's_cls_token', 's_trans_enc_layers.0.PA', 's_trans_enc_layers.1.PA'} <= set(before)
    x = torch.from_numpy(gold['x']).to(dev)
    label = torch.tensor([3, 41], device=dev)
    for _ in range(2):
        loss = eng.train_step(x, label)
        assert bool(torch.isfinite(loss))
    same = [n for n, p in m.named_parameters() if torch.equal(p.detach(), before[n])]
    assert not same, same


def test_v24_strict_load_of_a_reference_style_checkpoint(tmp_path):
    dev = _gpu()
    m, gold = _model('tv24_triple', dev)
    path = str(tmp_path / 'v24.pt')
    torch.save({k: v.cpu() for k, v in m.state_dict().items()}, path)
    m2, _ = _model('tv24_triple', dev)
    with torch.no_grad():
        for p in m2.parameters():
            p.zero_()
    m2.load_state_dict(torch.load(path), strict=True)
    m.eval()
    m2.eval()
    x = torch.from_numpy(gold['x']).to(dev)
    with torch.no_grad():
        assert torch.equal(m(x)[0], m2(x)[0])
