"""GPU parity of the encoder kernels (csrc/encoder.hip: agcn_tokens_*, agcn_mha_*, agcn_ln_*) against the fp64 tensor-code
composition of the same maths on the CPU (ops.tokens_ref / mha_ref / add_ln_ref, themselves held against torch's own
modules by tests/test_v17_cpu.py).  ``-m gpu``.

Tolerance: 1e-4 of max(1, max|ref|) for ctx, dqkv, LayerNorm and token gradients (the rule of test_gpu_tconv.py); 1e-4
of the tensor's own maximum for prob and avg (values <= 1); the token forward is a gather plus one add and is compared
bit for bit with its fp32 tensor-code form.  The shapes are the smallest at which each hazard exists (see SHAPES).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [
    # N, L, H, dh
    (1, 2, 1, 1),          # smallest legal shape
    (2, 21, 2, 200),       # shipped configuration
    (2, 21, 16, 25),       # dh not a multiple of 4
    (2, 6, 2, 144),        # Kinetics head width
    (1, 64, 2, 16),        # a 64-row tile exactly ...
    (1, 65, 2, 16),        # ... and one row over
    (1, 201, 2, 200),      # the workload's L
    (1, 601, 1, 8),        # longest positional table
    (1, 640, 1, 256),      # domain corner
]
MASKS = ['none', 'forward', 'backward', 'frame']
TOL = 1e-4


def _gpu():
    import agcn_amd  # noqa: F401
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device('cuda:0')


def rel(a, ref):
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    return float((a - ref).abs().max() / max(1.0, float(ref.abs().max())))


def own(a, ref):
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    return float((a - ref).abs().max() / max(float(ref.abs().max()), 1e-30))


def _mask_args(mask, N, L, g):
    null = None
    if mask == 'frame':
        null = (torch.rand(N, L, generator=g) < 0.5).to(torch.uint8)
        null[:, 0] = 0                                   # token 0 (CLS) is never null
    return null, {'none': 0, 'frame': 0, 'forward': 1, 'backward': 2}[mask]


def _mha_case(shape, mask, p_drop=0.0, qscale=1.0, seed=0):
    """Inputs and the fp64 reference: ctx, avg, prob, dqkv for the loss sum(ctx * r)."""
    from agcn_amd import ops
    N, L, H, dh = shape
    g = torch.Generator().manual_seed(1000 * seed + L * 7 + dh)
    qkv = torch.randn(N, L, 3 * H * dh, generator=g).float()
    qkv[..., :H * dh] *= 1.5 * qscale                    # logits q.k/sqrt(dh) ~ 1.5 N(0, 1): a peaked softmax
    r = torch.randn(N, L, H * dh, generator=g).float()
    null, causal = _mask_args(mask, N, L, g)
    keep, scale = None, 1.0
    if p_drop > 0:
        keep = (torch.rand(N, H, L, L, generator=g) >= p_drop).to(torch.uint8)
        scale = 1.0 / (1.0 - p_drop)
    q64 = qkv.double().requires_grad_(True)
    ctx, avg, prob = ops.mha_ref(q64, H, null, causal, keep, scale, need_avg=True, want_prob=True)
    (ctx * r.double()).sum().backward()
    return dict(qkv=qkv, r=r, null=null, causal=causal, keep=keep, scale=scale,
                ctx=ctx.detach(), avg=avg.detach(), prob=prob.detach(), dqkv=q64.grad)


def _run_mha(c, H, dev, need_avg=True, grad=True):
    from agcn_amd import ops
    dv = lambda t: None if t is None else t.to(dev)      # noqa: E731
    qkv = c['qkv'].to(dev).requires_grad_(grad)
    ctx, avg = ops.MHAFunction.apply(qkv, H, dv(c['null']), c['causal'], dv(c['keep']), c['scale'], need_avg)
    dq = None
    if grad:
        (ctx * c['r'].to(dev)).sum().backward()
        dq = qkv.grad
    torch.cuda.synchronize()
    return ctx, avg, dq


@pytest.mark.parametrize('mask', MASKS)
@pytest.mark.parametrize('shape', SHAPES)
def test_mha_vs_fp64(shape, mask):
    from agcn_amd import lib
    dev = _gpu()
    N, L, H, dh = shape
    c = _mha_case(shape, mask)
    assert float(c['prob'].max()) > 2.0 / L or L <= 2          # not a flat softmax
    ctx, avg, dq = _run_mha(c, H, dev)
    # (the note is per thread: this thread launched the forward, autograd's the backward)
    assert lib.load().agcn_last_kernel().decode().startswith('mha_fwd_kernel L=%d dh=%d' % (L, dh))
    errs = dict(ctx=rel(ctx, c['ctx']), avg=own(avg, c['avg']), dqkv=rel(dq, c['dqkv']))
    print(shape, mask, errs)
    assert all(e < TOL for e in errs.values()), errs
    assert tuple(avg.shape) == (N, L, L) and not avg.requires_grad


@pytest.mark.parametrize('shape', [SHAPES[1], SHAPES[2], SHAPES[5]])
def test_mha_prob_is_the_softmax_before_dropout(shape):
    """prob (saved for backward) against fp64, with and without a keep mask: the same tensor either way."""
    from agcn_amd import lib
    dev = _gpu()
    N, L, H, dh = shape
    Lb = lib.load()
    for p_drop in (0.0, 0.2):
        c = _mha_case(shape, 'frame', p_drop=p_drop)
        qkv = c['qkv'].to(dev)
        ctx = torch.empty(N, L, H * dh, device=dev)
        prob = torch.full((N, H, L, L), float('nan'), device=dev)
        avg = torch.empty(N, L, L, device=dev)
        keep = None if c['keep'] is None else c['keep'].to(dev)
        rc = Lb.agcn_mha_fwd(qkv.data_ptr(), c['null'].to(dev).data_ptr(), c['causal'],
                             None if keep is None else keep.data_ptr(), c['scale'], ctx.data_ptr(), prob.data_ptr(),
                             avg.data_ptr(), N, L, H, dh, torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        torch.cuda.synchronize()
        assert own(prob, c['prob']) < TOL and own(avg, c['avg']) < TOL and rel(ctx, c['ctx']) < TOL


def test_mha_keep_mask():
    dev = _gpu()
    shape = (2, 21, 2, 200)
    c = _mha_case(shape, 'forward', p_drop=0.2)
    assert 0.1 < 1.0 - float(c['keep'].float().mean()) < 0.3
    ctx, avg, dq = _run_mha(c, shape[2], dev)
    errs = dict(ctx=rel(ctx, c['ctx']), avg=own(avg, c['avg']), dqkv=rel(dq, c['dqkv']))
    assert all(e < TOL for e in errs.values()), errs


def test_mha_inference_form():
    """No gradient wanted: prob = NULL, and with need_avg False also avg = NULL (one workgroup per head)."""
    dev = _gpu()
    shape = (2, 21, 2, 200)
    c = _mha_case(shape, 'frame')
    with torch.no_grad():
        ctx, avg, _ = _run_mha(c, shape[2], dev, need_avg=False, grad=False)
        assert avg is None and rel(ctx, c['ctx']) < TOL
        ctx, avg, _ = _run_mha(c, shape[2], dev, need_avg=True, grad=False)
        assert rel(ctx, c['ctx']) < TOL and own(avg, c['avg']) < TOL


def test_mha_large_logits_need_max_subtraction():
    """q scaled by 30: logits near 100, whose exponentials overflow fp32 without the row maximum subtracted."""
    dev = _gpu()
    shape = (1, 65, 2, 16)
    c = _mha_case(shape, 'none', qscale=30.0)
    s = torch.einsum('nihd,njhd->nhij', c['qkv'][..., :32].reshape(1, 65, 2, 16).double(),
                     c['qkv'][..., 32:64].reshape(1, 65, 2, 16).double()) / 4.0
    s = s * 1.5                                                   # (_mha_case's own scale of q)
    assert float(s.max()) > 89.0                                  # exp overflows fp32 above 88.7
    ctx, avg, dq = _run_mha(c, shape[2], dev)
    assert bool(torch.isfinite(ctx).all()) and bool(torch.isfinite(dq).all())
    errs = dict(ctx=rel(ctx, c['ctx']), avg=own(avg, c['avg']), dqkv=rel(dq, c['dqkv']))
    assert all(e < TOL for e in errs.values()), errs


def test_mha_fully_masked_row_is_zero():
    from agcn_amd import ops
    dev = _gpu()
    N, L, H, dh = 1, 21, 2, 25
    g = torch.Generator().manual_seed(9)
    qkv = torch.randn(N, L, 3 * H * dh, generator=g).float().to(dev).requires_grad_(True)
    null = torch.ones(N, L, dtype=torch.uint8)          # every token null: every row of every head fully masked
    ctx, avg = ops.MHAFunction.apply(qkv, H, null.to(dev), 0, None, 1.0, True)
    ctx.sum().backward()
    torch.cuda.synchronize()
    assert float(ctx.detach().abs().max()) == 0.0 and float(avg.abs().max()) == 0.0
    assert float(qkv.grad.abs().max()) == 0.0
    null[:, 3] = 0                                       # one live token: rows of null tokens see it alone
    ctx, avg = ops.MHAFunction.apply(qkv, H, null.to(dev), 0, None, 1.0, True)
    want, wavg = ops.mha_ref(qkv.detach().double().cpu(), H, null, 0, need_avg=True)
    assert rel(ctx, want) < TOL and own(avg, wavg) < TOL
    assert float((avg[:, :3, 3] - 1).abs().max()) < 1e-6


@pytest.mark.parametrize('with_b', [False, True])
@pytest.mark.parametrize('D', [1, 25, 400, 2048])
def test_layernorm_vs_fp64(D, with_b):
    from agcn_amd import ops
    dev = _gpu()
    g = torch.Generator().manual_seed(D + with_b)
    R = (3, 43)                                           # 129 rows: one per wave in the backward, 3 waves idle
    a = torch.randn(*R, D, generator=g).float()
    b = torch.randn(*R, D, generator=g).float() if with_b else None
    w = torch.rand(D, generator=g).float() + 0.5
    w[D // 2] = 0.0                                       # the normalised value cannot be recovered from the output
    bias = torch.randn(D, generator=g).float()
    r = torch.randn(*R, D, generator=g).float()
    ts64 = [t if t is None else t.double().requires_grad_(True) for t in (a, b, w, bias)]
    (ops.add_ln_ref(*ts64, 1e-5) * r.double()).sum().backward()
    ref = ops.add_ln_ref(*ts64, 1e-5).detach()
    ts = [t if t is None else t.to(dev).requires_grad_(True) for t in (a, b, w, bias)]
    out = ops.AddLayerNormFunction.apply(*ts, 1e-5)
    (out * r.to(dev)).sum().backward()
    torch.cuda.synchronize()
    errs = {'out': rel(out, ref), 'da': rel(ts[0].grad, ts64[0].grad), 'dw': rel(ts[2].grad, ts64[2].grad),
            'dbias': rel(ts[3].grad, ts64[3].grad)}
    if with_b:
        errs['db'] = rel(ts[1].grad, ts64[1].grad)
    print(D, with_b, errs)
    assert all(e < TOL for e in errs.values()), errs


def test_layernorm_many_rows_per_wave():
    """More rows than backward waves (R = 1300 > 1024: 2 rows per wave, 650 waves in 163 workgroups, the last two waves
    of the grid without a row)."""
    from agcn_amd import ops
    dev = _gpu()
    g = torch.Generator().manual_seed(4)
    a, w, bias = torch.randn(1300, 25, generator=g), torch.rand(25, generator=g) + 0.5, torch.randn(25, generator=g)
    r = torch.randn(1300, 25, generator=g)
    ts64 = [t.double().requires_grad_(True) for t in (a, w, bias)]
    (ops.add_ln_ref(ts64[0], None, ts64[1], ts64[2], 1e-5) * r.double()).sum().backward()
    ts = [t.to(dev).requires_grad_(True) for t in (a, w, bias)]
    (ops.AddLayerNormFunction.apply(ts[0], None, ts[1], ts[2], 1e-5) * r.to(dev)).sum().backward()
    for x, y in zip(ts, ts64):
        assert rel(x.grad, y.grad) < TOL


@pytest.mark.parametrize('with_pe', [False, True])
@pytest.mark.parametrize('with_cls', [False, True])
@pytest.mark.parametrize('dims', [(16, 10, 25, 2), (16, 3, 18, 2), (1, 1, 1, 1), (16, 100, 25, 2)])
def test_tokens(dims, with_cls, with_pe):
    from agcn_amd import ops
    dev = _gpu()
    C, Tp, V, M = dims
    N, D = 2, V * C
    L = M * Tp + with_cls
    g = torch.Generator().manual_seed(C + Tp + V)
    x = torch.randn(N * M, C, Tp, V, generator=g).float()
    cls = torch.randn(1, 1, D, generator=g).float() if with_cls else None
    pe = torch.randn(1, L + 3, D, generator=g).float() if with_pe else None
    r = torch.randn(N, L, D, generator=g).float()
    ts64 = [t if t is None else t.double().requires_grad_(True) for t in (x, cls, pe)]
    (ops.tokens_ref(*ts64, M) * r.double()).sum().backward()
    ts = [t if t is None else t.to(dev).requires_grad_(True) for t in (x, cls, pe)]
    tok = ops.TokensFunction.apply(*ts, M)
    (tok * r.to(dev)).sum().backward()
    torch.cuda.synchronize()
    assert torch.equal(tok.detach().cpu(), ops.tokens_ref(x, cls, pe, M))          # bit for bit
    for a, b in zip(ts, ts64):
        if a is not None:
            assert rel(a.grad, b.grad) < TOL
    if with_pe:
        assert float(ts[2].grad[:, L:].abs().max()) == 0.0                         # rows no token reads


def test_bit_reproducible():
    """Forward and backward of the three Functions twice in one process: the same bits."""
    from agcn_amd import ops
    dev = _gpu()
    g = torch.Generator().manual_seed(21)
    N, L, H, dh, M, C, V = 3, 21, 2, 200, 2, 16, 25
    D = H * dh
    x = torch.randn(N * M, C, 10, V, generator=g).to(dev)
    cls, pe = torch.randn(1, 1, D, generator=g).to(dev), torch.randn(1, 30, D, generator=g).to(dev)
    lw, lb = (torch.rand(D, generator=g) + 0.5).to(dev), torch.randn(D, generator=g).to(dev)
    keep = (torch.rand(N, H, L, L, generator=g) >= 0.2).to(torch.uint8).to(dev)
    null = (torch.rand(N, L, generator=g) < 0.3).to(torch.uint8)
    null[:, 0] = 0
    null = null.to(dev)
    runs = []
    for _ in range(2):
        leaves = [t.clone().requires_grad_(True) for t in (x, cls, pe, lw, lb)]
        tok = ops.TokensFunction.apply(leaves[0], leaves[1], leaves[2], M)
        qkv = torch.cat((tok, 0.5 * tok, tok.flip(1)), dim=-1) * 0.3          # (elementwise: no vendor GEMM in this test)
        ctx, avg = ops.MHAFunction.apply(qkv, H, null, 1, keep, 1.25, True)
        out = ops.AddLayerNormFunction.apply(tok, ctx, leaves[3], leaves[4], 1e-5)
        torch.sin(out).sum().backward()
        runs.append([tok, ctx, avg, out] + [t.grad for t in leaves])
    torch.cuda.synchronize()
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    assert all(float(t.detach().abs().max()) > 0 for t in runs[0])
