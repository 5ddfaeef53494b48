"""Host-side operators of the AGCN hot path: thin wrappers over the C-ABI (``lib.py``) and the
``torch.autograd.Function``s that chain them into unit_gcn / unit_tcn / TCN_GCN_unit forward+backward.

Tensors are (N', C, T, V) contiguous fp32 on the GPU, allocated by PyTorch's caching allocator; the
extension never allocates or keeps device memory.  Everything here launches on the current stream.

Maths: SURVEY.md Appendix A (checked against the reference ``agcn.py:92-109`` by the oracle tests).
"""
import collections
import math
import os
import weakref

import numpy as np
import torch

from . import lib as _lib

BN_EPS = 1e-5
BN_MOMENTUM = 0.1


def _L():
    return _lib.load()


def _empty(shape, like):
    return torch.empty(shape, dtype=torch.float32, device=like.device)


def _ws(nbytes, like):
    """Byte workspace (packed weight images etc.) from the caching allocator."""
    return torch.empty((int(nbytes) + 3) // 4, dtype=torch.float32, device=like.device)


def _conv_ws(Cin, Cout, T, V, taps, stride, like, pad=None):
    pad = (taps - 1) // 2 if pad is None else pad
    n = _L().agcn_tconv_workspace(Cin, Cout, T, V, taps, stride, pad)
    return _ws(n, like), n


def _gcn_ws(C, Cout, T, V, like):
    n = _L().agcn_gcn_workspace(C, Cout, T, V)
    return _ws(n, like), n


def _scratch(width, like):
    """Scratch for the two-stage column reductions (agcn_colsum_scratch_bytes)."""
    nbytes = _L().agcn_colsum_scratch_bytes(int(width))
    return torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=like.device)


# ------------------------------------------------------------------------------------------------
# thin wrappers (one C entry point each)
# ------------------------------------------------------------------------------------------------

# ---- side stream for the weight gradients (AGCN_SIDE_STREAM=0 disables): they do not feed the backward's critical path
# (dx), so they run beside the backward-data kernels and the two fill the tails of each other's grids (+1 % on the
# training step, same-box A/B; results are bitwise the same: no kernel changes, only their placement) ----
_SIDE = {}


def side_stream_enabled():
    return os.environ.get('AGCN_SIDE_STREAM', '1') != '0'


_SIDE_SCOPE = [0]     # > 0 while a backward that joins once at its end is running (TCNGCNUnitFunction)


def _side_run(fn, inputs):
    """Run fn() on the side stream after everything enqueued so far on the current stream; returns its result.  The
    caller must _side_join() before the results are consumed on the current stream.  Only inside the fused unit's
    backward: the stand-alone unit_gcn / unit_tcn nodes (AAGCN) join right after their one weight-gradient kernel, which
    measured 1.2 % SLOWER than no side stream at all."""
    if not side_stream_enabled() or _SIDE_SCOPE[0] <= 0:
        return fn()
    main = torch.cuda.current_stream()
    dev = main.device_index
    side = _SIDE.get(dev)
    if side is None:
        side = _SIDE[dev] = torch.cuda.Stream(device=dev)
    side.wait_stream(main)
    with torch.cuda.stream(side):
        out = fn()
    for t in inputs:
        if t is not None:
            t.record_stream(side)
    outs = out if isinstance(out, (tuple, list)) else (out,)
    for t in outs:
        if torch.is_tensor(t):
            t.record_stream(main)
    return out


def _side_join():
    if side_stream_enabled():
        main = torch.cuda.current_stream()
        side = _SIDE.get(main.device_index)
        if side is not None:
            main.wait_stream(side)


def fused_amax_enabled():
    """AGCN_FUSED_AMAX=0: the split-fp16 convolutions compute their operand's maximum in a pass of their own (A/B)."""
    return os.environ.get('AGCN_FUSED_AMAX', '1') != '0'


# max |out| of the last unit output a BatchNorm pass produced, for the f16x3 chain of the unit that consumes it:
# (weak reference to the tensor, its version counter, the device scalar).  Taken only by the very tensor object it
# describes, unmodified since; anything else makes the chain take the maximum with a pass of its own.
_OUT_AMAX = [None]
_OUT_AMAX_STATS = [0, 0]      # [misses, hits] of _take_out_amax (diagnostic)


def _note_out_amax(t, amax):
    _OUT_AMAX[0] = (weakref.ref(t), t._version, amax) if amax is not None else None


def _take_out_amax(t):
    e = _OUT_AMAX[0]
    hit = e is not None and e[0]() is t and t._version == e[1]
    _OUT_AMAX_STATS[int(hit)] += 1
    return e[2] if hit else None


def conv_out_frames(T, taps, stride, pad=None):
    """Output frames of the (taps x 1) temporal convolution; pad None = (taps-1)//2 (reference unit_tcn / TCNUnit
    with pad=True), 0 for TCNUnit(pad=False) (aagcn.py:194)."""
    pad = (taps - 1) // 2 if pad is None else pad
    return (T + 2 * pad - taps) // stride + 1


def conv_fwd(x, w, b, stride=1, want_stats=False, x_amax=None, pad=None):
    """y = conv2d(x, w(k,1), b, stride=(s,1), padding=(pad,0)), pad None = (k-1)//2; optional per-channel (sum,sumsq)
    partials.  Every kernel size 1..9, stride 1..9 and padding 0..(k-1)//2 (agcn_tconv_fwd)."""
    N, Cin, T, V = x.shape
    Cout, Cin2, taps, one = w.shape
    assert Cin2 == Cin and one == 1
    pad = (taps - 1) // 2 if pad is None else pad
    To = conv_out_frames(T, taps, stride, pad)
    if To < 1:
        raise ValueError(f"agcn_amd: a {taps}-frame kernel with padding {pad} does not fit {T} frames")
    y = _empty((N, Cout, To, V), x)
    stats = None
    if want_stats:
        nt = _L().agcn_tconv_stats_tiles(Cin, Cout, To, V, taps, stride, pad)
        stats = _empty((N * nt, 2, Cout), x)
    ws, nb = _conv_ws(Cin, Cout, T, V, taps, stride, x, pad)
    # x_amax: 1-element tensor with max |x| left by bn_act_fwd(..., want_amax=True): the split-fp16 temporal convolution
    # then skips its own pass over x
    _lib.call("agcn_tconv_fwd", x, w, b, y, stats, ws, nb, N, Cin, Cout, T, V, taps, stride, pad, x_amax)
    return y, stats


def conv_bwd_data(dy, w, x_shape, stride=1, out=None, accumulate=False, add1=None, mask1=None, add2=None,
                  mask2=None, dy_amax=None, pad=None):
    N, Cin, T, V = x_shape
    Cout, _, taps, _ = w.shape
    pad = (taps - 1) // 2 if pad is None else pad
    dx = out if out is not None else _empty(x_shape, dy)
    ws, nb = _conv_ws(Cin, Cout, T, V, taps, stride, dy, pad)
    _lib.call("agcn_tconv_bwd_data", dy, w, dx, int(accumulate), add1, mask1, add2, mask2, ws, nb, N, Cin, Cout, T, V,
              taps, stride, pad, dy_amax)
    return dx


def conv_bwd_weight(dy, x, w_shape, stride=1, dy_amax=None, x_amax=None, pad=None):
    """dy_amax / x_amax: device scalars max |dy| / max |x| left behind by their producers; with both, the tap-free
    gradients run on f16x3 (agcn_tconv_bwd_weight)."""
    N, Cin, T, V = x.shape
    Cout, _, taps, _ = w_shape
    pad = (taps - 1) // 2 if pad is None else pad
    nbytes = _L().agcn_tconv_bwd_weight_workspace(N, Cin, Cout, T, V, taps, stride, pad)
    ws = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=x.device)
    dw = _empty(tuple(w_shape), x)
    _lib.call("agcn_tconv_bwd_weight", dy, x, dw, ws, nbytes, N, Cin, Cout, T, V, taps, stride, pad, dy_amax, x_amax)
    return dw


def adjacency_fwd(tp, A, PA, alpha=None):
    """tp: (N, 6Ci, T, V) theta/phi; returns P (softmax) and adj = [alpha*]P + A + PA, both (N,3,V,V)."""
    N, C6, T, V = tp.shape
    Ci = C6 // 6
    nt = _L().agcn_scores_num_tiles(V, T)
    spart = _empty((N, 3, nt, V, V), tp)
    P = _empty((N, 3, V, V), tp)
    adj = _empty((N, 3, V, V), tp)
    _lib.call("agcn_adjacency_fwd", tp, A, PA, alpha, spart, P, adj, N, Ci, T, V)
    return P, adj


def adjacency_fused_supported(C, Ci, T, V):
    return bool(_L().agcn_adjacency_fused_supported(int(C), int(Ci), int(T), int(V)))


def adjacency_recompute():
    """Backward policy of the adaptive branch: recompute theta/phi on chip from x (AGCN_ADJ_RECOMPUTE=1: nothing of
    size 6*Ci*T*V is kept per layer) or re-read the copy the fused forward leaves behind as a by-product (default:
    measured faster on MI355X)."""
    return os.environ.get('AGCN_ADJ_RECOMPUTE', '0') == '1'


def adjacency_fused_fwd(x, wab, bab, A, PA, alpha=None, keep_tp=False, x_amax_out=None, x_amax=None):
    """P, adj straight from x: [theta;phi] = wab.x + bab is formed and reduced on chip (no tp round trip); wab
    (6Ci, C[,1,1]).  keep_tp: also return theta/phi, written once as a by-product (never re-read by the forward).
    x_amax_out: optional 1-element tensor that receives max |x| (the pass reads all of x anyway); x_amax: the same
    scalar where the producer of x already took it."""
    N, C, T, V = x.shape
    Ci = wab.shape[0] // 6
    tp = _empty((N, 6 * Ci, T, V), x) if keep_tp else None
    nt = _L().agcn_scores_num_tiles(V, T)
    spart = _empty((N, 3, nt, V, V), x)
    P = _empty((N, 3, V, V), x)
    adj = _empty((N, 3, V, V), x)
    nb = _L().agcn_adjacency_fused_workspace(C, Ci)
    ws = _ws(nb, x)
    _lib.call("agcn_adjacency_fused_fwd_ex", x, wab.reshape(6 * Ci, C), bab, A, PA, alpha, tp, spart, P, adj,
              x_amax_out, x_amax, ws, nb, N, C, Ci, T, V)
    return (P, adj, tp) if keep_tp else (P, adj)


def first_layer_enabled():
    """AGCN_FIRST_LAYER=0 keeps the 3-channel layer on the generic kernels (A/B)."""
    return os.environ.get('AGCN_FIRST_LAYER', '1') != '0'


def gcn_first_fwd(x, adj, wcat, bias, wdown, bdown, want_stats=False):
    """First-layer unit_gcn forward (C <= 4): ypre = bias + sum_i Wd_i (x . adj_i) and dpre = bdown + Wdown x with
    their BatchNorm partials, one pass over x."""
    N, C, T, V = x.shape
    Cout = wcat.shape[0]
    ypre, dpre = _empty((N, Cout, T, V), x), _empty((N, Cout, T, V), x)
    st = st2 = None
    if want_stats:
        nt = _L().agcn_gcn_first_tiles(T, V)
        st, st2 = _empty((N * nt, 2, Cout), x), _empty((N * nt, 2, Cout), x)
    wdown2 = wdown.reshape(Cout, C).contiguous()
    _lib.call("agcn_gcn_first_fwd", x, adj, wcat, bias, wdown2, bdown, ypre, st, dpre, st2, N, C, Cout, T, V)
    return ypre, st, dpre, st2


def aggregate_project_fwd(x, adj, wcat, bias, want_stats=False, x_amax=None):
    """y = sum_i Wd_i (x . adj_i) + bias ; wcat: (Cout, 3C) = [Wd_0 | Wd_1 | Wd_2]."""
    N, C, T, V = x.shape
    Cout = wcat.shape[0]
    y = _empty((N, Cout, T, V), x)
    stats = None
    if want_stats:
        stats = _empty((_L().agcn_gcn_stats_slots(N, C, Cout, T, V), 2, Cout), x)
    ws, nb = _gcn_ws(C, Cout, T, V, x)
    _lib.call("agcn_gcn_aggregate_project_fwd_ex", x, adj, wcat, bias, y, stats, ws, nb, N, C, Cout, T, V, x_amax)
    return y, stats


def aggregate_project_bwd_data(dy, adj, wcat, x_shape, out=None, accumulate=False, add1=None, mask1=None,
                               add2=None, mask2=None, dtp=None, wab=None, dy_amax=None, dtp_amax=None):
    """dx (+)= sum_i Wd_i^T (dy . adj_i^T) + add1*[mask1] + add2*[mask2] [+ wab^T dtp].  The masks are fp32 tensors
    (> 0 passes) or, both of them, int32 sign bit masks (bn_act_fwd(..., want_bits=True)).  dtp/wab: the 1x1 term of
    the adaptive branch fused into the same pass (only where fused_bwd_data_supported says so)."""
    N, C, T, V = x_shape
    Cout = wcat.shape[0]
    dx = out if out is not None else _empty(x_shape, dy)
    ws, nb = _gcn_ws(C, Cout, T, V, dy)
    kinds = {m.dtype for m in (mask1, mask2) if m is not None}
    if len(kinds) > 1:
        raise RuntimeError("agcn_amd: mask1 and mask2 must be of one kind (fp32 tensors or int32 sign bit masks)")
    mbits = int(torch.int32 in kinds)
    # the masks are declared const float* and hold either kind under mask_bits: checked here, passed as addresses
    mp = _lib.ptr_bits if mbits else _lib.ptr
    K2, w2 = 0, None
    if dtp is not None:
        K2 = dtp.shape[1]
        w2 = wab.reshape(K2, C)
    else:
        dtp_amax = None
    _lib.call("agcn_gcn_aggregate_project_bwd_data_ex", dy, adj, wcat, dtp, w2, K2, dx, int(accumulate), add1,
              mp(mask1), add2, mp(mask2), mbits, ws, nb, N, C, Cout, T, V, dy_amax, dtp_amax)
    return dx


def fused_bwd_data_supported(C, Cout, V):
    return bool(_L().agcn_gcn_bwd_data_fused_supported(int(C), int(Cout), int(V)))


def project_bwd_weight(dy, x, adj, Cout, dy_amax=None, x_amax=None):
    N, C, T, V = x.shape
    nbytes = _L().agcn_gcn_project_bwd_weight_workspace(N, C, Cout, T, V)
    ws = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=x.device)
    dw = _empty((Cout, 3 * C), x)
    _lib.call("agcn_gcn_project_bwd_weight_ex", dy, x, adj, dw, ws, nbytes, N, C, Cout, T, V, dy_amax, x_amax)
    return dw


def adjacency_bwd(dy, wcat, x, tp, P, alpha=None, wab=None, bab=None, dy_amax=None, x_amax=None):
    """Gradient of the adaptive adjacency branch.  Returns dPA (3,V,V), dtp (N,6Ci,T,V), dbab (6Ci), dalpha, dadj and
    the device scalar max |dtp| its producer left behind (None where it does not: the consumers take it themselves).
    tp = None: theta/phi were never stored (adjacency_fused_fwd); they are recomputed from x, wab, bab on chip."""
    N, C, T, V = x.shape
    Cout = wcat.shape[0]
    Ci = (tp.shape[1] if tp is not None else wab.shape[0]) // 6
    nslots = _L().agcn_dadj_num_slots(C, V, T)
    if nslots <= 0:
        raise ValueError(f"agcn_amd: the adjacency gradient does not support {C} input channels (V = {V}): supported are "
                         "widths below 64 and multiples of 64, with V <= 32")
    dpart = _empty((N, 3, nslots, V, V), x)
    ws, nb = _gcn_ws(C, Cout, T, V, x)
    _lib.call("agcn_gcn_dadj_ex", dy, wcat, x, dpart, ws, nb, N, C, Cout, T, V, dy_amax, x_amax)
    dadj = _empty((N, 3, V, V), x)
    dS = _empty((N, 3, V, V), x)
    dPA = _empty((3, V, V), x)
    dal_part = _empty((N * 3,), x) if alpha is not None else None
    _lib.call("agcn_adjacency_bwd_softmax", dpart, P, alpha, dadj, dS, dPA, dal_part, N, Ci, T, V, nslots)
    nt = _L().agcn_scores_num_tiles(V, T)
    dtp = _empty((N, 6 * Ci, T, V), x)
    dbpart = _empty((N * nt, 6 * Ci), x)
    dbab = _empty((6 * Ci,), x)
    scratch = _scratch(6 * Ci, x)
    dtp_amax = None
    if tp is None:
        nb = _L().agcn_adjacency_fused_workspace(C, Ci)
        ws = _ws(nb, x)
        _lib.call("agcn_adjacency_fused_bwd_scores", x, wab.reshape(6 * Ci, C), bab, dS, dtp, dbpart, scratch, dbab, ws,
                  nb, N, C, Ci, T, V)
    else:
        dtp_amax = _empty((1,), x) if fused_amax_enabled() else None
        _lib.call("agcn_adjacency_bwd_scores_ex", tp, dS, dtp, dbpart, scratch, dbab, dtp_amax, N, Ci, T, V)
    dalpha = dal_part.sum() if dal_part is not None else None
    return dPA, dtp, dbab, dalpha, dadj, dtp_amax


def stc_row_reduce(y, g=None, wv=None, wt=None, want_t=False, want_v=False, scale_t=1.0, scale_v=1.0):
    """One pass over y (N,C,T,V) [times g elementwise]: out_t (N,C,T) = scale_t * sum_v wv[n,v]*y*g and / or
    out_v (N,C,V) = scale_v * sum_t wt[...,t]*y*g ; wv (N,V), wt (N,T) or (N,C,T); None weights = ones."""
    N, C, T, V = y.shape
    out_t = _empty((N, C, T), y) if want_t else None
    out_v = _empty((N, C, V), y) if want_v else None
    per_row = int(wt is not None and wt.dim() == 3)
    _lib.call("agcn_stc_row_reduce", y, g, wv, wt, per_row, out_t, out_v, float(scale_t), float(scale_v), N, C, T, V)
    return out_t, out_v


# ---- the small operators around the unit stack (csrc/small_ops.hip): deterministic, no vendor library --------------
def linear_fwd(x, w, b, act=0):
    """out = act(x @ w.T + b); act 0 identity, 1 ReLU, 2 "1 + sigmoid".  x (N, K), w (O, K)."""
    N, K = x.shape
    O = w.shape[0]
    out = _empty((N, O), x)
    _lib.call("agcn_linear_fwd", x, w, b, out, N, K, O, int(act))
    return out


def linear_bwd(dout, out, x, w, act=0, need_din=True):
    """Returns din (or None), dw, db of linear_fwd."""
    N, K = x.shape
    O = w.shape[0]
    dpre = _empty((N, O), x)
    din = _empty((N, K), x) if need_din else None
    dw, db = _empty((O, K), x), _empty((O,), x)
    _lib.call("agcn_linear_bwd", dout, out, x, w, dpre, din, dw, db, N, K, O, int(act))
    return din, dw, db


def gate_conv_fwd(x, w, b):
    """a (N, L) = 1 + sigmoid(Conv1d(C -> 1, Ks, padding (Ks-1)/2)(x)); x (N, C, L), w (1, C, Ks), b (1)."""
    N, C, L = x.shape
    Ks = w.shape[-1]
    a = _empty((N, L), x)
    _lib.call("agcn_gate_conv_fwd", x, w.reshape(C, Ks), b, a, N, C, L, Ks)
    return a


def gate_conv_bwd(da, a, x, w):
    """Returns dx (N, C, L), dw (1, C, Ks), db (1) of gate_conv_fwd given da = dL/da."""
    N, C, L = x.shape
    Ks = w.shape[-1]
    dpre = _empty((N, L), x)
    dx, dw, db = _empty((N, C, L), x), _empty((1, C, Ks), x), _empty((1,), x)
    _lib.call("agcn_gate_conv_bwd", da, a, x, w.reshape(C, Ks), dpre, dx, dw, db, N, C, L, Ks)
    return dx, dw, db


class DataBNFunction(torch.autograd.Function):
    """The model prologue (reference agcn.py:163-165): x (N, C, T, V, M) -> permute/view (N, M*V*C, T) -> BatchNorm1d ->
    view/permute -> (N*M, C, T, V), as three small deterministic kernels (statistics, finalize, apply).
    args: x, weight, bias, running_mean, running_var, training, sync"""

    @staticmethod
    def forward(ctx, x, w, b, rm, rv, training, sync=None):
        x = x.contiguous()
        N, C, T, V, M = x.shape
        CH = C * V * M
        if training:
            part = _empty((N, 2, CH), x)
            _lib.call("agcn_data_bn_stats", x, part, N, C, T, V, M)
            (st,), gcount = _bn_coeffs(True, [part], N * T, [(w, b, rm, rv)], sync, N)
        else:
            (st,), gcount = _bn_coeffs(False, [None], N * T, [(w, b, rm, rv)], None, N)
        out = _empty((N * M, C, T, V), x)
        _lib.call("agcn_data_bn_apply", x, st.scale, st.shift, out, N, C, T, V, M)
        ctx.st, ctx.sync, ctx.gcount, ctx.training = st, sync, gcount, training
        ctx.save_for_backward(x, w)
        return out

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        st, sync = ctx.st, ctx.sync
        dy = dy.contiguous()
        N, C, T, V, M = x.shape
        CH = C * V * M
        # the reduce stage feeds the statistics' correction terms of dx (train) and dgamma / dbeta; with frozen statistics
        # (eval) dx = gamma*invstd_run*dy is the apply stage with the two sums at zero (exactly: its correction terms are
        # products with 0) and the sums, taken at the running mean / invstd, are needed for dgamma / dbeta only
        ng = ctx.needs_input_grad
        sums = None
        if ctx.training or ng[1] or ng[2]:
            part = _empty((N, 2, CH), x)
            _lib.call("agcn_data_bn_bwd_reduce", dy, x, st.mean, st.invstd, part, N, C, T, V, M)
            sums = _colsum(part, N, 2 * CH)
        scale = 1.0
        if ctx.training and sync is not None:
            sums = _allreduce_sum(sums, sync)
            scale = 1.0 / sync.world       # global sums, restored by the gradient average of the data-parallel step
        dx = dgamma = dbeta = None
        if ng[0]:
            dx = torch.empty_like(x)
            corr = sums if ctx.training else torch.zeros(2 * CH, dtype=torch.float32, device=x.device)
            _lib.call("agcn_data_bn_bwd_apply", dy, x, w, st.mean, st.invstd, corr, float(ctx.gcount), dx, N, C, T, V,
                      M)
        if sums is not None:
            dbeta, dgamma = sums[:CH], sums[CH:]
            if scale != 1.0:
                dbeta, dgamma = dbeta * scale, dgamma * scale
        return dx, dgamma, dbeta, None, None, None, None


def data_bn_supported(bn):
    """Plain / synchronised BatchNorm1d only (GhostBatchNorm1d keeps its own module path)."""
    return type(bn) in (torch.nn.BatchNorm1d, torch.nn.SyncBatchNorm)


class PoolFCFunction(torch.autograd.Function):
    """The model epilogue (reference agcn.py:179-183): mean over (T, V) per person, mean over persons, Linear.
    args: x (N*M, C, T, V), fc weight (K, C), fc bias (K), M"""

    @staticmethod
    def forward(ctx, x, w, b, M):
        x = x.contiguous()
        NM, C, T, V = x.shape
        N = NM // M
        rowmean, pooled = _empty((NM, C), x), _empty((N, C), x)
        _lib.call("agcn_pool_fwd", x, rowmean, pooled, N, M, C, T * V)
        logits = linear_fwd(pooled, w, b, 0)
        ctx.save_for_backward(pooled, logits, w)
        ctx.shape, ctx.M = (NM, C, T, V), M
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        pooled, logits, w = ctx.saved_tensors
        NM, C, T, V = ctx.shape
        M = ctx.M
        dpooled, dw, db = linear_bwd(dlogits.contiguous(), logits, pooled, w, 0, need_din=True)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = _empty((NM, C, T, V), pooled)
            _lib.call("agcn_pool_bwd", dpooled, dx, NM // M, M, C, T * V)
        return dx, dw, db, None


class STCAttentionFunction(torch.autograd.Function):
    """AAGCN's three attention gates (reference aagcn.py:59-116 applied at :268-270) as ONE autograd node:
        y3 = y * (1+se_s[n,v]) * (1+se_t[n,t]) * (1+se_c[n,c])
    Full-tensor work = HIP passes (forward: two reductions + one apply = 3 reads, 1 write of the activation; backward:
    one pass over (dout, y), one over y, one apply = 4 reads, 1 write); the gate networks (Conv1d C->1 over joints /
    frames, two Linears) act on (N,C,V) / (N,C,T) / (N,C) tensors and run as ordinary tensor code, differentiated by
    explicit small kernels too (gate_conv_* / linear_* above).
    args: y, sa_w (1,C,Ks), sa_b (1), ta_w (1,C,9), ta_b (1), fc1_w, fc1_b, fc2_w, fc2_b"""

    @staticmethod
    def _gates(m_s, mv1, sa_w, sa_b, ta_w, ta_b, f1w, f1b, f2w, f2b, a_s=None):
        """a_s (N,V) from mean_t y; a_t (N,T) from mean_v y1; a_c (N,C) from mean_t(a_t * mean_v y1).  The gate
        networks are the deterministic kernels of csrc/small_ops.hip (gate convolution, small Linear).
        Returns (a_s, a_t, a_c, m_c, h) with m_c / h the channel gate's input and hidden activations."""
        if a_s is None:
            a_s = gate_conv_fwd(m_s, sa_w, sa_b)
        if mv1 is None:
            return a_s, None, None, None, None
        a_t = gate_conv_fwd(mv1, ta_w, ta_b)
        m_c = (mv1 * a_t.unsqueeze(1)).mean(-1)
        h = linear_fwd(m_c, f1w, f1b, 1)
        a_c = linear_fwd(h, f2w, f2b, 2)
        return a_s, a_t, a_c, m_c, h

    @staticmethod
    def forward(ctx, y, sa_w, sa_b, ta_w, ta_b, f1w, f1b, f2w, f2b):
        y = y.contiguous()
        N, C, T, V = y.shape
        par = (sa_w, sa_b, ta_w, ta_b, f1w, f1b, f2w, f2b)
        _, m_s = stc_row_reduce(y, want_v=True, scale_v=1.0 / T)                         # mean_t y
        a_s = STCAttentionFunction._gates(m_s, None, *par)[0]
        mv1, _ = stc_row_reduce(y, wv=a_s, want_t=True, scale_t=1.0 / V)                 # mean_v y*(1+se_s)
        _, a_t, a_c, m_c, h = STCAttentionFunction._gates(m_s, mv1, *par, a_s=a_s)
        out = torch.empty_like(y)
        # the gated tensor feeds the f16x3 temporal convolution (and its weight gradient): leave its maximum behind
        o_amax = _empty((1,), y) if fused_amax_enabled() else None
        INFER_STATS['stc_apply'] += 1
        _lib.call("agcn_stc_apply_ex", y, a_s, a_t, a_c, out, o_amax, N, C, T, V)
        _note_out_amax(out, o_amax)
        ctx.save_for_backward(y, m_s, mv1, a_s, a_t, a_c, m_c, h, *par)
        return out

    @staticmethod
    def backward(ctx, dout):
        y, m_s, mv1, a_s, a_t, a_c, m_c, h, *par = ctx.saved_tensors
        sa_w, sa_b, ta_w, ta_b, f1w, f1b, f2w, f2b = par
        dout = dout.contiguous()
        N, C, T, V = y.shape
        # one pass over (dout, y): P1[n,c,t] = sum_v a_s dout*y ; P2[n,c,v] = sum_t a_t dout*y
        P1, P2 = stc_row_reduce(y, g=dout, wv=a_s, wt=a_t, want_t=True, want_v=True)
        da_c = (P1 * a_t.unsqueeze(1)).sum(-1).contiguous()
        da_t = (P1 * a_c.unsqueeze(-1)).sum(1)
        da_s = (P2 * a_c.unsqueeze(-1)).sum(1)
        # channel gate: a_c = 1 + sigmoid(fc2(relu(fc1(m_c)))), m_c = mean_t(a_t * mv1)
        dh, df2w, df2b = linear_bwd(da_c, a_c, h, f2w, 2)
        dm_c, df1w, df1b = linear_bwd(dh, h, m_c, f1w, 1)
        da_t = (da_t + (dm_c.unsqueeze(-1) * mv1).sum(1) / T).contiguous()
        dmv1 = dm_c.unsqueeze(-1) * a_t.unsqueeze(1) / T
        # temporal gate: a_t = 1 + sigmoid(conv_9(mv1))
        dmv1_t, dta_w, dta_b = gate_conv_bwd(da_t, a_t, mv1, ta_w)
        dmv1 = ((dmv1 + dmv1_t) / V).contiguous()       # mv1 = (1/V) sum_v y*a_s
        # its two other consumers: y (folded into the apply pass below) and a_s
        _, R = stc_row_reduce(y, wt=dmv1, want_v=True)
        da_s = (da_s + R.sum(1)).contiguous()
        # spatial gate: a_s = 1 + sigmoid(conv_V(m_s)), m_s = (1/T) sum_t y
        dm_s, dsa_w, dsa_b = gate_conv_bwd(da_s, a_s, m_s, sa_w)
        dms = (dm_s / T).contiguous()
        dy = torch.empty_like(y)
        _lib.call("agcn_stc_bwd_apply", dout, a_s, a_t, a_c, dmv1, dms, dy, N, C, T, V)
        return dy, dsa_w, dsa_b, dta_w, dta_b, df1w, df1b, df2w, df2b


class BNState:
    """Per-BatchNorm forward products kept for the backward.  ``S`` > 1: GhostBatchNorm (reference
    model/layers/module/ghostbatchnorm.py:77-120) -- the statistics are per virtual sub-batch s = n % S, which is an
    ordinary BatchNorm over (N/S, S*C, T, V): the HIP stages are simply called with that shape (channel index of a row
    = (n*C + c) % (S*C) = (n % S)*C + c), the coefficient vectors hold S*C entries and the shared weight/bias are
    repeated S times; nothing in the kernels changes.  ``eval``: the stage ran on the frozen running statistics; ``mean``
    / ``invstd`` are then copies of the running mean and 1/sqrt(running_var + eps) and ``bn_bwd`` takes the one-pass
    eval-mode backward (always plain BatchNorm: S = 1)."""
    __slots__ = ("mean", "invstd", "scale", "shift", "S", "eval")

    def __init__(self):
        self.S = 1
        self.eval = False


class SyncBN:
    """BatchNorm statistics policy of ONE unit's HIP BatchNorm stages, carried by the calling module and stored on the
    autograd context (no process-global state: two models with different policies can live in one process).
    ``None`` = per replica (reference nn.DataParallel semantics, utils/processor.py:336-343).  ``SyncBN(world, group)``
    = synchronised over the process group like the reference's DDP path (SyncBatchNorm.convert_sync_batchnorm,
    processor.py:295): the per-channel sums are all-reduced between the two stages of the forward statistics (ONE
    collective for the main and the down/residual BatchNorm together) and of the backward (one collective)."""
    __slots__ = ("world", "group")

    def __init__(self, world, group=None):
        self.world, self.group = int(world), group


def sync_of(bn_module):
    """SyncBN policy implied by a BatchNorm module: the reference converts the model with
    ``SyncBatchNorm.convert_sync_batchnorm`` before DDP (processor.py:295); the HIP units only borrow the BN modules'
    parameters, so the conversion is honoured by looking at the module's class."""
    import torch.distributed as dist
    if isinstance(bn_module, torch.nn.SyncBatchNorm) and dist.is_available() and dist.is_initialized():
        world = dist.get_world_size(bn_module.process_group)
        if world > 1:
            return SyncBN(world, bn_module.process_group)
    return None


def _colsum(slab, nslots, width):
    out = _empty((width,), slab)
    scratch = _scratch(width, slab)
    _lib.call("agcn_colsum", slab, int(nslots), int(width), scratch, out)
    return out


COLLECTIVES = {'bn': 0, 'grad': 0}      # diagnostic: collectives issued so far (bench.py reports them per step)


def _allreduce_sum(t, sync):
    import torch.distributed as dist
    COLLECTIVES['bn'] += 1
    dist.all_reduce(t, op=dist.ReduceOp.SUM, group=sync.group)
    return t


def sync_stats(stats_parts, count, sync):
    """Global (sum, sumsq) of several BatchNorm stages of one unit with ONE all-reduce: every slab is reduced over its
    slots locally, the per-channel sums travel in one buffer, and each stage gets back a 1-slot slab.  Every rank must
    hold the same number of elements per channel (equal per-rank batches: the trainer's sampler pads like torch's
    DistributedSampler), so the global count is count * world.  Returns [slab (1,2,C) ...]."""
    sums = [_colsum(sp, sp.shape[0], sp.shape[1] * sp.shape[2]) for sp in stats_parts]
    buf = torch.cat(sums) if len(sums) > 1 else sums[0]
    _allreduce_sum(buf, sync)
    out, o = [], 0
    for sp in stats_parts:
        w = sp.shape[1] * sp.shape[2]
        out.append(buf[o:o + w].view(1, 2, sp.shape[2]))
        o += w
    return out


def bn_train_coeffs(stats_part, count, gamma, beta, running_mean, running_var, momentum=BN_MOMENTUM, eps=BN_EPS):
    """stats_part: (slots, 2, C) partial (sum, sumsq); count: elements per channel behind them (python number)."""
    C = gamma.numel()
    st = BNState()
    st.mean, st.invstd = _empty((C,), gamma), _empty((C,), gamma)
    st.scale, st.shift = _empty((C,), gamma), _empty((C,), gamma)
    nslots = stats_part.shape[0]
    scratch = _scratch(2 * C, gamma)
    _lib.call("agcn_bn_stats_finalize", stats_part, nslots, C, float(count), gamma, beta, running_mean, running_var,
              float(momentum), float(eps), scratch, st.mean, st.invstd, st.scale, st.shift)
    return st


def bn_eval_coeffs(gamma, beta, running_mean, running_var, eps=BN_EPS):
    C = gamma.numel()
    st = BNState()
    st.eval = True
    st.scale, st.shift = _empty((C,), gamma), _empty((C,), gamma)
    st.mean, st.invstd = _empty((C,), gamma), _empty((C,), gamma)     # frozen statistics, for the eval-mode backward
    _lib.call("agcn_bn_eval_coeff_ex", gamma, beta, running_mean, running_var, float(eps), C, st.scale, st.shift,
              st.mean, st.invstd)
    return st


def bn_act_fwd(y1, st1, r=None, st2=None, relu=True, want_bits=False, amax_out=None):
    """out = act(scale1*y1 + shift1 + res); res = 0 (r None) | r (st2 None) | scale2*r + shift2.
    want_bits: also return the sign bit mask of ``out`` (int32 words, 32 elements each) for the BatchNorm backward."""
    N, C, T, V = y1.shape
    if st1.S > 1:                      # GhostBatchNorm: (N, C) rows regrouped as (N/S, S*C)
        N, C = N // st1.S, C * st1.S
    out = torch.empty_like(y1)
    bits = torch.empty((y1.numel() + 31) // 32, dtype=torch.int32, device=y1.device) if want_bits else None
    mode = 0 if r is None else (1 if st2 is None else 2)
    # amax_out: optional 1-element tensor that receives max |out| (for the split-fp16 kernels that read `out` next)
    _lib.call("agcn_bn_act_fwd_ex", y1, st1.scale, st1.shift, r, st2.scale if st2 else None, st2.shift if st2 else None,
              out, bits, amax_out, N, C, T * V, mode, int(relu))
    return (out, bits) if want_bits else out


EVAL_BWD_STATS = {'sums': 0, 'nosums': 0}     # diagnostic: agcn_bn_bwd_eval launches with / without the row partials


def _mask_arg(mask):
    """(address, mask_bits) of a ReLU mask: the fp32 activation tensor (0) or its int32 sign bit words (1).  One C
    parameter takes either kind under the flag, so the kind is checked here and the address is what travels."""
    mbits = int(mask is not None and mask.dtype == torch.int32)
    return (_lib.ptr_bits(mask) if mbits else _lib.ptr(mask)), mbits


def bn_bwd_eval(dout, mask, y1, st1, y2=None, st2=None, want_sums=True, amax_out=None):
    """Backward through out = act(bn1(y1) [+ bn2(y2)] [+ identity]) with FROZEN statistics (``bn_eval_coeffs`` states):
    dy = scale[c] * dout * mask in one streaming pass (agcn_bn_bwd_eval), the parameter gradients from its row partials
    (agcn_bn_bwd_eval_finalize).  No sync collective, no GhostBatchNorm regrouping: eval is plain per-channel BN.
    Returns dy1, dgamma1, dbeta1, dbias1, dy2, dgamma2, dbeta2, dbias2: dbias = scale * sum dz is the gradient of the
    bias of the convolution in front of the BN (not zero here: only a batch mean would cancel it).  want_sums=False:
    y1 / y2 are not read and every parameter gradient is None."""
    N, C, T, V = dout.shape
    two = st2 is not None
    dy1 = torch.empty_like(dout)
    dy2 = torch.empty_like(dout) if two else None
    part = _empty((N * C * 3,), dout) if want_sums else None
    mptr, mbits = _mask_arg(mask)
    EVAL_BWD_STATS['sums' if want_sums else 'nosums'] += 1
    _lib.call("agcn_bn_bwd_eval", dout, mptr, mbits, y1 if want_sums else None, st1.scale,
              y2 if (want_sums and two) else None, st2.scale if two else None, int(want_sums), part, dy1, dy2, amax_out,
              N, C, T * V)
    if not want_sums:
        return dy1, None, None, None, dy2, None, None, None
    dg1, db1, dc1 = _empty((C,), dout), _empty((C,), dout), _empty((C,), dout)
    dg2 = db2 = dc2 = None
    if two:
        dg2, db2, dc2 = _empty((C,), dout), _empty((C,), dout), _empty((C,), dout)
    _lib.call("agcn_bn_bwd_eval_finalize", part, N, C, st1.scale, st1.mean, st1.invstd, st2.scale if two else None,
              st2.mean if two else None, st2.invstd if two else None, dg1, db1, dc1, dg2, db2, dc2)
    return dy1, dg1, db1, dc1, dy2, dg2, db2, dc2


def _bn_bwd_two_stage(grad, ins, outs, part, coef, amax_out, N, C, TV, sync, gcount):
    """The train-mode BatchNorm backward as reduce + apply instead of the fused ``agcn_bn_bwd``: where the apply stage
    also leaves max |dy1| behind (``amax_out``, for the split-fp16 kernels that read dy1 next) and / or the per-channel
    sums are all-reduced in between (``sync``).  grad = (dout, mask address, mask_bits), ins / outs: bn_bwd's tuples."""
    dout, mptr, mbits = grad
    _lib.call("agcn_bn_bwd_reduce", dout, mptr, mbits, ins[0], ins[4], part, N, C, TV)
    sums, nslots, total, scale = part, N, float(N) * float(TV), 1.0
    if sync is not None:
        # one collective for both branches; dgamma/dbeta come out as GLOBAL sums, scaled by 1/world so that the
        # gradient average of the data-parallel step restores them (every rank holds the same value)
        sums, nslots, scale = _allreduce_sum(_colsum(part, N, 3 * C), sync), 1, 1.0 / sync.world
        total = float(gcount) if gcount is not None else total * sync.world
    _lib.call("agcn_bn_bwd_apply_ex", sums, nslots, total, scale, dout, mptr, mbits, *ins, coef, *outs, amax_out, N, C,
              TV)


def bn_bwd(dout, mask, y1, gamma1, st1, y2=None, gamma2=None, st2=None, sync=None, gcount=None, amax_out=None,
           want_sums=True, bias_out=None):
    """Backward through out = relu(bn1(y1) [+ bn2(y2)] [+ identity]).  ``mask``: the fp32 output tensor (positive
    elements pass) or the int32 sign bit mask of ``bn_act_fwd(..., want_bits=True)``; None = no ReLU.
    Returns dy1, dgamma1, dbeta1, dy2, dgamma2, dbeta2 (branch-2 entries None without y2).
    Eval-mode states (frozen statistics) go to ``bn_bwd_eval``: ``want_sums=False`` skips the parameter gradients there,
    and ``bias_out`` (a list) receives the gradients of the two convolution biases in front of the BatchNorms, which
    train mode does not have (they are exactly zero)."""
    if st1.eval:
        dy1, dg1, db1, dc1, dy2, dg2, db2, dc2 = bn_bwd_eval(dout, mask, y1, st1, y2, st2 if y2 is not None else None,
                                                             want_sums, amax_out)
        if bias_out is not None:
            bias_out[:] = [dc1, dc2]
        return dy1, dg1, db1, dy2, dg2, db2
    N, C, T, V = y1.shape
    S = st1.S
    if S > 1:                          # GhostBatchNorm: see BNState; gamma repeated S times, dgamma/dbeta folded below
        N, C = N // S, C * S
        gamma1 = gamma1.repeat(S)
        gamma2 = gamma2.repeat(S) if gamma2 is not None else None
    part = _empty((N * C * 3,), y1)
    coef = _empty((6 * C,), y1)
    dy1 = torch.empty_like(y1)
    dg1, db1 = _empty((C,), y1), _empty((C,), y1)
    dy2 = dg2 = db2 = None
    if y2 is not None:
        dy2 = torch.empty_like(y2)
        dg2, db2 = _empty((C,), y1), _empty((C,), y1)
    grad = (dout, *_mask_arg(mask))
    ins = (y1, gamma1, st1.mean, st1.invstd, y2, gamma2, st2.mean if st2 else None, st2.invstd if st2 else None)
    outs = (dy1, dg1, db1, dy2, dg2, db2)
    if sync is None and amax_out is None:
        _lib.call("agcn_bn_bwd", *grad, *ins, part, coef, *outs, N, C, T * V)
    else:
        _bn_bwd_two_stage(grad, ins, outs, part, coef, amax_out, N, C, T * V, sync, gcount)
    if S > 1:                          # the weight / bias are shared by the S virtual sub-batches
        dg1, db1 = dg1.view(S, -1).sum(0), db1.view(S, -1).sum(0)
        if dg2 is not None:
            dg2, db2 = dg2.view(S, -1).sum(0), db2.view(S, -1).sum(0)
    return dy1, dg1, db1, dy2, dg2, db2


# ------------------------------------------------------------------------------------------------
# unit_gcn / unit_tcn forward and backward as plain functions; each forward returns its output and the state object
# its backward takes
# ------------------------------------------------------------------------------------------------

class _GCNState:
    """What gcn_forward leaves for gcn_backward.  ``x_amax`` / ``g_amax``: device scalars max |x| / max |out| (None
    where nobody took them); gamma1 / gamma2: the weights of the main and the `down` BatchNorm."""
    __slots__ = ('x', 'tp', 'P', 'adj', 'ypre', 'dpre', 'bits', 'bn1', 'bn2', 'sync', 'count', 'x_amax', 'g_amax',
                 'wab', 'bab', 'wd', 'gamma1', 'wdown', 'gamma2', 'alpha')

    def __init__(self, x, tp, P, adj, ypre, dpre, bits, bn1, bn2, sync, count, x_amax, g_amax, wab, bab, wd, gamma1,
                 wdown, gamma2, alpha):
        self.x, self.tp, self.P, self.adj, self.ypre, self.dpre, self.bits = x, tp, P, adj, ypre, dpre, bits
        self.bn1, self.bn2, self.sync, self.count, self.x_amax, self.g_amax = bn1, bn2, sync, count, x_amax, g_amax
        self.wab, self.bab, self.wd, self.gamma1, self.wdown, self.gamma2 = wab, bab, wd, gamma1, wdown, gamma2
        self.alpha = alpha


class _TCNState:
    """What tcn_forward leaves for tcn_backward.  ``g_amax``: device scalar max |g| or None; ``resx`` / ``rpre`` /
    ``wres`` / ``gamma2``: input, pre-BatchNorm output and parameters of the convolutional residual (else None)."""
    __slots__ = ('g', 'zpre', 'rpre', 'out', 'bits', 'bn1', 'bn2', 'sync', 'count', 'g_amax', 'resx', 'w', 'gamma1',
                 'wres', 'gamma2', 'stride', 'relu', 'pad')

    def __init__(self, g, zpre, rpre, out, bits, bn1, bn2, sync, count, g_amax, resx, w, gamma1, wres, gamma2, stride,
                 relu, pad):
        self.g, self.zpre, self.rpre, self.out, self.bits, self.bn1, self.bn2 = g, zpre, rpre, out, bits, bn1, bn2
        self.sync, self.count, self.g_amax, self.resx, self.w, self.gamma1 = sync, count, g_amax, resx, w, gamma1
        self.wres, self.gamma2, self.stride, self.relu, self.pad = wres, gamma2, stride, relu, pad


def _bn_coeffs(training, stats, count, bns, sync=None, nsamples=None):
    """Coefficients of the BatchNorm stages of one unit (main [+ down/residual]): ``stats`` / ``bns`` are parallel
    lists of partial-sum slabs and (weight, bias, running_mean, running_var).  Returns ([BNState ...], global count)."""
    S = bns[0][2].numel() // bns[0][0].numel()        # GhostBatchNorm keeps S*C running statistics
    if not training:                                  # eval: plain BN on the first C running entries (reference
        out = []                                      # ghostbatchnorm.py:108-117; .eval() has averaged them over S)
        for w, b, rm, rv in bns:
            C = w.numel()
            out.append(bn_eval_coeffs(w, b, rm[:C].contiguous(), rv[:C].contiguous()))
        return out, count
    if S > 1:
        if nsamples is None or nsamples % S:
            raise RuntimeError(f"agcn_amd: GhostBatchNorm with {S} splits needs a batch (x persons) divisible by {S}")
        stats = [_ghost_regroup(sp, S, nsamples) for sp in stats]
        bns = [(w.repeat(S), b.repeat(S), rm, rv) for w, b, rm, rv in bns]
        count = count // S
    if sync is not None:
        stats = sync_stats(stats, count, sync)
        count = count * sync.world
    note_params_changed()                             # running statistics are about to be rewritten in place
    res = [bn_train_coeffs(sp, count, *bn) for sp, bn in zip(stats, bns)]
    for st in res:
        st.S = S
    return res, count


def _ghost_regroup(stats_part, S, nsamples):
    """(N*nt, 2, C) per-(sample, tile) partial sums -> (N/S*nt, 2, S*C): sample n = n'*S + s feeds virtual channel
    s*C + c of row n' (GhostBatchNorm views (N, C, ...) as (N/S, S*C, ...), ghostbatchnorm.py:98-99)."""
    slots, two, C = stats_part.shape
    nt = slots // nsamples
    return stats_part.view(nsamples // S, S, nt, two, C).permute(0, 2, 3, 1, 4).reshape(nsamples // S * nt, two, S * C)


def _adjacency(x, wab, bab, A, PA, alpha, *, keep_tp, x_amax, want_amax):
    """The mixing matrices adj (N,3,V,V) of one unit_gcn by the one route that applies: theta/phi formed and reduced on
    chip (adjacency_fused_fwd), the theta/phi convolution followed by adjacency_fwd, or -- wab None (NonAdaptiveGCN) --
    the fixed graph A expanded.  keep_tp: a backward will follow; the fused route then either keeps nothing (the
    backward recomputes theta/phi, adjacency_bwd with tp = None) or lets the kernel drop a copy for the backward to
    re-read (adjacency_recompute).  x_amax: max |x| where the producer of x left it behind; want_amax: the caller can
    use it, so the fused route, which reads all of x anyway, takes it along the way where nobody has.
    Returns (P, adj, tp, x_amax)."""
    N, C, T, V = x.shape
    if wab is None:
        return None, A.unsqueeze(0).expand(N, 3, V, V).contiguous(), None, x_amax
    if not adjacency_fused_supported(C, wab.shape[0] // 6, T, V):
        tp, _ = conv_fwd(x, wab, bab)
        P, adj = adjacency_fwd(tp, A, PA, alpha)
        return P, adj, tp, x_amax
    amax_here = _empty((1,), x) if want_amax and x_amax is None and fused_amax_enabled() else None
    if keep_tp and not adjacency_recompute():
        P, adj, tp = adjacency_fused_fwd(x, wab, bab, A, PA, alpha, keep_tp=True, x_amax_out=amax_here, x_amax=x_amax)
    else:
        tp = None
        P, adj = adjacency_fused_fwd(x, wab, bab, A, PA, alpha, x_amax_out=amax_here, x_amax=x_amax)
    return P, adj, tp, x_amax if amax_here is None else amax_here


def gcn_forward(x, A, PA, wab, bab, wd, bd, bn, down, training, alpha=None, sync=None, need_bwd=True):
    """unit_gcn.forward (reference agcn.py:92-109) and AAGCN's GCNUnit core (aagcn.py:164-177, 264-266).
    wab: (6Ci, C, 1, 1) rows [a0|b0|a1|b1|a2|b2]; wd: (Cout, 3C); bd: summed conv_d biases;
    bn = (weight, bias, running_mean, running_var); down = None | (w, b, bn_w, bn_b, bn_rm, bn_rv).
    AGCN: adj = P + A + PA.  AAGCN: A = None, adj = PA + alpha*P.  wab = None (NonAdaptiveGCN): adj = A.
    Returns (out, _GCNState)."""
    N, C, T, V = x.shape
    count = N * T * V
    first = down is not None and first_layer_enabled() and bool(_L().agcn_gcn_first_supported(C, wd.shape[0], V))
    # max |x| left behind by the pass that produced x (None: nobody did); the 3-channel first layer does not use it
    x_amax = None if first else _take_out_amax(x)
    P, adj, tp, x_amax = _adjacency(x, wab, bab, A, PA, alpha, keep_tp=need_bwd, x_amax=x_amax, want_amax=not first)
    if first:
        # 3-channel first layer: aggregate+project and the `down` convolution in one pass over x (csrc/gcn_first.hip)
        ypre, st, dpre, st2 = gcn_first_fwd(x, adj, wd, bd, down[0], down[1], want_stats=training)
    else:
        ypre, st = aggregate_project_fwd(x, adj, wd, bd, want_stats=training, x_amax=x_amax)
        dpre, st2 = conv_fwd(x, down[0], down[1], want_stats=training) if down is not None else (None, None)
    if down is not None:
        (bn1, bn2), gcount = _bn_coeffs(training, [st, st2], count, [bn, down[2:]], sync, N)
        r = dpre
    else:
        (bn1,), gcount = _bn_coeffs(training, [st], count, [bn], sync, N)
        bn2, r = None, x
    g_amax = _empty((1,), x) if fused_amax_enabled() else None   # max |out| for the temporal convolution that reads it
    # (bits: sign bit mask of `out` for the BatchNorm backward, 32x less traffic than `out`)
    out, bits = bn_act_fwd(ypre, bn1, r, bn2, relu=True, want_bits=True, amax_out=g_amax)
    wdown, gamma2 = (down[0], down[2]) if down is not None else (None, None)
    return out, _GCNState(x, tp, P, adj, ypre, dpre, bits, bn1, bn2, sync, gcount, x_amax, g_amax, wab, bab, wd, bn[0],
                          wdown, gamma2, alpha)


def _bias_grad(slot, k, n, like, needed=True):
    """Gradient of a convolution bias in front of a BatchNorm: ``slot[k]`` in eval mode (bn_bwd's ``bias_out``), exact
    zeros in train mode where the batch mean cancels the bias; None where the eval backward skipped the sums."""
    if slot and slot[k] is not None:
        return slot[k]
    if slot:                   # eval mode with want_sums=False: nobody asked for it
        return None
    return torch.zeros(n, dtype=torch.float32, device=like.device) if needed else None


def gcn_backward(s, dout, extra_add=None, extra_mask=None, want_sums=True):
    """Backward of gcn_forward.  ``extra_add`` (masked by ``extra_mask``) is an additional dx contribution folded
    into the epilogue of the first dx kernel (the TCN_GCN_unit identity residual).  want_sums=False (eval mode only): no
    BatchNorm parameter or conv bias in front of one wants a gradient, the partial sums are skipped.
    Returns dx, dPA, dwab, dbab, dwd, dbd, dgamma, dbeta, dwdown, dbdown, dgamma_down, dbeta_down, dalpha."""
    x, tp, adj, ypre, dpre, wab, wd, wdown = s.x, s.tp, s.adj, s.ypre, s.dpre, s.wab, s.wd, s.wdown
    Cout = wd.shape[0]
    dy_amax = _empty((1,), dout) if fused_amax_enabled() else None   # max |dypre| for the f16x3 backward-data chain
    dbias = []                # eval mode: gradients of the conv_d / down biases (train mode: exactly zero, left empty)
    dypre, dg1, db1, ddpre, dg2, db2 = bn_bwd(dout, s.bits, ypre, s.gamma1, s.bn1, dpre, s.gamma2, s.bn2, sync=s.sync,
                                              gcount=s.count, amax_out=dy_amax, want_sums=want_sums, bias_out=dbias)
    x_amax = s.x_amax
    dwd = _side_run(lambda: project_bwd_weight(dypre, x, adj, Cout, dy_amax, x_amax), (dypre, x, adj, dy_amax, x_amax))
    dPA = dwab = dbab = dalpha = dtp = dtp_amax = None
    if wab is not None:   # adjacency branch first: its dtp rides along in the dx kernel where that is supported
        dPA, dtp, dbab, dalpha, _, dtp_amax = adjacency_bwd(dypre, wd, x, tp, s.P, s.alpha, wab, s.bab,
                                                            dy_amax=dy_amax, x_amax=x_amax)
        dwab = _side_run(lambda: conv_bwd_weight(dtp, x, wab.shape, 1, dtp_amax, x_amax), (dtp, x, dtp_amax, x_amax))
    fuse = dtp is not None and fused_bwd_data_supported(x.shape[1], Cout, x.shape[3])
    ftp = dict(dtp=dtp, wab=wab, dtp_amax=dtp_amax) if fuse else {}
    if dpre is None:      # identity `down`: dx += dout * (out > 0)
        dx = aggregate_project_bwd_data(dypre, adj, wd, x.shape, add1=dout, mask1=s.bits, add2=extra_add,
                                        mask2=extra_mask, dy_amax=dy_amax, **ftp)
    else:
        dx = aggregate_project_bwd_data(dypre, adj, wd, x.shape, add1=extra_add, mask1=extra_mask, dy_amax=dy_amax,
                                        **ftp)
    if dtp is not None and not fuse:
        conv_bwd_data(dtp, wab, x.shape, out=dx, accumulate=True)
    dwdown = None
    if dpre is not None:
        dwdown = _side_run(lambda: conv_bwd_weight(ddpre, x, wdown.shape), (ddpre, x))
        conv_bwd_data(ddpre, wdown, x.shape, out=dx, accumulate=True)
    _side_join()
    dbd = _bias_grad(dbias, 0, Cout, dout)
    dbdown = _bias_grad(dbias, 1, Cout, dout, dpre is not None)
    return dx, dPA, dwab, dbab, dwd, dbd, dg1, db1, dwdown, dbdown, dg2, db2, dalpha


def tcn_forward(g, w, b, bn, stride, res_x, res, relu, training, sync=None, pad=None, g_amax=None):
    """unit_tcn.forward (reference agcn.py:48-50) optionally fused with the TCN_GCN_unit tail
    relu(tcn(g) + residual(x)) (agcn.py:127-129).  res = None (no residual) | 'identity' |
    (w, b, bn_w, bn_b, bn_rm, bn_rv) for the unit_tcn(kernel_size=1, stride) residual.  pad: temporal padding of the
    convolution (None = (k-1)//2; TCNUnit(pad=False): 0).  g_amax: device scalar max |g| where the producer of g left
    it behind (the fused unit: the GCN state's; a stand-alone node: _take_out_amax(g)).  Returns (out, _TCNState)."""
    N, C, T, V = g.shape
    if res is not None:
        To = conv_out_frames(T, w.shape[2], stride, pad)
        Tr = res_x.shape[2] if isinstance(res, str) else conv_out_frames(res_x.shape[2], 1, stride, 0)
        if Tr != To:
            raise RuntimeError(f"agcn_amd: the residual has {Tr} frames but the temporal convolution ({w.shape[2]} taps, "
                               f"stride {stride}, padding {(w.shape[2] - 1) // 2 if pad is None else pad}) gives {To} "
                               f"for {T} input frames; they must agree (the reference fails here too)")
    zpre, st = conv_fwd(g, w, b, stride, want_stats=training, x_amax=g_amax, pad=pad)
    To = zpre.shape[2]
    count = N * To * V
    rpre = bn2 = wres = gamma2 = None
    if res is None or isinstance(res, str):
        (bn1,), gcount = _bn_coeffs(training, [st], count, [bn], sync, N)
        r = None if res is None else res_x
    else:
        r, st2 = conv_fwd(res_x, res[0], res[1], stride, want_stats=training)
        (bn1, bn2), gcount = _bn_coeffs(training, [st, st2], count, [bn, res[2:]], sync, N)
        rpre, wres, gamma2 = r, res[0], res[2]
    o_amax = _empty((1,), g) if fused_amax_enabled() else None   # max |out| for the next unit's f16x3 chain
    out, bits = bn_act_fwd(zpre, bn1, r, bn2, relu=relu, want_bits=True, amax_out=o_amax)
    _note_out_amax(out, o_amax)
    return out, _TCNState(g, zpre, rpre, out, bits, bn1, bn2, sync, gcount, g_amax, res_x, w, bn[0], wres, gamma2,
                          stride, relu, pad)


def tcn_backward(s, dout, join=True, want_sums=True):
    """Backward of tcn_forward; want_sums as in gcn_backward.  Returns dg, dw, dbias, dgamma, dbeta and, of the
    convolutional residual (else None), drpre, dw_res, dbias_res, dgamma_res, dbeta_res."""
    w, wres, g, stride, pad, g_amax = s.w, s.wres, s.g, s.stride, s.pad, s.g_amax
    mask = s.bits if s.relu else None
    dz_amax = _empty((1,), dout) if fused_amax_enabled() else None   # max |dzpre| for the backward-data convolution
    dbias = []                # eval mode: gradients of the temporal / residual conv biases
    dzpre, dg1, db1, drpre, dg2, db2 = bn_bwd(dout, mask, s.zpre, s.gamma1, s.bn1, s.rpre, s.gamma2, s.bn2, sync=s.sync,
                                              gcount=s.count, amax_out=dz_amax, want_sums=want_sums, bias_out=dbias)
    # (the device scalars are inputs of the side-stream kernels too: dz_amax dies with this frame, possibly before the join)
    dw = _side_run(lambda: conv_bwd_weight(dzpre, g, w.shape, stride, dz_amax, g_amax, pad=pad),
                   (dzpre, g, dz_amax, g_amax))
    dg = conv_bwd_data(dzpre, w, g.shape, stride, dy_amax=dz_amax, pad=pad)
    dwres = None
    if drpre is not None:
        resx = s.resx
        dwres = _side_run(lambda: conv_bwd_weight(drpre, resx, wres.shape, stride), (drpre, resx))
    if join:
        _side_join()
    Cout = w.shape[0]
    return (dg, dw, _bias_grad(dbias, 0, Cout, dout), dg1, db1,
            drpre, dwres, _bias_grad(dbias, 1, Cout, dout, drpre is not None), dg2, db2)


# ---- BN-folded inference (eval mode under no_grad): adjacency + two kernels per TCN_GCN_unit ----------------------
ERR_UNSUPPORTED = _lib.ERR_UNSUPPORTED


def _launched(name, *args):
    """``_lib.call`` for the entry points a caller may fall back from: False where the library reports the shape
    unsupported (nothing was launched), True when the work is enqueued; every other status raises."""
    rc = _lib.status(name, *args)
    if rc != ERR_UNSUPPORTED:
        _lib.check(rc, name)
    return rc != ERR_UNSUPPORTED

# Parameters and BatchNorm running statistics are written through RAW POINTERS by the training path (agcn_sgd_step on the
# flat buffer, agcn_bn_stats_finalize), which moves neither data_ptr nor the tensors' version counters.  Everything that
# caches something derived from them (the folded inference weights) keys on this counter too; it is bumped by every
# optimiser step and every training-mode BatchNorm stage.
_PARAM_EPOCH = [0]


def note_params_changed():
    _PARAM_EPOCH[0] += 1


def infer_fold_enabled():
    """AGCN_INFER_FOLD=0 keeps the eval forward on the unfused passes (A/B and debugging)."""
    return os.environ.get('AGCN_INFER_FOLD', '1') != '0'


# diagnostic counters of the eval-mode routes (never read by a compute path).  'aagcn_unit_fused': units of EITHER model
# (AGCN TCN_GCN_unit, AAGCN TCNGCNUnit) that ran folded end to end through unit_infer; 'tconv_infer': folded temporal
# convolutions; 'stc_apply': launches of the stand-alone gate pass agcn_stc_apply that the folded AAGCN unit replaces
INFER_STATS = {'aagcn_unit_fused': 0, 'tconv_infer': 0, 'stc_apply': 0}


def _fold(bn):
    """(scale, shift) of an eval-mode BatchNorm: y = scale * x + shift  (reference nn.BatchNorm2d in eval mode).
    GhostBatchNorm keeps S*C running statistics and evaluates with the first C of them (ghostbatchnorm.py; .eval() has
    collated them over the S sub-batches): the same entries ``_bn_coeffs`` reads."""
    w, b, rm, rv = bn
    C = w.numel()
    s = w / torch.sqrt(rv[:C] + BN_EPS)
    return s, b - rm[:C] * s


def _fold_conv(w, b, bn):
    """Weights and bias of ``bn(conv(x; w, b))`` in eval mode as one convolution; w (Cout, Cin, k, 1)."""
    s, sh = _fold(bn)
    return (w * s[:, None, None, None]).contiguous(), (b * s + sh).contiguous()


def gcn_unit_infer(x, adj, wcat, bias, res=None, x2=None, w2=None, relu=True):
    """y = act(bias + sum_i W_i (x . adj_i) [+ res] [+ W2 . x2]); None when only the exact-f32 kernels apply."""
    N, C, T, V = x.shape
    Cout = wcat.shape[0]
    K2 = 0 if x2 is None else x2.shape[1]
    nbytes = _L().agcn_gcn_unit_infer_workspace(C, Cout, K2, T, V)
    ws = _ws(nbytes, x)
    y = _empty((N, Cout, T, V), x)
    ok = _launched("agcn_gcn_unit_infer", x, adj, wcat, bias, res, x2, w2, K2, 1 if relu else 0, y, ws, nbytes, N, C, Cout,
                   T, V)
    return y if ok else None


def conv9_infer(x, w, b, res=None, relu=True, stride=1):
    """y = act(b + conv9x1(x; w, stride) [+ res]); None when only the exact-f32 kernels apply."""
    N, Cin, T, V = x.shape
    Cout = w.shape[0]
    To = conv_out_frames(T, 9, stride)
    ws, nbytes = _conv_ws(Cin, Cout, T, V, 9, stride, x)
    y = _empty((N, Cout, To, V), x)
    ok = _launched("agcn_conv9_infer", x, w, b, res, 1 if relu else 0, y, ws, nbytes, N, Cin, Cout, T, V, stride)
    return y if ok else None


def tconv_infer(x, w, b, a_s=None, a_t=None, a_c=None, res=None, relu=True, stride=1, pad=None, x_amax=None):
    """y = act(b + tconv(x * a_s[n,v] * a_t[n,t] * a_c[n,c]; w (k,1), stride, pad) [+ res]) with the BatchNorm already
    folded into w, b (agcn_tconv_infer): every kernel size / stride / padding of ``conv_fwd``; the gates (each optional)
    multiply x on load, the gated tensor is never stored.  None where the library reports the shape unsupported."""
    N, Cin, T, V = x.shape
    Cout, Cin2, taps, one = w.shape
    assert Cin2 == Cin and one == 1
    pad = (taps - 1) // 2 if pad is None else pad
    To = conv_out_frames(T, taps, stride, pad)
    if To < 1:
        raise ValueError(f"agcn_amd: a {taps}-frame kernel with padding {pad} does not fit {T} frames")
    ws, nbytes = _conv_ws(Cin, Cout, T, V, taps, stride, x, pad)
    y = _empty((N, Cout, To, V), x)
    if not _launched("agcn_tconv_infer", x, w, b, a_s, a_t, a_c, res, 1 if relu else 0, y, ws, nbytes, N, Cin, Cout, T,
                     V, taps, stride, pad, x_amax):
        return None
    INFER_STATS['tconv_infer'] += 1
    return y


def _cache_key(srcs):
    return (_PARAM_EPOCH[0],) + tuple((t.data_ptr(), t._version) for t in srcs if t is not None)


def tcn_infer(x, w, b, bn, stride, pad, cache=None):
    """Eval-mode stand-alone TCNUnit / unit_tcn (reference aagcn.py:194-207): bn(conv(x)) as one folded convolution."""
    key = _cache_key([w, b, *bn])
    f = cache.get('folded') if cache is not None else None
    if f is None or f[0] != key:
        f = (key,) + _fold_conv(w, b, bn)
        if cache is not None:
            cache['folded'] = f
    return tconv_infer(x.contiguous(), f[1], f[2], relu=False, stride=stride, pad=pad)


# ---- one description of a unit's parameters -----------------------------------------------------------------------------
# The models describe a TCN_GCN_unit (AGCN) / TCNGCNUnit (AAGCN) as a dict ``p`` of its raw parameters:
#   conv_d [(w, b)]*3, ab [(wa, ba, wb, bb)]*3 | None (NonAdaptiveGCN), A fixed graph | None, PA | None, alpha | None,
#   gbn (weight, bias, running_mean, running_var), down None | (w, b, *bn)                       -- the unit_gcn part
#   tw, tb, tbn, res_mode (0 none, 1 identity, 2 conv), res None | (w, b, *bn), stride, pad,
#   attn None | (sa_w, sa_b, ta_w, ta_b, fc1_w, fc1_b, fc2_w, fc2_b)                             -- the rest of the unit
# AGCN is the case A and PA both present, alpha = attn = None.  pack_gcn / pack_tcn lay it out as the autograd
# Functions' arguments, _fold_unit as the folded inference weights.
_NONE6 = (None,) * 6


def _pack_wb(p):
    """Parameters in the layout the kernels take: theta/phi weights and biases stacked row-wise [a0|b0|a1|b1|a2|b2]
    (None without an adaptive branch), projection weights side by side [Wd0|Wd1|Wd2], conv_d biases summed.  Ordinary
    differentiable tensor code: the gradients reach the individual conv_a / conv_b / conv_d parameters through it."""
    wab = bab = None
    if p['ab'] is not None:
        wab = torch.cat([t for wa, _, wb, _ in p['ab'] for t in (wa, wb)], 0)
        bab = torch.cat([t for _, ba, _, bb in p['ab'] for t in (ba, bb)], 0)
    (w0, b0), (w1, b1), (w2, b2) = p['conv_d']
    Cout, C = w0.shape[:2]
    return wab, bab, torch.cat([w0.view(Cout, C), w1.view(Cout, C), w2.view(Cout, C)], dim=1), b0 + b1 + b2


def pack_gcn(p):
    """UnitGCNFunction's / TCNGCNUnitFunction's arguments 'A' .. 'dbn_rv' from the unit_gcn part of ``p``."""
    return (p['A'], p['PA'], *_pack_wb(p), *p['gbn'], *(p['down'] or _NONE6))


def pack_tcn(p):
    """TCNResidualFunction's / TCNGCNUnitFunction's arguments 'tw' .. 'stride' from ``p``."""
    return (p['tw'], p['tb'], *p['tbn'], p['res_mode'], *(p['res'] or _NONE6), p['stride'])


def _fold_unit(p):
    """Eval-mode weights of the unit ``p`` with every BatchNorm folded into the contraction in front of it; pure tensor
    code on whatever device / float dtype the parameters have.  Returns (wdf, bias, w2, twf, tbf, rwf, rbf, wab, bab):
    g = relu(bias + wdf . [x.adj_0; x.adj_1; x.adj_2] + (w2 . x | x)) is the unit_gcn with its BatchNorm and the conv
    `down` (w2 None: identity) folded, (twf, tbf) / (rwf, rbf) the folded temporal / residual convolutions (the latter
    None without a convolutional residual), wab / bab the packed theta/phi parameters."""
    wab, bab, wd, bd = _pack_wb(p)
    s1, sh1 = _fold(p['gbn'])
    wdf = (wd * s1[:, None]).contiguous()
    bias = bd * s1 + sh1
    w2 = None
    if p['down'] is not None:
        dw, db = p['down'][:2]
        s2, sh2 = _fold(p['down'][2:])
        w2 = (dw.reshape(dw.shape[0], dw.shape[1]) * s2[:, None]).contiguous()
        bias = bias + db * s2 + sh2
    twf, tbf = _fold_conv(p['tw'], p['tb'], p['tbn'])
    rwf, rbf = _fold_conv(*p['res'][:2], p['res'][2:]) if p['res'] is not None else (None, None)
    return wdf, bias.contiguous(), w2, twf, tbf, rwf, rbf, wab, bab


def unit_infer(x, p, cache=None):
    """Eval-mode TCN_GCN_unit (reference agcn.py:92-109, 48-50, 127-129) / AAGCN TCNGCNUnit (aagcn.py:164-177, 264-271,
    194-207, 316-321) from its description ``p`` (above) with every BatchNorm folded into the contraction in front of
    it: adjacency, one aggregate+project kernel (unit BN and conv `down` folded; residual add / ReLU in its epilogue),
    [AAGCN: the two reduction passes and the few-KB gate networks of ``STCAttentionFunction.forward`` -- no
    ``agcn_stc_apply``: the gated tensor is never written], [the folded 1x1 stride residual conv], one
    ``agcn_tconv_infer`` (gates on load, residual add + ReLU in its epilogue).
    Returns None where the fused kernels do not apply (3-channel first layer, C < 32, AGCN_GEMM=f32, whatever
    agcn_gcn_unit_infer rejects): the caller runs the unfused eval passes.  ``cache`` (a dict owned by the module) keeps
    the folded and packed weights between calls, keyed on the parameter epoch and every source tensor's (data_ptr,
    version)."""
    x = x.contiguous()
    N, C, T, V = x.shape
    # decided before anything is folded or launched: agcn_gcn_unit_infer exists on the chained split kernels only
    # (AGCN_GEMM=bf16x6 / bf16) and from 32 channels on.  (A shape it still rejects below has run the adjacency once
    # more than needed: the caller's unfused passes compute it again.)
    if C < 32 or _L().agcn_gemm_mode() not in (b'bf16x6', b'bf16'):
        return None
    srcs = [t for wb in p['conv_d'] for t in wb] + [t for q in (p['ab'] or ()) for t in q]
    srcs += [*p['gbn'], p['tw'], p['tb'], *p['tbn'], *(p['down'] or ()), *(p['res'] or ())]
    key = _cache_key(srcs)
    f = cache.get('folded') if cache is not None else None
    if f is None or f[0] != key:
        f = (key,) + _fold_unit(p)
        if cache is not None:
            cache['folded'] = f
    _, wdf, bias, w2, twf, tbf, rwf, rbf, wab, bab = f
    _, adj, _, _ = _adjacency(x, wab, bab, p['A'], p['PA'], p['alpha'], keep_tp=False, x_amax=None, want_amax=False)
    if w2 is None:
        g = gcn_unit_infer(x, adj, wdf, bias, res=x)
    else:
        g = gcn_unit_infer(x, adj, wdf, bias, x2=x, w2=w2)
    if g is None:
        return None
    a_s = a_t = a_c = None
    if p['attn'] is not None:        # exactly STCAttentionFunction.forward up to (and without) its apply pass
        _, m_s = stc_row_reduce(g, want_v=True, scale_v=1.0 / T)                         # mean_t g
        a_s = STCAttentionFunction._gates(m_s, None, *p['attn'])[0]
        mv1, _ = stc_row_reduce(g, wv=a_s, want_t=True, scale_t=1.0 / V)                 # mean_v g*(1+se_s)
        _, a_t, a_c, _, _ = STCAttentionFunction._gates(m_s, mv1, *p['attn'], a_s=a_s)
    if p['res_mode'] == 0:
        r = None
    elif p['res_mode'] == 1:
        r = x
    else:
        r, _ = conv_fwd(x, rwf, rbf, p['stride'])
    y = tconv_infer(g, twf, tbf, a_s, a_t, a_c, res=r, relu=True, stride=p['stride'], pad=p['pad'])
    if y is not None:
        INFER_STATS['aagcn_unit_fused'] += 1
    return y


# ---- skeleton preprocessing on the device (csrc/prenorm.hip) -----------------------------------------------------------
def _axis(pair):
    if pair is None:
        return -1, -1
    j0, j1 = (int(j) for j in pair)
    if j0 < 0 or j1 < 0:
        raise ValueError(f"agcn_amd: joint indices are 0-based and non-negative, got {pair}")
    return j0, j1


def skel_append(ring, frame, slot, count, moving_avg=1):
    """frame (Mmax, V, 3) into slot ``slot`` of the device ring (Mmax, Tmax, V, 3); ``count`` = frames present
    including this one.  ``moving_avg`` k > 1: once count >= k the slot holds the mean of the last k slots
    (agcn_skel_append).  The host owns slot and count; nothing is read back."""
    Mmax, Tmax, V, C = ring.shape
    if C != 3 or tuple(frame.shape) != (Mmax, V, 3):
        raise ValueError(f"agcn_amd: skel_append takes a ({Mmax}, {V}, 3) frame for this ring, got {tuple(frame.shape)}")
    _lib.call("agcn_skel_append", frame, ring, Mmax, Tmax, V, int(slot), int(count), int(moving_avg))


def prenorm(x, num_select=None, origin=0, frames=None, zaxis=(0, 1), zaxis2=None, xaxis=(8, 4), pad=True, center=True,
            center_firstframe=False):
    """Body selection + pre_normalization of raw skeletons x (N, M, Tmax, V, 3) -> (N, 3, T, V, K) (agcn_prenorm).
    Logical frame t is slot (origin + t) mod Tmax; ``frames`` T defaults to Tmax.  ``num_select`` K: the K most active
    of the M bodies, most active first; None keeps all M in their order.  Returns (out, selected (N, K) int32,
    energy (N, M) or None), all on the device.

    A frame (joint) counts as null iff ALL its values are zero.  The reference tests ``sum() == 0``; the two differ only
    where a non-null frame or joint sums to exactly zero by cancellation."""
    if (center or center_firstframe) and center == center_firstframe:
        raise ValueError("agcn_amd: center and center_firstframe exclude each other")
    if x.dim() != 5 or x.shape[-1] != 3:
        raise ValueError(f"agcn_amd: prenorm takes (N, M, T, V, 3), got {tuple(x.shape)}")
    N, M, Tmax, V, _ = x.shape
    T = Tmax if frames is None else int(frames)
    select = num_select is not None
    K = int(num_select) if select else M
    out = _empty((N, 3, T, V, K), x)
    sel = torch.empty((N, K), dtype=torch.int32, device=x.device)
    energy = _empty((N, M), x) if select else None
    (z0, z1), (x0, x1), (zz0, zz1) = _axis(zaxis), _axis(xaxis), _axis(zaxis2)
    _lib.call("agcn_prenorm", x, out, sel, energy, N, M, K, T, Tmax, int(origin), V, 1 if select else 0,
              1 if pad else 0, 1 if center else (2 if center_firstframe else 0), z0, z1, x0, x1, zz0, zz1)
    return out, sel, energy


def _plan(t, n, what):
    """An (n,) int32 index array of a plan (None passes through); the device is checked where its pointer is taken."""
    if t is not None and (t.dim() != 1 or t.dtype != torch.int32 or (n is not None and t.numel() != n)):
        raise ValueError(f"agcn_amd: {what} must be a 1-D int32 tensor" + (f" of length {n}" if n is not None else "")
                         + f", got {t.dtype} {tuple(t.shape)}")
    return t


def prenorm_windows(pool, start, length, block=None, frames=None, num_select=None, zaxis=(0, 1), zaxis2=None,
                    xaxis=(8, 4), pad=True, center=True, center_firstframe=False):
    """``prenorm`` of N windows of a pool (nblocks, M, Tmax, V, 3) in one launch (agcn_prenorm_windows): window n is
    ``length[n]`` frames from slot ``start[n]`` (wrapping at Tmax) of block ``block[n]`` (None: block 0), the frames
    after them null whatever the pool holds there.  start / length / block: int32 tensors (N,) on the device, clamped
    into the pool by the kernel.  ``frames`` T (the window length of the output) defaults to Tmax.  Returns what
    ``prenorm`` returns, with the same bits for the same logical window."""
    if (center or center_firstframe) and center == center_firstframe:
        raise ValueError("agcn_amd: center and center_firstframe exclude each other")
    if pool.dim() != 5 or pool.shape[-1] != 3:
        raise ValueError(f"agcn_amd: prenorm_windows takes a pool (nblocks, M, Tmax, V, 3), got {tuple(pool.shape)}")
    nblocks, M, Tmax, V, _ = pool.shape
    T = Tmax if frames is None else int(frames)
    if not 1 <= T <= Tmax:
        raise ValueError(f"agcn_amd: prenorm_windows needs 1 <= frames <= Tmax = {Tmax}, got {T}")
    if start is None or length is None:
        raise ValueError("agcn_amd: prenorm_windows needs start and length")
    N = _plan(start, None, 'start').numel()
    if N < 1:
        raise ValueError("agcn_amd: prenorm_windows needs at least one window")
    _plan(length, N, 'length')
    _plan(block, N, 'block')
    select = num_select is not None
    K = int(num_select) if select else M
    out = _empty((N, 3, T, V, K), pool)
    sel = torch.empty((N, K), dtype=torch.int32, device=pool.device)
    energy = _empty((N, M), pool) if select else None
    (z0, z1), (x0, x1), (zz0, zz1) = _axis(zaxis), _axis(xaxis), _axis(zaxis2)
    _lib.call("agcn_prenorm_windows", pool, out, sel, energy, block, start, length, N, nblocks, M, K, T, Tmax, V,
              1 if select else 0, 1 if pad else 0, 1 if center else (2 if center_firstframe else 0), z0, z1, x0, x1,
              zz0, zz1)
    return out, sel, energy


def skel_smooth(raw, moving_avg=1):
    """A recording raw (L, Mmax, V, 3), time-major -> (Mmax, L, V, 3), body-major, with ``skel_append``'s recursive
    moving average run over all its frames (agcn_skel_smooth): bit for bit what a ring holds after appending the frames
    one by one.  ``moving_avg`` 1 is a transposing copy."""
    if raw.dim() != 4 or raw.shape[-1] != 3:
        raise ValueError(f"agcn_amd: skel_smooth takes a recording (L, Mmax, V, 3), got {tuple(raw.shape)}")
    L, Mmax, V, _ = raw.shape
    if not 1 <= int(moving_avg) <= L:
        raise ValueError(f"agcn_amd: skel_smooth needs 1 <= moving_avg <= L = {L}, got {moving_avg}")
    out = _empty((Mmax, L, V, 3), raw)
    _lib.call("agcn_skel_smooth", raw, out, Mmax, L, V, int(moving_avg))
    return out


def skel_append_many(rings, frames, slot, count, moving_avg=1):
    """One frame into each of S rings in one launch (agcn_skel_append_many): rings (S, Mmax, Tmax, V, 3), frames
    (S, Mmax, V, 3), slot / count int32 tensors (S,) on the device as ``skel_append`` takes them per ring; slot < 0
    leaves that ring untouched."""
    if rings.dim() != 5 or rings.shape[-1] != 3:
        raise ValueError(f"agcn_amd: skel_append_many takes rings (S, Mmax, Tmax, V, 3), got {tuple(rings.shape)}")
    S, Mmax, Tmax, V, _ = rings.shape
    if tuple(frames.shape) != (S, Mmax, V, 3):
        raise ValueError(f"agcn_amd: skel_append_many takes ({S}, {Mmax}, {V}, 3) frames for these rings, got "
                         f"{tuple(frames.shape)}")
    _plan(slot, S, 'slot')
    _plan(count, S, 'count')
    _lib.call("agcn_skel_append_many", frames, rings, slot, count, S, Mmax, Tmax, V, int(moving_avg))


# ---- bone and motion input streams from joint data (csrc/streams.hip) -----------------------------------------------------
STREAMS = ('joint', 'bone', 'joint_motion', 'bone_motion')
STREAM_MAX_V = 32


def stream_hip_enabled():
    """AGCN_STREAM_HIP=0 runs the streams as tensor code (``streams_ref`` / ``streams_bwd_ref``): for A/B."""
    return os.environ.get('AGCN_STREAM_HIP', '1') != '0'


def _stream_parents(parent, V):
    """The parent table as a tuple of V Python ints in [0, V), checked on the host (the C entry checks it again)."""
    if torch.is_tensor(parent) or isinstance(parent, np.ndarray):
        parent = parent.tolist()
    parent = tuple(parent)
    if len(parent) != V:
        raise ValueError(f"agcn_amd: the parent table has {len(parent)} entries for {V} joints")
    if any(isinstance(p, bool) or int(p) != p or not 0 <= int(p) < V for p in parent):
        raise ValueError(f"agcn_amd: every parent must be a joint index in [0, {V}), got {list(parent)}")
    return tuple(int(p) for p in parent)


def _stream_tensor(t, shape, like, what):
    """One (N, C, T, V, M) tensor of a streams call: shape, dtype, layout and device, before any launch."""
    if not torch.is_tensor(t) or t.dim() != 5 or (shape is not None and tuple(t.shape) != tuple(shape)):
        want = "a 5-D (N, C, T, V, M) tensor" if shape is None else f"a tensor of shape {tuple(shape)}"
        raise ValueError(f"agcn_amd: {what} must be {want}, got {tuple(t.shape) if torch.is_tensor(t) else type(t)}")
    if not t.is_contiguous():
        raise ValueError(f"agcn_amd: {what} must be contiguous (N, C, T, V, M), got strides {t.stride()}")
    if like is not None and (t.device != like.device or t.dtype != like.dtype):
        raise ValueError(f"agcn_amd: {what} must be {like.dtype} on {like.device}, got {t.dtype} on {t.device}")
    if t.is_cuda and stream_hip_enabled() and t.dtype != torch.float32:
        raise ValueError(f"agcn_amd: {what} must be float32 for the HIP route, got {t.dtype}")
    if not t.dtype.is_floating_point:
        raise ValueError(f"agcn_amd: {what} must be a floating-point tensor, got {t.dtype}")
    if t.numel() == 0:
        raise ValueError(f"agcn_amd: {what} is empty: {tuple(t.shape)}")
    return t


def _stream_want(want):
    want = (want,) if isinstance(want, str) else tuple(want)
    if not want or len(set(want)) != len(want) or any(w not in STREAMS[1:] for w in want):
        raise ValueError(f"agcn_amd: want is a non-empty selection of {STREAMS[1:]} without repeats, got {want}")
    return want


def _motion_ref(x):
    return torch.cat((x[:, :, 1:] - x[:, :, :-1], torch.zeros_like(x[:, :, :1])), 2)


def streams_ref(x, parent, want=('bone',)):
    """The tensor-code form of ``skeleton_streams`` (any device, any floating dtype): the same subtractions in the same
    order, so the same bits in fp32.  -> dict."""
    want = _stream_want(want)
    parent = _stream_parents(parent, x.shape[3])
    out = {}
    if 'bone' in want or 'bone_motion' in want:
        bone = x - x.index_select(3, torch.tensor(parent, dtype=torch.long, device=x.device))
        if 'bone' in want:
            out['bone'] = bone
        if 'bone_motion' in want:
            out['bone_motion'] = _motion_ref(bone)
    if 'joint_motion' in want:
        out['joint_motion'] = _motion_ref(x)
    return {w: out[w] for w in want}


def _motion_t_ref(d):
    """motion^T: (t > 0 ? d[t-1] : 0) - (t < T-1 ? d[t] : 0)"""
    z = torch.zeros_like(d[:, :, :1])
    return torch.cat((z, d[:, :, :-1]), 2) - torch.cat((d[:, :, :-1], z), 2)


def _bone_t_ref(d, parent):
    """bone^T: d[v] - sum over the children c of v (ascending) of d[c]"""
    out = d.clone()
    for c, p in enumerate(parent):
        out[:, :, :, p] -= d[:, :, :, c]
    return out


def streams_bwd_ref(cot, parent, weights=(1.0, 1.0, 1.0, 1.0)):
    """The tensor-code form of ``streams_bwd``.  cot: dict stream name -> cotangent (absent or None: nothing)."""
    dx = None
    for name, w in zip(STREAMS, weights):
        d = cot.get(name)
        if d is None:
            continue
        if name.endswith('motion'):
            d = _motion_t_ref(d)
        if name.startswith('bone'):
            d = _bone_t_ref(d, parent)
        dx = w * d if dx is None else dx + w * d
    if dx is None:
        raise ValueError("agcn_amd: streams_bwd needs at least one cotangent")
    return dx


def streams_bwd(cot, parent, weights=(1.0, 1.0, 1.0, 1.0)):
    """The transpose of the streams in one launch (agcn_streams_bwd): cot maps 'joint' / 'bone' / 'joint_motion' /
    'bone_motion' to cotangents (N, C, T, V, M) (absent or None: nothing), ``weights`` the four factors in that order ->
        dx = w_j d_joint + w_b bone^T(d_bone) + w_jm motion^T(d_jm) + w_bm bone^T(motion^T(d_bm)),
    added in that order, a joint's children ascending.  CPU tensors and AGCN_STREAM_HIP=0 run ``streams_bwd_ref``."""
    if any(k not in STREAMS for k in cot):
        raise ValueError(f"agcn_amd: streams_bwd takes cotangents named {STREAMS}, got {sorted(cot)}")
    given = [cot.get(k) for k in STREAMS]
    first = next((d for d in given if d is not None), None)
    if first is None:
        raise ValueError("agcn_amd: streams_bwd needs at least one cotangent")
    _stream_tensor(first, None, None, 'cotangent')
    for k, d in zip(STREAMS, given):
        if d is not None:
            _stream_tensor(d, first.shape, first, f'd_{k}')
    N, C, T, V, M = first.shape
    parent = _stream_parents(parent, V)
    weights = tuple(float(w) for w in weights)
    if len(weights) != 4:
        raise ValueError("agcn_amd: streams_bwd takes four weights (joint, bone, joint_motion, bone_motion)")
    if not (first.is_cuda and stream_hip_enabled()):
        return streams_bwd_ref(dict(zip(STREAMS, given)), parent, weights)
    if V > STREAM_MAX_V:
        raise ValueError(f"agcn_amd: the stream kernels take at most {STREAM_MAX_V} joints, got {V}")
    dx = torch.empty_like(first)
    _lib.call("agcn_streams_bwd", *given, dx, parent, *weights, N, C, T, V, M)
    return dx


class StreamsFunction(torch.autograd.Function):
    """x (N, C, T, V, M) -> the streams named in ``want`` (a tuple of tensors in that order), one agcn_streams_fwd launch;
    the backward is one agcn_streams_bwd launch over whichever cotangents arrive.  CPU tensors and AGCN_STREAM_HIP=0 run
    the tensor-code forms.  args: x, parent (tuple of ints), want (tuple of names), out (dict name -> tensor, or None)"""

    @staticmethod
    def forward(ctx, x, parent, want, out):
        ctx.parent, ctx.want = parent, want
        ctx.set_materialize_grads(False)
        if not (x.is_cuda and stream_hip_enabled()):
            res = streams_ref(x, parent, want)
            if out is not None:
                for w in want:
                    out[w].copy_(res[w])
                res = out
            return tuple(res[w] for w in want)
        N, C, T, V, M = x.shape
        res = {w: (out[w] if out is not None else torch.empty_like(x)) for w in want}
        _lib.call("agcn_streams_fwd", x, res.get('bone'), res.get('joint_motion'), res.get('bone_motion'), parent,
                  N, C, T, V, M)
        return tuple(res[w] for w in want)

    @staticmethod
    def backward(ctx, *grads):
        cot = {w: g.contiguous() for w, g in zip(ctx.want, grads) if g is not None}
        if not cot:
            return None, None, None, None
        return streams_bwd(cot, ctx.parent), None, None, None


def skeleton_streams(x, parent, want=('bone',), out=None):
    """Bone and motion streams of joint data x (N, C, T, V, M), contiguous (reference data_gen/gen_bone_data.py,
    gen_motion_data.py): bone = x - x[parent], joint_motion[t] = x[t+1] - x[t] (0 in the last frame), bone_motion = the
    motion of the bone tensor.  ``parent``: V joint indices in [0, V) (``Graph().bone_parents``), host data.  ``want``: a
    non-empty selection of 'bone', 'joint_motion', 'bone_motion'; all of them come out of ONE launch that reads x once
    -> dict name -> tensor.  ``out``: optional dict of preallocated tensors to write into (no autograd then).
    Differentiable in x.  Everything is checked here, before any launch."""
    want = _stream_want(want)
    _stream_tensor(x, None, None, 'x')
    V = x.shape[3]
    parent = _stream_parents(parent, V)
    if x.is_cuda and stream_hip_enabled() and V > STREAM_MAX_V:
        raise ValueError(f"agcn_amd: the stream kernels take at most {STREAM_MAX_V} joints, got {V}")
    if out is not None:
        if x.requires_grad and torch.is_grad_enabled():
            raise ValueError("agcn_amd: skeleton_streams writes into `out` only where no gradient is recorded")
        if set(out) != set(want):
            raise ValueError(f"agcn_amd: out must hold exactly the wanted streams {want}, got {sorted(out)}")
        for w in want:
            _stream_tensor(out[w], x.shape, x, f'out[{w!r}]')
        ptrs = [x.data_ptr()] + [out[w].data_ptr() for w in want]
        if len(set(ptrs)) != len(ptrs):
            raise ValueError("agcn_amd: the outputs of skeleton_streams must not alias x or each other")
    return dict(zip(want, StreamsFunction.apply(x, parent, want, out)))


# ---- the autograd nodes ---------------------------------------------------------------------------------------------------
class _Args:
    """The argument names of one autograd Function's forward, declared once next to it: the positions looked up in
    ``needs_input_grad`` and the order of the gradients its backward returns are derived from the names, and a name
    that is not an argument is a KeyError."""
    __slots__ = ('names', 'index')

    def __init__(self, *names):
        self.names, self.index = names, {n: i for i, n in enumerate(names)}

    def positions(self, *names):
        return tuple(self.index[n] for n in names)

    def grads(self, **by_name):
        """The backward's return value: the given gradients at their arguments' positions, None everywhere else."""
        out = [None] * len(self.names)
        for n, g in by_name.items():
            out[self.index[n]] = g
        return tuple(out)


_GCN_ARGS = ('A', 'PA', 'wab', 'bab', 'wd', 'bd', 'bn_w', 'bn_b', 'bn_rm', 'bn_rv',
             'down_w', 'down_b', 'dbn_w', 'dbn_b', 'dbn_rm', 'dbn_rv')                              # = pack_gcn(p)
_TCN_ARGS = ('tw', 'tb', 'tbn_w', 'tbn_b', 'tbn_rm', 'tbn_rv',
             'res_mode', 'rw', 'rb', 'rbn_w', 'rbn_b', 'rbn_rm', 'rbn_rv', 'stride')                # = pack_tcn(p)
# eval mode: the BatchNorm partial sums only where a BN parameter or a conv bias in front of it wants a gradient
_GCN_SUMS = ('bd', 'bn_w', 'bn_b', 'down_b', 'dbn_w', 'dbn_b')
_TCN_SUMS = ('tb', 'tbn_w', 'tbn_b', 'rb', 'rbn_w', 'rbn_b')


def _wants(ctx, positions):
    ng = ctx.needs_input_grad
    return any(ng[i] for i in positions)


def _down(down_w, down_b, dbn_w, dbn_b, dbn_rm, dbn_rv):
    return None if down_w is None else (down_w, down_b, dbn_w, dbn_b, dbn_rm, dbn_rv)


def _residual(res_mode, rw, rb, rbn_w, rbn_b, rbn_rm, rbn_rv):
    return None if res_mode == 0 else ('identity' if res_mode == 1 else (rw, rb, rbn_w, rbn_b, rbn_rm, rbn_rv))


class UnitGCNFunction(torch.autograd.Function):
    """unit_gcn / GCNUnit core as its own autograd node."""
    ARGS = _Args('x', *_GCN_ARGS, 'training', 'alpha', 'sync')
    SUMS = ARGS.positions(*_GCN_SUMS)

    @staticmethod
    def forward(ctx, x, A, PA, wab, bab, wd, bd, bn_w, bn_b, bn_rm, bn_rv, down_w, down_b, dbn_w, dbn_b, dbn_rm,
                dbn_rv, training, alpha=None, sync=None):
        out, ctx.gs = gcn_forward(x.contiguous(), A, PA, wab, bab, wd, bd, (bn_w, bn_b, bn_rm, bn_rv),
                                  _down(down_w, down_b, dbn_w, dbn_b, dbn_rm, dbn_rv), training, alpha, sync,
                                  need_bwd=any(ctx.needs_input_grad))
        _note_out_amax(out, ctx.gs.g_amax)     # stand-alone node: a unit_tcn may read this tensor next
        return out

    @staticmethod
    def backward(ctx, dout):
        dx, dPA, dwab, dbab, dwd, dbd, dg1, db1, dwdown, dbdown, dg2, db2, dalpha = gcn_backward(
            ctx.gs, dout.contiguous(), want_sums=_wants(ctx, UnitGCNFunction.SUMS))
        ctx.gs = None
        if dalpha is not None:
            dalpha = dalpha.reshape(1)
        return UnitGCNFunction.ARGS.grads(x=dx, PA=dPA, wab=dwab, bab=dbab, wd=dwd, bd=dbd, bn_w=dg1, bn_b=db1,
                                          down_w=dwdown, down_b=dbdown, dbn_w=dg2, dbn_b=db2, alpha=dalpha)


class UnitTCNFunction(torch.autograd.Function):
    """unit_tcn / TCNUnit (no residual, no ReLU) as its own autograd node."""
    ARGS = _Args('x', 'tw', 'tb', 'tbn_w', 'tbn_b', 'tbn_rm', 'tbn_rv', 'stride', 'training', 'sync', 'pad')
    SUMS = ARGS.positions('tb', 'tbn_w', 'tbn_b')

    @staticmethod
    def forward(ctx, x, tw, tb, tbn_w, tbn_b, tbn_rm, tbn_rv, stride, training, sync=None, pad=None):
        x = x.contiguous()
        out, ctx.ts = tcn_forward(x, tw, tb, (tbn_w, tbn_b, tbn_rm, tbn_rv), stride, None, None, False, training, sync,
                                  pad, g_amax=_take_out_amax(x))
        return out

    @staticmethod
    def backward(ctx, dout):
        dg, dw, dbias, dg1, db1, _, _, _, _, _ = tcn_backward(ctx.ts, dout.contiguous(),
                                                              want_sums=_wants(ctx, UnitTCNFunction.SUMS))
        ctx.ts = None
        return UnitTCNFunction.ARGS.grads(x=dg, tw=dw, tb=dbias, tbn_w=dg1, tbn_b=db1)


class TCNResidualFunction(torch.autograd.Function):
    """relu(bn(tconv(g)) + residual(x)) as its own autograd node (AAGCN: the attention gates sit between the GCN core
    and this).  pad: of the temporal convolution (None = (k-1)//2)."""
    ARGS = _Args('g', 'x', *_TCN_ARGS, 'training', 'sync', 'pad')
    SUMS = ARGS.positions(*_TCN_SUMS)

    @staticmethod
    def forward(ctx, g, x, tw, tb, tbn_w, tbn_b, tbn_rm, tbn_rv, res_mode, rw, rb, rbn_w, rbn_b, rbn_rm, rbn_rv, stride,
                training, sync=None, pad=None):
        g = g.contiguous()
        x = x.contiguous() if x is not None else None
        out, ctx.ts = tcn_forward(g, tw, tb, (tbn_w, tbn_b, tbn_rm, tbn_rv), stride, x,
                                  _residual(res_mode, rw, rb, rbn_w, rbn_b, rbn_rm, rbn_rv), True, training, sync, pad,
                                  g_amax=_take_out_amax(g))     # (left by the attention gates / the unit_gcn node)
        ctx.res_mode = res_mode
        return out

    @staticmethod
    def backward(ctx, dout):
        s = ctx.ts
        dout = dout.contiguous()
        dg, dw, dtb, dg1, db1, drpre, dwres, drb, dg2, db2 = tcn_backward(
            s, dout, want_sums=_wants(ctx, TCNResidualFunction.SUMS))
        dx = None
        if ctx.res_mode == 1:
            dx = torch.where(s.out > 0, dout, torch.zeros_like(dout))
        elif ctx.res_mode == 2:
            dx = conv_bwd_data(drpre, s.wres, s.resx.shape, s.stride)
        ctx.ts = None
        return TCNResidualFunction.ARGS.grads(g=dg, x=dx, tw=dw, tb=dtb, tbn_w=dg1, tbn_b=db1, rw=dwres, rb=drb,
                                              rbn_w=dg2, rbn_b=db2)


class TCNGCNUnitFunction(torch.autograd.Function):
    """TCN_GCN_unit = relu(tcn1(gcn1(x)) + residual(x)) as ONE autograd node, so that every dx contribution is
    accumulated in a contraction epilogue instead of separate elementwise passes."""
    ARGS = _Args('x', *_GCN_ARGS, *_TCN_ARGS, 'training', 'sync')
    GCN_SUMS, TCN_SUMS = ARGS.positions(*_GCN_SUMS), ARGS.positions(*_TCN_SUMS)

    @staticmethod
    def forward(ctx, x, A, PA, wab, bab, wd, bd, bn_w, bn_b, bn_rm, bn_rv, down_w, down_b, dbn_w, dbn_b, dbn_rm,
                dbn_rv, tw, tb, tbn_w, tbn_b, tbn_rm, tbn_rv, res_mode, rw, rb, rbn_w, rbn_b, rbn_rm, rbn_rv, stride,
                training, sync=None):
        x = x.contiguous()
        g, ctx.gs = gcn_forward(x, A, PA, wab, bab, wd, bd, (bn_w, bn_b, bn_rm, bn_rv),
                                _down(down_w, down_b, dbn_w, dbn_b, dbn_rm, dbn_rv), training, sync=sync,
                                need_bwd=any(ctx.needs_input_grad))
        out, ctx.ts = tcn_forward(g, tw, tb, (tbn_w, tbn_b, tbn_rm, tbn_rv), stride, x,
                                  _residual(res_mode, rw, rb, rbn_w, rbn_b, rbn_rm, rbn_rv), True, training, sync,
                                  g_amax=ctx.gs.g_amax)
        ctx.res_mode = res_mode
        return out

    @staticmethod
    def backward(ctx, dout):
        gs, ts = ctx.gs, ctx.ts
        dout = dout.contiguous()
        cls = TCNGCNUnitFunction
        _SIDE_SCOPE[0] += 1
        try:
            dg, dtw, dtbias, dtg, dtb, drpre, drw, drbias, drg, drb = tcn_backward(      # (gcn_backward joins)
                ts, dout, join=False, want_sums=_wants(ctx, cls.TCN_SUMS))
            extra = dict(extra_add=dout, extra_mask=ts.bits) if ctx.res_mode == 1 else {}
            dx, dPA, dwab, dbab, dwd, dbd, dg1, db1, dwdown, dbdown, dg2, db2, _ = gcn_backward(
                gs, dg, want_sums=_wants(ctx, cls.GCN_SUMS), **extra)
        finally:
            _SIDE_SCOPE[0] -= 1
        if ctx.res_mode == 2:
            conv_bwd_data(drpre, ts.wres, gs.x.shape, ts.stride, out=dx, accumulate=True)
        ctx.gs = ctx.ts = None
        return cls.ARGS.grads(x=dx, PA=dPA, wab=dwab, bab=dbab, wd=dwd, bd=dbd, bn_w=dg1, bn_b=db1, down_w=dwdown,
                            down_b=dbdown, dbn_w=dg2, dbn_b=db2, tw=dtw, tb=dtbias, tbn_w=dtg, tbn_b=dtb, rw=drw,
                            rb=drbias, rbn_w=drg, rbn_b=drb)


# the names above are the forward signatures: an argument added to one and not to the other fails here, at import
for _f in (UnitGCNFunction, UnitTCNFunction, TCNResidualFunction, TCNGCNUnitFunction):
    assert _f.forward.__code__.co_varnames[1:_f.forward.__code__.co_argcount] == _f.ARGS.names, _f.__name__


# ------------------------------------------------------------------------------------------------
# transformer-encoder head of aagcn_v17 (csrc/encoder.hip): tokens, attention core, add + LayerNorm; for the spatial head
# of aagcn_v24: tokens over joints (one sequence per frame window) and the attention core with an additive bias
# ------------------------------------------------------------------------------------------------
def encoder_hip_enabled():
    """AGCN_ENCODER_HIP=0 runs the encoder head as the tensor-code composition of the same maths (``tokens_ref``,
    ``mha_ref``, ``add_ln_ref``): for A/B, and as the in-process comparison of the dropout path."""
    return os.environ.get('AGCN_ENCODER_HIP', '1') != '0'


# diagnostic counters (never read by a compute path): encoder layers that ran on the HIP kernels / as tensor code
ENCODER_STATS = {'layers_hip': 0, 'layers_tensor': 0}


class TokensFunction(torch.autograd.Function):
    """x (N*M, C, T', V), cls (1, 1, D) or None, pe (1, rows >= L, D) or None -> tok (N, L, D): token cls + m*T' + t,
    feature v*C + c, plus the positional rows (reference aagcn_v17.py:290-299).  args: x, cls, pe, M"""

    @staticmethod
    def forward(ctx, x, cls, pe, M):
        x = x.contiguous()
        NM, C, Tp, V = x.shape
        N, D = NM // M, V * C
        L = M * Tp + (cls is not None)
        cls_ = None if cls is None else cls.contiguous()
        pe_ = None if pe is None else pe.contiguous()
        tok = _empty((N, L, D), x)
        _lib.call("agcn_tokens_fwd", x, cls_, pe_, 0 if pe is None else pe.shape[-2], tok, N, M, C, Tp, V)
        ctx.dims = (N, M, C, Tp, V, cls is not None, None if pe is None else tuple(pe.shape))
        return tok

    @staticmethod
    def backward(ctx, dtok):
        N, M, C, Tp, V, has_cls, pe_shape = ctx.dims
        dtok = dtok.contiguous()
        ng = ctx.needs_input_grad
        dx = _empty((N * M, C, Tp, V), dtok) if ng[0] else None
        dcls = _empty((1, 1, V * C), dtok) if (has_cls and ng[1]) else None
        dpe = _empty(pe_shape, dtok) if (pe_shape is not None and ng[2]) else None
        _lib.call("agcn_tokens_bwd", dtok, dx, dcls, dpe, int(has_cls), 0 if dpe is None else pe_shape[-2], N, M, C, Tp,
                  V)
        return dx, dcls, dpe, None


def tokens_ref(x, cls, pe, M):
    """The tensor-code form of TokensFunction (any device, any dtype)."""
    NM, C, Tp, V = x.shape
    N = NM // M
    tok = x.reshape(N, M, C, Tp, V).permute(0, 1, 3, 4, 2).reshape(N, M * Tp, V * C)
    if cls is not None:
        tok = torch.cat((cls.expand(N, 1, V * C), tok), dim=1)
    if pe is not None:
        tok = tok + pe[:, :tok.size(1), :]
    return tok


def _spatial_dims(x, cls, pe, M, what):
    if x.dim() != 4 or M < 1 or x.shape[0] % M != 0:
        raise ValueError(f"agcn_amd.ops.{what}: x must be (N*M, C, T', V) with M = {M}, got {tuple(x.shape)}")
    NM, C, Tp, V = x.shape
    L = M * V + (cls is not None)
    if cls is not None and tuple(cls.shape) != (1, 1, C):
        raise ValueError(f"agcn_amd.ops.{what}: cls must be (1, 1, {C}), got {tuple(cls.shape)}")
    if pe is not None and (pe.dim() != 3 or pe.shape[0] != 1 or pe.shape[2] != C or pe.shape[1] < L):
        raise ValueError(f"agcn_amd.ops.{what}: pe must be (1, rows >= {L}, {C}), got {tuple(pe.shape)}")
    return NM // M, C, Tp, V, L


class SpatialTokensFunction(torch.autograd.Function):
    """x (N*M, C, T', V), cls (1, 1, C) or None, pe (1, rows >= L, C) or None -> tok (N*T', L, C), L = cls + M*V: one
    sequence per frame window, token cls + m*V + v, feature c, plus the positional rows (reference aagcn_v24.py:287-292).
    args: x, cls, pe, M"""

    @staticmethod
    def forward(ctx, x, cls, pe, M):
        N, C, Tp, V, L = _spatial_dims(x, cls, pe, M, 'SpatialTokensFunction')
        x = x.contiguous()
        cls_ = None if cls is None else cls.contiguous()
        pe_ = None if pe is None else pe.contiguous()
        tok = _empty((N * Tp, L, C), x)
        _lib.call("agcn_tokens_spatial_fwd", x, cls_, pe_, 0 if pe is None else pe.shape[-2], tok, N, M, C, Tp, V)
        ctx.dims = (N, M, C, Tp, V, cls is not None, None if pe is None else tuple(pe.shape))
        return tok

    @staticmethod
    def backward(ctx, dtok):
        N, M, C, Tp, V, has_cls, pe_shape = ctx.dims
        dtok = dtok.contiguous()
        ng = ctx.needs_input_grad
        dx = _empty((N * M, C, Tp, V), dtok) if ng[0] else None
        dcls = _empty((1, 1, C), dtok) if (has_cls and ng[1]) else None
        dpe = _empty(pe_shape, dtok) if (pe_shape is not None and ng[2]) else None
        ws, nbytes = None, 0
        if dcls is not None or dpe is not None:
            nbytes = _L().agcn_tokens_spatial_bwd_workspace(N, M, C, Tp, V, int(has_cls))
            ws = _ws(nbytes, dtok)
        _lib.call("agcn_tokens_spatial_bwd", dtok, dx, dcls, dpe, int(has_cls), 0 if dpe is None else pe_shape[-2], ws,
                  nbytes, N, M, C, Tp, V)
        return dx, dcls, dpe, None


def tokens_spatial_ref(x, cls, pe, M):
    """The tensor-code form of SpatialTokensFunction (any device, any dtype)."""
    N, C, Tp, V, L = _spatial_dims(x, cls, pe, M, 'tokens_spatial_ref')
    tok = x.reshape(N, M, C, Tp, V).permute(0, 3, 1, 4, 2).reshape(N * Tp, M * V, C)
    if cls is not None:
        tok = torch.cat((cls.expand(N * Tp, 1, C), tok), dim=1)
    if pe is not None:
        tok = tok + pe[:, :tok.size(1), :]
    return tok


class MHAFunction(torch.autograd.Function):
    """The attention core of one encoder layer on the packed in_proj output.
    args: qkv (N, L, 3D), H, null_tok (N, L) uint8 or None, causal (0 none, 1 j <= i, 2 j >= i), keep (N, H, L, L) uint8
    or None, keep_scale, need_avg -> ctx (N, L, D), avg (N, L, L) or None (head mean after dropout; not differentiable)"""

    @staticmethod
    def forward(ctx, qkv, H, null_tok, causal, keep, keep_scale, need_avg):
        qkv = qkv.contiguous()
        N, L, D3 = qkv.shape
        D = D3 // 3
        dh = D // H
        out = _empty((N, L, D), qkv)
        need_bwd = ctx.needs_input_grad[0]
        prob = _empty((N, H, L, L), qkv) if need_bwd else None
        avg = _empty((N, L, L), qkv) if need_avg else None
        _lib.call("agcn_mha_fwd", qkv, null_tok, int(causal), keep, float(keep_scale), out, prob, avg, N, L, H, dh)
        if need_bwd:
            ctx.save_for_backward(qkv, prob, keep)
        ctx.dims, ctx.keep_scale = (N, L, H, dh), float(keep_scale)
        if avg is not None:
            ctx.mark_non_differentiable(avg)
        return out, avg

    @staticmethod
    def backward(ctx, dout, _davg):
        qkv, prob, keep = ctx.saved_tensors
        N, L, H, dh = ctx.dims
        dout = dout.contiguous()
        dqkv = torch.empty_like(qkv)
        ws = _empty((N, H, L, L), qkv)
        _lib.call("agcn_mha_bwd", dout, qkv, prob, keep, ctx.keep_scale, dqkv, ws, ws.numel() * 4, N, L, H, dh)
        return dqkv, None, None, None, None, None, None


def _check_bias(bias, L, H, what):
    """bias (Hb, L, L), Hb in {1, H}: the additive attention bias of aagcn_v24, checked before any foreign call."""
    if bias.dim() != 3 or tuple(bias.shape[1:]) != (L, L) or bias.shape[0] not in (1, H):
        raise ValueError(f"agcn_amd.ops.{what}: bias must be (Hb, L, L) with Hb in (1, {H}) and L = {L}, got "
                         f"{tuple(bias.shape)}")


class MHABiasFunction(torch.autograd.Function):
    """MHAFunction with an additive bias on the logits (aagcn_v24's ``alpha * PA``): softmax(q k^T / sqrt(dh) + bias),
    the bias added before the masks and the row maximum.
    args: qkv (N, L, 3D), H, bias (Hb, L, L) with Hb in {1, H} or None, null_tok, causal, keep, keep_scale, need_avg ->
    ctx, avg.  dbias is the score gradient summed over the N sequences (and over the heads when Hb = 1), in a fixed
    order (agcn_mha_bias_grad).  bias None: MHAFunction's launches, bit for bit."""

    @staticmethod
    def forward(ctx, qkv, H, bias, null_tok, causal, keep, keep_scale, need_avg):
        if qkv.dim() != 3 or qkv.shape[-1] % (3 * H) != 0:
            raise ValueError(f"agcn_amd.ops.MHABiasFunction: qkv must be (N, L, 3*H*dh) with H = {H}, got "
                             f"{tuple(qkv.shape)}")
        qkv = qkv.contiguous()
        N, L, D3 = qkv.shape
        D = D3 // 3
        dh = D // H
        Hb = 0
        if bias is not None:
            _check_bias(bias, L, H, 'MHABiasFunction')
            bias = bias.contiguous()
            Hb = bias.shape[0]
        if null_tok is not None and tuple(null_tok.shape) != (N, L):
            raise ValueError(f"agcn_amd.ops.MHABiasFunction: null_tok must be {(N, L)}, got {tuple(null_tok.shape)}")
        if keep is not None and tuple(keep.shape) != (N, H, L, L):
            raise ValueError(f"agcn_amd.ops.MHABiasFunction: keep must be {(N, H, L, L)}, got {tuple(keep.shape)}")
        out = _empty((N, L, D), qkv)
        need_bwd = ctx.needs_input_grad[0] or ctx.needs_input_grad[2]
        prob = _empty((N, H, L, L), qkv) if need_bwd else None
        avg = _empty((N, L, L), qkv) if need_avg else None
        if bias is None:
            _lib.call("agcn_mha_fwd", qkv, null_tok, int(causal), keep, float(keep_scale), out, prob, avg, N, L, H, dh)
        else:
            _lib.call("agcn_mha_bias_fwd", qkv, bias, Hb, null_tok, int(causal), keep, float(keep_scale), out, prob, avg,
                      N, L, H, dh)
        if need_bwd:
            ctx.save_for_backward(qkv, prob, keep)
        ctx.dims, ctx.keep_scale, ctx.Hb = (N, L, H, dh), float(keep_scale), Hb
        if avg is not None:
            ctx.mark_non_differentiable(avg)
        return out, avg

    @staticmethod
    def backward(ctx, dout, _davg):
        qkv, prob, keep = ctx.saved_tensors
        N, L, H, dh = ctx.dims
        dout = dout.contiguous()
        dqkv = torch.empty_like(qkv)
        ds = _empty((N, H, L, L), qkv)
        _lib.call("agcn_mha_bwd", dout, qkv, prob, keep, ctx.keep_scale, dqkv, ds, ds.numel() * 4, N, L, H, dh)
        dbias = None
        if ctx.Hb and ctx.needs_input_grad[2]:
            dbias = _empty((ctx.Hb, L, L), qkv)
            nbytes = _L().agcn_mha_bias_grad_workspace(N, L, H, ctx.Hb)
            if nbytes == 0:
                raise RuntimeError(f"agcn_amd.ops.MHABiasFunction: no bias gradient for N={N} L={L} H={H} Hb={ctx.Hb}")
            ws = _ws(nbytes, qkv)
            _lib.call("agcn_mha_bias_grad", ds, dbias, ws, nbytes, N, L, H, ctx.Hb)
        return (dqkv if ctx.needs_input_grad[0] else None), None, dbias, None, None, None, None, None


def mha_ref(qkv, H, null_tok=None, causal=0, keep=None, keep_scale=1.0, need_avg=False, want_prob=False, bias=None):
    """The tensor-code form of MHAFunction / MHABiasFunction (any device, any dtype); want_prob also returns the softmax
    before dropout; bias (Hb, L, L), Hb in {1, H}, is added to the scaled logits."""
    N, L, D3 = qkv.shape
    D = D3 // 3
    dh = D // H
    q, k, v = (t.reshape(N, L, H, dh).transpose(1, 2) for t in qkv.split(D, dim=-1))
    s = (q @ k.transpose(-1, -2)) / (dh ** 0.5)
    if bias is not None:
        _check_bias(bias, L, H, 'mha_ref')
        s = s + bias[None]
    masked = torch.zeros(N, 1, L, L, dtype=torch.bool, device=qkv.device)
    if null_tok is not None:
        nt = null_tok.bool()
        masked = masked | (nt[:, None, :, None] & nt[:, None, None, :])
    if causal:
        i = torch.arange(L, device=qkv.device)
        masked = masked | ((i[None, :] > i[:, None]) if causal == 1 else (i[None, :] < i[:, None]))[None, None]
    s = s.masked_fill(masked, float('-inf'))
    dead = masked.all(-1, keepdim=True)
    p = torch.softmax(s.masked_fill(dead, 0.0), dim=-1).masked_fill(dead, 0.0)
    pd = p if keep is None else p * (keep.to(p.dtype) * keep_scale)
    out = (pd @ v).transpose(1, 2).reshape(N, L, D)
    avg = pd.mean(1) if need_avg else None
    return (out, avg, p) if want_prob else (out, avg)


class AddLayerNormFunction(torch.autograd.Function):
    """out = LayerNorm(a + b) over the last dimension (b None: of a).  args: a, b, weight, bias, eps"""

    @staticmethod
    def forward(ctx, a, b, weight, bias, eps):
        a = a.contiguous()
        b = None if b is None else b.contiguous()
        D = a.shape[-1]
        R = a.numel() // D
        out = torch.empty_like(a)
        mean, rstd = _empty((R,), a), _empty((R,), a)
        _lib.call("agcn_ln_fwd", a, b, weight, bias, float(eps), out, mean, rstd, R, D)
        ctx.save_for_backward(a, b, weight, mean, rstd)
        return out

    @staticmethod
    def backward(ctx, dout):
        a, b, weight, mean, rstd = ctx.saved_tensors
        dout = dout.contiguous()
        D = a.shape[-1]
        R = a.numel() // D
        dx = torch.empty_like(a)
        dg, db = _empty((D,), a), _empty((D,), a)
        ws = _empty(((min(R, 1024) + 3) * 2 * D,), a)      # one (dgamma, dbeta) row per wave: encoder_plan.h
        _lib.call("agcn_ln_bwd", dout, a, b, weight, mean, rstd, dx, dg, db, ws, ws.numel() * 4, R, D)
        return dx, (dx if b is not None else None), dg, db, None


def add_ln_ref(a, b, weight, bias, eps):
    """The tensor-code form of AddLayerNormFunction."""
    x = a if b is None else a + b
    return torch.nn.functional.layer_norm(x, (x.shape[-1],), weight, bias, eps)


# ------------------------------------------------------------------------------------------------
# base SGN, eval-mode inference (csrc/sgn.hip): sampler, joint-level module, frame-level module + fc
# ------------------------------------------------------------------------------------------------
def sgn_hip_enabled():
    """AGCN_SGN_HIP=0 runs SGN's eval forward as the tensor-code composition of the same maths (model/sgn.py): for A/B."""
    return os.environ.get('AGCN_SGN_HIP', '1') != '0'


# diagnostic counters (never read by a compute path): launches of the three kernels, and SGN forwards that ran as
# tensor code (grad mode, train(), a CPU tensor, AGCN_SGN_HIP=0)
SGN_STATS = {'frames_hip': 0, 'clip_hip': 0, 'sample_hip': 0, 'forward_tensor': 0}


def sgn_frames(x, wimg, V, want_g=True):
    """The joint-level module of SGN on x (N, seg, V*3) with the folded weight image ``wimg`` (model/sgn.py) ->
    feat (N, seg, 256), the maximum over the joints of gcn3's output, and g (N, seg, V, V) (None without want_g)."""
    if x.dim() != 3 or x.shape[2] != 3 * V:
        raise ValueError(f"agcn_amd: sgn_frames takes (N, seg, {3 * V}), got {tuple(x.shape)}")
    N, seg, _ = x.shape
    feat = _empty((N, seg, 256), x)
    g = _empty((N, seg, V, V), x) if want_g else None
    _lib.call("agcn_sgn_frames", x, wimg, wimg.numel(), feat, g, N, seg, V)
    SGN_STATS['frames_hip'] += 1
    return feat, g


def sgn_clip(feat, wimg, num_class):
    """The frame-level module and the classifier of SGN on feat (N, seg, 256) -> logits (N, num_class)."""
    N, seg, C = feat.shape
    if C != 256:
        raise ValueError(f"agcn_amd: sgn_clip takes (N, seg, 256), got {tuple(feat.shape)}")
    logits = _empty((N, num_class), feat)
    _lib.call("agcn_sgn_clip", feat, wimg, wimg.numel(), logits, N, seg, num_class)
    SGN_STATS['clip_hip'] += 1
    return logits


def sgn_draws(N, S, seg, device, generator=None):
    """(N, S, seg) random 32-bit patterns for ``sgn_sample``, drawn on the device (no sync).  The sampler reduces them
    modulo an interval width of at most a few hundred rows: the bias of that at 32 bits is below 1e-7.  ``generator``: a
    torch.Generator of that device instead of its default one."""
    return torch.randint(0, 1 << 32, (N, S, seg), dtype=torch.int64, device=device, generator=generator).to(torch.int32)


def _sgn_sample_args(name, win, r, seg):
    """The window and draw checks of ``sgn_sample`` and ``sgn_sample_bwd`` (``name``: the one that was called) ->
    (r as int32, N, T, V, K, S)."""
    if win.dim() != 5 or win.shape[1] != 3:
        raise ValueError(f"agcn_amd: {name} takes windows (N, 3, T, V, 2), got {tuple(win.shape)}")
    N, _, T, V, K = win.shape
    if K != 2:
        raise ValueError(f"agcn_amd: {name} interleaves exactly two selected bodies, got {K}")
    if r.dtype == torch.uint32:
        r = r.view(torch.int32)
    if r.dim() != 3 or r.shape[0] != N or r.shape[2] != seg or r.dtype != torch.int32:
        raise ValueError(f"agcn_amd: {name} takes draws ({N}, S, {seg}) int32, got {r.dtype} {tuple(r.shape)}")
    return r, N, T, V, K, r.shape[1]


def sgn_sample(win, r, seg):
    """NTUDataLoaders.to_fix_length (equal-interval branch) on normalised windows win (N, 3, T, V, 2) in ``prenorm``'s
    output layout (agcn_sgn_sample): null rows dropped, the two bodies interleaved by frame, fewer than ``seg`` rows
    zero-padded, and one row per interval and draw.  r (N, S, seg): the draws as 32-bit patterns in an int32 (or uint32)
    tensor, read as unsigned.  Returns (out (N, S, seg, V*3), L (N,) int32 row counts), on the device."""
    r, N, T, V, K, S = _sgn_sample_args("sgn_sample", win, r, seg)
    out = _empty((N, S, seg, V * 3), win)
    L = torch.empty((N,), dtype=torch.int32, device=win.device)
    _lib.call("agcn_sgn_sample", win, r, out, L, N, T, V, K, S, seg)
    SGN_STATS['sample_hip'] += 1
    return out, L


# ------------------------------------------------------------------------------------------------
# base SGN, the training / evaluation collate (csrc/sgn.hip::sgn_collate_kernel): the reference's three collates
# (feeders/loader.py:109-201) on a dataset that lives on the device
# ------------------------------------------------------------------------------------------------
# diagnostic counters (a dict of its own: SGN_STATS is compared whole by its tests)
SGN_COLLATE_STATS = dict(collate_hip=0, collate_ref=0)


def sgn_rotation_angles(N, theta, device, generator=None):
    """(N, 3) rotation angles in radians, uniform in [-theta, theta), from the device's generator (no sync): the
    counterpart of ``sgn_draws`` for the rotation of ``sgn_collate`` (reference feeders/tools.py::torch_transform)."""
    return torch.empty((N, 3), dtype=torch.float32, device=device).uniform_(-float(theta), float(theta),
                                                                            generator=generator)


def sgn_rotation_ref(angles):
    """angles (N, 3) -> R (N, 3, 3) fp32 numpy, R = (Rz . Ry) . Rx with the reference's matrices
    (feeders/tools.py::_rot: the transposes of the usual right-handed ones) -- what ``sgn_rotation`` in sgn_plan.h builds."""
    a = np.asarray(angles.detach().cpu().numpy() if torch.is_tensor(angles) else angles, dtype=np.float32).reshape(-1, 3)
    c, s = np.cos(a), np.sin(a)
    R = np.zeros((3, a.shape[0], 3, 3), dtype=np.float32)
    R[:, :, 0, 0] = R[:, :, 1, 1] = R[:, :, 2, 2] = 1.0
    rx, ry, rz = R
    rx[:, 1, 1], rx[:, 1, 2], rx[:, 2, 1], rx[:, 2, 2] = c[:, 0], s[:, 0], -s[:, 0], c[:, 0]
    ry[:, 0, 0], ry[:, 0, 2], ry[:, 2, 0], ry[:, 2, 2] = c[:, 1], -s[:, 1], s[:, 1], c[:, 1]
    rz[:, 0, 0], rz[:, 0, 1], rz[:, 1, 0], rz[:, 1, 1] = c[:, 2], s[:, 2], -s[:, 2], c[:, 2]
    return np.matmul(np.matmul(rz, ry), rx)


def _sgn_collate_args(pool, r, seg, index, angles):
    """The checks of ``sgn_collate`` and ``sgn_collate_ref`` -> (r as int32, N, S)."""
    if pool.dim() != 5 or pool.shape[1] != 3 or pool.shape[4] != 2 or pool.shape[0] < 1:
        raise ValueError(f"agcn_amd: sgn_collate takes a pool (P, 3, T, V, 2), got {tuple(pool.shape)}")
    if r.dtype == torch.uint32:
        r = r.view(torch.int32)
    if r.dim() != 3 or r.shape[0] < 1 or r.shape[1] < 1 or r.shape[2] != seg or r.dtype != torch.int32:
        raise ValueError(f"agcn_amd: sgn_collate takes draws (N, S, {seg}) int32, got {r.dtype} {tuple(r.shape)}")
    N, S = r.shape[0], r.shape[1]
    if index is None:
        if N > pool.shape[0]:
            raise ValueError(f"agcn_amd: sgn_collate without an index collates the first N samples: N = {N} > P = "
                             f"{pool.shape[0]}")
    elif index.dtype != torch.int64 or tuple(index.shape) != (N,):
        raise ValueError(f"agcn_amd: sgn_collate takes index ({N},) int64, got {index.dtype} {tuple(index.shape)}")
    if angles is not None and (angles.dtype != torch.float32 or tuple(angles.shape) != (N, 3)):
        raise ValueError(f"agcn_amd: sgn_collate takes angles ({N}, 3) fp32, got {angles.dtype} {tuple(angles.shape)}")
    P, _, T, V, _ = pool.shape
    if not (T <= 2048 and 2 <= V <= 32 and S * seg <= (1 << 20)):
        raise ValueError(f"agcn_amd: sgn_collate: T = {T}, V = {V}, S * seg = {S * seg} outside the sampler's domain "
                         f"(T <= 2048, 2 <= V <= 32, S * seg <= 2^20)")
    return r, N, S


def sgn_collate_ref(pool, r, seg, index=None, angles=None, want_subject=False):
    """The specification of ``sgn_collate`` as numpy on the host (and its route for CPU tensors and AGCN_SGN_HIP=0):
    same arguments, same results, returned on ``pool``'s device.  Per clip n: sample ``index[n]`` (n without an index;
    outside [0, P): zeros, L = 0); row (t, m) is kept iff body m's frame t is not all zero, rows in (t, m) order; fewer
    than ``seg`` rows are followed by zero rows; b_k = rint(k * (L / seg)) in fp64; draw s takes row
    b_k + r[n, s, k] % (b_{k+1} - b_k); the subject flag is the body m of that row (0 for a padding row); with angles
    every joint of a picked row becomes R_n . p (``sgn_rotation_ref``), in fp32."""
    r, N, S = _sgn_collate_args(pool, r, seg, index, angles)
    pn = pool.detach().cpu().numpy()
    rn = r.detach().cpu().numpy().view(np.uint32).astype(np.int64)
    idx = np.arange(N) if index is None else index.detach().cpu().numpy()
    P, _, T, V, _ = pn.shape
    out = np.zeros((N, S, seg, V * 3), dtype=np.float32)
    subj = np.zeros((N, S, seg), dtype=np.float32)
    Ls = np.zeros((N,), dtype=np.int32)
    bodies = np.arange(2 * T) & 1
    for n in range(N):
        if not 0 <= idx[n] < P:
            continue
        rows = np.transpose(pn[idx[n]], (1, 3, 2, 0)).reshape(T * 2, V * 3)        # (t, m) major, (v, c) minor
        keep = (rows != 0).any(1)
        kept = int(keep.sum())
        if kept == 0:
            continue
        L = max(kept, seg)
        rows = np.concatenate([rows[keep], np.zeros((L - kept, V * 3), dtype=np.float32)])
        body = np.concatenate([bodies[keep], np.zeros((L - kept,), dtype=np.int64)]).astype(np.float32)
        b = np.rint(np.arange(seg + 1, dtype=np.float64) * (float(L) / float(seg))).astype(np.int64)
        pick = np.clip(b[:-1] + rn[n] % np.maximum(b[1:] - b[:-1], 1), 0, L - 1)    # (S, seg)
        out[n], subj[n], Ls[n] = rows[pick], body[pick], L
    if angles is not None:
        R = sgn_rotation_ref(angles)[:, None, None, None]                           # (N, 1, 1, 1, 3, 3)
        p = out.reshape(N, S, seg, V, 3)
        x, y, z = p[..., 0:1], p[..., 1:2], p[..., 2:3]
        out = (R[..., 0] * x + R[..., 1] * y + R[..., 2] * z).astype(np.float32).reshape(N, S, seg, V * 3)
    SGN_COLLATE_STATS['collate_ref'] += 1
    dev = pool.device
    return (torch.from_numpy(out).to(dev), torch.from_numpy(Ls).to(dev),
            torch.from_numpy(subj).to(dev) if want_subject else None)


def sgn_collate(pool, r, seg, index=None, angles=None, want_subject=False):
    """The reference's SGN collates (feeders/loader.py::collate_fn_fix_train / _val / _test) as one launch
    (agcn_sgn_collate) on a dataset ``pool`` (P, 3, T, V, 2) that lives on the device.  r (N, S, seg): the draws, as for
    ``sgn_sample``.  index (N,) int64 on the device: the samples to collate (None: the first N); an index outside
    [0, P) gives a zero clip and L = 0.  angles (N, 3) radians: the training rotation, shared by a sample's S draws
    (None: none, and then the values are ``sgn_sample``'s bits).  Returns (x (N, S, seg, V*3), L (N,) int32, subject
    flags (N, S, seg) or None).  A CPU pool, or AGCN_SGN_HIP=0, runs ``sgn_collate_ref``."""
    if not (pool.is_cuda and sgn_hip_enabled()):
        return sgn_collate_ref(pool, r, seg, index, angles, want_subject)
    r, N, S = _sgn_collate_args(pool, r, seg, index, angles)
    P, _, T, V, K = pool.shape
    for name, t in (('r', r), ('index', index), ('angles', angles)):
        if t is not None and not (t.device == pool.device and t.is_contiguous()):
            raise ValueError(f"agcn_amd: sgn_collate takes a contiguous {name} on {pool.device}")
    out = _empty((N, S, seg, V * 3), pool)
    L = torch.empty((N,), dtype=torch.int32, device=pool.device)
    subj = _empty((N, S, seg), pool) if want_subject else None
    _lib.call("agcn_sgn_collate", pool, index, r, angles, out, subj, L, P, N, T, V, K, S, seg)
    SGN_COLLATE_STATS['collate_hip'] += 1
    return out, L, subj


# ------------------------------------------------------------------------------------------------
# base SGN, input gradients in eval mode (csrc/sgn_bwd.hip): the backward of the two launches above with respect to x,
# and the adjoint of the sampler.  The parameter gradients are further down (csrc/sgn_wgrad.hip).
# ------------------------------------------------------------------------------------------------
# diagnostic counters of the backward launches (a dict of its own: SGN_STATS is compared whole by its tests)
SGN_GRAD_STATS = dict(clip_bwd=0, frames_bwd=0, sample_bwd=0)


def _sgn_clip_bwd(fam, feat, wimg, wimg_t, dlogits, block, tape):
    """The clip backward of the family ``fam`` (``_SGN`` / ``_SGN15``; ``block``: () / (heads, d_head, ff)) -> dfeat, or
    with ``tape`` the taping instantiation (the same dfeat bits) -> (dfeat, tape)."""
    name = fam.prefix + ("_clip_bwd_tape" if tape else "_clip_bwd")
    if feat.dim() != 3 or feat.shape[2] != 256:
        raise ValueError(f"agcn_amd: {name} takes feat (N, seg, 256), got {tuple(feat.shape)}")
    N, seg, _ = feat.shape
    if dlogits.dim() != 2 or dlogits.shape[0] != N or (tape and dlogits.shape[1] < 1):
        raise ValueError(f"agcn_amd: {name} takes dlogits ({N}, num_class), got {tuple(dlogits.shape)}")
    nc = dlogits.shape[1]
    tp = _tape(getattr(_L(), f"agcn_{fam.prefix}_clip_tape_floats"), (N, seg, nc) + block, feat, name) if tape else None
    dfeat = _empty((N, seg, 256), feat)
    _lib.call("agcn_" + name, feat, wimg, wimg.numel(), wimg_t, wimg_t.numel(), dlogits, dfeat, N, seg, nc, *block,
              *((tp, tp.numel()) if tape else ()))
    (fam.wgrad_stats if tape else fam.bwd_stats)["clip_bwd_tape" if tape else "clip_bwd"] += 1
    return (dfeat, tp) if tape else dfeat


def _sgn_frames_bwd(fam, x, wimg, wimg_t, dfeat, V, block, tape):
    """The frames backward of the family ``fam`` -> dx, or with ``tape`` the taping instantiation (the same dx bits) ->
    (dx, tape)."""
    name = fam.prefix + ("_frames_bwd_tape" if tape else "_frames_bwd")
    if x.dim() != 3 or x.shape[2] != 3 * V:
        raise ValueError(f"agcn_amd: {name} takes (N, seg, {3 * V}), got {tuple(x.shape)}")
    N, seg, _ = x.shape
    if tuple(dfeat.shape) != (N, seg, 256):
        raise ValueError(f"agcn_amd: {name} takes dfeat ({N}, {seg}, 256), got {tuple(dfeat.shape)}")
    tp = _tape(getattr(_L(), f"agcn_{fam.prefix}_frames_tape_floats"), (N, seg, V) + block, x, name) if tape else None
    dx = _empty((N, seg, 3 * V), x)
    ws = _empty((max(1, getattr(_L(), f"agcn_{fam.prefix}_frames_bwd_workspace")(N, seg, V) // 4),), x)
    _lib.call("agcn_" + name, x, wimg, wimg.numel(), wimg_t, wimg_t.numel(), dfeat, dx, ws, ws.numel() * 4, N, seg, V,
              *block, *((tp, tp.numel()) if tape else ()))
    (fam.wgrad_stats if tape else fam.bwd_stats)["frames_bwd_tape" if tape else "frames_bwd"] += 1
    return (dx, tp) if tape else dx


def sgn_clip_bwd(feat, wimg, wimg_t, dlogits):
    """d logits (N, num_class) -> d feat (N, seg, 256) through fc, the maximum over the frames and the two convolutions
    of the frame-level module, recomputed from feat (N, seg, 256).  wimg: the forward image, wimg_t: the transposed one."""
    return _sgn_clip_bwd(_SGN, feat, wimg, wimg_t, dlogits, (), tape=False)


def sgn_frames_bwd(x, wimg, wimg_t, dfeat, V):
    """d feat (N, seg, 256) -> dx (N, seg, V*3) through the joint-level module, recomputed from x, and the dif coupling
    between the frames of a clip."""
    return _sgn_frames_bwd(_SGN, x, wimg, wimg_t, dfeat, V, (), tape=False)


def sgn_sample_bwd(win, r, dout, seg):
    """The adjoint of ``sgn_sample``: dout (N, S, seg, V*3) -> dwin (N, 3, T, V, 2).  Every picked row's gradient is added
    to its source row of the window (a row picked by several draws accumulates, in the order s major, k minor); padding
    rows and empty windows contribute nothing."""
    r, N, T, V, K, S = _sgn_sample_args("sgn_sample_bwd", win, r, seg)
    if tuple(dout.shape) != (N, S, seg, V * 3):
        raise ValueError(f"agcn_amd: sgn_sample_bwd takes dout ({N}, {S}, {seg}, {V * 3}), got {tuple(dout.shape)}")
    dwin = _empty(tuple(win.shape), win)
    _lib.call("agcn_sgn_sample_bwd", win, r, dout, dwin, N, T, V, K, S, seg)
    SGN_GRAD_STATS['sample_bwd'] += 1
    return dwin


class SGNInputGradFunction(torch.autograd.Function):
    """SGN's eval forward as the two fused launches, differentiable with respect to x alone (the parameters are frozen:
    model/sgn.py routes here only then).  args: x, wf, wc, wf_t, wc_t, V, num_class -> logits, g (g is not
    differentiable)."""

    @staticmethod
    def forward(ctx, x, wf, wc, wf_t, wc_t, V, num_class):
        x = x.contiguous()
        feat, g = sgn_frames(x, wf, V)
        logits = sgn_clip(feat, wc, num_class)
        ctx.save_for_backward(x, feat, wf, wc, wf_t, wc_t)
        ctx.V = V
        ctx.mark_non_differentiable(g)
        return logits, g

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dlogits, _dg):
        x, feat, wf, wc, wf_t, wc_t = ctx.saved_tensors
        dfeat = sgn_clip_bwd(feat, wc, wc_t, dlogits.contiguous())
        return sgn_frames_bwd(x, wf, wf_t, dfeat, ctx.V), None, None, None, None, None, None


# ------------------------------------------------------------------------------------------------
# base SGN, parameter gradients in eval mode (the taping backward of csrc/sgn_bwd.hip and the reductions of
# csrc/sgn_wgrad.hip): frozen-BatchNorm fine-tuning.  The kernels give the
# gradient with respect to the two folded weight images, in the images' layout; torch autograd takes it through the
# fold (model/sgn.py::SGN._folded) to the parameters.  Batch statistics: further down (csrc/sgn_stats.hip).
# ------------------------------------------------------------------------------------------------
# diagnostic counters of these launches (a dict of its own: SGN_STATS and SGN_GRAD_STATS are compared whole by their tests)
SGN_WGRAD_STATS = dict(clip_bwd_tape=0, frames_bwd_tape=0, frames_wgrad=0, clip_wgrad=0)
# a batch whose tapes would be larger is processed in chunks of whole clips
SGN_MAX_TAPE_BYTES = 512 << 20

# What tells the two models of the family apart in the host code they share (the backward launches, the chunked image
# backward, the fine-tuning Functions): the prefix of the C entries, the name in messages, and the counter dicts of the
# plain and of the taping backward launches.  ``_SGN15`` stands with its counters further down.
_SgnFamily = collections.namedtuple('_SgnFamily', 'prefix what bwd_stats wgrad_stats')
_SGN = _SgnFamily('sgn', 'SGN', SGN_GRAD_STATS, SGN_WGRAD_STATS)


def _sgn_layout(items):
    """[(name, shape)] -> [(name, offset, shape)]: the sections of an image back to back, offsets in floats."""
    out, o = [], 0
    for name, shape in items:
        out.append((name, o, shape))
        o += math.prod(shape)
    return out


def _sgn_emb_sections(p):
    """The two 1x1 layers of an input embedding under the prefix ``p``."""
    return [(p + '1_w', (3, 64)), (p + '1_b', (64,)), (p + '2_w', (64, 64)), (p + '2_b', (64,))]


def sgn_image_sections(V, seg, num_class):
    """The sections of the two folded weight images in their order (csrc/sgn_plan.h: SgnFramesW, SgnClipW) ->
    (frames, clip), each a list of (name, offset, shape)."""
    frames = _sgn_layout([('aff', (4, V, 3))] + _sgn_emb_sections('je') + _sgn_emb_sections('de')
                         + [('spa1', (V, 64)), ('g_w', (128, 512)), ('g_b', (512,)), ('c1_w', (256, 128)), ('c1_b', (128,)),
                            ('c2_w', (256, 256)), ('c2_b', (256,)), ('c3_w', (512, 256)), ('c3_b', (256,))])
    clip = _sgn_layout([('tem1', (seg, 256)), ('t1_w', (768, 256)), ('t1_b', (256,)), ('t2_w', (256, 512)),
                        ('t2_b', (512,)), ('fc_w', (512, num_class)), ('fc_b', (num_class,))])
    return frames, clip


def _sgn_ref_views(name, plan, x, wf, wc, V, seg, sections):
    """The checks of the two tensor-code references (``name``: the one that was called, ``plan``: the header of its
    layout) and the two flat images as their ``sections`` -> ({name: view} of the frames image, of the clip image)."""
    if x.dim() != 3 or x.shape[1] != seg or x.shape[2] != 3 * V:
        raise ValueError(f"agcn_amd: {name} takes (N, {seg}, {3 * V}), got {tuple(x.shape)}")
    views = []
    for img, secs in zip((wf, wc), sections):
        if img.numel() != secs[-1][1] + math.prod(secs[-1][2]):
            raise ValueError(f"agcn_amd: {name}: the images do not have the sizes of {plan}")
        views.append({n: img[o:o + math.prod(s)].reshape(s) for n, o, s in secs})
    return views


def _sgn_ref_input(x, f, V, seg, pos, vel):
    """The input side both models share, from the views ``f`` of a frames image: the affine of the two DataNorms, the
    embeddings under the prefixes ``pos`` (of x) and ``vel`` (of the frame difference), summed -> (N, seg, V, 64)."""
    relu = torch.relu
    N = x.shape[0]
    xr = x.reshape(N, seg, V, 3)
    dif = torch.cat([xr.new_zeros(N, 1, V, 3), xr[:, 1:] - xr[:, :-1]], dim=1)

    def emb(v, p):
        return relu(relu(v @ f[p + '1_w'] + f[p + '1_b']) @ f[p + '2_w'] + f[p + '2_b'])

    return emb(xr * f['aff'][0] + f['aff'][1], pos) + emb(dif * f['aff'][2] + f['aff'][3], vel)


def sgn_image_forward_ref(x, wf, wc, V, seg, num_class):
    """The tensor-code form of the fused SGN forward: x (N, seg, V*3) and the two flat folded images -> (logits, g),
    differentiable in x, wf and wc.  The CPU route of SGNFineTuneFunction and the comparison of its image gradients."""
    f, c = _sgn_ref_views("sgn_image_forward_ref", "csrc/sgn_plan.h", x, wf, wc, V, seg,
                          sgn_image_sections(V, seg, num_class))
    relu = torch.relu
    N = x.shape[0]
    h = torch.cat([_sgn_ref_input(x, f, V, seg, 'je', 'de'), f['spa1'].expand(N, seg, V, 64)], dim=3)
    gg = h @ f['g_w'] + f['g_b']
    g = torch.softmax(gg[..., :256] @ gg[..., 256:].transpose(-1, -2), dim=-1)
    for l in ('c1', 'c2', 'c3'):
        h = relu(torch.cat([g @ h, h], dim=3) @ f[l + '_w'] + f[l + '_b'])
    H = h.amax(2) + c['tem1']
    Hp = torch.nn.functional.pad(H, (0, 0, 1, 1))
    taps = torch.cat([Hp[:, dt:dt + seg] for dt in range(3)], dim=2)
    y2 = relu(relu(taps @ c['t1_w'] + c['t1_b']) @ c['t2_w'] + c['t2_b'])
    return y2.amax(1) @ c['fc_w'] + c['fc_b'], g


def _tape(query, args, like, what):
    n = query(*args)
    if n == 0:
        raise ValueError(f"agcn_amd: {what}: {args} is outside the kernels' domain")
    return _empty((n,), like)


def sgn_clip_bwd_tape(feat, wimg, wimg_t, dlogits):
    """``sgn_clip_bwd`` (the same dfeat bits) that also writes the clip tape (csrc/sgn_wgrad_plan.h: SgnClipTape) ->
    (dfeat, tape)."""
    return _sgn_clip_bwd(_SGN, feat, wimg, wimg_t, dlogits, (), tape=True)


def sgn_frames_bwd_tape(x, wimg, wimg_t, dfeat, V):
    """``sgn_frames_bwd`` (the same dx bits) that also writes the frames tape (SgnFramesTape) -> (dx, tape)."""
    return _sgn_frames_bwd(_SGN, x, wimg, wimg_t, dfeat, V, (), tape=True)


def _sgn_wgrad_ws(fam, args, rows_per_split, like):
    """The workspace of a reduction of the family ``fam``; ``args``: its size query's, without ``rows_per_split``."""
    if rows_per_split < 0:
        raise ValueError(f"agcn_amd: rows_per_split must be >= 0, got {rows_per_split}")
    n = getattr(_L(), f"agcn_{fam.prefix}_wgrad_workspace")(*args, rows_per_split)
    if n == 0:
        raise ValueError(f"agcn_amd: {fam.what} parameter gradients: {args} is outside the kernels' domain")
    return _empty((n // 4,), like)


def sgn_frames_wgrad(x, wimg, tape, V, num_class, rows_per_split=0):
    """The frames tape -> the gradient of the frames image, in its layout."""
    N, seg, _ = x.shape
    if tape.numel() < _L().agcn_sgn_frames_tape_floats(N, seg, V) or x.shape[2] != 3 * V:
        raise ValueError(f"agcn_amd: sgn_frames_wgrad: a tape of {tape.numel()} floats is not the tape of {tuple(x.shape)}")
    ws = _sgn_wgrad_ws(_SGN, (N, seg, V, num_class), rows_per_split, x)
    d_w = _empty((wimg.numel(),), x)
    _lib.call("agcn_sgn_frames_wgrad", x, wimg, tape, d_w, ws, ws.numel() * 4, N, seg, V, rows_per_split)
    SGN_WGRAD_STATS['frames_wgrad'] += 1
    return d_w


def sgn_clip_wgrad(tape, dfeat, dlogits, wimg, V, rows_per_split=0):
    """The clip tape, dfeat and dlogits -> the gradient of the clip image, in its layout."""
    N, seg, _ = dfeat.shape
    nc = dlogits.shape[1]
    if tape.numel() < _L().agcn_sgn_clip_tape_floats(N, seg, nc) or tuple(dlogits.shape) != (N, nc):
        raise ValueError(f"agcn_amd: sgn_clip_wgrad: a tape of {tape.numel()} floats is not the tape of {tuple(dfeat.shape)}")
    ws = _sgn_wgrad_ws(_SGN, (N, seg, V, nc), rows_per_split, dfeat)
    d_w = _empty((wimg.numel(),), dfeat)
    _lib.call("agcn_sgn_clip_wgrad", tape, dfeat, dlogits, d_w, ws, ws.numel() * 4, N, seg, nc, rows_per_split)
    SGN_WGRAD_STATS['clip_wgrad'] += 1
    return d_w


def _sgn_tape_chunk(fam, args, N, frames_floats, clip_floats, max_tape_bytes, most):
    """``sgn_tape_chunk`` / ``sgn15_tape_chunk`` from the floats of the two tapes of one clip; at most ``most`` clips."""
    if frames_floats == 0 or clip_floats == 0:
        raise ValueError(f"agcn_amd: {fam.what} parameter gradients: {args} is outside the kernels' domain")
    return max(1, min(N, most, int(max_tape_bytes) // (4 * (frames_floats + clip_floats))))


def sgn_tape_chunk(N, seg, V, num_class, max_tape_bytes):
    """Clips per chunk: as many whole clips as fit ``max_tape_bytes`` of tape (both tapes are linear in the clips), at
    least one."""
    return _sgn_tape_chunk(_SGN, (seg, V, num_class), N, _L().agcn_sgn_frames_tape_floats(1, seg, V),
                           _L().agcn_sgn_clip_tape_floats(1, seg, num_class), max_tape_bytes, N)


def _sgn_chunked_backward(step, chunk, x, feat, dlogits):
    """The image backward of both models in chunks of ``chunk`` whole clips -> (dx, d_wf, d_wc).  ``step(x, feat,
    dlogits)`` of one chunk -> (dx, d_wf, d_wc) is the family's: the taping clip backward, the taping frames backward and
    the two reductions; its tapes are gone when it returns.  dx is concatenated in clip order and the chunks' image
    gradients are added in ascending chunk order."""
    dxs, d_wf, d_wc = [], None, None
    for n0 in range(0, x.shape[0], chunk):
        dx, gf, gc = step(x[n0:n0 + chunk], feat[n0:n0 + chunk], dlogits[n0:n0 + chunk])
        dxs.append(dx)
        d_wf = gf if d_wf is None else d_wf + gf
        d_wc = gc if d_wc is None else d_wc + gc
    return (dxs[0] if len(dxs) == 1 else torch.cat(dxs)), d_wf, d_wc


def _sgn_image_backward(x, feat, wf, wc, wf_t, wc_t, dlogits, V, rows_per_split, max_tape_bytes):
    """-> (dx, d_wf, d_wc) of base SGN, chunked under ``max_tape_bytes`` of tape."""
    nc = dlogits.shape[1]

    def step(xs, fe, dl):
        dfeat, ctape = sgn_clip_bwd_tape(fe, wc, wc_t, dl)
        dx, ftape = sgn_frames_bwd_tape(xs, wf, wf_t, dfeat, V)
        return (dx, sgn_frames_wgrad(xs, wf, ftape, V, nc, rows_per_split),
                sgn_clip_wgrad(ctape, dfeat, dl, wc, V, rows_per_split))

    return _sgn_chunked_backward(step, sgn_tape_chunk(x.shape[0], x.shape[1], V, nc, max_tape_bytes), x, feat, dlogits)


def _sgn_finetune_ref(ctx, ref, x, wf, wc):
    """The CPU route of the two fine-tuning Functions: ``ref(x, wf, wc)``, a tensor-code image reference with the logits
    first, under ``enable_grad`` on fresh leaves, kept for ``_sgn_finetune_backward`` -> its outputs, detached."""
    with torch.enable_grad():
        leaves = [t.detach().requires_grad_(True) for t in (x, wf, wc)]
        out = ref(*leaves)
    ctx.ref = (leaves, out[0])
    return tuple(t.detach() for t in out)


def _sgn_finetune_backward(ctx, image_backward, dlogits):
    """The backward of the two fine-tuning Functions -> (dx or None, d_wf, d_wc): autograd of the kept reference on the
    CPU route, otherwise the family's ``image_backward`` on the saved tensors and ``ctx.geometry``."""
    if ctx.ref is not None:
        leaves, logits = ctx.ref
        with torch.enable_grad():
            dx, d_wf, d_wc = torch.autograd.grad(logits, leaves, dlogits)
    else:
        dx, d_wf, d_wc = image_backward(*ctx.saved_tensors, dlogits.contiguous(), *ctx.geometry, 0, SGN_MAX_TAPE_BYTES)
    return (dx if ctx.needs_input_grad[0] else None), d_wf, d_wc


def sgn_image_gradients(x, wf, wc, wf_t, wc_t, cot, V, num_class, rows_per_split=0, max_tape_bytes=SGN_MAX_TAPE_BYTES):
    """The fused eval forward and the gradient of sum(logits * cot) with respect to x and to the two folded images ->
    (logits, g, dx, d_wf, d_wc); d_wf / d_wc have the layout of wf / wc."""
    with torch.no_grad():
        x = x.detach().contiguous()
        feat, g = sgn_frames(x, wf, V)
        logits = sgn_clip(feat, wc, num_class)
        cot = cot.detach().to(logits).contiguous()
        if tuple(cot.shape) != tuple(logits.shape):
            raise ValueError(f"agcn_amd: sgn_image_gradients takes cot {tuple(logits.shape)}, got {tuple(cot.shape)}")
        return (logits, g) + _sgn_image_backward(x, feat, wf, wc, wf_t, wc_t, cot, V, rows_per_split, max_tape_bytes)


class SGNFineTuneFunction(torch.autograd.Function):
    """SGN's eval forward as the two fused launches, differentiable with respect to x and the two folded weight images
    (built in grad mode by model/sgn.py, so autograd continues through the fold to the parameters).  args: x, wf, wc,
    wf_t, wc_t, V, num_class -> logits, g (g is not differentiable).  A CPU tensor runs ``sgn_image_forward_ref``."""

    @staticmethod
    def forward(ctx, x, wf, wc, wf_t, wc_t, V, num_class):
        ctx.geometry = (V,)
        if not x.is_cuda:
            logits, g = _sgn_finetune_ref(ctx, lambda *leaves: sgn_image_forward_ref(*leaves, V, x.shape[1], num_class),
                                          x, wf, wc)
        else:
            x = x.contiguous()
            feat, g = sgn_frames(x, wf.detach(), V)
            logits = sgn_clip(feat, wc.detach(), num_class)
            ctx.ref = None
            ctx.save_for_backward(x, feat, wf, wc, wf_t, wc_t)
        ctx.mark_non_differentiable(g)
        return logits, g

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dlogits, _dg):
        return _sgn_finetune_backward(ctx, _sgn_image_backward, dlogits) + (None,) * 4


# ---- what model/sgn.py and model/sgn_v15.py share around these routes ----
def _sgn_t(w):
    """Conv / linear weight (Cout, Cin, ...) -> the (Cin, Cout) row-major image the kernels read."""
    return w.flatten(1).t()


def sgn_input_gradient(x, wf, wc, wf_t, wc_t, cot, V, num_class):
    """The fused eval forward of base SGN and dx = d sum(logits * cot) / dx as four launches -> (logits, g, dx)."""
    with torch.no_grad():
        x = x.detach().contiguous()
        feat, g = sgn_frames(x, wf, V)
        logits = sgn_clip(feat, wc, num_class)
        dfeat = sgn_clip_bwd(feat, wc, wc_t, cot.detach().to(logits).contiguous())
        return logits, g, sgn_frames_bwd(x, wf, wf_t, dfeat, V)


def sgn_composition_gradients(forward_tensor, x, cot, params=()):
    """The eval-mode gradients of sum(logits * cot) by torch autograd on a model's tensor-code composition
    ``forward_tensor(x)`` -> (logits, second output) -> (logits, second output, dx, one gradient or None per parameter
    of ``params``), all detached.  The second output is a tensor (base SGN's g) or SGN v15's dict of tensors, lists of
    tensors and None."""
    with torch.enable_grad():
        xg = x.detach().requires_grad_(True)
        logits, aux = forward_tensor(xg)
        grads = torch.autograd.grad((logits * cot.detach().to(logits)).sum(), [xg] + list(params), allow_unused=True)
    if isinstance(aux, dict):
        aux = {k: ([a.detach() for a in v] if isinstance(v, list) else None if v is None else v.detach())
               for k, v in aux.items()}
    else:
        aux = aux.detach()
    return logits.detach(), aux, grads[0], grads[1:]


def sgn_named_gradients(named, grads):
    """[(name, parameter)] and one gradient or None each -> {name: gradient}, zeros where autograd found no path."""
    return {n: (torch.zeros_like(p) if g is None else g) for (n, p), g in zip(named, grads)}


def sgn_fold_gradients(images, image_grads, named):
    """The gradients of the folded images ``images`` = (wf, wc), built in grad mode by the model's fold, taken through
    that fold to the trainable parameters ``named`` = [(name, parameter)] -> {name: gradient}.  An image none of whose
    parameters asks for a gradient (head-only fine-tuning) carries no graph and is skipped; a parameter without a path
    to the images gets zeros; nothing trainable gives {}."""
    params = [p for _, p in named]
    live = [(w, g) for w, g in zip(images, image_grads) if w.requires_grad]
    grads = (torch.autograd.grad([w for w, _ in live], params, [g for _, g in live], allow_unused=True)
             if live else (None,) * len(params))
    return sgn_named_gradients(named, grads)


def sgn_update_running_stats(model, stats, momentum=None, reset=True):
    """``recalibrate_bn`` of both models behind their ``batch_statistics``: ``stats`` {BatchNorm module name: (mean,
    biased var, count)} -> ``running_mean``, ``running_var`` (unbiased, n / (n - 1)) and ``num_batches_tracked`` updated in
    place exactly as one train-mode forward of the batch would.  ``momentum=None``: the cumulative average, a float: the
    exponential one.  ``reset`` calls ``reset_running_stats()`` first."""
    with torch.no_grad():
        for name, (mean, var, count) in stats.items():
            bn = model.get_submodule(name)
            if reset:
                bn.reset_running_stats()
            bn.num_batches_tracked.add_(1)
            f = 1.0 / float(bn.num_batches_tracked) if momentum is None else float(momentum)
            bn.running_mean.mul_(1.0 - f).add_(mean.to(bn.running_mean), alpha=f)
            bn.running_var.mul_(1.0 - f).add_(var.to(bn.running_var) * (count / (count - 1)), alpha=f)
    return stats


# ------------------------------------------------------------------------------------------------
# base SGN, batch statistics of its seven BatchNorms (csrc/sgn_stats.hip): the forward half of train-mode BatchNorm.
# BatchNorm k sees activations normalised by the batch statistics of the BatchNorms in front of it, so the statistics come
# from sequential passes, each the fused forward cut off at one BatchNorm, on a freshly folded image.
# ------------------------------------------------------------------------------------------------
# the BatchNorm modules of model/sgn.py::SGN in dependency order, and the (kind, layer) of the pass that measures each
SGN_BN_NAMES = ('joint_embed.cnn.0.bn', 'dif_embed.cnn.0.bn', 'gcn1.bn', 'gcn2.bn', 'gcn3.bn', 'cnn.bn1', 'cnn.bn2')
SGN_STATS_INPUT, SGN_STATS_FRAMES, SGN_STATS_CLIP = 0, 1, 2

# diagnostic counters of these launches (a dict of its own, like SGN_WGRAD_STATS)
SGN_BNSTATS_STATS = dict(input_stats=0, frames_stats=0, clip_stats=0, stats_finalize=0)

SGN_MAX_STATS_BYTES = 64 << 20


def _sgn_stats_part(kind, layer, N, seg, V, like):
    n = _L().agcn_sgn_stats_part_floats(kind, layer, N, seg, V)
    if n == 0:
        raise ValueError(f"agcn_amd: SGN batch statistics: pass {(kind, layer)} of {(N, seg, V)} is outside the kernels' domain")
    return _empty((n,), like)


def sgn_input_stats(x, V):
    """Per clip and feature the (sum, M2 about the clip's mean) of x and of dif over the seg frames: x (N, seg, V*3) ->
    part (N, 2, 2 * 3V), features [x | dif] each in [v*3 + c] order."""
    if x.dim() != 3 or x.shape[2] != 3 * V:
        raise ValueError(f"agcn_amd: sgn_input_stats takes (N, seg, {3 * V}), got {tuple(x.shape)}")
    N, seg, _ = x.shape
    part = _sgn_stats_part(SGN_STATS_INPUT, 0, N, seg, V, x)
    _lib.call("agcn_sgn_input_stats", x, part, part.numel(), N, seg, V)
    SGN_BNSTATS_STATS['input_stats'] += 1
    return part.view(N, 2, 6 * V)


def sgn_frames_stats(x, wimg, layer, V):
    """``sgn_frames`` cut off at gcn<layer>'s product, on an image whose gcn<layer> BatchNorm is folded as the identity ->
    part (N * seg, 2, C): per frame and channel the sum over the V joints and M2 about the frame's mean."""
    if x.dim() != 3 or x.shape[2] != 3 * V:
        raise ValueError(f"agcn_amd: sgn_frames_stats takes (N, seg, {3 * V}), got {tuple(x.shape)}")
    N, seg, _ = x.shape
    part = _sgn_stats_part(SGN_STATS_FRAMES, layer, N, seg, V, x)
    _lib.call("agcn_sgn_frames_stats", x, wimg, wimg.numel(), part, part.numel(), layer, N, seg, V)
    SGN_BNSTATS_STATS['frames_stats'] += 1
    return part.view(N * seg, 2, -1)


def sgn_clip_stats(feat, wimg, layer, num_class):
    """``sgn_clip`` cut off at cnn<layer>'s output, on an image whose bn<layer> is folded as the identity -> part
    (N * tiles, 2, C): per (clip, 32-frame tile) and channel the sum over the tile's valid frames and M2 about their mean."""
    if feat.dim() != 3 or feat.shape[2] != 256:
        raise ValueError(f"agcn_amd: sgn_clip_stats takes feat (N, seg, 256), got {tuple(feat.shape)}")
    N, seg, _ = feat.shape
    part = _sgn_stats_part(SGN_STATS_CLIP, layer, N, seg, 2, feat)
    _lib.call("agcn_sgn_clip_stats", feat, wimg, wimg.numel(), part, part.numel(), layer, N, seg, num_class)
    SGN_BNSTATS_STATS['clip_stats'] += 1
    return part.view(-1, 2, part.numel() // (2 * N * ((seg + 31) // 32)))


def _sgn_stats_finalize(entry, counters, C, part, kind, layer, N, seg, V, carry, want_carry):
    """``agcn_<entry>_finalize`` on ``part`` with its workspace, for both models."""
    if C == 0 or (carry is not None and (carry.dtype != torch.float64 or tuple(carry.shape) != (3, C)
                                         or not carry.is_contiguous() or carry.device != part.device)):
        raise ValueError(f"agcn_amd: {entry}_finalize: pass {(kind, layer)} takes a carry (3, {C}) float64")
    mean, var = _empty((C,), part), _empty((C,), part)
    out = torch.empty((3, C), dtype=torch.float64, device=part.device) if want_carry else None
    nbytes = getattr(_L(), f"agcn_{entry}_finalize_workspace")(kind, layer, N, seg, V)
    ws = torch.empty((max(1, nbytes // 8),), dtype=torch.float64, device=part.device)
    _lib.call(f"agcn_{entry}_finalize", part.view(-1), part.numel(), kind, layer, N, seg, V, carry, out, mean, var, ws,
              nbytes)
    counters['stats_finalize'] += 1
    return mean, var, out


def sgn_stats_finalize(part, kind, layer, N, seg, V, carry=None, want_carry=False):
    """Merge the groups of ``part`` (pairwise update, fp64 state: the groups of a clip in ascending index, then the clips
    in ascending index) on top of the optional ``carry`` ((3, C) float64: count, mean, M2) -> (mean (C,), biased var
    (C,), carry_out or None)."""
    return _sgn_stats_finalize('sgn_stats', SGN_BNSTATS_STATS, _L().agcn_sgn_stats_channels(kind, layer, V), part, kind,
                               layer, N, seg, V, carry, want_carry)


def sgn_stats_clip_bytes(seg, V):
    """Bytes of the largest partial buffer of a pass per clip (every partial buffer is linear in the clips)."""
    per = 4 * max(_L().agcn_sgn_stats_part_floats(k, l, 1, seg, V)
                  for k, l in ((SGN_STATS_INPUT, 0), (SGN_STATS_FRAMES, 3), (SGN_STATS_CLIP, 2)))
    if per == 0:
        raise ValueError(f"agcn_amd: SGN batch statistics: {(seg, V)} is outside the kernels' domain")
    return per


def sgn_stats_chunk(N, seg, V, max_part_bytes):
    """Clips per chunk: as many whole clips as keep every partial buffer under ``max_part_bytes``, at least one."""
    return max(1, min(N, int(max_part_bytes) // sgn_stats_clip_bytes(seg, V)))


def _sgn_stats_runner(N, seg, V, chunk):
    """-> run(kind, layer, src, launch, finalize): one pass over ``src`` (x or feat) in chunks of ``chunk`` whole clips,
    the finalize's carry state passing from chunk to chunk -> (mean, var).  Both models' passes."""
    def run(kind, layer, src, launch, finalize=sgn_stats_finalize):
        carry = None
        for n0 in range(0, N, chunk):
            part = launch(src[n0:n0 + chunk])
            n = min(chunk, N - n0)
            mean, var, carry = finalize(part, kind, layer, n, seg, V, carry, want_carry=n0 + chunk < N)
        return mean, var

    return run


def _sgn_stats_input_pass(run, x, V, names, known, out):
    """The pass of the two input BatchNorms ``names`` (position / joint, velocity / dif), the same in both models:
    ``out`` takes them in the kernels' feature order [v*3 + c], ``known`` in the module's c*V + v."""
    mean, var = run(SGN_STATS_INPUT, 0, x, lambda xs: sgn_input_stats(xs, V))
    for i, name in enumerate(names):
        out[name] = (mean[i * 3 * V:(i + 1) * 3 * V], var[i * 3 * V:(i + 1) * 3 * V])
        known[name] = tuple(t.view(V, 3).t().reshape(-1) for t in out[name])


def sgn_batch_statistics(x, fold, V, num_class, max_part_bytes=SGN_MAX_STATS_BYTES):
    """The batch statistics of SGN's seven BatchNorms on x (N, seg, V*3) as ONE batch, and the forward under them ->
    (logits, g, {name: (mean, biased var)}) with the names of ``SGN_BN_NAMES``; the two input BatchNorms in the kernels'
    feature order [v*3 + c].  ``fold(known, identity)`` -> (frames image, clip image): the caller's fold with the
    BatchNorms in the dict ``known`` {name: (mean, var)} on those statistics and the BatchNorm ``identity`` (a name or
    None) as scale 1, shift 0 (model/sgn.py::SGN._batch_images or the incremental ``_batch_folder``, the same bits);
    ``known`` only grows between calls and holds the two input BatchNorms in their module's order c*V + v.  Seven passes in dependency order, each chunked by whole clips under ``max_part_bytes`` with the
    finalize's carry state, so the chunking does not change a bit; then the existing full-depth launches on the final
    images."""
    if x.dim() != 3 or x.shape[2] != 3 * V:
        raise ValueError(f"agcn_amd: sgn_batch_statistics takes (N, seg, {3 * V}), got {tuple(x.shape)}")
    x = x.detach().contiguous()
    N, seg, _ = x.shape
    run = _sgn_stats_runner(N, seg, V, sgn_stats_chunk(N, seg, V, max_part_bytes))
    known, out = {}, {}
    _sgn_stats_input_pass(run, x, V, SGN_BN_NAMES[:2], known, out)
    for layer in (1, 2, 3):
        name = SGN_BN_NAMES[1 + layer]
        wf, _ = fold(known, name)
        known[name] = out[name] = run(SGN_STATS_FRAMES, layer, x, lambda xs: sgn_frames_stats(xs, wf, layer, V))
    wf, _ = fold(known, None)
    feat, g = sgn_frames(x, wf, V)
    for layer in (1, 2):
        name = SGN_BN_NAMES[4 + layer]
        _, wc = fold(known, name)
        known[name] = out[name] = run(SGN_STATS_CLIP, layer, feat, lambda fs: sgn_clip_stats(fs, wc, layer, num_class))
    _, wc = fold(known, None)
    return sgn_clip(feat, wc, num_class), g, out


# ------------------------------------------------------------------------------------------------
# SGN v15, the attention SGN: eval-mode inference (csrc/sgn_v15.hip; layouts in csrc/sgn_v15_plan.h)
# ------------------------------------------------------------------------------------------------
# diagnostic counters of the two launches (a dict of its own: SGN_STATS is compared whole by its tests)
SGN15_STATS = dict(frames_hip=0, clip_hip=0)
# clips per pair of launches: a larger batch goes through in chunks of whole clips (model/sgn_v15.py), with the same bits
# (a clip's result does not depend on its batch).  At seg <= 32 this stays inside the entries' limits (about 2M frames
# for agcn_sgn15_frames, 524 287 clips for agcn_sgn15_clip: csrc/sgn_v15_plan.h).
SGN15_MAX_CLIPS = 1 << 15


def sgn15_weights_floats(V, seg, num_class, spatial, temporal):
    """(floats of the frames image, of the clip image) for the blocks ``spatial`` / ``temporal`` = (heads, d_head, ff),
    or None outside the kernels' domain (csrc/sgn_v15_plan.h)."""
    nf = _L().agcn_sgn15_frames_weights(V, *spatial)
    nc = _L().agcn_sgn15_clip_weights(seg, num_class, *temporal)
    return (nf, nc) if nf and nc else None


def sgn15_image_sections(V, seg, num_class, spatial, temporal):
    """The sections of the two folded weight images of SGN v15 in their order (csrc/sgn_v15_plan.h) -> (frames, clip),
    each a list of (name, offset, shape).  ``spatial`` / ``temporal``: (heads, d_head, ff) of the two blocks.  A block
    (din -> dout) is qkv_w (din, 3 inner) = [Wq d_head^-1/2 | Wk | Wv] with the attention BatchNorm folded, qkv_b, o_w
    (inner, din), o_b, f1_w (din, ff) with the feed-forward BatchNorm folded, f1_b, f2_w = [W2 ; Wr] (ff + din, dout),
    f2_b = b2 + br."""
    def block(p, din, dout, heads, d_head, ff):
        inner = heads * d_head
        return [(p + 'qkv_w', (din, 3 * inner)), (p + 'qkv_b', (3 * inner,)), (p + 'o_w', (inner, din)), (p + 'o_b', (din,)),
                (p + 'f1_w', (din, ff)), (p + 'f1_b', (ff,)), (p + 'f2_w', (ff + din, dout)), (p + 'f2_b', (dout,))]

    frames = _sgn_layout([('aff', (4, V, 3))] + _sgn_emb_sections('pe') + _sgn_emb_sections('ve') + [('spa', (V, 64))]
                         + block('s_', 128, 256, *spatial))
    clip = _sgn_layout([('tem', (seg, 256))] + block('t_', 256, 512, *temporal)
                       + [('fc_w', (512, num_class)), ('fc_b', (num_class,))])
    return frames, clip


def sgn15_frames(x, wimg, V, heads, d_head, ff, want_attn=False):
    """The joint-level module of SGN v15 on x (N, seg, V*3) with the folded frames image -> (feat (N, seg, 256), the
    maximum over the joints of the spatial block's output WITHOUT tem_emb (``sgn15_clip`` adds it), attn (N*seg, heads,
    V, V) or None)."""
    if x.dim() != 3 or x.shape[2] != 3 * V:
        raise ValueError(f"agcn_amd: sgn15_frames takes (N, seg, {3 * V}), got {tuple(x.shape)}")
    N, seg, _ = x.shape
    feat = _empty((N, seg, 256), x)
    attn = _empty((N * seg, heads, V, V), x) if want_attn else None
    _lib.call("agcn_sgn15_frames", x, wimg, wimg.numel(), feat, attn, N, seg, V, heads, d_head, ff)
    SGN15_STATS['frames_hip'] += 1
    return feat, attn


def sgn15_clip(feat, wimg, num_class, heads, d_head, ff, want_attn=False):
    """The frame-level module and the classifier of SGN v15 on feat (N, seg, 256) -> (logits (N, num_class), attn (N,
    heads, seg, seg) or None)."""
    if feat.dim() != 3 or feat.shape[2] != 256:
        raise ValueError(f"agcn_amd: sgn15_clip takes (N, seg, 256), got {tuple(feat.shape)}")
    N, seg, _ = feat.shape
    logits = _empty((N, num_class), feat)
    attn = _empty((N, heads, seg, seg), feat) if want_attn else None
    _lib.call("agcn_sgn15_clip", feat, wimg, wimg.numel(), logits, attn, N, seg, num_class, heads, d_head, ff)
    SGN15_STATS['clip_hip'] += 1
    return logits, attn


# diagnostic counters of the input-gradient launches (again a dict of its own: SGN15_STATS is compared whole)
SGN15_BWD_STATS = dict(clip_bwd=0, frames_bwd=0)


def sgn15_bwd_weights_floats(V, seg, num_class, spatial, temporal):
    """(floats of the transposed frames image, of the transposed clip image), or None outside the kernels' domain
    (csrc/sgn_v15_bwd_plan.h)."""
    nf = _L().agcn_sgn15_frames_bwd_weights(V, *spatial)
    nc = _L().agcn_sgn15_clip_bwd_weights(seg, num_class, *temporal)
    return (nf, nc) if nf and nc else None


def sgn15_bwd_image_sections(spatial, temporal):
    """The sections of the two TRANSPOSED weight images of the SGN v15 input gradient in their order
    (csrc/sgn_v15_bwd_plan.h: Sgn15FramesWT, Sgn15ClipWT) -> (frames, clip), each a list of (name, offset, shape, source):
    the section is the transpose of section ``source`` of the forward image (``sgn15_image_sections``)."""
    def lay(items):
        return [(src + '_t', o, shape, src) for src, o, shape in _sgn_layout(items)]

    def block(p, din, dout, heads, d_head, ff):
        inner = heads * d_head
        return [(p + 'qkv_w', (3 * inner, din)), (p + 'o_w', (din, inner)), (p + 'f1_w', (ff, din)),
                (p + 'f2_w', (dout, ff + din))]

    return (lay([('pe2_w', (64, 64)), ('ve2_w', (64, 64))] + block('s_', 128, 256, *spatial)),
            lay(block('t_', 256, 512, *temporal)))


def sgn15_transpose_images(wf, wc, V, seg, num_class, spatial, temporal):
    """The two transposed images from the two forward images."""
    out = []
    for img, fwd, bwd in zip((wf, wc), sgn15_image_sections(V, seg, num_class, spatial, temporal),
                             sgn15_bwd_image_sections(spatial, temporal)):
        at = {n: (o, s) for n, o, s in fwd}
        out.append(torch.cat([img[at[src][0]:at[src][0] + math.prod(at[src][1])].view(at[src][1]).t().reshape(-1)
                              for _, _, _, src in bwd]))
    return tuple(out)


def sgn15_clip_bwd(feat, wimg, wimg_t, dlogits, heads, d_head, ff):
    """d logits (N, num_class) -> d feat (N, seg, 256) through fc, the maximum over the frames and the temporal block of
    SGN v15, recomputed from feat (N, seg, 256) as ``sgn15_frames`` returns it.  wimg: the forward clip image, wimg_t: the
    transposed one."""
    return _sgn_clip_bwd(_SGN15, feat, wimg, wimg_t, dlogits, (heads, d_head, ff), tape=False)


def sgn15_frames_bwd(x, wimg, wimg_t, dfeat, V, heads, d_head, ff):
    """d feat (N, seg, 256) -> dx (N, seg, V*3) through the maximum over the joints, the spatial block and the input side
    of SGN v15, recomputed from x, and the velocity's coupling between the frames of a clip."""
    return _sgn_frames_bwd(_SGN15, x, wimg, wimg_t, dfeat, V, (heads, d_head, ff), tape=False)


def sgn15_forward_ref(x, wf, wc, V, seg, num_class, spatial, temporal):
    """The tensor-code form of the fused SGN v15 forward, reading ONLY the two flat folded images: the CPU-checkable
    specification of the fold and the layout.  x (N, seg, V*3) -> (logits, feat (N, seg, 256) as ``sgn15_frames`` returns
    it, spatial attn (N*seg, heads, V, V), temporal attn (N, heads, seg, seg))."""
    f, c = _sgn_ref_views("sgn15_forward_ref", "csrc/sgn_v15_plan.h", x, wf, wc, V, seg,
                          sgn15_image_sections(V, seg, num_class, spatial, temporal))
    N = x.shape[0]

    def block(t, w, p, heads, d_head):
        """t (B, R, din)"""
        B, R, _ = t.shape
        q, k, v = ((t @ w[p + 'qkv_w'] + w[p + 'qkv_b']).reshape(B, R, 3, heads, d_head).permute(2, 0, 3, 1, 4))
        a = torch.softmax(q @ k.transpose(-1, -2), dim=-1)                       # d_head^-1/2 is folded into q
        t1 = (a @ v).transpose(1, 2).reshape(B, R, heads * d_head) @ w[p + 'o_w'] + w[p + 'o_b'] + t
        hid = torch.relu(t1 @ w[p + 'f1_w'] + w[p + 'f1_b'])
        return torch.cat([hid, t1], dim=2) @ w[p + 'f2_w'] + w[p + 'f2_b'], a

    h = torch.cat([_sgn_ref_input(x, f, V, seg, 'pe', 've'), f['spa'].expand(N, seg, V, 64)], dim=3)
    y, sa = block(h.reshape(N * seg, V, 128), f, 's_', spatial[0], spatial[1])
    feat = y.reshape(N, seg, V, 256).amax(2)
    z, ta = block(feat + c['tem'], c, 't_', temporal[0], temporal[1])
    return z.amax(1) @ c['fc_w'] + c['fc_b'], feat, sa, ta


# ------------------------------------------------------------------------------------------------
# SGN v15, parameter gradients in eval mode (the taping backward of csrc/sgn_v15_bwd.hip and the reductions of
# csrc/sgn_v15_wgrad.hip): frozen-BatchNorm fine-tuning.  The kernels give the gradient with respect to the two folded
# weight images, in the images' layout; torch autograd takes it through the fold (model/sgn_v15.py::SGN._folded) to the
# parameters.  ``spatial`` / ``temporal`` are (heads, d_head, ff) of the two blocks.
# ------------------------------------------------------------------------------------------------
# diagnostic counters of these launches (a dict of its own, like SGN_WGRAD_STATS)
SGN15_WGRAD_STATS = dict(clip_bwd_tape=0, frames_bwd_tape=0, frames_wgrad=0, clip_wgrad=0)
# None, or a callable(label) that tools/sgn_v15_finetune.py sets to record a device event behind the taping launches
# ('tape') and behind the reductions ('reduce') of every chunk
SGN15_WGRAD_MARK = None
_SGN15 = _SgnFamily('sgn15', 'SGN v15', SGN15_BWD_STATS, SGN15_WGRAD_STATS)


def sgn15_clip_bwd_tape(feat, wimg, wimg_t, dlogits, heads, d_head, ff):
    """``sgn15_clip_bwd`` (the same dfeat bits) that also writes the clip tape (csrc/sgn_v15_wgrad_plan.h: Sgn15ClipTape)
    -> (dfeat, tape)."""
    return _sgn_clip_bwd(_SGN15, feat, wimg, wimg_t, dlogits, (heads, d_head, ff), tape=True)


def sgn15_frames_bwd_tape(x, wimg, wimg_t, dfeat, V, heads, d_head, ff):
    """``sgn15_frames_bwd`` (the same dx bits) that also writes the frames tape (Sgn15FramesTape) -> (dx, tape)."""
    return _sgn_frames_bwd(_SGN15, x, wimg, wimg_t, dfeat, V, (heads, d_head, ff), tape=True)


def sgn15_frames_wgrad(x, wimg, tape, V, heads, d_head, ff, rows_per_split=0):
    """x and the frames tape -> the gradient of the frames image ``wimg``, in its layout."""
    N, seg, _ = x.shape
    if x.shape[2] != 3 * V or tape.numel() < _L().agcn_sgn15_frames_tape_floats(N, seg, V, heads, d_head, ff):
        raise ValueError(f"agcn_amd: sgn15_frames_wgrad: a tape of {tape.numel()} floats is not the tape of {tuple(x.shape)}")
    ws = _sgn_wgrad_ws(_SGN15, (N, seg, V, 0, heads, d_head, ff), rows_per_split, x)
    d_w = _empty((wimg.numel(),), x)
    _lib.call("agcn_sgn15_frames_wgrad", x, tape, tape.numel(), d_w, d_w.numel(), ws, ws.numel() * 4, N, seg, V, heads,
              d_head, ff, rows_per_split)
    SGN15_WGRAD_STATS['frames_wgrad'] += 1
    return d_w


def sgn15_clip_wgrad(tape, dlogits, wimg, seg, heads, d_head, ff, rows_per_split=0):
    """The clip tape and dlogits (N, num_class) -> the gradient of the clip image ``wimg``, in its layout."""
    N, nc = dlogits.shape
    if tape.numel() < _L().agcn_sgn15_clip_tape_floats(N, seg, nc, heads, d_head, ff):
        raise ValueError(f"agcn_amd: sgn15_clip_wgrad: a tape of {tape.numel()} floats is not the tape of {(N, seg, nc)}")
    ws = _sgn_wgrad_ws(_SGN15, (N, seg, 0, nc, heads, d_head, ff), rows_per_split, dlogits)
    d_w = _empty((wimg.numel(),), dlogits)
    _lib.call("agcn_sgn15_clip_wgrad", tape, tape.numel(), dlogits, d_w, d_w.numel(), ws, ws.numel() * 4, N, seg, nc, heads,
              d_head, ff, rows_per_split)
    SGN15_WGRAD_STATS['clip_wgrad'] += 1
    return d_w


def sgn15_tape_chunk(N, seg, V, num_class, spatial, temporal, max_tape_bytes):
    """Clips per chunk: as many whole clips as fit ``max_tape_bytes`` of tape (both tapes are linear in the clips), at
    least one and at most ``SGN15_MAX_CLIPS``."""
    return _sgn_tape_chunk(_SGN15, (seg, V, num_class, spatial, temporal), N,
                           _L().agcn_sgn15_frames_tape_floats(1, seg, V, *spatial),
                           _L().agcn_sgn15_clip_tape_floats(1, seg, num_class, *temporal), max_tape_bytes, SGN15_MAX_CLIPS)


def _sgn15_image_backward(x, feat, wf, wc, wf_t, wc_t, dlogits, V, spatial, temporal, rows_per_split, max_tape_bytes):
    """-> (dx, d_wf, d_wc) of SGN v15, chunked under ``max_tape_bytes`` of tape and ``SGN15_MAX_CLIPS``."""
    seg = x.shape[1]

    def step(xs, fe, dl):
        dfeat, ctape = sgn15_clip_bwd_tape(fe, wc, wc_t, dl, *temporal)
        dx, ftape = sgn15_frames_bwd_tape(xs, wf, wf_t, dfeat, V, *spatial)
        if SGN15_WGRAD_MARK:
            SGN15_WGRAD_MARK('tape')
        gf = sgn15_frames_wgrad(xs, wf, ftape, V, *spatial, rows_per_split=rows_per_split)
        gc = sgn15_clip_wgrad(ctape, dl, wc, seg, *temporal, rows_per_split=rows_per_split)
        if SGN15_WGRAD_MARK:
            SGN15_WGRAD_MARK('reduce')
        return dx, gf, gc

    chunk = sgn15_tape_chunk(x.shape[0], seg, V, dlogits.shape[1], spatial, temporal, max_tape_bytes)
    return _sgn_chunked_backward(step, chunk, x, feat, dlogits)


def sgn15_fused_forward(x, wf, wc, V, num_class, spatial, temporal, want_attn=False):
    """The two forward launches per chunk of at most ``SGN15_MAX_CLIPS`` whole clips (a clip's result does not depend on
    its batch) -> (logits, feat, spatial attn or None, temporal attn or None).  ``wc`` may be a callable(feat) -> clip
    image, for an image that depends on feat of the whole batch (``sgn15_batch_statistics``): then every frames launch
    runs before the first clip launch."""
    parts = []
    if callable(wc):
        fs = [sgn15_frames(x[lo:lo + SGN15_MAX_CLIPS], wf, V, *spatial, want_attn=want_attn)
              for lo in range(0, x.shape[0], SGN15_MAX_CLIPS)]
        wc = wc(fs[0][0] if len(fs) == 1 else torch.cat([f for f, _ in fs]))
        for feat, sa in fs:
            logits, ta = sgn15_clip(feat, wc, num_class, *temporal, want_attn=want_attn)
            parts.append((logits, feat, sa, ta))
    else:
        for lo in range(0, x.shape[0], SGN15_MAX_CLIPS):      # one pair of launches unless the batch exceeds their limit
            feat, sa = sgn15_frames(x[lo:lo + SGN15_MAX_CLIPS], wf, V, *spatial, want_attn=want_attn)
            logits, ta = sgn15_clip(feat, wc, num_class, *temporal, want_attn=want_attn)
            parts.append((logits, feat, sa, ta))
    return parts[0] if len(parts) == 1 else tuple(None if p[0] is None else torch.cat(p) for p in zip(*parts))


def sgn15_input_gradient(x, wf, wc, wf_t, wc_t, cot, V, num_class, spatial, temporal, want_attn=False):
    """The fused eval forward of SGN v15 and dx = d sum(logits * cot) / dx, the two backward launches over the forward's
    chunks of clips -> (logits, spatial attn or None, temporal attn or None, dx)."""
    with torch.no_grad():
        x = x.detach()
        cot = cot.detach().to(x).contiguous()
        logits, feat, sa, ta = sgn15_fused_forward(x, wf, wc, V, num_class, spatial, temporal, want_attn)
        dxs = []
        for lo in range(0, x.shape[0], SGN15_MAX_CLIPS):
            hi = lo + SGN15_MAX_CLIPS
            dfeat = sgn15_clip_bwd(feat[lo:hi], wc, wc_t, cot[lo:hi], *temporal)
            dxs.append(sgn15_frames_bwd(x[lo:hi], wf, wf_t, dfeat, V, *spatial))
        return logits, sa, ta, dxs[0] if len(dxs) == 1 else torch.cat(dxs)


def sgn15_image_gradients(x, wf, wc, wf_t, wc_t, cot, V, num_class, spatial, temporal, rows_per_split=0,
                          max_tape_bytes=SGN_MAX_TAPE_BYTES):
    """The fused eval forward of SGN v15 and the gradient of sum(logits * cot) with respect to x and to the two folded
    images -> (logits, dx, d_wf, d_wc); d_wf / d_wc have the layout of wf / wc.  The batch goes through in chunks of
    whole clips under both ``max_tape_bytes`` of tape and ``SGN15_MAX_CLIPS``."""
    with torch.no_grad():
        x = x.detach().contiguous()
        logits, feat, _, _ = sgn15_fused_forward(x, wf, wc, V, num_class, spatial, temporal)
        cot = cot.detach().to(logits).contiguous()
        if tuple(cot.shape) != tuple(logits.shape):
            raise ValueError(f"agcn_amd: sgn15_image_gradients takes cot {tuple(logits.shape)}, got {tuple(cot.shape)}")
        return (logits,) + _sgn15_image_backward(x, feat, wf, wc, wf_t, wc_t, cot, V, spatial, temporal, rows_per_split,
                                                 max_tape_bytes)


class SGN15FineTuneFunction(torch.autograd.Function):
    """SGN v15's eval forward as the two fused launches, differentiable with respect to x and the two folded weight
    images (built in grad mode by model/sgn_v15.py, so autograd continues through the fold to the parameters).  args: x,
    wf, wc, wf_t, wc_t, V, num_class, spatial, temporal -> logits.  A CPU tensor runs ``sgn15_forward_ref``."""

    @staticmethod
    def forward(ctx, x, wf, wc, wf_t, wc_t, V, num_class, spatial, temporal):
        ctx.geometry = (V, spatial, temporal)
        if not x.is_cuda:
            return _sgn_finetune_ref(
                ctx, lambda *leaves: sgn15_forward_ref(*leaves, V, x.shape[1], num_class, spatial, temporal), x, wf, wc)[0]
        x = x.contiguous()
        logits, feat, _, _ = sgn15_fused_forward(x, wf.detach(), wc.detach(), V, num_class, spatial, temporal)
        ctx.ref = None
        ctx.save_for_backward(x, feat, wf, wc, wf_t, wc_t)
        return logits

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dlogits):
        return _sgn_finetune_backward(ctx, _sgn15_image_backward, dlogits) + (None,) * 6


# ------------------------------------------------------------------------------------------------
# SGN v15, batch statistics of its six BatchNorms (csrc/sgn_v15_stats.hip; the two input ones through the base SGN's input
# pass): the forward half of train-mode BatchNorm, as sequential passes, each the fused forward cut off at one BatchNorm.
# A pass never reads a section that depends on the BatchNorm it measures, so its images only need the EARLIER BatchNorms
# on their batch statistics (csrc/sgn_v15_stats_plan.h).
# ------------------------------------------------------------------------------------------------
# the BatchNorm modules of model/sgn_v15.py::SGN in dependency order: the two DataNorms, then n_a and n_f of each block
SGN15_BN_NAMES = ('feature_extractor.pos_embed.norm.bn', 'feature_extractor.vel_embed.norm.bn',
                  'spatial_mha.transformer.layers.l1.attn.norm.fn', 'spatial_mha.transformer.layers.l1.ffn.norm.fn',
                  'temporal_mha.transformer.layers.l1.attn.norm.fn', 'temporal_mha.transformer.layers.l1.ffn.norm.fn')
SGN15_STATS_FRAMES, SGN15_STATS_CLIP = 1, 2

# diagnostic counters of these launches (a dict of its own; the input pass counts in SGN_BNSTATS_STATS)
SGN15_BNSTATS_STATS = dict(frames_stats=0, clip_stats=0, stats_finalize=0)
# None, or a callable(label) that tools/sgn_v15_recalibrate.py sets to record a device event behind every pass and fold
SGN15_BNSTATS_MARK = None


def _sgn15_stats_part(kind, layer, N, seg, V, like):
    n = _L().agcn_sgn15_stats_part_floats(kind, layer, N, seg, V)
    if n == 0:
        raise ValueError(f"agcn_amd: SGN v15 batch statistics: pass {(kind, layer)} of {(N, seg, V)} is outside the kernels' domain")
    return _empty((n,), like)


def sgn15_frames_stats(x, wimg, layer, V, heads, d_head, ff):
    """``sgn15_frames`` cut off at the token tile [pos + vel | spa] (layer 1: the spatial block's n_a) or behind the
    attention half of the block (layer 2: n_f, on x1) -> part (N * seg, 2, 128): per frame and channel the sum over the V
    joints and M2 about the frame's mean."""
    if x.dim() != 3 or x.shape[2] != 3 * V:
        raise ValueError(f"agcn_amd: sgn15_frames_stats takes (N, seg, {3 * V}), got {tuple(x.shape)}")
    N, seg, _ = x.shape
    part = _sgn15_stats_part(SGN15_STATS_FRAMES, layer, N, seg, V, x)
    _lib.call("agcn_sgn15_frames_stats", x, wimg, wimg.numel(), part, part.numel(), layer, N, seg, V, heads, d_head, ff)
    SGN15_BNSTATS_STATS['frames_stats'] += 1
    return part.view(N * seg, 2, 128)


def sgn15_clip_stats(feat, wimg, layer, num_class, heads, d_head, ff):
    """``sgn15_clip`` cut off behind its load of feat + tem (layer 1: the temporal block's n_a) or behind the attention
    half of the block (layer 2: n_f) -> part (N, 2, 256): per clip and channel the sum over the seg frames and M2 about
    the clip's mean."""
    if feat.dim() != 3 or feat.shape[2] != 256:
        raise ValueError(f"agcn_amd: sgn15_clip_stats takes feat (N, seg, 256), got {tuple(feat.shape)}")
    N, seg, _ = feat.shape
    part = _sgn15_stats_part(SGN15_STATS_CLIP, layer, N, seg, 2, feat)
    _lib.call("agcn_sgn15_clip_stats", feat, wimg, wimg.numel(), part, part.numel(), layer, N, seg, num_class, heads, d_head,
              ff)
    SGN15_BNSTATS_STATS['clip_stats'] += 1
    return part.view(N, 2, 256)


def sgn15_stats_finalize(part, kind, layer, N, seg, V, carry=None, want_carry=False):
    """``sgn_stats_finalize`` for a pass of SGN v15: the same merge order and carry state."""
    return _sgn_stats_finalize('sgn15_stats', SGN15_BNSTATS_STATS, _L().agcn_sgn15_stats_channels(kind, layer), part, kind,
                               layer, N, seg, V, carry, want_carry)


def sgn15_stats_clip_bytes(seg, V):
    """Bytes of the largest partial buffer of a pass per clip (every partial buffer is linear in the clips)."""
    floats = (_L().agcn_sgn_stats_part_floats(SGN_STATS_INPUT, 0, 1, seg, V),
              _L().agcn_sgn15_stats_part_floats(SGN15_STATS_FRAMES, 1, 1, seg, V),
              _L().agcn_sgn15_stats_part_floats(SGN15_STATS_CLIP, 1, 1, seg, V))
    if min(floats) == 0:
        raise ValueError(f"agcn_amd: SGN v15 batch statistics: {(seg, V)} is outside the kernels' domain")
    return 4 * max(floats)


def sgn15_stats_chunk(N, seg, V, max_part_bytes):
    """Clips per chunk: as many whole clips as keep every partial buffer under ``max_part_bytes``, at least one and at
    most ``SGN15_MAX_CLIPS``."""
    return max(1, min(N, SGN15_MAX_CLIPS, int(max_part_bytes) // sgn15_stats_clip_bytes(seg, V)))


def sgn15_batch_statistics(x, fold, V, num_class, spatial, temporal, max_part_bytes=SGN_MAX_STATS_BYTES):
    """The batch statistics of SGN v15's six BatchNorms on x (N, seg, V*3) as ONE batch, and the forward under them ->
    (logits, {name: (mean, biased var)}) with the names of ``SGN15_BN_NAMES``; the two input BatchNorms in the kernels'
    feature order [v*3 + c].  ``fold(known)`` -> (frames image, clip image): the caller's fold with the BatchNorms in the
    dict ``known`` {name: (mean, var)} on those statistics (model/sgn_v15.py::SGN._batch_images or the incremental
    ``_batch_folder``, the same bits in the sections a pass reads); ``known`` only grows between calls and holds the two
    input BatchNorms in their module's order c*V + v.  The input pass (the base SGN's), the two passes of the spatial
    block, the full-depth frames launch, the two passes of the temporal block and the full-depth clip launch, each pass
    chunked by whole clips under ``max_part_bytes`` and ``SGN15_MAX_CLIPS`` with the finalize's carry state, so the
    chunking does not change a bit."""
    if x.dim() != 3 or x.shape[2] != 3 * V:
        raise ValueError(f"agcn_amd: sgn15_batch_statistics takes (N, seg, {3 * V}), got {tuple(x.shape)}")
    x = x.detach().contiguous()
    N, seg, _ = x.shape
    run = _sgn_stats_runner(N, seg, V, sgn15_stats_chunk(N, seg, V, max_part_bytes))
    mark = SGN15_BNSTATS_MARK or (lambda label: None)
    known, out = {}, {}
    mark('start')
    _sgn_stats_input_pass(run, x, V, SGN15_BN_NAMES[:2], known, out)
    mark('input')

    def block(kind, names, which, src, launch):
        for layer, name in zip((1, 2), names):
            img = fold(known)[which]
            mark('fold')
            known[name] = out[name] = run(kind, layer, src, lambda s: launch(s, img, layer), sgn15_stats_finalize)
            mark(f"{'frames' if which == 0 else 'clip'}{layer}")

    block(SGN15_STATS_FRAMES, SGN15_BN_NAMES[2:4], 0, x, lambda xs, wf, layer: sgn15_frames_stats(xs, wf, layer, V, *spatial))

    def clip_image(feat):
        mark('frames_full')
        block(SGN15_STATS_CLIP, SGN15_BN_NAMES[4:6], 1, feat,
              lambda fs, wc, layer: sgn15_clip_stats(fs, wc, layer, num_class, *temporal))
        wc = fold(known)[1]
        mark('fold')
        return wc

    wf = fold(known)[0]
    mark('fold')
    logits = sgn15_fused_forward(x, wf, clip_image, V, num_class, spatial, temporal)[0]
    mark('clip_full')
    return logits, out
