"""Shared by tests/test_gcn_width_cpu.py and tests/test_gpu_gcn_width.py: the table of channel widths that walks the routing
of unit_gcn's aggregate+project kernels (csrc/conv_gemm.hip, gcn_chain.hip, wgrad_chain.hip, conv_wgrad.hip) and of the
two-kernel adjacency path (csrc/adjacency.hip), a seeded recipe for their operands (no model, no fixture), the fp64
reference, its mutants, the per-channel metric, and a model of the routing in the default arithmetic mode and under
AGCN_GEMM=f32, which the GPU test holds against ``agcn_last_kernel()``.

Which case of ``CASES`` (C, Cout, T, V) reaches which cell (N = 2 everywhere).  K is the streamed width and M the row
count of a contraction: forward K = C, M = Cout; backward-data K = Cout, M = C, fused term K2 = 6 * (Cout // 4).
ws<TM, KCB, NCB2> is gcn_ws_kernel (TM 32-row tiles per block, KCB = 4: the K128 form, NCB2 plain stages), chainB is
gcn_chain_kernel at B-row blocks, f32 the exact conv_gemm_kernel.  dadj: `one` = exact kernel in one launch, `3x` = one
launch per subset, dchain<TM> gpc g = gcn_dadj_chain_kernel, `refused` = AGCN_ERR_UNSUPPORTED.  wgrad: pc / wc = the
producer-consumer / single-role kernel of wgrad_chain.hip, ex2 / ex4 = conv_wgrad_kernel at 64 / 128 rows.

   0 (1, 1, 1, 15)      one channel, one frame: fwd f32; bwd chain32; no fused term (K2 = 0); dadj one; wgrad ex2
   1 (2, 48, 7, 20)     fwd f32; bwd K = 48 -> ws<1,2,0>; fused K2 = 72 -> ws<1,2,3>; dadj one; wgrad ex2
   2 (3, 100, 9, 25)    fwd f32; bwd K = 100, M = 3: chain32 (the K128 form needs M > 32); dadj one; wgrad wc (C <= 32)
   3 (21, 24, 17, 25)   dadj one (3C = 63 <= 64), two frame tiles of the exact kernel; bwd K = 24: chain32
   4 (22, 24, 17, 32)   dadj 3x (3C = 66), three frame tiles at V = 32; bwd chain32; fused K2 = 36 (two ragged stages)
   5 (24, 24, 5, 18)    the v24 width: K2 = 36; dadj 3x
   6 (31, 33, 6, 25)    fwd f32 (C = 31); bwd K = 33, M = 31: ws<1,2,0>; fused K2 = 48: ws<1,2,2>
   7 (33, 31, 3, 20)    fwd K = 33, M = 31: ws<1,2,0>; bwd K = 31, M = 33: chain64; infer supported from here on
   8 (32, 40, 9, 18)    fwd K = 32: chain64 with M = 40 ragged; bwd K = 40, M = 32: ws<1,2,0>; fused K2 = 60: ws<1,2,2>
   9 (48, 72, 7, 25)    fwd ws<2,2,0>; bwd K = 72, M = 48: ws<2,4,0>; fused: chain64; infer with x2 (32): ws<2,2,1>
  10 (63, 65, 5, 15)    fwd K = 63 ws<2,2,0>; bwd K = 65 ws<2,4,0>; dadj 3x at its widest; wgrad ex2 (C = 63)
  11 (64, 60, 6, 25)    fwd K = 64 ws<2,2,0>; bwd K = 60 ws<2,2,0>; fused K2 = 90: ws<2,2,3>; dchain<2> gpc 1, Cout % 8 = 4
  12 (64, 100, 3, 18)   bwd K = 100: ws<2,4,0>; fused: chain64; dchain<2> Cout % 8 = 4 over four stages; wgrad pc
  13 (128, 129, 9, 20)  fwd K = 128, M = 129: ws<2,4,0>; bwd K = 129, M = 128: chain128; dchain<4> gpc 1, Cout % 8 = 1
  14 (64, 4, 7, 32)     fwd M = 4: ws<1,2,0>; bwd K = 4: chain64; dchain<2> with Cout < 8; wgrad ex2
  15 (65, 64, 5, 25)    fwd K = 65: ws<2,4,0>; bwd K = 64, M = 65: ws<2,2,0>; fused K2 = 96: ws<2,2,3>; dadj refused
  16 (80, 96, 1, 18)    one frame; fwd / bwd ws<2,4,0>; fused: chain64; dadj refused; wgrad ex2 (C = 80)
  17 (96, 160, 6, 15)   fwd K = 96 ws<2,4,0>; bwd K = 160, M = 96: chain64; dadj refused
  18 (192, 200, 3, 25)  fwd / bwd chain64 (K > 128); dchain<2> gpc 3; wgrad pc at 64 channels x two row blocks
  19 (256, 24, 5, 20)   fwd M = 24: chain32; bwd K = 24, M = 256: chain128; dchain<4> gpc 2 with a narrow output; wgrad ex2
  20 (320, 64, 3, 18)   fwd chain64; bwd K = 64 ws<2,2,0>; fused K2 = 96 ws<2,2,3>; dchain<2> gpc 5; wgrad wc
  21 (40, 128, 7, 25)   fwd ws<2,2,0>; bwd K = 128, M = 40: ws<2,4,0>; wgrad ex4 (Cout % 128 = 0 off the chain); dadj 3x

The operands are rounded to fp32 before the reference is taken, so a kernel answers for its own arithmetic only.
What makes these inputs able to show an error is asserted in tests/test_gcn_width_cpu.py."""
import math

import torch

N = 2
BAR = 1e-4                   # tests/test_gpu_kernels.py: TOL, here per output channel
STATS_FACTOR = 10            # the BatchNorm partials (test_gpu_kernels.py)
DB_BAR = 2e-3                # the adjacency db sums (test_gpu_kernels.py)
DTP_BAR = 2e-4               # dtp against its own maximum (test_gpu_kernels.py: stricter than max(1, .) on these values)
CAUGHT = 100 * BAR           # a mutant counts as caught when the metric shows it two decades above the bar
CAUGHT_SHARE = 1.0           # of the (case, mutant) pairs at which the mutant applies
MIN_CHANNEL_SHARE = 0.25     # every output channel's maximum against its tensor's
X2_WIDTH = 32                # the folded 1x1 operand of gcn_unit_infer (a multiple of 32: one plain stage)

CASES = ((1, 1, 1, 15), (2, 48, 7, 20), (3, 100, 9, 25), (21, 24, 17, 25), (22, 24, 17, 32), (24, 24, 5, 18),
         (31, 33, 6, 25), (33, 31, 3, 20), (32, 40, 9, 18), (48, 72, 7, 25), (63, 65, 5, 15), (64, 60, 6, 25),
         (64, 100, 3, 18), (128, 129, 9, 20), (64, 4, 7, 32), (65, 64, 5, 25), (80, 96, 1, 18), (96, 160, 6, 15),
         (192, 200, 3, 25), (256, 24, 5, 20), (320, 64, 3, 18), (40, 128, 7, 25))
# one seed per case: the first of 100 * case + 1, + 2, ... at which the reference meets ``conditions`` (``search``)
SEEDS = (1, 114, 203, 301, 401, 501, 601, 701, 801, 901, 1001, 1101, 1201, 1301, 1401, 1501, 1601, 1701, 1801, 1901, 2001,
         2101)
# the exact kernels at every width: C < 32, 33..64, 65..128 and > 128
F32_SUBSET = (5, 8, 11, 13, 17, 18)
# the two-kernel adjacency path (Ci, T, V) off the fused kernel's widths {16, 32, 64}; V = 15 is below its V >= 16
ADJ_CASES = ((1, 5, 15), (6, 9, 25), (25, 7, 18), (6, 3, 15))
ADJ_SEEDS = (5001, 5101, 5201, 5301)


def case_id(case):
    return 'x'.join(str(v) for v in case)


def fused_width(Cout):
    return 6 * (Cout // 4)


# ---- the routing, as the sources decide it (gcn_fwd_route, gcn_bwd_data_route, agcn_gcn_chain, gcn_dadj_route,
# gcn_wgrad_route, agcn_wgrad_chain).  A prefix of what agcn_last_kernel() reports; None: refused. ----
def _chain(M, K, K2):
    if K > 32 and ((K <= 64 and K2 <= 96) or (K <= 128 and K2 == 0 and M > 32)):
        tm, ncb2 = (1 if M <= 32 else 2), (K2 + 31) // 32
        if K <= 64:
            return 'gcn_ws_kernel<%d, 2, %d>' % (tm, ncb2)
        if tm == 2 and ncb2 == 0:
            return 'gcn_ws_kernel<2, 4, 0>'
    return 'gcn_chain_kernel<%d, 0, 4, true>' % (4 if M % 128 == 0 else (1 if M <= 32 else 2))


def route(op, C, Cout, f32=False, K2=0):
    """op: fwd | bwd | fused | infer | dadj | wgrad.  K2: the plain-stage operand's width (fused, infer)."""
    if op == 'fwd':
        if f32 or C < 32:
            return 'conv_gemm_kernel<1, 1, %d, 4, 2, 2, 8, 4, 0>' % (2 if Cout % 128 == 0 else 1)
        return _chain(Cout, C, 0)
    if op == 'bwd':
        if f32:
            return 'conv_gemm_kernel<1, 2, %d, 4, 2, 2, 8, 4, 0>' % (2 if C % 128 == 0 else 1)
        return _chain(C, Cout, 0)
    if op == 'fused':
        return None if f32 or K2 <= 0 else _chain(C, Cout, K2)
    if op == 'infer':
        return None if f32 or C < 32 else _chain(Cout, C, K2)
    if op == 'dadj':
        if not f32 and C % 64 == 0:
            return 'gcn_dadj_chain_kernel<4, 8, true>' if C % 128 == 0 else 'gcn_dadj_chain_kernel<2, 4, true>'
        if C >= 64 and C % 64 != 0:
            return None
        exact = 'conv_gemm_kernel<1, 0, 1, 4, 2, 1, 64, 2, 1>'
        return exact + ' [one launch per subset]' if C < 64 < 3 * C else exact
    if op == 'wgrad':
        if not f32 and Cout >= 64 and (C % 64 == 0 or C <= 32):
            if C % 64 == 0 and not (C % 128 != 0 and Cout <= 64):
                return 'wgrad_pc_kernel<1, 2, %d,' % (4 if C % 128 == 0 else 2)
            return 'wgrad_chain_kernel<1, %d,' % (4 if Cout > 64 and C % 64 == 0 else 2)
        return 'conv_wgrad_kernel<1, 1, %d>' % (4 if Cout % 128 == 0 else 2)
    raise KeyError(op)


def dadj_gpc(C):
    """row blocks per subset of the chained adjacency gradient"""
    return C // (128 if C % 128 == 0 else 64)


# the kernel families the table's comments name; tests/test_gcn_width_cpu.py asserts the model of the routing puts a case
# on each, tests/test_gpu_gcn_width.py that the device agrees with the model
FAMILIES = ('gcn_ws_kernel<1, 2, 0>', 'gcn_ws_kernel<2, 2, 0>', 'gcn_ws_kernel<2, 2, 1>', 'gcn_ws_kernel<1, 2, 2>',
            'gcn_ws_kernel<2, 2, 3>', 'gcn_ws_kernel<1, 2, 3>', 'gcn_ws_kernel<2, 4, 0>', 'gcn_chain_kernel<1, 0, 4, true>',
            'gcn_chain_kernel<2, 0, 4, true>', 'gcn_chain_kernel<4, 0, 4, true>', 'conv_gemm_kernel<1, 1, 1, 4, 2, 2, 8, 4, 0>',
            'gcn_dadj_chain_kernel<4, 8, true>', 'gcn_dadj_chain_kernel<2, 4, true>',
            'conv_gemm_kernel<1, 0, 1, 4, 2, 1, 64, 2, 1>', 'conv_gemm_kernel<1, 0, 1, 4, 2, 1, 64, 2, 1> [one launch per subset]',
            'wgrad_pc_kernel<1, 2, 4,', 'wgrad_pc_kernel<1, 2, 2,', 'wgrad_chain_kernel<1, 2,', 'conv_wgrad_kernel<1, 1, 2>',
            'conv_wgrad_kernel<1, 1, 4>')


def routes_of(case, f32=False):
    C, Cout = case[:2]
    r = {op: route(op, C, Cout, f32) for op in ('fwd', 'bwd', 'dadj', 'wgrad')}
    r['fused'] = route('fused', C, Cout, f32, fused_width(Cout))
    r['infer'] = route('infer', C, Cout, f32, 0)
    r['infer_x2'] = route('infer', C, Cout, f32, X2_WIDTH)
    return r


# ---- the recipe ----
def _rn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float64)


def grad_scale(C, Cout, V):
    """standard deviation of dx under the recipe: 3 Cout V terms of variance 0.09 / (3 C)"""
    return 0.3 * math.sqrt(Cout * V / C)


def make(case, seed):
    """fp64 tensors holding fp32 values.  Every row of wcat has the norm a N(0, 1 / 3C) row is expected to have, so that
    the output channels share one scale at any width; the addends and the prior are of the gradient's order."""
    C, Cout, T, V = case
    g = torch.Generator().manual_seed(seed)
    p = dict(x=_rn(g, N, C, T, V), adj=0.3 * _rn(g, N, 3, V, V), bias=0.1 * _rn(g, Cout), dy=_rn(g, N, Cout, T, V))
    w = _rn(g, Cout, 3 * C)
    p['wcat'] = w / w.norm(dim=1, keepdim=True)
    gs = grad_scale(C, Cout, V)
    for k in ('add1', 'add2', 'prior'):
        p[k] = gs * _rn(g, N, C, T, V)
    for k in ('mask1', 'mask2'):
        p[k] = _rn(g, N, C, T, V)
    K2 = fused_width(Cout)
    if K2:
        p['dtp'] = _rn(g, N, K2, T, V)
        p['wab'] = gs * _rn(g, K2, C) / math.sqrt(K2)
    ys = 0.3 * math.sqrt(V)
    p['res'] = ys * _rn(g, N, Cout, T, V)
    p['x2'] = _rn(g, N, X2_WIDTH, T, V)
    p['w2'] = ys * _rn(g, Cout, X2_WIDTH) / math.sqrt(X2_WIDTH)
    return {k: v.float().double() for k, v in p.items()}


# ---- the reference and its mutants ----
def _shift8(t, K):
    """the last 8-channel group of dim 1 read from channels K-8..K-1: what meets the weights of channels K0..K-1"""
    K0 = K // 8 * 8
    idx = torch.arange(K)
    idx[K0:] = K - 8 + (idx[K0:] - K0)
    return t[:, idx]


def _keep(t, n, dim=1):
    out = t.clone()
    out.narrow(dim, n, t.shape[dim] - n).zero_()
    return out


def _rows(t, block, how, dim):
    """rows of `dim` beyond the last full block: dropped, or copied from the block before"""
    M = t.shape[dim]
    full = M // block * block
    out = t.clone()
    tail = out.narrow(dim, full, M - full)
    if how == 'drop':
        tail.zero_()
    else:
        tail.copy_(t.narrow(dim, full - block, M - full))
    return out


MUTANTS = ('k_shift8', 'k_drop16', 'k_drop32', 'm_drop32', 'm_drop64', 'm_dup32', 'm_dup64', 'slot_clobber', 'w_swap',
           'adj_t', 'k2_drop')


def applies(mut, case):
    C, Cout = case[:2]
    K2 = fused_width(Cout)
    if mut == 'k_shift8':
        return any(K % 8 and K > 8 for K in (C, Cout))
    if mut in ('k_drop16', 'k_drop32'):
        b = int(mut[6:])
        return any(K % b for K in (C, Cout))
    if mut in ('m_drop32', 'm_drop64'):
        b = int(mut[6:])
        return any(M % b for M in (C, Cout))
    if mut in ('m_dup32', 'm_dup64'):
        b = int(mut[5:])
        return any(M % b and M > b for M in (C, Cout))
    if mut == 'slot_clobber':
        return any((i * C) // 64 != ((i + 1) * C - 1) // 64 for i in range(3))      # a subset's rows span two blocks
    if mut == 'w_swap':
        return C > 1
    if mut == 'adj_t':
        return True
    if mut == 'k2_drop':
        return K2 % 32 != 0
    raise KeyError(mut)


def reference(p, mut=None):
    """y, the BatchNorm sums, dx (plain), dx2 (accumulate + both masked addends), dx3 (one addend), dx5 (fused term, where
    K2 > 0), dw and dadj of the formulas of tests/test_gpu_kernels.py::_gcn_ref and the v24 dadj test, by fp64 einsum.
    mut: one of MUTANTS, a width bug these kernels could have."""
    x, adj, dy = p['x'], p['adj'], p['dy']
    _, C, T, V = x.shape
    Cout = dy.shape[1]
    w3 = p['wcat'].view(Cout, 3, C)
    if mut == 'w_swap':
        w3 = p['wcat'].view(Cout, C, 3).transpose(1, 2)
    adj_b = adj.transpose(2, 3) if mut == 'adj_t' else adj
    xk, dyk = x, dy                                           # the streamed operands of the channel contractions
    if mut == 'k_shift8':
        xk = _shift8(x, C) if C % 8 and C > 8 else x
        dyk = _shift8(dy, Cout) if Cout % 8 and Cout > 8 else dy
    if mut in ('k_drop16', 'k_drop32'):
        b = int(mut[6:])
        xk, dyk = _keep(x, C // b * b), _keep(dy, Cout // b * b)
    g = torch.einsum('nctu,niuv->nictv', xk, adj)
    y = torch.einsum('oic,nictv->notv', w3, g) + p['bias'].view(1, -1, 1, 1)
    h = torch.einsum('oic,notv->nictv', w3, dyk)
    dx = torch.einsum('nictv,niuv->nctu', h, adj_b)
    dw = torch.einsum('notv,nictv->oic', dy, torch.einsum('nctu,niuv->nictv', x, adj_b))
    hx, xx = h, x
    if mut == 'slot_clobber':                                 # rows (i, c) in 64-row blocks: a subset's last block wins
        keep = torch.zeros(3, C, dtype=torch.bool)
        for i in range(3):
            blk = (i * C + torch.arange(C)) // 64
            keep[i] = blk == blk.max()
        hx = h * keep.view(1, 3, C, 1, 1)
    dadj = torch.einsum('nctu,nictv->niuv', xx, hx)
    if mut and mut.startswith('m_'):
        how, b = ('drop', int(mut[6:])) if mut.startswith('m_drop') else ('dup', int(mut[5:]))
        if Cout % b and (how == 'drop' or Cout > b):
            y, dw = _rows(y, b, how, 1), _rows(dw, b, how, 0)
        if C % b and (how == 'drop' or C > b):
            dx = _rows(dx, b, how, 1)
            dadj = torch.einsum('nctu,nictv->niuv', _rows(x, b, how, 1), _rows(h, b, how, 2))
    out = dict(y=y, ssum=y.sum((0, 2, 3)), ssq=(y * y).sum((0, 2, 3)), dx=dx, dw=dw.reshape(Cout, 3 * C), dadj=dadj)
    out['dx2'] = dx + p['prior'] + p['add1'] * (p['mask1'] > 0) + p['add2'] * (p['mask2'] > 0)
    out['dx3'] = dx + p['add1']
    if 'dtp' in p:
        dtp = p['dtp']
        if mut == 'k2_drop':
            dtp = _keep(dtp, dtp.shape[1] // 32 * 32)
        out['term'] = torch.einsum('kc,nktv->nctv', p['wab'], dtp)
        out['dx5'] = dx + out['term']
    return out


def infer_reference(p, y, res=False, x2=False, relu=True):
    out = y
    if res:
        out = out + p['res']
    if x2:
        out = out + torch.einsum('ok,nktv->notv', p['w2'], p['x2'])
    return out.clamp_min(0) if relu else out


# ---- the metric: max |a - ref| over a channel / max(1, max |ref| over that channel) ----
CHANNEL_DIMS = dict(y=(1,), dx=(1,), dx2=(1,), dx3=(1,), dx5=(1,), dw=(0,), dadj=(0, 1), infer=(1,))


def channel_max(t, keep):
    red = [d for d in range(t.dim()) if d not in keep]
    return t.abs().amax(red) if red else t.abs()


def channel_err(a, ref, keep):
    a, ref = a.detach().double().cpu().reshape(ref.shape), ref.detach().double().cpu()
    return float((channel_max(a - ref, keep) / channel_max(ref, keep).clamp_min(1.0)).max())


def tensor_err(a, ref):
    a, ref = a.detach().double().cpu().reshape(ref.shape), ref.detach().double().cpu()
    return float((a - ref).abs().max() / max(1.0, float(ref.abs().max())))


def conditions(case, p, ref):
    """what makes the comparison able to fail: a list of the conditions this case misses (empty: all met)"""
    miss = []
    for k in ('y', 'dx', 'dx2', 'dx3', 'dx5', 'dw', 'dadj'):
        if k in ref:
            cm = channel_max(ref[k], CHANNEL_DIMS[k])
            if float(cm.min()) < MIN_CHANNEL_SHARE * float(cm.max()):
                miss.append('%s: a channel at %.3f of the tensor' % (k, float(cm.min() / cm.max())))
    gmax = float(ref['dx'].abs().max())
    for k in ('mask1', 'mask2'):
        pos = float((p[k] > 0).double().mean())
        if not 0.25 < pos < 0.75:
            miss.append('%s: %.2f positive' % (k, pos))
    for k in ('add1', 'add2', 'prior'):
        if not 0.25 * gmax < float(p[k].abs().max()) < 4 * gmax:
            miss.append('%s: not of the order of the gradient' % k)
    if 'term' in ref and float(ref['term'].abs().max()) < 0.25 * gmax:
        miss.append('fused term: below a quarter of dx')
    return miss


def search(case, index, tries=50):
    for seed in range(100 * index + 1, 100 * index + 1 + tries):
        p = make(case, seed)
        if not conditions(case, p, reference(p)):
            return seed
    raise RuntimeError('no seed for %r' % (case,))


# ---- the adjacency path ----
def make_adj(case, seed):
    Ci, T, V = case
    g = torch.Generator().manual_seed(seed)
    scale = 1.5 * (Ci * T) ** 0.25                            # softmax logits of standard deviation ~2
    p = dict(tp=scale * _rn(g, N, 6 * Ci, T, V), A=0.2 * _rn(g, 3, V, V), PA=0.05 * _rn(g, 3, V, V), dadj=_rn(g, N, 3, V, V))
    return {k: v.float().double() for k, v in p.items()}


def adj_reference(p):
    """P, adj of reference agcn.py:99-102 and the gradients of sum(adj * dadj) with respect to PA and theta/phi"""
    tp = p['tp'].clone().requires_grad_(True)
    PA = p['PA'].clone().requires_grad_(True)
    n, C6, T, V = tp.shape
    Ci = C6 // 6
    Ps = []
    for i in range(3):
        th = tp[:, (2 * i) * Ci:(2 * i + 1) * Ci].permute(0, 3, 1, 2).reshape(n, V, Ci * T)
        ph = tp[:, (2 * i + 1) * Ci:(2 * i + 2) * Ci].reshape(n, Ci * T, V)
        Ps.append(torch.softmax(torch.matmul(th, ph) / (Ci * T), dim=-2))
    P = torch.stack(Ps, 1)
    adj = P + p['A'] + PA
    (adj * p['dadj']).sum().backward()
    return dict(P=P.detach(), adj=adj.detach(), dPA=PA.grad, dtp=tp.grad, db=tp.grad.sum((0, 2, 3)))
