"""The aagcn_v17 encoder head alone, at the shape of the reference yaml (N = 64, L = 201, D = 400, H = 2, F = 1600,
3 layers, dropout 0.2), and the whole aagcn_v17 training step at batch 64, T = 300.

    python tools/bench_encoder.py [--iters 30] [--warmup 5] [--reps 5] [--no-step]
    python tools/bench_encoder.py --v24        # the aagcn_v24 head instead: 6400 sequences x 51 tokens x 144, H = 3

One JSON line per part: tokens, attention core, add + LayerNorm (HIP kernels against the tensor-code composition that
AGCN_ENCODER_HIP=0 selects), the four projections + activation of a layer (F.linear / ATen on either path), one whole
layer, the 3-layer head and the training step.  Forward is timed under autograd (it saves what the backward reads),
backward = (forward + backward) - forward.  Method: device events around `iters` calls after `warmup` calls per shape;
the two paths alternate inside one process, `reps` rounds, and the line gives the median and the min..max spread.
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, M, C, TP, V, H, LAYERS, P_DROP = 64, 2, 16, 100, 25, 2, 3, 0.2
D, FF, L = V * C, 4 * V * C, 1 + M * TP


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def fwd_bwd(make_out, leaves):
    """(forward only, forward + backward) closures over fresh leaves; the loss is sum(out * r) with a fixed r."""
    r = [None]

    def fwd():
        return make_out()

    def both():
        for t in leaves:
            t.grad = None
        out = make_out()
        if r[0] is None:
            r[0] = torch.randn_like(out)
        out.backward(r[0])
    return fwd, both


def report(name, variants, args, extra=None):
    """variants: {label: (fwd, both)}; alternated round by round."""
    times = {k: {'fwd': [], 'both': []} for k in variants}
    for _ in range(args.reps):
        for k, (f, b) in variants.items():
            times[k]['fwd'].append(timed(f, args.iters, args.warmup))
            times[k]['both'].append(timed(b, args.iters, args.warmup))
    line = {'part': name}
    for k, t in times.items():
        fm, bm = statistics.median(t['fwd']), statistics.median(t['both'])
        line[k] = {'fwd_ms': round(fm, 4), 'bwd_ms': round(bm - fm, 4), 'fwd_bwd_ms': round(bm, 4),
                   'fwd_bwd_min_max_ms': [round(min(t['both']), 4), round(max(t['both']), 4)]}
    if extra:
        line.update(extra)
    print(json.dumps(line), flush=True)
    return line


def v24_case(args, dev):
    """The spatial head of aagcn_v24 at the shape of its yaml (batch 64, T' = 100: 6400 sequences of 51 tokens, width 144,
    3 heads, 3 layers, add_A single, cossin, CLS_MASK, dropout 0.2): the spatial tokens, the attention core with the
    bias (forward, backward and the bias gradient), and the whole head as the model runs it (forward_postprocess: tokens,
    3 layers, the masked mean), HIP kernels against AGCN_ENCODER_HIP=0."""
    from agcn_amd import ops
    from agcn_amd.model import aagcn_v24
    n, m_, c, tp, v, h = 64, 2, 144, 100, 25, 3
    seqs, ltok = n * tp, 1 + m_ * v
    g = torch.Generator(device=dev).manual_seed(24)
    rnd = lambda *s: torch.randn(*s, device=dev, generator=g)      # noqa: E731
    leaf = lambda *s: rnd(*s).requires_grad_(True)                 # noqa: E731
    x, cls, pe = leaf(n * m_, c, tp, v), leaf(1, 1, c), leaf(1, 100, c)
    report('v24_spatial_tokens', {
        'hip': fwd_bwd(lambda: ops.SpatialTokensFunction.apply(x, cls, pe, m_), [x, cls, pe]),
        'tensor': fwd_bwd(lambda: ops.tokens_spatial_ref(x, cls, pe, m_), [x, cls, pe])}, args,
        {'bytes_fwd': 4 * (x.numel() + seqs * ltok * c)})
    qkv, bias = leaf(seqs, ltok, 3 * c), leaf(1, ltok, ltok)
    keep = (torch.rand(seqs, h, ltok, ltok, device=dev, generator=g) >= P_DROP).to(torch.uint8)
    ks = 1.0 / (1.0 - P_DROP)
    flops = 4.0 * seqs * h * ltok * ltok * (c // h)
    report('v24_attention_core_bias', {
        'hip': fwd_bwd(lambda: ops.MHABiasFunction.apply(qkv, h, bias, None, 0, keep, ks, False)[0], [qkv, bias]),
        'tensor': fwd_bwd(lambda: ops.mha_ref(qkv, h, None, 0, keep, ks, False, bias=bias)[0], [qkv, bias])}, args,
        {'flop_fwd': flops, 'flop_bwd': 2.5 * flops, 'workgroups_fwd': seqs * h * ((ltok + 15) // 16)})
    model = aagcn_v24.Model(graph='graph.ntu_rgb_d.Graph', graph_args=dict(labeling_mode='spatial'), kernel_size=3,
                            pad=False, s_trans_cfg=dict(num_heads=h, model_dim=c, ffn_dim=4 * c, dropout=P_DROP,
                                                        activation='gelu', prenorm=False, num_layers=LAYERS),
                            add_A='single', pos_enc='cossin', classifier_type='CLS_MASK', model_layers=101).to(dev).train()
    with torch.no_grad():
        model.alpha.fill_(0.8)
    model.attn_mask = (torch.rand(n, tp, 1, device=dev, generator=g) < 0.3)
    size = torch.Size((n, 3, 3 * tp, v, m_))
    feat = leaf(n * m_, c, tp, v)
    leaves = [feat] + [p for k, p in model.named_parameters() if k.startswith(('s_', 'alpha'))]

    def head(flag):
        def f():
            os.environ['AGCN_ENCODER_HIP'] = flag
            return model.forward_postprocess(feat, size)[0]
        return f
    report('v24_head_3_layers', {'hip': fwd_bwd(head('1'), leaves), 'tensor': fwd_bwd(head('0'), leaves)}, args,
           {'sequences': seqs, 'tokens': ltok, 'width': c, 'heads': h, 'layers': LAYERS})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--no-step', action='store_true', help='skip the whole-model training step')
    ap.add_argument('--v24', action='store_true', help='the aagcn_v24 spatial head instead of the aagcn_v17 parts')
    args = ap.parse_args()
    import agcn_amd  # noqa: F401
    from agcn_amd import ops
    from agcn_amd.model import aagcn_v17
    assert torch.cuda.is_available(), "bench_encoder.py measures on the GPU"
    dev = torch.device('cuda:0')
    if args.v24:
        v24_case(args, dev)
        return
    g = torch.Generator(device=dev).manual_seed(1)
    rnd = lambda *s: torch.randn(*s, device=dev, generator=g)      # noqa: E731
    leaf = lambda *s: rnd(*s).requires_grad_(True)                 # noqa: E731

    # tokens
    x, cls, pe = leaf(N * M, C, TP, V), leaf(1, 1, D), leaf(1, 601, D)
    report('tokens', {'hip': fwd_bwd(lambda: ops.TokensFunction.apply(x, cls, pe, M), [x, cls, pe]),
                      'tensor': fwd_bwd(lambda: ops.tokens_ref(x, cls, pe, M), [x, cls, pe])}, args,
           {'bytes_fwd': 4 * (x.numel() + N * L * D)})

    # attention core (keep mask drawn beforehand, as the layer does per call)
    qkv = leaf(N, L, 3 * D)
    keep = (torch.rand(N, H, L, L, device=dev, generator=g) >= P_DROP).to(torch.uint8)
    ks = 1.0 / (1.0 - P_DROP)
    flops = 4.0 * N * H * L * L * (D // H)
    report('attention_core', {
        'hip': fwd_bwd(lambda: ops.MHAFunction.apply(qkv, H, None, 0, keep, ks, False)[0], [qkv]),
        'tensor': fwd_bwd(lambda: ops.mha_ref(qkv, H, None, 0, keep, ks, False)[0], [qkv])}, args,
        {'flop_fwd': flops, 'flop_bwd': 2.5 * flops})
    report('attention_core_no_dropout', {
        'hip': fwd_bwd(lambda: ops.MHAFunction.apply(qkv, H, None, 0, None, 1.0, False)[0], [qkv]),
        'tensor': fwd_bwd(lambda: ops.mha_ref(qkv, H, None, 0, None, 1.0, False)[0], [qkv])}, args)

    # add + LayerNorm (two per layer)
    a, b, w, bias = leaf(N, L, D), leaf(N, L, D), leaf(D), leaf(D)
    report('add_layernorm', {'hip': fwd_bwd(lambda: ops.AddLayerNormFunction.apply(a, b, w, bias, 1e-5), [a, b, w, bias]),
                             'tensor': fwd_bwd(lambda: ops.add_ln_ref(a, b, w, bias, 1e-5), [a, b, w, bias])}, args,
           {'bytes_fwd': 4 * 3 * a.numel()})

    # the four projections and the activation of one layer: the same vendor GEMMs on either path
    t = leaf(N, L, D)
    w_in, w_out, w1, w2 = leaf(3 * D, D), leaf(D, D), leaf(FF, D), leaf(D, FF)
    b_in, b_out, b1, b2 = leaf(3 * D), leaf(D), leaf(FF), leaf(D)

    def projections():
        q = F.linear(t, w_in, b_in)
        o = F.linear(q[..., :D], w_out, b_out)
        return F.linear(F.gelu(F.linear(o, w1, b1)), w2, b2)
    gemm_flops = 2.0 * N * L * D * (3 * D + D + 2 * FF)
    proj = report('projections', {'aten': fwd_bwd(projections, [t, w_in, w_out, w1, w2, b_in, b_out, b1, b2])}, args,
                  {'flop_fwd': gemm_flops})

    # one layer and the 3-layer head, training mode with dropout 0.2
    layer = aagcn_v17.TransformerEncoderLayerExt(D, H, FF, P_DROP, 'gelu', 1e-5, True, pre_norm=False).to(dev).train()
    head = torch.nn.ModuleList([aagcn_v17.TransformerEncoderLayerExt(D, H, FF, P_DROP, 'gelu', 1e-5, True)
                                for _ in range(LAYERS)]).to(dev).train()
    src = leaf(N, L, D)

    def run_layers(mods, flag):
        def f():
            os.environ['AGCN_ENCODER_HIP'] = flag
            y = src
            for m_ in mods:
                y, _ = m_(y, need_attn=False)
            return y
        return f
    lay = report('layer', {'hip': fwd_bwd(run_layers([layer], '1'), [src]),
                           'tensor': fwd_bwd(run_layers([layer], '0'), [src])}, args)
    report('head_3_layers', {'hip': fwd_bwd(run_layers(head, '1'), [src]),
                             'tensor': fwd_bwd(run_layers(head, '0'), [src])}, args)
    print(json.dumps({'part': 'projections_share_of_layer',
                      'hip': round(proj['aten']['fwd_bwd_ms'] / lay['hip']['fwd_bwd_ms'], 3),
                      'tensor': round(proj['aten']['fwd_bwd_ms'] / lay['tensor']['fwd_bwd_ms'], 3)}), flush=True)

    if args.no_step:
        return
    # the whole training step of the shipped configuration
    from agcn_amd.trainer import TrainEngine, synthetic_batch
    model = aagcn_v17.Model(graph='graph.ntu_rgb_d.Graph', graph_args=dict(labeling_mode='spatial'), kernel_size=3,
                            pad=False, trans_num_heads=H, trans_model_dim=C, trans_ffn_dim=FF // V,
                            trans_dropout=P_DROP, trans_activation='gelu', trans_num_layers=LAYERS, pos_enc='False',
                            classifier_type='CLS', model_layers=101, attn_masking='False').to(dev)
    eng = TrainEngine(model, base_lr=0.01)
    data, label = synthetic_batch(N, T=TP * 3, device=dev)

    def step(flag):
        def f():
            os.environ['AGCN_ENCODER_HIP'] = flag
            eng.train_step(data, label)
        return f
    times = {'hip': [], 'tensor': []}
    for _ in range(args.reps):
        for k, flag in (('hip', '1'), ('tensor', '0')):
            times[k].append(timed(step(flag), max(5, args.iters // 3), args.warmup))
    print(json.dumps({'part': 'train_step_batch64_T300',
                      **{k: {'step_ms': round(statistics.median(v), 3), 'min_max_ms': [round(min(v), 3), round(max(v), 3)],
                             'samples_per_s': round(N / statistics.median(v) * 1e3, 1)} for k, v in times.items()}}),
          flush=True)


if __name__ == '__main__':
    main()
