"""Latency and throughput of SGN recognition at the deployed shape (reference infer/inference.py:140-150: V = 15, window
300, two selected bodies, multi_test S = 5, seg = 20): one window per prediction, and 64 windows per batch.
    python tools/sgn_bench.py [--iters 200] [--warmup 30] [--batches 1,64] [--out FILE]
Three paths run on the same normalised windows, alternating iteration by iteration so that they share whatever else the
machine is doing: ``hip`` (ops.sgn_sample + the fused SGN forward), ``tensor`` (the same with AGCN_SGN_HIP=0: the
tensor-code composition of the model, same sampler) and ``aagcn`` (the AAGCN of tools/online_bench.py on the whole
window, for scale).

Per part, by device events: select + normalise (ops.prenorm), sample (draws + ops.sgn_sample), frames / clip
(``hip``) or model (``tensor``, ``aagcn``), and the rest (mean over the draws, softmax, argmax, the synchronising copy
of the scores).  End to end: the host clock around the whole prediction, which ends in that copy.  Every figure is the
median over --iters iterations after --warmup with the 10th..90th percentile; weight images are cached before anything
is timed.  Needs a GPU; prints one JSON line per measurement."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
import online_bench as ob  # noqa: E402

V, FRAMES, S, SEG = 15, 300, 5, 20
ZAXIS, XAXIS = (8, 1), (2, 5)


def build_sgn():
    import agcn_amd  # noqa: F401
    from model.sgn import SGN
    model = SGN(num_class=60, num_point=V, seg=SEG)
    bench.randomize_like_training(model, 0)
    with torch.no_grad():                      # the reference initialises gcn*.w to zero: give the g.x branch weights
        for gcn in (model.gcn1, model.gcn2, model.gcn3):
            gcn.w.cnn.weight.copy_(gcn.w1.cnn.weight.flip(0))
    return model


def predict(path, raw, sgn, aagcn, ev):
    """One prediction of N windows -> (scores + label on the host, part names); events ev[0..5] around the parts."""
    from agcn_amd import ops
    N = raw.shape[0]
    with torch.no_grad():
        ev[0].record()
        win, _, _ = ops.prenorm(raw, num_select=ob.SELECTED, zaxis=ZAXIS, xaxis=XAXIS)
        ev[1].record()
        if path == 'aagcn':
            ev[2].record()
            logits = aagcn(win)
            logits = logits[0] if isinstance(logits, tuple) else logits
            ev[3].record()
            ev[4].record()
        else:
            rows, _ = ops.sgn_sample(win, ops.sgn_draws(N, S, SEG, win.device), SEG)
            x = rows.view(N * S, SEG, V * 3)
            ev[2].record()
            if path == 'hip':
                wf, wc = sgn._images()
                feat, _ = ops.sgn_frames(x, wf, V, want_g=False)
                ev[3].record()
                logits = ops.sgn_clip(feat, wc, sgn.num_class)
            else:
                logits, _ = sgn(x)
                ev[3].record()
            ev[4].record()
            logits = logits.view(N, S, -1).mean(1)
        scores = torch.softmax(logits, 1)
        both = torch.cat((scores, torch.argmax(scores, 1, keepdim=True).to(scores.dtype)), 1).cpu()
        ev[5].record()
    return both


PARTS = {'hip': ('select+normalise', 'sample', 'frames', 'clip', 'rest'),
         'tensor': ('select+normalise', 'sample', 'model', None, 'rest'),
         'aagcn': ('select+normalise', None, 'model', None, 'rest')}


def run(batch, args, out):
    from agcn_amd import ops
    dev = torch.device('cuda:0')
    sgn = build_sgn().to(dev).eval()
    aagcn = ob.build('aagcn_v15')[0].to(dev).eval()
    stream = ob.make_stream(FRAMES + batch, V)
    raw = torch.stack([torch.from_numpy(stream[b:b + FRAMES, :, 0]).transpose(0, 1) for b in range(batch)])
    raw = raw.contiguous().to(dev)             # (N, tracked, T, V, 3)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
    times = {p: {k: [] for k in PARTS[p] if k} | {'end_to_end': []} for p in PARTS}
    labels = {}
    for it in range(args.warmup + args.iters):
        for path in PARTS:
            os.environ['AGCN_SGN_HIP'] = '0' if path == 'tensor' else '1'
            before = dict(ops.SGN_STATS)
            t0 = time.perf_counter()
            both = predict(path, raw, sgn, aagcn, ev)
            t1 = time.perf_counter()
            ev[5].synchronize()
            ran = {k: ops.SGN_STATS[k] - before[k] for k in before}
            want = dict(hip=(1, 1, 1, 0), tensor=(0, 0, 1, 1), aagcn=(0, 0, 0, 0))[path]
            assert tuple(ran[k] for k in ('frames_hip', 'clip_hip', 'sample_hip', 'forward_tensor')) == want, (path, ran)
            labels[path] = both[:, -1].long().tolist()
            if it >= args.warmup:
                for k, (a, b) in zip(PARTS[path], zip(ev[:-1], ev[1:])):
                    if k:
                        times[path][k].append(a.elapsed_time(b))
                times[path]['end_to_end'].append((t1 - t0) * 1e3)
    os.environ.pop('AGCN_SGN_HIP', None)
    med = {p: {k: ob.report(f'sgn_v15_b{batch}', p, k, xs, out) for k, xs in times[p].items()} for p in PARTS}
    h, t, a = med['hip'], med['tensor'], med['aagcn']
    print(f'# batch {batch}: hip end to end {h["end_to_end"]:.3f} ms (sample {h["sample"]:.3f}, frames {h["frames"]:.3f}, '
          f'clip {h["clip"]:.3f}, rest {h["rest"]:.3f}) = {batch / h["end_to_end"] * 1e3:.0f} windows/s; tensor '
          f'{t["end_to_end"]:.3f} ms (model {t["model"]:.3f}) = {t["end_to_end"] / h["end_to_end"]:.2f}x the hip time; '
          f'aagcn {a["end_to_end"]:.3f} ms (model {a["model"]:.3f})', flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=30)
    ap.add_argument('--batches', default='1,64')
    ap.add_argument('--out', default=None, help='also append the JSON lines to this file')
    args = ap.parse_args()
    if args.iters < 200:
        print('# fewer than 200 timed predictions: a rehearsal, not a measurement', flush=True)
    if not torch.cuda.is_available():
        raise SystemExit('sgn_bench needs a GPU: there is nothing to measure without one')
    out = open(args.out, 'a') if args.out else None
    print('# ' + json.dumps(dict(device=torch.cuda.get_device_name(0), host_cores=os.cpu_count(), joints=V, frames=FRAMES,
                                draws=S, seg=SEG, iters=args.iters, warmup=args.warmup)), flush=True)
    for b in args.batches.split(','):
        run(int(b), args, out)
    if out:
        out.close()


if __name__ == '__main__':
    main()
