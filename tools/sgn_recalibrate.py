"""Re-estimate SGN's seven BatchNorms on site data (AdaBN), and what that costs on the two routes of this commit:
    python tools/sgn_recalibrate.py --data windows.npy [--weights IN.pt] --out OUT.pt [--momentum M]
    python tools/sgn_recalibrate.py [--iters 30] [--warmup 10] [--repeats 3] [--batches 1,64] [--report FILE]
With --data: windows.npy holds normalised windows (N, 3, T, V, 2) in ``ops.prenorm``'s output layout (the format of
tools/sgn_finetune.py); they are sampled with S = 5 seeded draws each (``ops.sgn_sample``) and the N * 5 clips go through
``SGN.recalibrate_bn`` as ONE batch; the state_dict with the new running statistics (the reference's names) is saved.

Without data: a seeded synthetic set at the deployed shape (V = 15, window 300, two selected bodies, S = 5, seg = 20), one
prediction's worth of windows (1 window = 5 clips) and 64 windows (320 clips).  ``hip``: ``SGN.batch_statistics`` on the
fused path (csrc/sgn_stats.hip); ``tensor``: the same call with AGCN_SGN_HIP=0, the tensor-code composition with its
BatchNorms in batch mode.  End to end = the host clock around ``recalibrate_bn`` ending in a device synchronisation.  On
the hip route each pass is also timed on its own by device events (the launch with its finalize; one fold of the two
weight images, which a call does once before it patches a section per BatchNorm).  A child reports the median over
--iters calls after --warmup; the parent the median and min..max of the --repeats children, each a fresh process, the two
routes alternating.  No threshold: the report says what came out.  Needs a GPU."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

V, FRAMES, S, SEG, NUM_CLASS = 15, 300, 5, 20, 60
ZAXIS, XAXIS = (8, 1), (2, 5)
MODES = ('hip', 'tensor')


def clips_of(win, seed=0):
    """Normalised windows (N, 3, T, V, 2) -> (N * S, seg, V * 3) with seeded draws."""
    import torch
    from agcn_amd import ops
    torch.manual_seed(seed)
    with torch.no_grad():
        rows, _ = ops.sgn_sample(win, ops.sgn_draws(win.shape[0], S, SEG, win.device), SEG)
    return rows.view(win.shape[0] * S, SEG, -1).contiguous()


def timed(fn, ev):
    ev[0].record()
    out = fn()
    ev[1].record()
    return out


def passes(model, x, iters, warmup):
    """Each pass of ``ops.sgn_batch_statistics`` on its own, by device events: {name: median ms}."""
    import torch
    from agcn_amd import ops
    N, seg, _ = x.shape
    _, _, stats = model.batch_statistics(x)
    known = {n: s[:2] for n, s in stats.items()}
    wf, wc = model._batch_images(known, None)
    feat, _ = ops.sgn_frames(x, wf, V)
    fin = lambda part, kind, layer: ops.sgn_stats_finalize(part, kind, layer, N, seg, V)     # noqa: E731
    jobs = {'fold of both images (once per call)': lambda: model._batch_images(known, 'gcn2.bn'),
            'input + finalize': lambda: fin(ops.sgn_input_stats(x, V), 0, 0),
            'frames full depth': lambda: ops.sgn_frames(x, wf, V),
            'clip full depth': lambda: ops.sgn_clip(feat, wc, NUM_CLASS)}
    for layer in (1, 2, 3):
        jobs[f'frames gcn{layer} + finalize'] = lambda layer=layer: fin(ops.sgn_frames_stats(x, wf, layer, V), 1, layer)
    for layer in (1, 2):
        jobs[f'clip cnn{layer} + finalize'] = lambda layer=layer: fin(ops.sgn_clip_stats(feat, wc, layer, NUM_CLASS), 2, layer)
    out = {}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    with torch.no_grad():
        for name, fn in jobs.items():
            ts = []
            for it in range(warmup + iters):
                timed(fn, ev)
                ev[1].synchronize()
                if it >= warmup:
                    ts.append(ev[0].elapsed_time(ev[1]))
            out[name] = statistics.median(ts)
    return out


def worker(args):
    import torch
    import online_bench as ob
    import sgn_bench as sb
    from agcn_amd import ops
    dev = torch.device('cuda:0')
    assert ops.sgn_hip_enabled() == (args.mode == 'hip')
    for batch in (int(b) for b in args.batches.split(',')):
        torch.manual_seed(0)
        model = sb.build_sgn().to(dev).eval()
        stream = ob.make_stream(FRAMES + batch, V)
        raw = torch.stack([torch.from_numpy(stream[b:b + FRAMES, :, 0]).transpose(0, 1) for b in range(batch)])
        with torch.no_grad():
            win, _, _ = ops.prenorm(raw.contiguous().to(dev), num_select=ob.SELECTED, zaxis=ZAXIS, xaxis=XAXIS)
        x = clips_of(win)
        config = f'sgn_v15_b{batch}'
        ts = []
        for it in range(args.warmup + args.iters):
            before = ops.SGN_STATS['forward_tensor'], ops.SGN_BNSTATS_STATS['frames_stats']
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            model.recalibrate_bn(x)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            ran = ops.SGN_STATS['forward_tensor'] - before[0], ops.SGN_BNSTATS_STATS['frames_stats'] - before[1]
            assert ran == ((0, 3) if args.mode == 'hip' else (1, 0)), ran
            if it >= args.warmup:
                ts.append((t1 - t0) * 1e3)
        var = float(model.cnn.bn2.running_var.mean())
        assert var == var, 'the running variance is not a number'
        print(json.dumps(dict(config=config, mode=args.mode, part='end_to_end', clips=x.shape[0],
                              median_ms=round(statistics.median(ts), 4), n=len(ts))), flush=True)
        if args.mode == 'hip':
            for name, ms in passes(model, x, args.iters, args.warmup).items():
                print(json.dumps(dict(config=config, mode=args.mode, part=name, clips=x.shape[0], median_ms=round(ms, 4),
                                      n=args.iters)), flush=True)


def recalibrate(args):
    import numpy as np
    import torch
    import agcn_amd  # noqa: F401
    from model.sgn import SGN
    dev = torch.device('cuda:0')
    win = torch.from_numpy(np.load(args.data).astype(np.float32)).to(dev)
    if win.dim() != 5 or win.shape[1] != 3 or win.shape[4] != 2:
        raise SystemExit(f'--data holds (N, 3, T, V, 2), got {tuple(win.shape)}')
    model = SGN(num_class=args.num_class, num_point=win.shape[3], seg=SEG)
    if args.weights:
        model.load_state_dict(torch.load(args.weights, map_location='cpu'))
    model = model.to(dev).eval()
    x = clips_of(win.contiguous())
    with torch.no_grad():
        before = model(x)[0].argmax(1)
    stats = model.recalibrate_bn(x, momentum=args.momentum)
    with torch.no_grad():
        after = model(x)[0].argmax(1)
    for name, (mean, var, count) in stats.items():
        print(f'{name}: {count} samples per channel, mean in [{float(mean.min()):.4f}, {float(mean.max()):.4f}], '
              f'variance in [{float(var.min()):.3e}, {float(var.max()):.3e}]')
    print(f'{int((before != after).sum())} of {x.shape[0]} clips changed their top class')
    torch.save({k: v.cpu() for k, v in model.state_dict().items()}, args.out)
    print(f'saved {args.out}')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--batches', default='1,64')
    ap.add_argument('--report', default=None, help='also write the report to this file')
    ap.add_argument('--child-timeout', type=float, default=300.0, help='seconds one child process may take')
    ap.add_argument('--data', default=None)
    ap.add_argument('--weights', default=None)
    ap.add_argument('--out', default=None, help='with --data: where the recalibrated state_dict goes')
    ap.add_argument('--momentum', type=float, default=None, help='with --data: exponential instead of cumulative average')
    ap.add_argument('--num-class', type=int, default=NUM_CLASS)
    ap.add_argument('--worker', action='store_true', help=argparse.SUPPRESS)
    ap.add_argument('--mode', choices=MODES, default='hip', help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    if args.data:
        if not args.out:
            raise SystemExit('--data needs --out')
        return recalibrate(args)
    lines = ['# ' + json.dumps(dict(joints=V, frames=FRAMES, draws=S, seg=SEG, iters=args.iters, warmup=args.warmup,
                                    repeats=args.repeats))]
    print(lines[0], flush=True)
    runs = {}
    for rep in range(args.repeats):
        for mode in MODES:
            cmd = [sys.executable, os.path.abspath(__file__), '--worker', '--mode', mode, '--iters', str(args.iters),
                   '--warmup', str(args.warmup), '--batches', args.batches]
            env = dict(os.environ, AGCN_SGN_HIP='1' if mode == 'hip' else '0')
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.child_timeout, env=env)
            except subprocess.TimeoutExpired:
                raise SystemExit(f'{mode} run {rep} did not finish in {args.child_timeout:.0f} s; it was killed')
            if r.returncode != 0:
                raise SystemExit(f'{mode} run {rep} failed:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}')
            for line in r.stdout.splitlines():
                if line.startswith('{'):
                    rec = json.loads(line)
                    runs.setdefault((rec['config'], mode, rec['part'], rec['clips']), []).append(rec['median_ms'])
    for (config, mode, part, clips), xs in runs.items():
        lines.append(json.dumps(dict(config=config, clips=clips, mode=mode, part=part, median_ms=round(statistics.median(xs), 4),
                                     min_ms=round(min(xs), 4), max_ms=round(max(xs), 4), runs=len(xs))))
    for config in sorted({k[0] for k in runs}):
        h, t = (next(v for k, v in runs.items() if k[:3] == (config, m, 'end_to_end')) for m in MODES)
        apart = max(h) < min(t) or max(t) < min(h)
        lines.append(f'# {config}: recalibrate_bn end to end: hip {statistics.median(h):.3f} ms ({min(h):.3f}..{max(h):.3f}), '
                     f'tensor {statistics.median(t):.3f} ms ({min(t):.3f}..{max(t):.3f}), tensor / hip = '
                     f'{statistics.median(t) / statistics.median(h):.2f}; '
                     + ('the ranges of the runs do not overlap' if apart else
                        'the ranges of the runs overlap: no difference beyond the spread'))
    print('\n'.join(lines[1:]), flush=True)
    if args.report:
        with open(args.report, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
