"""Which joints and frames drove an SGN prediction, and what asking costs, at the deployed shape (V = 15, window 300, two
selected bodies, multi_test S = 5, seg = 20): ``predict`` followed by ``explain`` (online._Recogniser.explain) for one
window per prediction and for 64 windows per batch.
    python tools/sgn_saliency.py [--iters 100] [--warmup 20] [--repeats 3] [--batches 1,64] [--out FILE]
Two routes are measured, each repeat of each in a fresh child process, alternating: ``hip`` (the fused forward and the
HIP input backward of csrc/sgn_bwd.hip) and ``tensor`` (AGCN_SGN_HIP=0: the tensor-code composition of the model under
torch autograd; sampler and its adjoint are the same kernels).  The comparison is between the two routes of this commit.
The model's random weights and the sampler's draws come from fixed seeds, so both routes explain the same prediction of
the same model and their maps are compared.

Per part, by device events: predict (select + normalise, sample, forward, softmax, the synchronising copy of the scores),
resample (ops.sgn_sample with the kept draws), the model's forward + input backward (``hip``: frames, clip, clip_bwd,
frames_bwd one by one; ``tensor``: as one part), sample_bwd, and the norm over xyz with the synchronising copy of the map.
End to end: the host clock around predict + explain, which ends in that copy.  A child reports the median over --iters
iterations after --warmup; the parent reports the median and the min..max of the --repeats children.  Before the
timings, the per-joint and per-frame maps of the first window's prediction (each normalised to sum 1).  Needs a GPU."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

V, FRAMES, S, SEG = 15, 300, 5, 20
ZAXIS, XAXIS = (8, 1), (2, 5)
PARTS = {'hip': ('predict', 'resample', 'frames', 'clip', 'clip_bwd', 'frames_bwd', 'sample_bwd', 'norm+copy'),
         'tensor': ('predict', 'resample', 'model fwd+bwd', None, None, None, 'sample_bwd', 'norm+copy')}


def once(mode, rec, raw, draws, ev):
    """predict + explain of the windows ``raw`` with events around the parts -> (saliency, classes) on the host."""
    import torch
    import online_bench as ob
    from agcn_amd import ops
    N, sgn = raw.shape[0], rec.model
    ev[0].record()
    rec.window, rec.selected, rec.energy = ops.prenorm(raw, num_select=ob.SELECTED, zaxis=ZAXIS, xaxis=XAXIS)
    _, scores, label = rec.forward(rec.window, draws)
    torch.cat((scores, label.to(scores.dtype).unsqueeze(1)), 1).cpu()            # predict's synchronising copy
    ev[1].record()
    with torch.no_grad():
        classes = torch.argmax(rec.logits, 1)
        cot = (torch.nn.functional.one_hot(classes, rec.logits.shape[1]).to(torch.float32) / S).repeat_interleave(S, 0)
        rows, _ = ops.sgn_sample(rec.window, rec.draws, SEG)
        x = rows.view(N * S, SEG, V * 3)
        ev[2].record()
        if mode == 'hip':
            wf, wc, wf_t, wc_t = sgn._images(transposed=True)
            feat, _ = ops.sgn_frames(x, wf, V)
            ev[3].record()
            logits = ops.sgn_clip(feat, wc, sgn.num_class)
            ev[4].record()
            dfeat = ops.sgn_clip_bwd(feat, wc, wc_t, cot)
            ev[5].record()
            dx = ops.sgn_frames_bwd(x, wf, wf_t, dfeat, V)
        else:
            _, _, dx = sgn.input_gradient(x, cot)
            for e in ev[3:6]:
                e.record()
        ev[6].record()
        dwin = ops.sgn_sample_bwd(rec.window, rec.draws, dx.view(N, S, SEG, -1), SEG)
        ev[7].record()
        sal = dwin.square().sum(1).sqrt().permute(0, 1, 3, 2).reshape(N, -1)
        both = torch.cat((sal, classes.to(sal.dtype).unsqueeze(1)), 1).cpu().numpy()
        ev[8].record()
    return both[:, :-1].reshape(N, FRAMES, 2, V), both[:, -1].astype('int64')


def worker(args):
    import numpy as np
    import torch
    import online_bench as ob
    import sgn_bench as sb
    from agcn_amd import online, ops
    mode = 'hip' if ops.sgn_hip_enabled() else 'tensor'
    dev = torch.device('cuda:0')
    torch.manual_seed(0)                       # the model's initialisation: the same weights in every child
    rec = online._Recogniser(sb.build_sgn(), max_frame=FRAMES, max_num_skeleton=ob.TRACKED, max_num_skeleton_true=ob.SELECTED,
                             num_joint=V, zaxis=ZAXIS, xaxis=XAXIS, sgn_preprocess=True, multi_test=S)
    for batch in (int(b) for b in args.batches.split(',')):
        stream = ob.make_stream(FRAMES + batch, V)
        raw = torch.stack([torch.from_numpy(stream[b:b + FRAMES, :, 0]).transpose(0, 1) for b in range(batch)])
        raw = raw.contiguous().to(dev)             # (N, tracked, T, V, 3)
        # the sampler's random numbers are fixed by a seed, so both routes (and every child) explain the same prediction
        # of the same draws; they are uploaded once, which leaves the few microseconds of ops.sgn_draws out of `predict`
        draws = np.random.default_rng(1000 + batch).integers(0, 1 << 32, (batch, S, SEG), dtype=np.uint64)
        draws = torch.from_numpy(draws.astype(np.uint32).view(np.int32)).to(dev)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(9)]
        times = {k: [] for k in PARTS[mode] if k} | {'explain': [], 'end_to_end': []}
        for it in range(args.warmup + args.iters):
            before = dict(ops.SGN_GRAD_STATS), ops.SGN_STATS['forward_tensor']
            t0 = time.perf_counter()
            sal, classes = once(mode, rec, raw, draws, ev)
            t1 = time.perf_counter()
            ev[8].synchronize()
            ran = tuple(ops.SGN_GRAD_STATS[k] - before[0][k] for k in ('clip_bwd', 'frames_bwd', 'sample_bwd'))
            assert ran == ((1, 1, 1) if mode == 'hip' else (0, 0, 1)), (mode, ran)
            assert ops.SGN_STATS['forward_tensor'] - before[1] == (0 if mode == 'hip' else 2)
            if it == 0:
                # the public call gives the same map as the chain timed here (bit for bit on the fused route; torch's
                # autograd makes no such promise)
                again, cls = rec.explain()
                assert np.array_equal(cls, classes) and np.isfinite(sal).all() and float(sal.max()) > 0
                assert np.array_equal(again, sal) if mode == 'hip' else np.allclose(again, sal, rtol=1e-4, atol=1e-6)
                if batch == 1:
                    total = float(sal[0].sum())
                    print(json.dumps(dict(mode=mode, map='per_joint', label=int(classes[0]),
                                          values=[round(float(v) / total, 4) for v in sal[0].sum((0, 1))])), flush=True)
                    print(json.dumps(dict(mode=mode, map='per_frame', label=int(classes[0]),
                                          frames_with_gradient=int((sal[0].sum((1, 2)) > 0).sum()),
                                          values=[round(float(v) / total, 4) for v in sal[0].sum((1, 2))])), flush=True)
            if it >= args.warmup:
                for k, (a, b) in zip(PARTS[mode], zip(ev[:-1], ev[1:])):
                    if k:
                        times[k].append(a.elapsed_time(b))
                times['explain'].append(ev[1].elapsed_time(ev[8]))
                times['end_to_end'].append((t1 - t0) * 1e3)
        for k, xs in times.items():
            print(json.dumps(dict(config=f'sgn_v15_b{batch}', mode=mode, part=k, median_ms=round(statistics.median(xs), 4),
                                  n=len(xs))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--batches', default='1,64')
    ap.add_argument('--out', default=None, help='also write the report to this file')
    ap.add_argument('--child-timeout', type=float, default=300.0, help='seconds one child process may take')
    ap.add_argument('--worker', action='store_true', help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    lines = ['# ' + json.dumps(dict(joints=V, frames=FRAMES, draws=S, seg=SEG, iters=args.iters, warmup=args.warmup,
                                    repeats=args.repeats))]
    print(lines[0], flush=True)
    runs, maps = {}, {}
    for rep in range(args.repeats):
        for mode in PARTS:
            env = dict(os.environ, AGCN_SGN_HIP='1' if mode == 'hip' else '0')
            cmd = [sys.executable, os.path.abspath(__file__), '--worker', '--iters', str(args.iters), '--warmup',
                   str(args.warmup), '--batches', args.batches]
            try:
                r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=args.child_timeout)
            except subprocess.TimeoutExpired:
                raise SystemExit(f'{mode} run {rep} did not finish in {args.child_timeout:.0f} s; it was killed')
            if r.returncode != 0:
                raise SystemExit(f'{mode} run {rep} failed:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}')
            for line in r.stdout.splitlines():
                if not line.startswith('{'):
                    continue
                rec = json.loads(line)
                if 'map' in rec:
                    if rep == 0:
                        maps[mode, rec['map']] = rec
                        lines.append(line)
                        print(line, flush=True)
                else:
                    assert rec['mode'] == mode
                    runs.setdefault((rec['config'], mode, rec['part']), []).append(rec['median_ms'])
    # both routes explained the same window with the same draws: the maps must tell the same story
    for name in ('per_joint', 'per_frame'):
        h, t = maps['hip', name], maps['tensor', name]
        worst = max(abs(a - b) for a, b in zip(h['values'], t['values']))
        lines.append(f'# {name} map, hip against tensor: label {h["label"]} / {t["label"]}, largest difference of the '
                     f'normalised values {worst:.1e} (printed to 4 decimals)')
        print(lines[-1], flush=True)
        if h['label'] == t['label'] and worst > 2e-4:      # 1e-4 is the rounding of the printed values
            raise SystemExit('the two routes do not agree on the explanation of one prediction')
    med = {}
    for (config, mode, part), xs in runs.items():
        med[config, mode, part] = statistics.median(xs)
        lines.append(json.dumps(dict(config=config, mode=mode, part=part, median_ms=round(statistics.median(xs), 4),
                                     min_ms=round(min(xs), 4), max_ms=round(max(xs), 4), runs=len(xs))))
        print(lines[-1], flush=True)
    for config in sorted({k[0] for k in runs}):
        h, t = (runs[config, m, 'end_to_end'] for m in PARTS)
        he, te = (runs[config, m, 'explain'] for m in PARTS)
        apart = max(h) < min(t) or max(t) < min(h)
        lines.append(f'# {config}: predict + explain end to end: hip {med[config, "hip", "end_to_end"]:.3f} ms '
                     f'({min(h):.3f}..{max(h):.3f}), tensor {med[config, "tensor", "end_to_end"]:.3f} ms '
                     f'({min(t):.3f}..{max(t):.3f}); explain alone: hip {statistics.median(he):.3f} ms '
                     f'({min(he):.3f}..{max(he):.3f}), tensor {statistics.median(te):.3f} ms ({min(te):.3f}..{max(te):.3f}); '
                     + ('the ranges of the runs do not overlap' if apart else
                        'the ranges of the runs overlap: no difference beyond the spread'))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
