"""Frozen-BatchNorm fine-tuning of SGN v15 at the deployed geometry (V = 15, seg = 20, heads 8 x 16, ff 128 / 8 x 32,
ff 256, multi_test 5), and what a step costs on the two routes of this commit:
    python tools/sgn_v15_finetune.py [--iters 30] [--warmup 10] [--repeats 3] [--batches 1,64] [--report FILE]
A step: SGN v15 in eval mode (BatchNorm on its running statistics) on a batch of sampled clips (batch x 5 clips of 20
frames) -> cross-entropy -> ``backward()`` -> ``torch.optim.Adam.step()``.  ``fused`` sets ``SGN.fused_finetune``: the two
forward launches, the taping backward kernels (csrc/sgn_v15_bwd.hip), the tape reductions of csrc/sgn_v15_wgrad.hip, torch
autograd only through the fold of the weight images.  ``tensor`` leaves the flag off: the tensor-code composition under
torch autograd (the behaviour without this route), which stores every activation of both attention blocks.  Model, clips
and labels come from fixed seeds, so both routes take the same steps and their losses are printed side by side.  Each
repeat of each route runs in a fresh child process, alternating.

Per part, by device events.  fused: forward (the fold and the two launches), loss + taping backward, reductions,
fold + optimiser (autograd through the fold, Adam).  tensor: forward, loss + backward, optimiser.  End to end: the host
clock around a step that ends in the copy of the loss.  Peak memory: ``torch.cuda.max_memory_allocated`` of the child
after its steps.  A child reports the median over --iters steps after --warmup; the parent the median and the min..max of
the --repeats children.  There is no threshold: the report says what came out.  Needs a GPU."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

V, S, SEG, NUM_CLASS = 15, 5, 20, 60
MODES = ('fused', 'tensor')
PARTS = {'fused': ('forward', 'loss+taping backward', 'reductions', 'fold+optimiser'),
         'tensor': ('forward', 'loss+backward', 'optimiser')}
LOSSES = 20
LR = 1e-4


def worker(args):
    import numpy as np
    import torch
    import bench
    import sgn_v15_bench as vb
    import agcn_amd  # noqa: F401
    from agcn_amd import ops
    from model.sgn_v15 import SGN
    dev = torch.device('cuda:0')
    fused = args.mode == 'fused'
    sp, tp = vb.HEADS['deployed']
    parts = PARTS[args.mode]
    for batch in (int(b) for b in args.batches.split(',')):
        clips = batch * S
        torch.manual_seed(0)                                 # the same initialisation in every child
        model = SGN(**vb.model_args(sp, tp))
        bench.randomize_like_training(model, 0)
        model = model.to(dev).eval()
        model.fused_finetune = fused
        opt = torch.optim.Adam(model.parameters(), lr=LR)
        rng = np.random.default_rng(3000 + batch)
        x = torch.from_numpy(rng.standard_normal((clips, SEG, 3 * V)).astype(np.float32)).to(dev)
        labels = torch.from_numpy(rng.integers(0, NUM_CLASS, batch)).to(dev).repeat_interleave(S)
        marks = []
        ops.SGN15_WGRAD_MARK = (lambda label: marks.append((label, _event(torch)))) if fused else None
        times = {k: [] for k in parts} | {'end_to_end': []}
        losses = []
        torch.cuda.reset_peak_memory_stats()
        for it in range(args.warmup + args.iters):
            before = ops.SGN_STATS['forward_tensor'], ops.SGN15_WGRAD_STATS['frames_wgrad']
            del marks[:]
            t0 = time.perf_counter()
            e0 = _event(torch)
            logits, _ = model(x)
            e1 = _event(torch)
            loss = torch.nn.functional.cross_entropy(logits, labels)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            e2 = _event(torch)
            opt.step()
            e3 = _event(torch)
            loss = float(loss)                               # the synchronising copy of the loss
            t1 = time.perf_counter()
            e3.synchronize()
            taped = ops.SGN15_WGRAD_STATS['frames_wgrad'] - before[1]
            assert (ops.SGN_STATS['forward_tensor'] - before[0], taped > 0) == ((0, True) if fused else (1, False))
            assert loss == loss, 'the loss is not a number'
            if it < LOSSES:
                losses.append(round(loss, 5))
            if it >= args.warmup:
                if fused:                                    # per chunk: ... 'tape' ... 'reduce'
                    tape = [e for label, e in marks if label == 'tape']
                    red = [e for label, e in marks if label == 'reduce']
                    starts = [e1] + red[:-1]
                    times[parts[0]].append(e0.elapsed_time(e1))
                    times[parts[1]].append(sum(a.elapsed_time(b) for a, b in zip(starts, tape)))
                    times[parts[2]].append(sum(a.elapsed_time(b) for a, b in zip(tape, red)))
                    times[parts[3]].append(red[-1].elapsed_time(e3))
                else:
                    for k, a, b in zip(parts, (e0, e1, e2), (e1, e2, e3)):
                        times[k].append(a.elapsed_time(b))
                times['end_to_end'].append((t1 - t0) * 1e3)
        L = ops._L()
        tape_mb = 4 * (L.agcn_sgn15_frames_tape_floats(clips, SEG, V, *sp)
                       + L.agcn_sgn15_clip_tape_floats(clips, SEG, NUM_CLASS, *tp)) / 2**20
        chunk = ops.sgn15_tape_chunk(clips, SEG, V, NUM_CLASS, sp, tp, ops.SGN_MAX_TAPE_BYTES)
        print(json.dumps(dict(config=f'sgn15_deployed_b{batch}', mode=args.mode, losses=losses, clips=clips,
                              tape_mib_per_step=round(tape_mb, 1), tape_chunks=-(-clips // chunk),
                              peak_mib=round(torch.cuda.max_memory_allocated() / 2**20, 1))), flush=True)
        for k, xs in times.items():
            print(json.dumps(dict(config=f'sgn15_deployed_b{batch}', mode=args.mode, part=k,
                                  median_ms=round(statistics.median(xs), 4), n=len(xs))), flush=True)
        del model, opt, x
        torch.cuda.empty_cache()


def _event(torch):
    e = torch.cuda.Event(enable_timing=True)
    e.record()
    return e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--batches', default='1,64')
    ap.add_argument('--report', default=None, help='also write the report to this file')
    ap.add_argument('--child-timeout', type=float, default=300.0, help='seconds one child process may take')
    ap.add_argument('--worker', action='store_true', help=argparse.SUPPRESS)
    ap.add_argument('--mode', choices=MODES, default='fused', help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    lines = ['# ' + json.dumps(dict(joints=V, draws=S, seg=SEG, lr=LR, iters=args.iters, warmup=args.warmup,
                                    repeats=args.repeats))]
    print(lines[0], flush=True)
    runs, heads, peaks = {}, {}, {}
    for rep in range(args.repeats):
        for mode in MODES:
            cmd = [sys.executable, os.path.abspath(__file__), '--worker', '--mode', mode, '--iters', str(args.iters),
                   '--warmup', str(args.warmup), '--batches', args.batches]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.child_timeout)
            except subprocess.TimeoutExpired:
                raise SystemExit(f'{mode} run {rep} did not finish in {args.child_timeout:.0f} s; it was killed')
            if r.returncode != 0:
                raise SystemExit(f'{mode} run {rep} failed:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}')
            for line in r.stdout.splitlines():
                if not line.startswith('{'):
                    continue
                rec = json.loads(line)
                if 'losses' in rec:
                    heads.setdefault((rec['config'], mode), rec)
                    peaks.setdefault((rec['config'], mode), []).append(rec['peak_mib'])
                else:
                    runs.setdefault((rec['config'], mode, rec['part']), []).append(rec['median_ms'])
    for config in sorted({k[0] for k in heads}):
        f, t = heads[config, 'fused'], heads[config, 'tensor']
        lines.append(f'# {config}: {f["clips"]} clips per step; the tape of a fused step: {f["tape_mib_per_step"]} MiB written '
                     f'and read at least once, in {f["tape_chunks"]} chunk(s)')
        lines.append(f'# {config}: peak device memory of a child: fused {statistics.median(peaks[config, "fused"]):.1f} MiB, '
                     f'tensor {statistics.median(peaks[config, "tensor"]):.1f} MiB')
        lines.append(f'# {config}: loss of the first {len(f["losses"])} steps, fused | tensor')
        lines += [f'#   step {i:2d}: {a:.5f} | {b:.5f}' for i, (a, b) in enumerate(zip(f['losses'], t['losses']))]
        worst = max(abs(a - b) for a, b in zip(f['losses'], t['losses']))
        lines.append(f'#   largest difference {worst:.1e}')
    for (config, mode, part), xs in runs.items():
        lines.append(json.dumps(dict(config=config, mode=mode, part=part, median_ms=round(statistics.median(xs), 4),
                                     min_ms=round(min(xs), 4), max_ms=round(max(xs), 4), runs=len(xs))))
    for config in sorted({k[0] for k in runs}):
        f, t = (runs[config, m, 'end_to_end'] for m in MODES)
        apart = max(f) < min(t) or max(t) < min(f)
        lines.append(f'# {config}: one step end to end: fused {statistics.median(f):.3f} ms ({min(f):.3f}..{max(f):.3f}), '
                     f'tensor {statistics.median(t):.3f} ms ({min(t):.3f}..{max(t):.3f}); '
                     + ('the ranges of the runs do not overlap' if apart else
                        'the ranges of the runs overlap: no difference beyond the spread'))
    print('\n'.join(lines[1:]), flush=True)
    if args.report:
        with open(args.report, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
