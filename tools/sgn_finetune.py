"""Frozen-BatchNorm fine-tuning of SGN at the deployed shape (V = 15, window 300, two selected bodies, S = 5 draws,
seg = 20), and what a step costs on the two routes of this commit:
    python tools/sgn_finetune.py [--iters 30] [--warmup 10] [--repeats 3] [--batches 1,64] [--report FILE]
    python tools/sgn_finetune.py --data windows.npy --labels labels.npy [--weights IN.pt] --out OUT.pt [--steps 100]
A step: ``ops.prenorm`` -> ``ops.sgn_sample`` with fresh draws -> SGN in eval mode (BatchNorm on its running statistics)
-> cross-entropy -> ``backward()`` -> ``torch.optim.Adam.step()``.  ``fused`` sets ``SGN.fused_finetune``: the fused
forward, the taping backward kernels (csrc/sgn_bwd.hip), the tape reductions of csrc/sgn_wgrad.hip, torch autograd only through the
fold of the weight images.  ``tensor`` leaves the flag off: the tensor-code composition under torch autograd.  Model,
windows, labels and draws come from fixed seeds, so both routes take the same steps and their losses are printed side by
side.  Each repeat of each route runs in a fresh child process, alternating.

Per part, by device events: data (select + normalise, draws, sample), forward, loss + backward, optimiser.  End to end:
the host clock around a step that ends in the copy of the loss.  A child reports the median over --iters steps after
--warmup; the parent the median and the min..max of the --repeats children.  There is no threshold: the report says what
came out, with the size of the tape a step writes and reads.  Needs a GPU.

With --data the tool fine-tunes for real on the fused route: windows.npy holds normalised windows (N, 3, T, V, 2) in
``ops.prenorm``'s output layout, labels.npy (N,) class indices; --weights a reference-format state_dict to start from;
the fine-tuned state_dict (the reference's names) is saved to --out."""
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
MODES = ('fused', 'tensor')
PARTS = ('data', 'forward', 'loss+backward', 'optimiser')
LOSSES = 20
LR = 1e-4


def step(model, opt, win, labels, seed, ev=None):
    """One fine-tuning step on normalised windows win (N, 3, T, V, 2) -> the loss (a device scalar)."""
    import torch
    from agcn_amd import ops
    N = win.shape[0]
    torch.manual_seed(seed)                                  # fresh draws every step, the same on both routes
    with torch.no_grad():
        rows, _ = ops.sgn_sample(win, ops.sgn_draws(N, S, SEG, win.device), SEG)
    x = rows.view(N * S, SEG, -1)
    if ev:
        ev[1].record()
    logits, _ = model(x)
    if ev:
        ev[2].record()
    loss = torch.nn.functional.cross_entropy(logits, labels.repeat_interleave(S))
    opt.zero_grad(set_to_none=True)
    loss.backward()
    if ev:
        ev[3].record()
    opt.step()
    if ev:
        ev[4].record()
    return loss


def worker(args):
    import numpy as np
    import torch
    import online_bench as ob
    import sgn_bench as sb
    from agcn_amd import ops
    dev = torch.device('cuda:0')
    for batch in (int(b) for b in args.batches.split(',')):
        torch.manual_seed(0)
        model = sb.build_sgn().to(dev).eval()
        model.fused_finetune = args.mode == 'fused'
        opt = torch.optim.Adam(model.parameters(), lr=LR)
        stream = ob.make_stream(FRAMES + batch, V)
        raw = torch.stack([torch.from_numpy(stream[b:b + FRAMES, :, 0]).transpose(0, 1) for b in range(batch)])
        raw = raw.contiguous().to(dev)             # (N, tracked, T, V, 3)
        labels = torch.from_numpy(np.random.default_rng(2000 + batch).integers(0, NUM_CLASS, batch)).to(dev)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
        times = {k: [] for k in PARTS} | {'end_to_end': []}
        losses = []
        for it in range(args.warmup + args.iters):
            before = ops.SGN_STATS['forward_tensor'], dict(ops.SGN_WGRAD_STATS)
            t0 = time.perf_counter()
            ev[0].record()
            with torch.no_grad():
                win, _, _ = ops.prenorm(raw, num_select=ob.SELECTED, zaxis=ZAXIS, xaxis=XAXIS)
            loss = float(step(model, opt, win, labels, 5000 + it, ev))       # the synchronising copy of the loss
            t1 = time.perf_counter()
            ev[4].synchronize()
            tape = ops.SGN_WGRAD_STATS['frames_wgrad'] - before[1]['frames_wgrad']
            assert (ops.SGN_STATS['forward_tensor'] - before[0], tape > 0) == ((0, True) if args.mode == 'fused' else (1, False))
            assert loss == loss, 'the loss is not a number'
            if it < LOSSES:
                losses.append(round(loss, 5))
            if it >= args.warmup:
                for k, a, b in zip(PARTS, ev[:-1], ev[1:]):
                    times[k].append(a.elapsed_time(b))
                times['end_to_end'].append((t1 - t0) * 1e3)
        clips = batch * S
        L = ops._L()
        tape_mb = 4 * (L.agcn_sgn_frames_tape_floats(clips, SEG, V) + L.agcn_sgn_clip_tape_floats(clips, SEG, NUM_CLASS)) / 2**20
        chunk = ops.sgn_tape_chunk(clips, SEG, V, NUM_CLASS, ops.SGN_MAX_TAPE_BYTES)
        print(json.dumps(dict(config=f'sgn_v15_b{batch}', mode=args.mode, losses=losses, clips=clips,
                              tape_mib_per_step=round(tape_mb, 1), tape_chunks=-(-clips // chunk))), flush=True)
        for k, xs in times.items():
            print(json.dumps(dict(config=f'sgn_v15_b{batch}', mode=args.mode, part=k,
                                  median_ms=round(statistics.median(xs), 4), n=len(xs))), flush=True)


def finetune(args):
    import numpy as np
    import torch
    import agcn_amd  # noqa: F401
    from model.sgn import SGN
    dev = torch.device('cuda:0')
    win = torch.from_numpy(np.load(args.data).astype(np.float32)).to(dev)
    labels = torch.from_numpy(np.load(args.labels).astype(np.int64)).to(dev)
    if win.dim() != 5 or win.shape[1] != 3 or win.shape[4] != 2 or labels.shape != (win.shape[0],):
        raise SystemExit(f'--data holds (N, 3, T, V, 2) and --labels (N,), got {tuple(win.shape)} and {tuple(labels.shape)}')
    model = SGN(num_class=args.num_class, num_point=win.shape[3], seg=SEG)
    if args.weights:
        model.load_state_dict(torch.load(args.weights, map_location='cpu'))
    model = model.to(dev).eval()
    model.fused_finetune = True
    opt = torch.optim.Adam(model.parameters(), lr=args.lr)
    for it in range(args.steps):
        idx = torch.randperm(win.shape[0], generator=torch.Generator().manual_seed(it))[:args.batch].to(dev)
        loss = float(step(model, opt, win[idx].contiguous(), labels[idx], 5000 + it))
        if it % 10 == 0 or it == args.steps - 1:
            print(f'step {it}: loss {loss:.5f}', flush=True)
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
    ap.add_argument('--labels', default=None)
    ap.add_argument('--weights', default=None)
    ap.add_argument('--out', default=None, help='with --data: where the fine-tuned state_dict goes')
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--lr', type=float, default=LR)
    ap.add_argument('--num-class', type=int, default=NUM_CLASS)
    ap.add_argument('--worker', action='store_true', help=argparse.SUPPRESS)
    ap.add_argument('--mode', choices=MODES, default='fused', help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    if args.data:
        if not (args.labels and args.out):
            raise SystemExit('--data needs --labels and --out')
        return finetune(args)
    lines = ['# ' + json.dumps(dict(joints=V, frames=FRAMES, draws=S, seg=SEG, lr=LR, iters=args.iters, warmup=args.warmup,
                                    repeats=args.repeats))]
    print(lines[0], flush=True)
    runs, heads = {}, {}
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
                else:
                    runs.setdefault((rec['config'], mode, rec['part']), []).append(rec['median_ms'])
    for config in sorted({k[0] for k in heads}):
        f, t = heads[config, 'fused'], heads[config, 'tensor']
        lines.append(f'# {config}: {f["clips"]} clips per step; the tape of a fused step: {f["tape_mib_per_step"]} MiB written '
                     f'and read at least once, in {f["tape_chunks"]} chunk(s)')
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
