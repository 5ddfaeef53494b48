"""What an SGN training step and an evaluation batch cost with their data path, at the NTU shape (V = 25, T = 300, two
bodies, seg = 20, batch 64), on seeded synthetic data:
    python tools/sgn_train_bench.py [--iters 30] [--warmup 10] [--repeats 3] [--report FILE]
A training step, as ``sgn_processor.SGNProcessor.train_step`` runs it: collate (draws, angles, ``ops.sgn_collate`` by index
from the dataset on the device, rotation theta 0.5) -> SGN in train mode (the tensor-code composition) -> label-smoothing
loss 0.1 -> ``backward()`` -> clip_grad_norm_ 1.0 -> ``torch.optim.Adam.step()``.  Three routes, each repeat of each in a
fresh child process under a time limit, alternating:
  device   the collate is the one HIP launch
  host     the same collate by ``ops.sgn_collate_ref`` (numpy, one process) on the host copy of the dataset, then the H2D
           copy of the batch; the rest of the step is the same
  eval     evaluation at multi_test = 5: collate of 64 samples x 5 draws -> the fused HIP forward on 320 clips -> mean
Per part, by device events: collate, forward, loss + backward (with the clip), optimiser.  On the host route the collate
interval is the time the device waits for the host: the events bracket the numpy work and the copy.  End to end: the host
clock around a step that ends in the copy of the loss.  A child reports the median over --iters steps after --warmup; the
parent the median and the min..max of the --repeats children.  The comparison is within one commit.  There is no
threshold: the report says what came out.  Needs a GPU."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

V, FRAMES, SEG, BATCH, S_EVAL, NUM_CLASS, POOL = 25, 300, 20, 64, 5, 60, 256
THETA, SMOOTHING, LR, WD = 0.5, 0.1, 1e-3, 1e-4
MODES = ('device', 'host', 'eval')
PARTS = {'device': ('collate', 'forward', 'loss+backward', 'optimiser'),
         'host': ('collate', 'forward', 'loss+backward', 'optimiser'), 'eval': ('collate', 'forward')}


def dataset():
    """(POOL, 3, T, V, 2) fp32 and labels: clips of 60..300 frames followed by the dataset's zero padding, the second
    body absent in half of them."""
    import numpy as np
    g = np.random.default_rng(0)
    data = g.standard_normal((POOL, 3, FRAMES, V, 2)).astype(np.float32)
    for i, n in enumerate(g.integers(60, FRAMES + 1, size=POOL)):
        data[i, :, n:] = 0
        if i % 2:
            data[i, ..., 1] = 0
    return data, g.integers(0, NUM_CLASS, size=POOL).astype(np.int64)


def worker(args):
    import torch
    import agcn_amd  # noqa: F401
    from agcn_amd import ops
    from agcn_amd.model.sgn import SGN
    from agcn_amd.sgn_processor import label_smoothing_loss
    dev = torch.device('cuda:0')
    mode = args.mode
    torch.manual_seed(0)
    data, label = dataset()
    host_pool = torch.from_numpy(data)
    pool, labels = host_pool.to(dev), torch.from_numpy(label).to(dev)
    model = SGN(num_class=NUM_CLASS, num_point=V, seg=SEG).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=LR, weight_decay=WD)
    S = S_EVAL if mode == 'eval' else 1
    parts = PARTS[mode]
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(parts) + 1)]
    times = {k: [] for k in parts} | {'end_to_end': []}
    for it in range(args.warmup + args.iters):
        order = torch.randperm(POOL, generator=torch.Generator().manual_seed(it))[:BATCH]
        torch.manual_seed(5000 + it)
        tensor_before = ops.SGN_STATS['forward_tensor']
        t0 = time.perf_counter()
        ev[0].record()
        if mode == 'host':
            r = torch.randint(0, 1 << 32, (BATCH, S, SEG), dtype=torch.int64).to(torch.int32)
            angles = torch.empty((BATCH, 3)).uniform_(-THETA, THETA)
            x, _, _ = ops.sgn_collate_ref(host_pool, r, SEG, index=order, angles=angles)
            x, y = x.to(dev), labels[order.to(dev)]
        else:
            index = order.to(dev)
            r = ops.sgn_draws(BATCH, S, SEG, dev)
            angles = ops.sgn_rotation_angles(BATCH, THETA, dev) if mode == 'device' else None
            x, _, _ = ops.sgn_collate(pool, r, SEG, index=index, angles=angles)
            y = labels[index]
        x = x.view(BATCH * S, SEG, 3 * V)
        ev[1].record()
        if mode == 'eval':
            model.eval()
            with torch.no_grad():
                logits, _ = model(x)
                out = logits.view(-1, S, NUM_CLASS).mean(1)
            ev[2].record()
            done = float(out.sum())                                   # the synchronising copy
            assert ops.SGN_STATS['forward_tensor'] == tensor_before, 'evaluation left the fused forward'
        else:
            model.train()
            logits, _ = model(x)
            ev[2].record()
            loss = label_smoothing_loss(logits, y, SMOOTHING)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            torch.nn.utils.clip_grad_norm_(model.parameters(), 1.0)
            ev[3].record()
            opt.step()
            ev[4].record()
            done = float(loss)                                        # the synchronising copy of the loss
        t1 = time.perf_counter()
        ev[-1].synchronize()
        assert done == done, 'not a number'
        if it >= args.warmup:
            for k, a, b in zip(parts, ev[:-1], ev[1:]):
                times[k].append(a.elapsed_time(b))
            times['end_to_end'].append((t1 - t0) * 1e3)
    for k, xs in times.items():
        print(json.dumps(dict(mode=mode, part=k, median_ms=round(statistics.median(xs), 4), n=len(xs))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--report', default=None, help='also write the report to this file')
    ap.add_argument('--child-timeout', type=float, default=240.0, help='seconds one child process may take')
    ap.add_argument('--worker', action='store_true', help=argparse.SUPPRESS)
    ap.add_argument('--mode', choices=MODES, default='device', help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    lines = ['# ' + json.dumps(dict(joints=V, frames=FRAMES, seg=SEG, batch=BATCH, multi_test=S_EVAL, pool=POOL, theta=THETA,
                                    smoothing=SMOOTHING, iters=args.iters, warmup=args.warmup, repeats=args.repeats))]
    print(lines[0], flush=True)
    runs = {}
    for rep in range(args.repeats):
        for mode in MODES:
            cmd = [sys.executable, os.path.abspath(__file__), '--worker', '--mode', mode, '--iters', str(args.iters),
                   '--warmup', str(args.warmup)]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.child_timeout)
            except subprocess.TimeoutExpired:
                raise SystemExit(f'{mode} run {rep} did not finish in {args.child_timeout:.0f} s; it was killed')
            if r.returncode != 0:
                raise SystemExit(f'{mode} run {rep} failed:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}')
            for line in r.stdout.splitlines():
                if line.startswith('{'):
                    rec = json.loads(line)
                    runs.setdefault((mode, rec['part']), []).append(rec['median_ms'])
    for (mode, part), xs in runs.items():
        lines.append(json.dumps(dict(mode=mode, part=part, median_ms=round(statistics.median(xs), 4),
                                     min_ms=round(min(xs), 4), max_ms=round(max(xs), 4), runs=len(xs))))

    def spread(key):
        xs = runs[key]
        return f'{statistics.median(xs):.3f} ms ({min(xs):.3f}..{max(xs):.3f})'
    d, h = runs['device', 'end_to_end'], runs['host', 'end_to_end']
    apart = max(d) < min(h) or max(h) < min(d)
    lines.append(f'# training step of {BATCH} clips end to end: device collate {spread(("device", "end_to_end"))}, host '
                 f'collate {spread(("host", "end_to_end"))}; '
                 + ('the ranges of the runs do not overlap' if apart else
                    'the ranges of the runs overlap: no difference beyond the spread'))
    lines.append(f'# collate alone: device {spread(("device", "collate"))}, host with its H2D copy '
                 f'{spread(("host", "collate"))}')
    e = statistics.median(runs['eval', 'end_to_end'])
    lines.append(f'# evaluation at multi_test = {S_EVAL}: {spread(("eval", "end_to_end"))} per batch of {BATCH} samples '
                 f'({BATCH * S_EVAL} clips): {BATCH / e * 1e3:.0f} samples/s')
    print('\n'.join(lines[1:]), flush=True)
    if args.report:
        with open(args.report, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
