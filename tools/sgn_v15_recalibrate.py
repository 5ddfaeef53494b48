"""What re-estimating SGN v15's six BatchNorms (``SGN.recalibrate_bn``: AdaBN, or after frozen-BatchNorm fine-tuning) costs
on the two routes of this commit:

    python tools/sgn_v15_recalibrate.py [--iters 30] [--warmup 10] [--repeats 3] [--out profiles/sgn_v15_recalibrate.txt]

Deployed shape: V = 15, seg = 20, 5 clips per window; both the deployed heads (8 x 16 ff 128 / 8 x 32 ff 256) and the
yaml's wide heads (1 x 512 ff 512 / 1 x 1024 ff 1024); 1 window (5 clips) and 64 windows (320 clips).  ``hip``:
``recalibrate_bn`` on the fused path (csrc/sgn_v15_stats.hip); ``tensor``: the same call with AGCN_SGN_HIP=0, the
tensor-code composition with its BatchNorms in batch mode and every dropout off.  End to end = the host clock around
``recalibrate_bn`` ending in a device synchronisation.  On the hip route each pass (the launches with their finalize) and
the folds are also timed by device events inside one call (``ops.SGN15_BNSTATS_MARK``).  A child reports the median over
--iters calls after --warmup; the parent the median and min..max of the --repeats children per route, each a fresh
process under its own time limit, the two routes alternating; it stops at the first child that fails.  No threshold: the
report says which route wins where.  The report is APPENDED to --out behind the lines that are not measurements.  Needs a
GPU."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from sgn_v15_bench import HEADS, S, SEG, V, WINDOWS, model_args  # noqa: E402

MODES = ('hip', 'tensor')
MARK = '# ---- measured by tools/sgn_v15_recalibrate.py ----'


def worker(args):
    import torch
    import bench
    import agcn_amd  # noqa: F401
    from agcn_amd import ops
    from model.sgn_v15 import SGN
    dev = torch.device('cuda:0')
    assert ops.sgn_hip_enabled() == (args.mode == 'hip')
    for heads, (sp, tp) in HEADS.items():
        model = SGN(**model_args(sp, tp))
        bench.randomize_like_training(model, 0)
        model = model.to(dev).eval()
        for windows in WINDOWS:
            torch.manual_seed(windows)
            x = torch.randn(windows * S, SEG, 3 * V, device=dev)
            ts, marks = [], {}
            for it in range(args.warmup + args.iters):
                before = ops.SGN_STATS['forward_tensor'], ops.SGN15_BNSTATS_STATS['frames_stats']
                events = []
                if args.mode == 'hip':
                    def mark(label):
                        e = torch.cuda.Event(enable_timing=True)
                        e.record()
                        events.append((label, e))
                    ops.SGN15_BNSTATS_MARK = mark
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                model.recalibrate_bn(x)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                ops.SGN15_BNSTATS_MARK = None
                ran = ops.SGN_STATS['forward_tensor'] - before[0], ops.SGN15_BNSTATS_STATS['frames_stats'] - before[1]
                assert ran == ((0, 2) if args.mode == 'hip' else (1, 0)), ran
                if it >= args.warmup:
                    ts.append((t1 - t0) * 1e3)
                    for (_, a), (label, b) in zip(events, events[1:]):
                        marks.setdefault(label, []).append(a.elapsed_time(b))
            var = float(model.get_submodule(ops.SGN15_BN_NAMES[-1]).running_var.mean())
            assert var == var, 'the running variance is not a number'
            rec = dict(heads=heads, windows=windows, clips=x.shape[0], mode=args.mode)
            print(json.dumps(dict(rec, part='end_to_end', median_ms=round(statistics.median(ts), 4))), flush=True)
            # 'fold' is recorded six times per call: the sum of the six
            folds = marks.pop('fold', None)
            if folds:
                per_call = [sum(folds[i:i + 6]) for i in range(0, len(folds), 6)]
                print(json.dumps(dict(rec, part='folds (6 per call)', median_ms=round(statistics.median(per_call), 4))), flush=True)
            for label, xs in marks.items():
                print(json.dumps(dict(rec, part=label, median_ms=round(statistics.median(xs), 4))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sgn_v15_recalibrate.txt'))
    ap.add_argument('--child-timeout', type=float, default=120.0, help='seconds one child process may take')
    ap.add_argument('--worker', action='store_true', help=argparse.SUPPRESS)
    ap.add_argument('--mode', choices=MODES, default='hip', help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('sgn_v15_recalibrate needs a GPU: there is nothing to measure without one')
    lines = [MARK, '# ' + json.dumps(dict(joints=V, seg=SEG, clips_per_window=S, iters=args.iters, warmup=args.warmup,
                                           repeats=args.repeats, device=torch.cuda.get_device_name(0)))]
    runs = {}
    for rep in range(args.repeats):
        for mode in MODES:
            cmd = [sys.executable, os.path.abspath(__file__), '--worker', '--mode', mode, '--iters', str(args.iters),
                   '--warmup', str(args.warmup)]
            env = dict(os.environ, AGCN_SGN_HIP='1' if mode == 'hip' else '0')
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.child_timeout, env=env)
            except subprocess.TimeoutExpired:
                raise SystemExit(f'{mode} run {rep} did not finish in {args.child_timeout:.0f} s; it was killed')
            if r.returncode != 0:
                raise SystemExit(f'{mode} run {rep} failed with status {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}')
            for line in r.stdout.splitlines():
                if line.startswith('{'):
                    rec = json.loads(line)
                    runs.setdefault((rec['heads'], rec['windows'], rec['clips'], mode, rec['part']), []).append(rec['median_ms'])
    for (heads, windows, clips, mode, part), xs in runs.items():
        lines.append(json.dumps(dict(heads=heads, windows=windows, clips=clips, mode=mode, part=part,
                                     median_ms=round(statistics.median(xs), 4), min_ms=round(min(xs), 4),
                                     max_ms=round(max(xs), 4), runs=len(xs))))
    for heads, windows in sorted({k[:2] for k in runs}):
        h, t = (next(v for k, v in runs.items() if k[:2] == (heads, windows) and k[3:] == (m, 'end_to_end')) for m in MODES)
        apart = max(h) < min(t) or max(t) < min(h)
        win = 'hip' if statistics.median(h) < statistics.median(t) else 'tensor'
        lines.append(f'# {heads} heads, {windows} window(s): recalibrate_bn end to end: hip {statistics.median(h):.3f} ms '
                     f'({min(h):.3f}..{max(h):.3f}), tensor {statistics.median(t):.3f} ms ({min(t):.3f}..{max(t):.3f}), '
                     f'tensor / hip = {statistics.median(t) / statistics.median(h):.2f}: '
                     + (f'{win} wins, the ranges of the runs do not overlap' if apart else
                        'the ranges of the runs overlap: no difference beyond the spread'))
    print('\n'.join(lines), flush=True)
    kept = []
    if os.path.exists(args.out):
        with open(args.out) as f:
            text = f.read()
        kept = text.split(MARK)[0].rstrip('\n').split('\n') if text.strip() else []
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(kept + ([''] if kept else []) + lines) + '\n')


if __name__ == '__main__':
    main()
