"""The bone / motion streams (ops.skeleton_streams forward, ops.streams_bwd) on the HIP route against the tensor-code route
(AGCN_STREAM_HIP=0) at (64, 3, 300, 25, 2) and (128, 3, 300, 18, 2), and one two-stream online predict against two
single-stream predicts.
    python tools/bench_streams.py [--processes 5] [--calls 50] [--out profiles/streams.txt]
Every figure is the median over --processes FRESH processes (this one starts them one after the other and never opens
the GPU itself) of the per-process median over --calls device-event-timed calls after a warm-up; the predicts are timed
with a host clock around predict(), which ends in its one synchronising copy.  Bytes = what the pass has to move through
HBM once: the forward reads x and writes three outputs (4 tensors), the backward reads four cotangents and writes dx (5
tensors); the neighbour reads hit cache.  The fraction of peak is against the 8.0 TB/s HBM3E specification."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(64, 3, 300, 25, 2), (128, 3, 300, 18, 2)]
HBM_PEAK = 8.0e12
DERIVED = ('bone', 'joint_motion', 'bone_motion')


def timed(fn, calls):
    import torch
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) for a, b in ev)


def child_streams(shape, calls):
    import torch
    import agcn_amd  # noqa: F401
    from agcn_amd import ops
    from agcn_amd.graph import kinetics, ntu_rgb_d
    dev = torch.device('cuda:0')
    parent = {25: ntu_rgb_d, 18: kinetics}[shape[3]].bone_parents
    g = torch.Generator(dev).manual_seed(0)
    x = torch.randn(shape, device=dev, generator=g)
    cot = {s: torch.randn(shape, device=dev, generator=g) for s in ops.STREAMS}
    fwd = lambda: ops.skeleton_streams(x, parent, DERIVED)          # noqa: E731
    bwd = lambda: ops.streams_bwd(cot, parent, (1.0, 0.5, -2.0, 3.0))  # noqa: E731
    with torch.no_grad():
        for fn in (fwd, bwd):
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        return {'fwd_ms': timed(fwd, calls), 'bwd_ms': timed(bwd, calls), 'hip': ops.stream_hip_enabled()}


def child_predict(calls):
    import numpy as np
    import torch
    import agcn_amd  # noqa: F401
    from agcn_amd.model.agcn import Model
    from agcn_amd.online import ActionRecognition
    nets = []
    for seed in (1, 2):
        torch.manual_seed(seed)
        nets.append(Model(num_class=60, num_point=25, num_person=2, graph='graph.ntu_rgb_d.Graph'))
    kw = dict(max_frame=300, max_num_skeleton=4, max_num_skeleton_true=2, num_joint=25)
    two = ActionRecognition(streams=[('joint', nets[0]), ('bone', nets[1])], alpha=(1.0, 1.0), **kw)
    singles = [ActionRecognition(model=n, **kw) for n in nets]
    rng = np.random.default_rng(0)
    for _ in range(300):
        f = np.zeros((4, 1, 25, 3), dtype=np.float32)
        f[:2, 0] = rng.standard_normal((2, 25, 3)) * 0.3 + (0.5, 2.3, 0.9)
        for r in [two] + singles:
            r.append_data(f)

    def clock(fn):
        for _ in range(3):
            fn()
        ts = []
        for _ in range(calls):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts)
    return {'two_stream_ms': clock(two.predict), 'two_singles_ms': clock(lambda: [r.predict() for r in singles])}


def spawn(args, env_extra, processes):
    """-> the per-process result dicts of `processes` fresh processes, run one after the other"""
    out = []
    for _ in range(processes):
        env = dict(os.environ, **env_extra)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child'] + args, env=env, capture_output=True,
                           text=True)
        if r.returncode != 0:
            raise RuntimeError(f'child {args} failed ({r.returncode}):\n{r.stderr[-3000:]}')
        out.append(json.loads(r.stdout.strip().splitlines()[-1]))
    return out


def med(results, key):
    vals = [r[key] for r in results]
    return statistics.median(vals), min(vals), max(vals)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--processes', type=int, default=5)
    ap.add_argument('--calls', type=int, default=50)
    ap.add_argument('--out', default=None)
    ap.add_argument('--child', nargs='+', default=None)
    args = ap.parse_args()
    if args.child:
        if args.child[0] == 'predict':
            res = child_predict(int(args.child[1]))
        else:
            res = child_streams(tuple(int(v) for v in args.child[1:6]), int(args.child[6]))
        print(json.dumps(res))
        return
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say(f'bone / motion streams: median of {args.processes} fresh processes, each the median of {args.calls} calls')
    for shape in SHAPES:
        tensor = 4
        for v in shape:
            tensor *= v
        res = {}
        for route, env in (('hip', {'AGCN_STREAM_HIP': '1'}), ('tensor', {'AGCN_STREAM_HIP': '0'})):
            rs = spawn(['streams'] + [str(v) for v in shape] + [str(args.calls)], env, args.processes)
            assert all(r['hip'] == (route == 'hip') for r in rs)
            res[route] = rs
        for key, ntens, what in (('fwd_ms', 4, 'forward  (3 streams)'), ('bwd_ms', 5, 'backward (4 cotangents)')):
            h, hlo, hhi = med(res['hip'], key)
            t, tlo, thi = med(res['tensor'], key)
            moved = ntens * tensor
            say(f'{shape} {what}: hip {h:.4f} ms (min {hlo:.4f} max {hhi:.4f}), {moved / 1e6:.1f} MB moved, '
                f'{moved / (h * 1e-3) / 1e12:.2f} TB/s = {100 * moved / (h * 1e-3) / HBM_PEAK:.0f}% of HBM peak; '
                f'tensor code {t:.4f} ms (min {tlo:.4f} max {thi:.4f}); '
                f'{"HIP" if h < t else "tensor code"} wins, x{max(h, t) / min(h, t):.2f}')
    rs = spawn(['predict', str(max(5, args.calls // 5))], {}, args.processes)
    a, alo, ahi = med(rs, 'two_stream_ms')
    b, blo, bhi = med(rs, 'two_singles_ms')
    say(f'online, window 300, AGCN joint + bone: one two-stream predict {a:.3f} ms (min {alo:.3f} max {ahi:.3f}); two '
        f'single-stream predicts {b:.3f} ms (min {blo:.3f} max {bhi:.3f}); '
        f'{"the two-stream predict" if a < b else "two single predicts"} wins, x{max(a, b) / min(a, b):.2f}')
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
