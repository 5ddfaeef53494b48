"""Latency and throughput of the SGN v15 eval forward at the online recogniser's shape (V = 15, seg = 20, multi_test 5):
one window (5 clips) and 64 windows (320 clips), for the deployed heads (8 x 16, ff 128 / 8 x 32, ff 256) and the
experiment yaml's heads (1 x 512, ff 512 / 1 x 1024, ff 1024).
    python tools/sgn_v15_bench.py [--rounds 5] [--iters 200] [--warmup 30] [--out profiles/sgn_v15.txt]
Two routes of the same commit are compared: ``hip`` (the two fused launches, csrc/sgn_v15.hip) and ``tensor`` (the same
call with AGCN_SGN_HIP=0: the tensor-code composition on vendor GEMMs).  Every round starts one fresh child process per
route, alternating, so that neither route inherits the other's caches or clocks; a child times --iters forwards after
--warmup by device events and reports its median.  The table gives, per figure, the median over the rounds and their
min..max.  ``hip`` is split into images (one uncached fold of the parameters into the two weight images, paid once per
parameter change, not per forward), the frames launch and the clip launch; ``forward`` is the whole ``model(x)`` with the
images cached.  Needs a GPU."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

V, SEG, S = 15, 20, 5
HEADS = {'deployed': ((8, 16, 128), (8, 32, 256)), 'yaml': ((1, 512, 512), (1, 1024, 1024))}
WINDOWS = (1, 64)


def model_args(spatial, temporal):
    """The experiment yaml's model arguments at the recogniser's shape with the given (heads, d_head, ff) per block."""
    def mha(d_model, heads, d_head, ff, ff_out):
        return dict(d_model=[d_model], nhead=[heads], d_head=[d_head], dim_feedforward=[ff], dim_feedforward_output=[ff_out],
                    dropout=0.1, activation='relu', num_layers=1, norm='bn', global_norm=False)
    return dict(num_class=60, num_point=V, num_segment=SEG, in_channels=3, bias=1, norm_type='bn', act_type='relu',
                spatial_mha_kwargs=mha(128, *spatial, 256), temporal_mha_kwargs=mha(256, *temporal, 512))


def child(args):
    import torch
    import bench
    import agcn_amd  # noqa: F401
    from agcn_amd import ops
    from model.sgn_v15 import SGN
    dev = torch.device('cuda:0')
    hip = ops.sgn_hip_enabled()

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        xs = []
        for it in range(args.warmup + args.iters):
            a.record()
            fn()
            b.record()
            b.synchronize()
            if it >= args.warmup:
                xs.append(a.elapsed_time(b))
        return statistics.median(xs)

    for name, (sp, tp) in HEADS.items():
        model = SGN(**model_args(sp, tp))
        bench.randomize_like_training(model, 0)
        model = model.to(dev).eval()
        for windows in WINDOWS:
            n = windows * S
            x = torch.randn(n, SEG, 3 * V, device=dev)
            out = dict(heads=name, windows=windows, clips=n, route='hip' if hip else 'tensor')
            with torch.no_grad():
                before = ops.SGN_STATS['forward_tensor']
                out['forward'] = timed(lambda: model(x))
                assert (ops.SGN_STATS['forward_tensor'] == before) == hip, 'the route is not the one asked for'
                if hip:
                    wf, wc, _, _ = model._images()
                    feat, _ = ops.sgn15_frames(x, wf, V, *sp)
                    out['frames'] = timed(lambda: ops.sgn15_frames(x, wf, V, *sp))
                    out['clip'] = timed(lambda: ops.sgn15_clip(feat, wc, 60, *tp))
                    if windows == 1:
                        def fold():
                            model._infer_cache.clear()
                            model._images()
                        out['images'] = timed(fold)
            print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=30)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sgn_v15.txt'))
    ap.add_argument('--child', action='store_true', help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('sgn_v15_bench needs a GPU: there is nothing to measure without one')
    rows = {}
    for rnd in range(args.rounds):
        for route in ('hip', 'tensor'):
            env = dict(os.environ, AGCN_SGN_HIP='1' if route == 'hip' else '0')
            r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', '--iters', str(args.iters), '--warmup',
                                str(args.warmup)], env=env, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                raise SystemExit(f'round {rnd}, route {route}: the child ended with {r.returncode}\n{r.stderr[-2000:]}')
            for line in r.stdout.splitlines():
                if line.startswith('{'):
                    d = json.loads(line)
                    for k in ('forward', 'frames', 'clip', 'images'):
                        if k in d:
                            rows.setdefault((d['heads'], d['windows'], d['route'], k), []).append(d[k])
    lines = ['# ' + json.dumps(dict(device=torch.cuda.get_device_name(0), joints=V, seg=SEG, draws=S, rounds=args.rounds,
                                    iters=args.iters, warmup=args.warmup)),
             '# ms per call: median over the rounds (min..max); one fresh process per route and round, alternating',
             f'{"heads":9} {"windows":>7} {"route":7} {"figure":8} {"median":>9} {"min":>9} {"max":>9}']
    for (heads, windows, route, k), xs in sorted(rows.items()):
        lines.append(f'{heads:9} {windows:7d} {route:7} {k:8} {statistics.median(xs):9.4f} {min(xs):9.4f} {max(xs):9.4f}')
    for heads in HEADS:
        for windows in WINDOWS:
            h = statistics.median(rows[(heads, windows, 'hip', 'forward')])
            t = statistics.median(rows[(heads, windows, 'tensor', 'forward')])
            lines.append(f'# {heads}, {windows} window(s): hip {h:.4f} ms, tensor {t:.4f} ms: the tensor route takes '
                         f'{t / h:.2f}x the hip time ({windows / h * 1e3:.0f} vs {windows / t * 1e3:.0f} windows/s)')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args.rounds < 5 or args.iters < 200:
        print('# fewer than 5 rounds of 200 timed forwards: a rehearsal, not a measurement')
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
