"""What asking an SGN v15 recogniser "why" costs at the online shape (V = 15, window 300, two bodies, multi_test 5, seg 20):
``predict`` alone and ``predict`` + ``explain`` (online._Recogniser) per call, for one window and for 64 windows, for the
deployed heads (8 x 16, ff 128 / 8 x 32, ff 256) and the experiment yaml's heads (1 x 512, ff 512 / 1 x 1024, ff 1024).
    python tools/sgn_v15_saliency.py [--rounds 5] [--iters 200] [--warmup 30] [--out profiles/sgn_v15_grad.txt]
Two routes of ``SGN.input_gradient`` are compared: ``hip`` (``fused_input_gradient = True``: the two forward launches and
the HIP backward of csrc/sgn_v15_bwd.hip) and ``composition`` (the flag off: the tensor-code composition under torch
autograd, the only route before the HIP backward existed).  The prediction itself is the fused forward on both.  Every
round starts one fresh child process per route, alternating; a child times --iters calls after --warmup (device events
around the whole call, which ends in its synchronising copy) and reports its median; the table gives the median over the
rounds and their min..max.  ``hip`` is also split into clip_bwd / frames_bwd / sample_bwd.  Both routes explain the same
windows with the same draws and weights; each child reports where its largest saliency lies and the report shows the two
side by side (tests/test_gpu_sgn_v15_grad.py compares whole maps).  Needs a GPU."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from sgn_v15_bench import HEADS, S, SEG, V, WINDOWS, model_args  # noqa: E402

FRAMES = 300
ROUTES = ('hip', 'composition')
FIGURES = ('predict', 'predict+explain', 'explain', 'clip_bwd', 'frames_bwd', 'sample_bwd')


def child(args):
    import numpy as np
    import torch
    import agcn_amd  # noqa: F401
    from agcn_amd import online, ops
    from model.sgn_v15 import SGN
    dev = torch.device('cuda:0')
    hip = args.route == 'hip'

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
        torch.manual_seed(0)                       # the model's initialisation: the same weights in every child
        model = SGN(**model_args(sp, tp))
        model.fused_input_gradient = hip
        rec = online._Recogniser(model, max_frame=FRAMES, max_num_skeleton=4, max_num_skeleton_true=2, num_joint=V,
                                 sgn_preprocess=True, multi_test=S)
        for windows in WINDOWS:
            g = torch.Generator().manual_seed(100 + windows)
            rec.window = torch.randn(windows, 3, FRAMES, V, 2, generator=g).to(dev)
            draws = np.random.default_rng(windows).integers(0, 1 << 32, (windows, S, SEG), dtype=np.uint64).astype(np.uint32)
            draws = torch.from_numpy(draws.view(np.int32)).to(dev)

            def predict():
                _, scores, label = rec.forward(rec.window, draws)
                return torch.cat((scores, label.to(scores.dtype).unsqueeze(1)), 1).cpu()

            def both():
                predict()
                return rec.explain()

            out = dict(heads=name, windows=windows, route=args.route)
            tensor, bwd = ops.SGN_STATS['forward_tensor'], dict(ops.SGN15_BWD_STATS)
            sal, classes = both()
            assert (ops.SGN_STATS['forward_tensor'] == tensor) == hip, 'the route is not the one asked for'
            assert (ops.SGN15_BWD_STATS['frames_bwd'] == bwd['frames_bwd'] + 1) == hip
            assert np.isfinite(sal).all() and sal.max() > 0
            out['top'] = [int(i) for i in np.unravel_index(int(sal.argmax()), sal.shape)]
            out['max'] = float(sal.max())
            out['predict'] = timed(predict)
            out['predict+explain'] = timed(both)
            out['explain'] = timed(rec.explain)
            if hip:
                with torch.no_grad():
                    wf, wc, _, _ = model._images()
                    wf_t, wc_t = model._images_t()
                    rows, _ = ops.sgn_sample(rec.window, rec.draws, SEG)
                    x = rows.view(windows * S, SEG, -1)
                    feat, _ = ops.sgn15_frames(x, wf, V, *sp)
                    cot = torch.randn(windows * S, 60, device=dev)
                    dfeat = ops.sgn15_clip_bwd(feat, wc, wc_t, cot, *tp)
                    dx = ops.sgn15_frames_bwd(x, wf, wf_t, dfeat, V, *sp)
                    out['clip_bwd'] = timed(lambda: ops.sgn15_clip_bwd(feat, wc, wc_t, cot, *tp))
                    out['frames_bwd'] = timed(lambda: ops.sgn15_frames_bwd(x, wf, wf_t, dfeat, V, *sp))
                    out['sample_bwd'] = timed(lambda: ops.sgn_sample_bwd(rec.window, rec.draws,
                                                                         dx.view(windows, S, SEG, -1), SEG))
            print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=30)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sgn_v15_grad.txt'))
    ap.add_argument('--child-timeout', type=float, default=600.0)
    ap.add_argument('--child', action='store_true', help=argparse.SUPPRESS)
    ap.add_argument('--route', default='hip', help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('sgn_v15_saliency needs a GPU: there is nothing to measure without one')
    rows, tops = {}, {}
    for rnd in range(args.rounds):
        for route in ROUTES:
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', '--route', route, '--iters',
                                    str(args.iters), '--warmup', str(args.warmup)], capture_output=True, text=True,
                                   timeout=args.child_timeout)
            except subprocess.TimeoutExpired:
                raise SystemExit(f'round {rnd}, route {route}: the child did not finish in {args.child_timeout:.0f} s')
            if r.returncode != 0:
                raise SystemExit(f'round {rnd}, route {route}: the child ended with {r.returncode}\n{r.stderr[-2000:]}')
            for line in r.stdout.splitlines():
                if line.startswith('{'):
                    d = json.loads(line)
                    tops[d['heads'], d['windows'], d['route']] = (d['top'], d['max'])
                    for k in FIGURES:
                        if k in d:
                            rows.setdefault((d['heads'], d['windows'], d['route'], k), []).append(d[k])
    lines = ['# ' + json.dumps(dict(device=torch.cuda.get_device_name(0), joints=V, frames=FRAMES, seg=SEG, draws=S,
                                    rounds=args.rounds, iters=args.iters, warmup=args.warmup)),
             '# ms per call: median over the rounds (min..max); one fresh process per route and round, alternating',
             f'{"heads":9} {"windows":>7} {"route":12} {"figure":16} {"median":>9} {"min":>9} {"max":>9}']
    for (heads, windows, route, k), xs in sorted(rows.items()):
        lines.append(f'{heads:9} {windows:7d} {route:12} {k:16} {statistics.median(xs):9.4f} {min(xs):9.4f} {max(xs):9.4f}')
    for heads in HEADS:
        for windows in WINDOWS:
            (ht, hm), (ct, cm) = (tops[heads, windows, r] for r in ROUTES)
            lines.append(f'# {heads}, {windows} window(s): the largest saliency is at {ht} ({hm:.6g}) on hip, at {ct} ({cm:.6g}) '
                         f'on the composition')
            for k in ('predict+explain', 'explain'):
                h, c = (rows[heads, windows, r, k] for r in ROUTES)
                apart = max(h) < min(c) or max(c) < min(h)
                lines.append(f'# {heads}, {windows} window(s), {k}: hip {statistics.median(h):.4f} ms, composition '
                             f'{statistics.median(c):.4f} ms: the composition takes '
                             f'{statistics.median(c) / statistics.median(h):.2f}x the hip time; '
                             + ('the ranges of the rounds do not overlap' if apart else 'the ranges of the rounds overlap'))
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args.rounds < 5 or args.iters < 200:
        print('# fewer than 5 rounds of 200 timed calls: a rehearsal, not a measurement')
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
