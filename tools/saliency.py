"""Input-gradient saliency of the 2s-AGCN joint model: |d logit_k / d x| from ONE eval-mode forward + backward (frozen
BatchNorm statistics, requires_grad on the input alone, so every BatchNorm stage runs the one-pass backward without its
parameter sums: agcn_bn_bwd_eval with want_sums = 0).
    python tools/saliency.py [--data clips.npy] [--weights state.pt] [--class K] [--batch 64] [--frames 300]
                             [--reps 5] [--repeats 5]
Without --data a seeded synthetic clip batch (N, 3, T, 25, 2) is used; --data is a .npy of that layout (the feeders' data
file), of which the first --batch clips are taken.  --class K: the logit to explain (default: each clip's arg max).
Prints, for the first clip, the per-joint map sum_{c,t,m} |g| and the per-frame map sum_{c,v,m} |g| (each normalised to
sum 1), then the time per clip: median of --repeats timed runs of --reps forward+backward passes after a warm-up, with
the min..max spread of the runs."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402


def saliency(model, x, k=None):
    """|d logit_k / d x| for a batch x (N, C, T, V, M); k None = each clip's own top class.  Returns (N, C, T, V, M)."""
    x = x.detach().requires_grad_(True)
    out = model(x)
    logits = out[0] if isinstance(out, tuple) else out
    idx = logits.argmax(1) if k is None else torch.full((x.shape[0],), int(k), device=x.device)
    logits.gather(1, idx[:, None]).sum().backward()
    return x.grad.abs()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--data', default=None)
    ap.add_argument('--weights', default=None)
    ap.add_argument('--class', dest='k', type=int, default=None)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--frames', type=int, default=300)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--repeats', type=int, default=5)
    args = ap.parse_args()
    from agcn_amd import ops
    dev = torch.device('cuda:0')
    model = bench.build_model('ntu_agcn')
    if args.weights:
        model.load_state_dict(torch.load(args.weights, map_location='cpu'))
    else:
        bench.randomize_like_training(model, 0)
    model = model.to(dev).eval()
    for p in model.parameters():
        p.requires_grad_(False)
    if args.data:
        x = torch.from_numpy(np.load(args.data, mmap_mode='r')[:args.batch].astype(np.float32)).to(dev)
    else:
        x = torch.randn(args.batch, 3, args.frames, 25, 2, device=dev, generator=torch.Generator(dev).manual_seed(0))
    before = dict(ops.EVAL_BWD_STATS)
    g = saliency(model, x, args.k)
    torch.cuda.synchronize()
    took = {k: ops.EVAL_BWD_STATS[k] - before[k] for k in before}
    assert took['sums'] == 0 and took['nosums'] > 0, took     # the input-gradient-only route, or the figures mean nothing
    joint = g[0].sum((0, 1, 3)).cpu().numpy()
    frame = g[0].sum((0, 2, 3)).cpu().numpy()
    np.set_printoptions(precision=4, suppress=True, linewidth=120)
    print('per-joint saliency of clip 0 (V = %d):' % joint.size)
    print(joint / max(joint.sum(), 1e-30))
    print('per-frame saliency of clip 0 (T = %d):' % frame.size)
    print(frame / max(frame.sum(), 1e-30))
    runs = []
    for _ in range(2):
        saliency(model, x, args.k)
    torch.cuda.synchronize()
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        for _ in range(args.reps):
            saliency(model, x, args.k)
        torch.cuda.synchronize()
        runs.append((time.perf_counter() - t0) / args.reps)
    med = statistics.median(runs)
    n = x.shape[0]
    print('saliency (eval forward + input-gradient backward, %d BatchNorm stages without sums): %.2f ms per batch of %d '
          '(min %.2f, max %.2f over %d runs), %.3f ms per clip'
          % (took['nosums'], med * 1e3, n, min(runs) * 1e3, max(runs) * 1e3, len(runs), med * 1e3 / n), flush=True)


if __name__ == '__main__':
    main()
