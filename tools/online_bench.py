"""Per-prediction latency of online recognition (``agcn_amd.online.ActionRecognition``): a window of 300 frames, four
tracked bodies, two selected, one frame in and one label out per iteration.
    python tools/online_bench.py [--iters 200] [--warmup 30] [--frames 300] [--configs agcn_v25,aagcn_v15] [--out FILE]
Two configurations: AGCN on the 25-joint NTU skeleton and AAGCN on the 15-joint OpenPose skeleton.  Each is measured
twice on the same stream: ``device`` (ring + selection + normalisation on the GPU: ops.skel_append / ops.prenorm) and
``host`` (the same preprocessing with torch ops on the CPU, then one host-to-device copy of the window), for comparison
on the machine at hand.

Per part: device events around append / selection + normalisation / model + softmax / score fetch (for ``host``: the
preprocessing by the host clock, then upload + model by events).  End to end: the host clock around the whole
iteration, which ends in the synchronising copy of the scores.  Every figure is the median over --iters iterations
after --warmup, with the 10th..90th percentile.  The ring is full and the model's folded weights are cached before
anything is timed.  Needs a GPU; prints one JSON line per measurement."""
import argparse
import json
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402

CONFIGS = {
    # name: (model module, joints, graph, zaxis, xaxis)
    'agcn_v25': ('agcn', 25, 'graph.ntu_rgb_d.Graph', (0, 1), (8, 4)),
    'aagcn_v15': ('aagcn', 15, 'graph.openpose_b25_j15.Graph', (8, 1), (2, 5)),
}
TRACKED, SELECTED = 4, 2


def build(name):
    import importlib
    import agcn_amd  # noqa: F401
    mod, v, graph, zaxis, xaxis = CONFIGS[name]
    Model = importlib.import_module('model.' + mod).Model
    model = Model(num_class=60, num_point=v, num_person=SELECTED, graph=graph, graph_args=dict(labeling_mode='spatial'))
    bench.randomize_like_training(model, 0)
    return model, v, zaxis, xaxis


def make_stream(n, v, seed=0):
    """(n, TRACKED, 1, V, 3): bodies 1 and 3 move all the time, body 0 passes through, body 2 never shows."""
    rng = np.random.default_rng(seed)
    frames = np.zeros((n, TRACKED, 1, v, 3), dtype=np.float32)
    t = np.arange(n)[:, None, None]
    for m, amp in ((1, 0.2), (3, 0.35), (0, 0.1)):
        pose = rng.standard_normal((1, v, 3)) * 0.35 + (0.3 + 0.6 * m, 2.5, 0.9)
        frames[:, m, 0] = pose + amp * np.sin(0.2 * t + rng.uniform(0, 6, (1, v, 3))) + 0.01 * rng.standard_normal((n, v, 3))
    frames[:, 0][(np.arange(n) % 170) > 40] = 0
    frames[::97, 3] = 0                                  # the tracker loses body 3 now and then
    return frames


# ---- the same preprocessing with torch ops on the host ---------------------------------------------------------------
def _rotation_onto(v, onto_z):
    """3x3 fp64 rotation taking v onto the z (x) axis about cross(v, axis), identity below the reference's thresholds."""
    e = np.array([0.0, 0.0, 1.0]) if onto_z else np.array([1.0, 0.0, 0.0])
    axis = np.cross(v, e)
    if np.abs(v).sum() < 1e-6:
        return np.eye(3)
    theta = math.acos(min(1.0, max(-1.0, float(np.dot(v / np.linalg.norm(v), e)))))
    if np.abs(axis).sum() < 1e-6 or abs(theta) < 1e-6:
        return np.eye(3)
    axis = axis / math.sqrt(np.dot(axis, axis))
    a = math.cos(theta / 2.0)
    b, c, d = -axis * math.sin(theta / 2.0)
    return np.array([[a * a + b * b - c * c - d * d, 2 * (b * c + a * d), 2 * (b * d - a * c)],
                     [2 * (b * c - a * d), a * a + c * c - b * b - d * d, 2 * (c * d + a * b)],
                     [2 * (b * d + a * c), 2 * (c * d - a * b), a * a + d * d - b * b - c * c]])


def host_prenorm(win, k, zaxis, xaxis):
    """win (M, T, V, 3) CPU tensor -> (1, 3, T, V, k): selection, padding, centring and the two rotations, vectorised."""
    M, T = win.shape[:2]
    valid = (win != 0).any(-1).any(-1)
    energy = []
    for m in range(M):
        s = win[m][valid[m]]
        energy.append(float(sum(s[..., c].std(unbiased=False) for c in range(3))) if len(s) else 0.0)
    order = sorted(range(M), key=lambda m: (energy[m], m), reverse=True)[:k]
    bodies = []
    for m in order:
        b = win[m]
        idx = torch.nonzero(valid[m])[:, 0]
        if len(idx):
            front = idx if not bool(valid[m, 0]) else torch.arange(int(idx[-1]) + 1)
            b = b[front[torch.arange(T) % len(front)]]
        bodies.append(b)
    s = torch.stack(bodies)
    s = (s - s[0:1, :, 1:2, :]) * (s != 0).any(-1, keepdim=True)
    R = np.eye(3)
    for lo, hi, onto_z in ((zaxis[0], zaxis[1], True), (xaxis[1], xaxis[0], False)):
        j = s[0, 0].double().numpy() @ R.T
        R = _rotation_onto(j[hi] - j[lo], onto_z) @ R
    out = s @ torch.from_numpy(R.T).float()
    return out.permute(3, 1, 2, 0).unsqueeze(0).contiguous(), order


class HostWindow:
    """The reference's sliding window on the host (shift by one frame per append once full)."""

    def __init__(self, frames, v):
        self.data, self.counter = torch.zeros(TRACKED, frames, v, 3), 0

    def append(self, frame):
        f = torch.from_numpy(frame[:, 0])
        if self.counter < self.data.shape[1]:
            self.data[:, self.counter] = f
            self.counter += 1
        else:
            self.data[:, :-1] = self.data[:, 1:].clone()
            self.data[:, -1] = f


def pct(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(round(q * (len(xs) - 1))))]


def report(name, mode, part, xs, out):
    rec = dict(config=name, mode=mode, part=part, median_ms=round(statistics.median(xs), 4), p10_ms=round(pct(xs, 0.1), 4),
               p90_ms=round(pct(xs, 0.9), 4), n=len(xs))
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        out.write(line + '\n')
    return rec['median_ms']


def run(name, args, out):
    from agcn_amd.online import ActionRecognition
    dev = torch.device('cuda:0')
    model, v, zaxis, xaxis = build(name)
    ar = ActionRecognition(model, max_frame=args.frames, max_num_skeleton=TRACKED, max_num_skeleton_true=SELECTED,
                           num_joint=v, zaxis=zaxis, xaxis=xaxis)
    stream = make_stream(args.frames + 2 * (args.warmup + args.iters), v)
    host = HostWindow(args.frames, v)
    for f in stream[:args.frames]:
        ar.append_data(f)
        host.append(f)
    pos = args.frames
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]

    # ---- device preprocessing ----
    parts = {k: [] for k in ('append', 'select+normalise', 'model+softmax', 'fetch', 'end_to_end')}
    for it in range(args.warmup + args.iters):
        f = stream[pos]
        pos += 1
        host.append(f)
        t0 = time.perf_counter()
        ev[0].record()
        ar.append_data(f)
        ev[1].record()
        win = ar.normalize()
        ev[2].record()
        _, scores, label = ar.forward(win)
        ev[3].record()
        both = torch.cat((scores[0], label.to(scores.dtype))).cpu()
        ev[4].record()
        t1 = time.perf_counter()
        ev[4].synchronize()
        if it >= args.warmup:
            for k, (a, b) in zip(('append', 'select+normalise', 'model+softmax', 'fetch'), zip(ev[:-1], ev[1:])):
                parts[k].append(a.elapsed_time(b))
            parts['end_to_end'].append((t1 - t0) * 1e3)
    dev_label = int(both[-1])
    med = {k: report(name, 'device', k, xs, out) for k, xs in parts.items()}

    # the two preprocessings agree on the window they are about to be compared on
    hw, order = host_prenorm(host.data, SELECTED, zaxis, xaxis)
    diff = float((hw.to(dev) - ar.window).abs().max())
    print(json.dumps(dict(config=name, check='host vs device window', max_abs_diff=diff, selected_host=order,
                          selected_device=ar.selected.cpu().tolist()[0])), flush=True)
    assert diff < 1e-4 and order == ar.selected.cpu().tolist()[0], 'host and device preprocessing disagree'

    # ---- host preprocessing ----
    parts = {k: [] for k in ('host_preprocess', 'upload+model+softmax', 'fetch', 'end_to_end')}
    for it in range(args.warmup + args.iters):
        f = stream[pos]
        pos += 1
        t0 = time.perf_counter()
        host.append(f)
        hw, _ = host_prenorm(host.data, SELECTED, zaxis, xaxis)
        tp = time.perf_counter()
        ev[0].record()
        _, scores, label = ar.forward(hw.to(dev))
        ev[1].record()
        both = torch.cat((scores[0], label.to(scores.dtype))).cpu()
        ev[2].record()
        t1 = time.perf_counter()
        ev[2].synchronize()
        if it >= args.warmup:
            parts['host_preprocess'].append((tp - t0) * 1e3)
            parts['upload+model+softmax'].append(ev[0].elapsed_time(ev[1]))
            parts['fetch'].append(ev[1].elapsed_time(ev[2]))
            parts['end_to_end'].append((t1 - t0) * 1e3)
    medh = {k: report(name, 'host', k, xs, out) for k, xs in parts.items()}
    share = med['select+normalise'] / med['model+softmax']
    print(f'# {name}: device end to end {med["end_to_end"]:.3f} ms (append {med["append"]:.3f}, select+normalise '
          f'{med["select+normalise"]:.3f} = {100 * share:.1f} % of the model\'s {med["model+softmax"]:.3f}, fetch '
          f'{med["fetch"]:.3f}); host preprocessing end to end {medh["end_to_end"]:.3f} ms (preprocess '
          f'{medh["host_preprocess"]:.3f}); label {dev_label}', flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=30)
    ap.add_argument('--frames', type=int, default=300)
    ap.add_argument('--configs', default='agcn_v25,aagcn_v15')
    ap.add_argument('--out', default=None, help='also append the JSON lines to this file')
    args = ap.parse_args()
    if args.iters < 200:
        print('# fewer than 200 timed predictions: a rehearsal, not a measurement', flush=True)
    if not torch.cuda.is_available():
        raise SystemExit('online_bench needs a GPU: there is nothing to measure without one')
    out = open(args.out, 'a') if args.out else None
    print('# ' + json.dumps(dict(device=torch.cuda.get_device_name(0), host_cores=os.cpu_count(),
                                torch_threads=torch.get_num_threads(), frames=args.frames, tracked=TRACKED,
                                selected=SELECTED, iters=args.iters, warmup=args.warmup)), flush=True)
    for name in args.configs.split(','):
        run(name, args, out)
    if out:
        out.close()


if __name__ == '__main__':
    main()
