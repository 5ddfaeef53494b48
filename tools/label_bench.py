"""Throughput of labelling a recording and of serving several streams (``agcn_amd.online.RecordingRecognition`` /
``MultiStreamRecognition``) against the frame-by-frame ``ActionRecognition`` loop, in one process.
    python tools/label_bench.py [--length 2000] [--frames 300] [--rounds 3] [--batches 1,8,32,64] [--streams 8,32]
                                [--ticks 60] [--configs agcn_v25,aagcn_v15] [--out FILE]
A synthetic recording of --length frames (tools/online_bench.py make_stream), a window of --frames, four tracked bodies,
two selected, a prediction after every frame.  Two configurations: AGCN at V = 25 and AAGCN at V = 15.

recording: predictions per second of (a) ``append_data`` + ``predict`` per frame and (b) ``label`` at every batch size
of --batches, by the host clock around work that ends in the final copy of the scores; the paths alternate for
--rounds rounds after one untimed pass that warms up every batch shape (the ragged last one included).  Reported: the
median of the rounds and their min..max.
parts: by device events, ``skel_smooth`` of the recording, ``prenorm_windows`` per batch and the forward per batch
(median over the batches of one labelling pass), and the forward alone on a random tensor of the batch-64 shape as
tools/infer_bench.py times it (the yardstick: the forward should dominate).
streams: ticks per second with one frame in and one prediction out per stream and tick, for S of --streams:
``MultiStreamRecognition`` against S separate ``ActionRecognition``, rings full, alternating for --rounds rounds of
--ticks ticks.
Needs a GPU; prints one JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import online_bench  # noqa: E402

TRACKED, SELECTED = online_bench.TRACKED, online_bench.SELECTED
OUT = None


def emit(**rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if OUT:
        OUT.write(line + '\n')


def rate(name, what, runs, **extra):
    """runs: units per second of every round -> the median and the spread."""
    med = statistics.median(runs)
    emit(config=name, measure=what, per_s=round(med, 1), min_per_s=round(min(runs), 1), max_per_s=round(max(runs), 1),
         spread_pct=round(100 * (max(runs) - min(runs)) / med, 1), rounds=len(runs), **extra)
    return med


def frame_by_frame(ar, rec):
    ar.reset()
    t0 = time.perf_counter()
    for f in rec:
        ar.append_data(f)
        ar.predict()
    return len(rec) / (time.perf_counter() - t0)


def labelled(rr, rec):
    t0 = time.perf_counter()
    scores, _, _ = rr.label(rec)
    return len(scores) / (time.perf_counter() - t0)


def parts(name, rr, rec, model, v, frames):
    """Device-event times of one labelling pass at rr.batch, and the bare forward at that batch."""
    from agcn_amd import ops
    from agcn_amd.online import window_plan_device
    ev = lambda: torch.cuda.Event(enable_timing=True)        # noqa: E731
    raw = rr._frames(rec, None, 'label')
    a, b = ev(), ev()
    a.record()
    sm = ops.skel_smooth(raw, rr.moving_avg)
    b.record()
    start, length, _ = window_plan_device(raw.shape[0], rr.max_frame, rr.device)
    marks = []
    for i in range(0, len(start), rr.batch):
        e = [ev(), ev(), ev()]
        e[0].record()
        win = rr.normalize(sm[None], start[i:i + rr.batch], length[i:i + rr.batch])
        e[1].record()
        rr.forward(win)
        e[2].record()
        if len(start) - i >= rr.batch:                       # full batches only
            marks.append(e)
    torch.cuda.synchronize()
    pre = statistics.median(e[0].elapsed_time(e[1]) for e in marks)
    fwd = statistics.median(e[1].elapsed_time(e[2]) for e in marks)
    x = torch.randn(rr.batch, 3, frames, v, SELECTED, device=rr.device)
    runs = []
    with torch.no_grad():
        for _ in range(3):
            model(x)
        torch.cuda.synchronize()
        for _ in range(5):
            t0 = time.perf_counter()
            for _ in range(10):
                model(x)
            torch.cuda.synchronize()
            runs.append((time.perf_counter() - t0) / 10)
    bare = statistics.median(runs)
    emit(config=name, measure='parts', batch=rr.batch, skel_smooth_ms=round(a.elapsed_time(b), 4),
         prenorm_windows_ms_per_batch=round(pre, 4), forward_ms_per_batch=round(fwd, 4),
         prenorm_share_of_forward=round(pre / fwd, 4), bare_forward_ms_per_batch=round(bare * 1e3, 4),
         bare_forward_clips_per_s=round(rr.batch / bare, 1), full_batches=len(marks))
    return rr.batch / bare


def recording(name, args, model, v, zaxis, xaxis):
    from agcn_amd.online import ActionRecognition, RecordingRecognition
    kw = dict(max_frame=args.frames, max_num_skeleton=TRACKED, max_num_skeleton_true=SELECTED, num_joint=v, zaxis=zaxis,
              xaxis=xaxis)
    rec = online_bench.make_stream(args.length, v)
    ar = ActionRecognition(model, **kw)
    rrs = {b: RecordingRecognition(model, batch=b, **kw) for b in args.batches}
    frame_by_frame(ar, rec[:args.frames + 20])               # warm-up: batch 1, then every batch shape
    for rr in rrs.values():
        labelled(rr, rec)
    runs = {k: [] for k in ['frame_by_frame'] + args.batches}
    for _ in range(args.rounds):
        runs['frame_by_frame'].append(frame_by_frame(ar, rec))
        for b, rr in rrs.items():
            runs[b].append(labelled(rr, rec))
    base = rate(name, 'frame_by_frame predictions', runs['frame_by_frame'], length=args.length)
    bare = parts(name, rrs[max(args.batches)], rec, model, v, args.frames)
    for b in args.batches:
        med = rate(name, 'label predictions', runs[b], batch=b, length=args.length)
        extra = dict(share_of_bare_forward=round(med / bare, 3)) if b == max(args.batches) else {}
        emit(config=name, measure='label vs frame_by_frame', batch=b, ratio=round(med / base, 2), **extra)


def streams(name, args, model, v, zaxis, xaxis, S):
    from agcn_amd.online import ActionRecognition, MultiStreamRecognition
    kw = dict(max_frame=args.frames, max_num_skeleton=TRACKED, max_num_skeleton_true=SELECTED, num_joint=v, zaxis=zaxis,
              xaxis=xaxis)
    need = args.frames + (args.rounds + 1) * args.ticks
    feed = np.stack([online_bench.make_stream(need, v, seed=s) for s in range(min(S, 4))])
    feed = feed[np.arange(S) % len(feed)]                                 # (S, need, M, 1, V, 3)
    ms = MultiStreamRecognition(model, S, **kw)
    singles = [ActionRecognition(model, **kw) for _ in range(S)]
    for t in range(args.frames):                                           # fill every ring, untimed
        ms.append_data(feed[:, t])
        for s, ar in enumerate(singles):
            ar.append_data(feed[s, t])

    def many(t0, n):
        c = time.perf_counter()
        for t in range(t0, t0 + n):
            ms.append_data(feed[:, t])
            ms.predict()
        return n / (time.perf_counter() - c)

    def separate(t0, n):
        c = time.perf_counter()
        for t in range(t0, t0 + n):
            for s, ar in enumerate(singles):
                ar.append_data(feed[s, t])
                ar.predict()
        return n / (time.perf_counter() - c)

    t = args.frames
    many(t, args.ticks), separate(t, args.ticks)                           # warm-up of the batch-S shape
    runs = dict(many=[], separate=[])
    for _ in range(args.rounds):
        t += args.ticks
        runs['many'].append(many(t, args.ticks))
        runs['separate'].append(separate(t, args.ticks))
    a = rate(name, 'multi_stream ticks', runs['many'], streams=S, ticks=args.ticks)
    b = rate(name, 'separate_recognisers ticks', runs['separate'], streams=S, ticks=args.ticks)
    emit(config=name, measure='multi_stream vs separate', streams=S, ratio=round(a / b, 2),
         predictions_per_s=round(a * S, 1))


def main():
    global OUT
    ap = argparse.ArgumentParser()
    ap.add_argument('--length', type=int, default=2000)
    ap.add_argument('--frames', type=int, default=300)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--batches', default='1,8,32,64')
    ap.add_argument('--streams', default='8,32')
    ap.add_argument('--ticks', type=int, default=60)
    ap.add_argument('--configs', default='agcn_v25,aagcn_v15')
    ap.add_argument('--out', default=None, help='also append the JSON lines to this file')
    args = ap.parse_args()
    args.batches = [int(b) for b in args.batches.split(',')]
    if not torch.cuda.is_available():
        raise SystemExit('label_bench needs a GPU: there is nothing to measure without one')
    OUT = open(args.out, 'a') if args.out else None
    emit(device=torch.cuda.get_device_name(0), host_cores=os.cpu_count(), torch_threads=torch.get_num_threads(),
         length=args.length, frames=args.frames, tracked=TRACKED, selected=SELECTED, rounds=args.rounds)
    for name in args.configs.split(','):
        model, v, zaxis, xaxis = online_bench.build(name)
        recording(name, args, model, v, zaxis, xaxis)
        for S in (int(s) for s in args.streams.split(',') if s):
            streams(name, args, model, v, zaxis, xaxis, S)
    if OUT:
        OUT.close()


if __name__ == '__main__':
    main()
