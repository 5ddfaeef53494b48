"""Label a recorded skeleton sequence: the prediction an online recogniser would have made after every ``--interval``-th
frame, computed in batches (``agcn_amd.online.RecordingRecognition``).
    python tools/label_recording.py RECORDING OUT.csv [--config agcn_v25 | --model model.aagcn.Model --model-args JSON]
        [--weights FILE] [--frames 300] [--tracked 4] [--selected 2] [--joints V] [--zaxis A B] [--xaxis A B]
        [--zaxis2 A B] [--moving-avg 1] [--interval 1] [--first 0] [--batch 64]
RECORDING is an ``.npy`` of shape (L, M, V, 3), or a directory in the format the reference's ``infer/inference.py``
reads: one comma-separated text file per frame, taken in sorted name order, one row per body, 3 * V values per row
(x, y, z of joint 0, of joint 1, ...).  Bodies beyond ``--tracked`` and joints beyond V are dropped; missing bodies, missing
values of a short row and empty files are zeros (a null body).  OUT.csv gets one line ``frame,label,score`` per
prediction, the score being the softmax score of the label.  Without ``--weights`` the model is randomly initialised,
which is good for timing and for nothing else.  Needs a GPU."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

CONFIGS = {
    # name: (model class, joints, graph, zaxis, xaxis): the two configurations of tools/online_bench.py
    'agcn_v25': ('model.agcn.Model', 25, 'graph.ntu_rgb_d.Graph', (0, 1), (8, 4)),
    'aagcn_v15': ('model.aagcn.Model', 15, 'graph.openpose_b25_j15.Graph', (8, 1), (2, 5)),
}


def _fit(rows, tracked, joints):
    """rows: a list of 1-D value arrays, one per body -> (tracked, joints, 3), cut or zero-filled."""
    out = np.zeros((tracked, joints * 3), dtype=np.float32)
    for m, r in enumerate(rows[:tracked]):
        n = min(len(r), joints * 3)
        out[m, :n] = r[:n]
    return out.reshape(tracked, joints, 3)


def read_directory(path, tracked, joints):
    """One comma-separated file per frame, in sorted name order -> (L, tracked, joints, 3) fp32."""
    names = sorted(n for n in os.listdir(path) if os.path.isfile(os.path.join(path, n)))
    if not names:
        raise SystemExit(f'label_recording: no frame files in {path}')
    frames = []
    for name in names:
        with open(os.path.join(path, name)) as f:
            rows = [np.array([float(x) for x in line.split(',') if x.strip()], dtype=np.float32)
                    for line in f if line.strip()]
        frames.append(_fit(rows, tracked, joints))
    return np.stack(frames)


def read_recording(path, tracked, joints):
    """An .npy (L, M, V', 3) or a directory of frame files -> (L, tracked, joints, 3) fp32."""
    if os.path.isdir(path):
        return read_directory(path, tracked, joints)
    a = np.load(path)
    if a.ndim == 5 and a.shape[2] == 1:                  # (L, M, 1, V, 3), as append_data takes frames
        a = a[:, :, 0]
    if a.ndim != 4 or a.shape[-1] != 3 or a.shape[0] < 1:
        raise SystemExit(f'label_recording: {path} holds {a.shape}, expected (L, M, V, 3)')
    out = np.zeros((a.shape[0], tracked, joints, 3), dtype=np.float32)
    m, v = min(tracked, a.shape[1]), min(joints, a.shape[2])
    out[:, :m, :v] = a[:, :m, :v]
    return out


def write_csv(path, ends, labels, scores):
    with open(path, 'w') as f:
        f.write('frame,label,score\n')
        for e, l, s in zip(ends, labels, scores):
            f.write(f'{int(e)},{int(l)},{float(s[int(l)]):.6f}\n')


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('recording')
    ap.add_argument('out')
    ap.add_argument('--config', choices=sorted(CONFIGS), default=None, help='model, joints, graph and axes in one')
    ap.add_argument('--model', default=None, help='dotted class path, e.g. model.aagcn.Model')
    ap.add_argument('--model-args', default=None, help='JSON dict of the model\'s constructor arguments')
    ap.add_argument('--weights', default=None)
    ap.add_argument('--num-class', type=int, default=60, help='with --config')
    ap.add_argument('--frames', type=int, default=300, help='the window')
    ap.add_argument('--tracked', type=int, default=4)
    ap.add_argument('--selected', type=int, default=2)
    ap.add_argument('--joints', type=int, default=None)
    ap.add_argument('--zaxis', type=int, nargs=2, default=None)
    ap.add_argument('--xaxis', type=int, nargs=2, default=None)
    ap.add_argument('--zaxis2', type=int, nargs=2, default=None)
    ap.add_argument('--moving-avg', type=int, default=1)
    ap.add_argument('--interval', type=int, default=1)
    ap.add_argument('--first', type=int, default=0)
    ap.add_argument('--batch', type=int, default=64)
    args = ap.parse_args()
    if (args.config is None) == (args.model is None):
        raise SystemExit('label_recording: give --config or --model')
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('label_recording needs a GPU: the recogniser has no CPU path')
    import agcn_amd  # noqa: F401
    from agcn_amd.online import RecordingRecognition
    if args.config:
        cls, joints, graph, zaxis, xaxis = CONFIGS[args.config]
        model_args = dict(num_class=args.num_class, num_point=joints, num_person=args.selected, graph=graph,
                          graph_args=dict(labeling_mode='spatial'))
    else:
        cls, joints, zaxis, xaxis = args.model, 25, (0, 1), (8, 4)
        model_args = json.loads(args.model_args) if args.model_args else {}
        joints = model_args.get('num_point', joints)
    joints = args.joints or joints
    rr = RecordingRecognition(cls, model_args, args.weights, max_frame=args.frames, max_num_skeleton=args.tracked,
                              max_num_skeleton_true=args.selected, num_joint=joints, moving_avg=args.moving_avg,
                              zaxis=tuple(args.zaxis or zaxis), xaxis=tuple(args.xaxis or xaxis),
                              zaxis2=tuple(args.zaxis2) if args.zaxis2 else None, batch=args.batch)
    rec = read_recording(args.recording, args.tracked, joints)
    scores, labels, ends = rr.label(rec, interval=args.interval, first=args.first)
    write_csv(args.out, ends, labels, scores)
    print(f'label_recording: {rec.shape[0]} frames, {len(ends)} predictions -> {args.out}')


if __name__ == '__main__':
    main()
