"""Generate tests/golden/sgn15_online_grad.npz, the online case of the SGN v15 input-gradient tests, in two steps:

    python tests/golden/make_golden_sgn_v15_online_grad.py record ROWS.npz     (on the GPU)
    python tests/golden/make_golden_sgn_v15_online_grad.py make ROWS.npz       (on the CPU)

record  feeds the frames of sgn_online_v15.npz to a v15 ``ActionRecognition`` (15 joints, sgn_preprocess, multi_test 2, a
        seg-4 model with the deployed heads) with injected draws and stores the rows it samples (S, seg, 45): they depend
        on the frames and the draws, not on the parameters.
make    searches the seed of the parameters (tests/sgn_v15_util.py::sgn15_state) on those rows until the margin condition
        of tests/sgn_v15_grad_util.py holds through the composition in fp64: every x-dependent ReLU pre-activation and
        every pooled top-1 minus top-2 gap at least max(2e-5, 4 x the fp32-vs-fp64 distance on that tensor) away from its
        switch.  tests/test_sgn_v15_grad_cpu.py asserts it again; the GPU test asserts that it samples the stored rows.
Only data is stored."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

from tests import sgn_v15_util as vu  # noqa: E402

V, SEG, S, WINDOW = 15, 4, 2, 36
ARGS = vu.model_args(V, SEG, 1, (8, 16, 128), (8, 32, 256))
RECOGNISER = dict(max_frame=WINDOW, max_num_skeleton=4, max_num_skeleton_true=2, num_joint=V, sgn_preprocess=True,
                  multi_test=S, zaxis=(8, 1), xaxis=(2, 5))
DRAW_SEED = 15


def draws():
    return np.random.default_rng(DRAW_SEED).integers(0, 2 ** 32, size=(1, S, SEG), dtype=np.uint32)


def record(path):
    import agcn_amd  # noqa: F401
    from agcn_amd import ops
    from agcn_amd.online import ActionRecognition
    ar = ActionRecognition(model='model.sgn_v15.SGN', model_args=ARGS, device='cuda:0', **RECOGNISER)
    for f in vu._npz('sgn_online_v15.npz')['frames']:
        ar.append_data(f)
    ar.predict(draws=draws())
    rows, _ = ops.sgn_sample(ar.window, ar.draws, ar.seg)
    np.savez(path, rows=rows.cpu().numpy(), draws=draws())


def make(path):
    from tests import sgn_v15_grad_util as gu
    with np.load(path) as f:
        rows, d = f['rows'].reshape(S, SEG, 3 * V), f['draws']
    assert np.array_equal(d, draws())
    scale = json.loads(str(vu._npz('sgn15_j15_deployed.npz')['meta']))['qk_scale']
    r32 = torch.from_numpy(rows)
    for seed in range(1601, 1701):
        meta = dict(seed=seed, qk_scale=scale, model_args=ARGS, recogniser=RECOGNISER, frames='sgn_online_v15.npz')
        t64 = gu.online_margins(gu.online_model(meta, torch.float64), r32.double())
        t32 = gu.online_margins(gu.online_model(meta), r32)
        m = {k: [max(gu.MARGIN_FLOOR, 4 * float((t32[k].double() - v).abs().max())), float(v.abs().min()),
                 float((t32[k].double() - v).abs().max())] for k, v in t64.items()}
        if all(found >= need for need, found, _ in m.values()):
            break
        print(f'seed {seed} rejected')
    else:
        raise SystemExit('no seed meets the margin condition')
    meta.update(margins=m, margin=min(v[1] for v in m.values()),
                sites=sum(v.numel() for k, v in t64.items() if not k.endswith('pool_gap')))
    out = os.path.join(HERE, 'sgn15_online_grad.npz')
    np.savez_compressed(out, meta=np.array(json.dumps(meta)), rows=rows, draws=d)
    print(f'seed {seed}: {meta["sites"]} sites, smallest distance to a switch {meta["margin"]:.2e}, {os.path.getsize(out)} bytes')


if __name__ == '__main__':
    {'record': record, 'make': make}[sys.argv[1]](sys.argv[2])
