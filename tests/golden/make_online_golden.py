"""Generate the fixtures of the online-recognition path by running the REFERENCE on the CPU:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_online_golden.py

  graph_openpose_b25_j15.npz   the reference graph's A
  prenorm_cases.npz            raw skeletons (N, M=2, T, V, 3) and data_gen/preprocess.py pre_normalization of them
  prenorm_long.npz             the same at T = 150, V = 25
  online_stream_v15.npz        29 frames through infer/data_preprocess.py DataPreprocessorV2 (window 24, 4 tracked
                               bodies, 2 selected), the normalised window and the selection after every append,
                               with moving_avg 1 and 3
  online_model_v15.npz         raw frames -> window of 36 -> reference aagcn.Model(num_point=15) logits and scores

Needs the reference checkout (as make_golden.py, whose loaders and seeded parameter recipe are imported, not edited).
Only data is stored.  Every fixture is written only if the conditions hold under which comparing against the reference
is fair (``check_null_tests``, ``check_energies``, the logit gap): the product tests "all values zero" where the
reference tests "sum is zero", and selection / labels are only comparable away from ties."""
import importlib
import json
import os
import sys
from functools import partial

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

import make_golden as mg  # noqa: E402
from make_golden import orc  # noqa: E402

CENTRE = np.array([0.3, 2.5, 0.9], dtype=np.float32)
AXES = {15: dict(zaxis=[8, 1], xaxis=[2, 5]), 25: dict(zaxis=[0, 1], xaxis=[8, 4]), 18: dict(zaxis=[0, 1], xaxis=[8, 4])}


def load_reference_online():
    """The reference's aagcn module (make_golden's loader, which also puts the reference first on sys.path) and its
    preprocessing modules."""
    ref = mg.load_reference_aagcn()
    for k in [k for k in sys.modules if k.split('.')[0] in ('infer', 'data_gen', 'utils')]:
        del sys.modules[k]
    pre = importlib.import_module('data_gen.preprocess')
    dp = importlib.import_module('infer.data_preprocess')
    gen = importlib.import_module('data_gen.ntu_gendata')
    assert all(m.__file__.startswith(mg.REF) for m in (pre, dp, gen))
    return ref, pre, dp, gen


# ---- fairness conditions ---------------------------------------------------------------------------------------------
def check_null_tests(s, what):
    """s (..., T, V, 3): no frame and no joint may sum to zero unless it is all zero."""
    s = np.asarray(s)
    fsum, fany = s.sum(-1).sum(-1), (s != 0).any(-1).any(-1)
    jsum, jany = s.sum(-1), (s != 0).any(-1)
    assert np.array_equal(fsum != 0, fany), f'{what}: a non-null frame sums to zero'
    assert np.array_equal(jsum != 0, jany), f'{what}: a non-null joint sums to zero'


def check_energies(energy, what):
    e = sorted(float(x) for x in energy if x != 0)
    for a, b in zip(e[:-1], e[1:]):
        assert (b - a) >= 0.01 * b, f'{what}: energies {a} and {b} are within 1 %'


def normalize_checked(pre, data, what, **kw):
    """pre_normalization of data (N, 3, T, V, M) with the null-test condition checked on the raw data, after centring
    and after every rotation."""
    to_s = lambda d: np.transpose(d, [0, 4, 2, 3, 1])          # noqa: E731
    check_null_tests(to_s(data), what + ' raw')
    stages = dict(zaxis=None, xaxis=None, zaxis2=None)
    for stage in (None, 'zaxis', 'xaxis'):
        if stage is not None:
            stages[stage] = kw.get(stage)
        part = pre.pre_normalization(data.copy(), **{**kw, **stages}, verbose=False, tqdm=False)
        check_null_tests(to_s(part), f'{what} after {stage or "centring"}')
    out = pre.pre_normalization(data.copy(), **kw, verbose=False, tqdm=False)
    check_null_tests(to_s(out), what + ' out')
    return out


# ---- prenorm_cases.npz -----------------------------------------------------------------------------------------------
def body(rng, t, v, shift, spread=0.35):
    """(T, V, 3): a skeleton that drifts and moves, joints normal around CENTRE."""
    pose = CENTRE + shift + spread * rng.standard_normal((1, v, 3))
    drift = np.cumsum(0.03 * rng.standard_normal((t, 1, 3)), axis=0)
    return (pose + drift + 0.05 * rng.standard_normal((t, v, 3))).astype(np.float32)


def sample(rng, t, v, kind, axes):
    s = np.stack([body(rng, t, v, np.zeros(3)), body(rng, t, v, np.array([0.8, 0.3, 0.0]))])      # M, T, V, 3
    mid = t // 2
    if kind == 'plain':
        pass
    elif kind == 'lead3':
        s[:, :3] = 0
    elif kind == 'lead70':                   # compaction across the 64-frame chunks of the kernel's prefix sum
        s[0, :70] = 0
        s[0, 90:97] = 0
        s[1, :5] = 0
        s[1, 64:128] = 0
    elif kind == 'tails':
        s[0, (3 * t) // 5:] = 0
        s[1, (2 * t) // 5:] = 0
    elif kind == 'gap':
        s[0, mid - 1:mid + 1] = 0
        s[1, 2:4] = 0
        s[1, t - 2:] = 0
    elif kind == 'second_empty':
        s[1] = 0
    elif kind == 'first_empty':
        s[0] = 0
    elif kind == 'scattered':
        s[0, [0, mid, t - 1]] = 0
        s[1, [mid, t - 1]] = 0
        s[1, :, 3] = 0
        s[0, 1:3, v - 1] = 0
    elif kind == 'spine_on_z':
        z0, z1 = axes['zaxis']
        s[0, 0, z1, :2] = s[0, 0, z0, :2]
        s[0, 0, z1, 2] = s[0, 0, z0, 2] + np.float32(0.4)
    elif kind == 'zero':
        s[:] = 0
    else:
        raise ValueError(kind)
    return s


BASE_KINDS = ['plain', 'lead3', 'tails', 'gap', 'second_empty', 'first_empty', 'scattered', 'spine_on_z', 'zero']
PRENORM_GROUPS = [
    # name, V, T, kinds, options on top of the shape's axes
    ('base_v15', 15, 7, BASE_KINDS, {}),
    ('base_v25', 25, 20, BASE_KINDS, {}),
    ('base_v18', 18, 33, BASE_KINDS, {}),
    ('firstframe_v25', 25, 20, ['plain', 'tails', 'gap', 'second_empty'], dict(center=False, center_firstframe=True)),
    ('nopad_v18', 18, 33, ['plain', 'lead3', 'tails', 'scattered'], dict(pad=False)),
    ('noz_v15', 15, 7, ['plain', 'lead3', 'gap'], dict(zaxis=None)),
    ('zaxis2_v25', 25, 20, ['plain', 'lead3', 'scattered'], dict(zaxis2=[1, 20])),
]


# beyond the three small shapes: more frames than one 64-frame chunk and more joints x frames than one workgroup has
# threads, in a file of its own (size)
LONG_GROUPS = [('long_v25', 25, 150, ['lead70', 'tails', 'scattered'], {})]


def make_prenorm_cases(pre, groups=PRENORM_GROUPS, seed=900, fname='prenorm_cases.npz'):
    out, names = {}, []
    for gi, (name, v, t, kinds, extra) in enumerate(groups):
        rng = np.random.default_rng(seed + gi)
        opts = dict(zaxis2=None, pad=True, center=True, center_firstframe=False)
        opts.update(AXES[v])
        opts.update(extra)
        raw = np.stack([sample(rng, t, v, kind, opts if opts['zaxis'] else AXES[v]) for kind in kinds])    # N, M, T, V, 3
        data = np.ascontiguousarray(np.transpose(raw, [0, 4, 2, 3, 1]))                                    # N, C, T, V, M
        ref = normalize_checked(pre, data, name, **opts)
        assert ref.dtype == np.float32 and ref.shape == data.shape
        if 'zero' in kinds:
            assert not ref[kinds.index('zero')].any()
        if 'spine_on_z' in kinds:        # the z rotation of that sample must have taken the identity branch
            i = kinds.index('spine_on_z')
            only_centred = pre.pre_normalization(data[i:i + 1].copy(), **{**opts, 'zaxis': None, 'xaxis': None},
                                                 verbose=False, tqdm=False)
            z_only = pre.pre_normalization(data[i:i + 1].copy(), **{**opts, 'xaxis': None}, verbose=False, tqdm=False)
            assert np.array_equal(only_centred, z_only)
        out[name + '.raw'] = raw
        out[name + '.ref'] = ref
        out[name + '.opts'] = np.array(json.dumps(opts))
        out[name + '.kinds'] = np.array(kinds)
        names.append(name)
        print(f'{name}: raw {raw.shape} |ref|max {np.abs(ref).max():.3f}')
    out['groups'] = np.array(names)
    np.savez_compressed(os.path.join(HERE, fname), **out)


# ---- streams -----------------------------------------------------------------------------------------------------------
def stream_frames(rng, n, v, starts, gaps, max_person=4):
    """(n, max_person, 1, V, 3): body m is present from frame starts[m] on, except at the frames gaps[m]."""
    frames = np.zeros((n, max_person, 1, v, 3), dtype=np.float32)
    for m, t0 in starts.items():
        amp = 1.0 + 0.6 * m                   # different size and activity per body: energies well apart
        b = body(rng, n, v, np.array([0.5 * m, 0.1 * m, 0.0]), spread=0.3 + 0.08 * m)
        b = (b + amp * 0.15 * np.sin(np.arange(n)[:, None, None] * 0.4 + rng.uniform(0, 6, (1, v, 3)))).astype(np.float32)
        for t in range(t0, n):
            if t not in gaps.get(m, ()):
                frames[t, m, 0] = b[t]
    return frames


def run_stream(pre, dp, gen, frames, window, moving_avg, num_skels, v, what):
    """Push the frames through the reference's DataPreprocessorV2; after every append the normalised window and the
    selection (energy.argsort()[::-1][:num_skels], as select_skeletons takes it)."""
    fn = partial(pre.pre_normalization, **AXES[v], verbose=False, tqdm=False)
    proc = dp.DataPreprocessorV2(num_joint=v, max_seq_length=window, max_person=frames.shape[1], moving_avg=moving_avg,
                                 aagcn_normalize_fn=fn)
    wins, sels = [], []
    for i, f in enumerate(frames):
        proc.append_data(f)
        energy = np.array([gen.get_nonzero_std(x) for x in proc.data])
        check_energies(energy, f'{what} append {i}')
        index = energy.argsort()[::-1][0:num_skels]
        chosen = proc.data[index][None]                                                   # 1, K, T, V, 3
        normalize_checked(pre, np.ascontiguousarray(np.transpose(chosen, [0, 4, 2, 3, 1])), f'{what} append {i}',
                          **AXES[v])
        win = proc.select_skeletons_and_normalize_data(num_skels, aagcn_normalize=True)
        assert win.shape == (1, 3, window, v, num_skels) and win.dtype == np.float32
        wins.append(win)
        sels.append(index.astype(np.int32))
    return np.stack(wins), np.stack(sels)


def make_online_stream(pre, dp, gen):
    v, window, n = 15, 24, 29
    frames = stream_frames(np.random.default_rng(950), n, v, starts={1: 2, 3: 4}, gaps={3: (9, 10)})
    out = dict(frames=frames, meta=np.array([v, window, 4, 2], dtype=np.int64))
    for k in (1, 3):
        wins, sels = run_stream(pre, dp, gen, frames, window, k, 2, v, f'stream ma{k}')
        out[f'win_ma{k}'], out[f'sel_ma{k}'] = wins, sels
        print(f'stream moving_avg={k}: windows {wins.shape}, selections {sorted(set(map(tuple, sels.tolist())))}')
    np.savez_compressed(os.path.join(HERE, 'online_stream_v15.npz'), **out)


MODEL_SEED, MODEL_STRESS, MODEL_CLASSES = 601, 3.0, 60


def make_online_model(ref, pre, dp, gen):
    v, window, n = 15, 36, 44
    record = (19, 35, 43)                         # filling, just full, after the ring has wrapped
    frames = stream_frames(np.random.default_rng(951), n, v, starts={0: 0, 2: 3}, gaps={2: (12,)})
    mk = dict(num_class=MODEL_CLASSES, num_point=v, num_person=2, graph='graph.openpose_b25_j15.Graph',
              graph_args=dict(labeling_mode='spatial'), model_layers=10)
    model = ref.Model(**mk)
    shapes = orc.aagcn_model_param_shapes(MODEL_CLASSES, v)
    assert set(shapes) == set(model.state_dict().keys()), set(shapes) ^ set(model.state_dict().keys())
    model.load_state_dict(orc.aagcn_randomized_state(shapes, MODEL_SEED, stress=MODEL_STRESS))
    model.eval()
    fn = partial(pre.pre_normalization, **AXES[v], verbose=False, tqdm=False)
    proc = dp.DataPreprocessorV2(num_joint=v, max_seq_length=window, max_person=4, moving_avg=1, aagcn_normalize_fn=fn)
    logits, scores = [], []
    for i, f in enumerate(frames):
        proc.append_data(f)
        if i not in record:
            continue
        energy = np.array([gen.get_nonzero_std(x) for x in proc.data])
        check_energies(energy, f'model stream append {i}')
        chosen = proc.data[energy.argsort()[::-1][0:2]][None]
        normalize_checked(pre, np.ascontiguousarray(np.transpose(chosen, [0, 4, 2, 3, 1])), f'model stream append {i}',
                          **AXES[v])
        win = proc.select_skeletons_and_normalize_data(2, aagcn_normalize=True)
        with torch.no_grad():
            lg, _ = model(torch.from_numpy(win))
            sc = torch.nn.functional.softmax(lg, 1)
        top = torch.sort(lg[0], descending=True).values
        assert float(top[0] - top[1]) > 1e-3, f'append {i}: the top two logits are within 1e-3'
        logits.append(lg[0].numpy())
        scores.append(sc[0].numpy())
    out = dict(frames=frames, record=np.array(record, dtype=np.int64), logits=np.stack(logits), scores=np.stack(scores),
               meta=np.array([v, window, 4, 2, MODEL_CLASSES, MODEL_SEED], dtype=np.int64),
               stress=np.float32(MODEL_STRESS))
    np.savez_compressed(os.path.join(HERE, 'online_model_v15.npz'), **out)
    print('model stream: labels', [int(x.argmax()) for x in logits], '|logit|max', float(np.abs(np.stack(logits)).max()))


def make_graph():
    A = importlib.import_module('graph.openpose_b25_j15').Graph(labeling_mode='spatial').A
    np.savez_compressed(os.path.join(HERE, 'graph_openpose_b25_j15.npz'), A=np.asarray(A, dtype=np.float64))


if __name__ == '__main__':
    torch.manual_seed(0)
    torch.set_num_threads(8)
    ref, pre, dp, gen = load_reference_online()
    assert importlib.import_module('graph.openpose_b25_j15').__file__.startswith(mg.REF)
    make_graph()
    make_prenorm_cases(pre)
    make_prenorm_cases(pre, LONG_GROUPS, 930, 'prenorm_long.npz')
    make_online_stream(pre, dp, gen)
    make_online_model(ref, pre, dp, gen)
