"""Shared by the SGN v15 tests and tests/golden/make_golden_sgn_v15.py: the case table, the seeded parameter recipe (the
fixtures store the seed, the key list and a checksum per tensor, not the parameters) and the fixture loaders."""
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')

NUM_CLASS = 60
# spatial, temporal: unscaled He weights saturate both softmaxes (one-hot maps).  The maker starts here and moves a block's
# scale in steps of 1.5 until its map is neither one-hot nor uniform; a fixture's meta holds the scales it was made with.
QK_SCALE = (0.7, 0.18)
# name: V, seg, bs, bias, spatial (heads, d_head, ff), temporal (heads, d_head, ff)
CASES = {
    'j3_seg2': (3, 2, 5, 1, (2, 64, 128), (4, 32, 128)),
    'j15_deployed': (15, 20, 5, 1, (8, 16, 128), (8, 32, 256)),
    'j25_yaml': (25, 20, 3, 1, (1, 512, 512), (1, 1024, 1024)),
    'j32_seg32': (32, 32, 1, 1, (4, 32, 256), (2, 64, 384)),
    'j7_seg12_nobias': (7, 12, 4, 0, (8, 16, 128), (8, 32, 256)),
    'j9_seg7_h2x256': (9, 7, 2, 1, (2, 256, 128), (2, 256, 384)),            # two sliced heads per block
    'j16_seg17_h16x16': (16, 17, 2, 1, (16, 16, 256), (8, 16, 384)),         # two groups of 16-wide heads; 16-wide heads in the clip block
}
TENSORS = ('logits', 'spatial_attn', 'temporal_attn', 'spa_emb', 'tem_emb', 'feat', 'pooled')


def mha_kwargs(d_model, heads, d_head, ff, ff_out):
    return dict(d_model=[d_model], nhead=[heads], d_head=[d_head], dim_feedforward=[ff], dim_feedforward_output=[ff_out],
                dropout=0.1, activation='relu', num_layers=1, norm='bn', global_norm=False)


def model_args(V, seg, bias, spatial, temporal, num_class=NUM_CLASS):
    """The reference's v15 experiment (config/nturgbd-cross-view/train_sgn_v15.yaml) at the case's sizes."""
    return dict(num_class=num_class, num_point=V, num_segment=seg, in_channels=3, bias=bias, dropout=0.0, dropout2d=0.2,
                c_multiplier=[1.0, 1.0, 1.0, 1.0], norm_type='bn', act_type='relu', input_position=1, input_velocity=1,
                semantic_joint=1, semantic_frame=1, semantic_class=0, semantic_joint_fusion=0, semantic_frame_fusion=1,
                semantic_frame_location=0, spatial_maxpool=1, temporal_maxpool=1,
                spatial_mha_kwargs=mha_kwargs(128, *spatial, 256), temporal_mha_kwargs=mha_kwargs(256, *temporal, 512))


def case_args(case):
    V, seg, _, bias, spatial, temporal = CASES[case]
    return model_args(V, seg, bias, spatial, temporal)


def sgn15_state(shapes, seed, qk_scale=QK_SCALE):
    """{key: numpy array} for the (key, shape) pairs of a v15 state_dict.  tests/sgn_util.py::sgn_state's recipe -- every
    tensor its own generator seeded by (seed, position in the sorted key list) -- with two changes: a BatchNorm is a
    module that owns a running_mean, and the to_q / to_k weights are multiplied by the block's ``qk_scale``.  The one-hot
    buffers are the class's own."""
    out = {}
    for i, key in enumerate(sorted(shapes)):
        shape = tuple(shapes[key])
        rng = np.random.default_rng([int(seed), i])
        owner, leaf = key.rsplit('.', 1)
        is_bn = owner + '.running_mean' in shapes
        if leaf == 'onehot':
            if 'spa_onehot' in key:            # (1, V, V, seg): one-hot over the joint
                v = np.broadcast_to(np.eye(shape[1], dtype=np.float32)[None, :, :, None], shape).copy()
            else:                              # (1, seg, V, seg): one-hot over the frame
                v = np.broadcast_to(np.eye(shape[1], dtype=np.float32)[None, :, None, :], shape).copy()
        elif leaf == 'num_batches_tracked':
            v = np.zeros(shape, dtype=np.int64)
        elif leaf == 'running_var' or (is_bn and leaf == 'weight'):
            v = rng.uniform(0.5, 1.5, shape).astype(np.float32)
        elif leaf == 'running_mean':
            v = (0.2 * rng.standard_normal(shape)).astype(np.float32)
        elif leaf == 'bias':
            v = (0.1 * rng.standard_normal(shape)).astype(np.float32)
        else:
            fan_in = int(np.prod(shape[1:]))
            v = (np.sqrt(2.0 / fan_in) * rng.standard_normal(shape)).astype(np.float32)
        if owner.endswith('.to_q') or owner.endswith('.to_k'):
            v = (v * np.float32(qk_scale[0 if key.startswith('spatial_mha.') else 1])).astype(np.float32)
        out[key] = v
    return out


def checksums(state):
    """fp64 (sum, sum of squares) per tensor, in sorted key order."""
    return np.array([[np.asarray(state[k], dtype=np.float64).sum(), np.square(np.asarray(state[k], dtype=np.float64)).sum()]
                     for k in sorted(state)])


def pack_state(out, state, keys):
    shapes = {k: tuple(state[k].shape) for k in keys}
    out['keys'] = np.array(list(keys))
    out['shapes'] = np.array(['x'.join(str(d) for d in shapes[k]) for k in keys])
    out['checksums'] = checksums(state)


_FILES = {}


def _npz(name):
    if name not in _FILES:
        with np.load(os.path.join(GOLDEN, name)) as f:
            _FILES[name] = {k: f[k] for k in f.files}
    return _FILES[name]


def _state_of(f):
    meta = json.loads(str(f['meta']))
    keys = [str(k) for k in f['keys']]
    shapes = {k: tuple(int(d) for d in s.split('x') if d) for k, s in zip(keys, (str(s) for s in f['shapes']))}
    state = sgn15_state(shapes, meta['seed'], tuple(meta['qk_scale']))
    assert np.array_equal(checksums(state), f['checksums']), 'the seeded recipe no longer reproduces the fixture'
    return meta, keys, shapes, state


def load_case(case):
    """-> dict(meta, keys, shapes, state, x and the reference's tensors): logits (bs, 60), spatial_attn (bs * seg, h, V,
    V), temporal_attn (bs, h, seg, seg), spa_emb (64, V), tem_emb (256, seg), feat (bs, seg, 256) = the maximum over the
    joints + tem_emb, pooled (bs, 512) = the maximum over the frames."""
    f = _npz(f'sgn15_{case}.npz')
    meta, keys, shapes, state = _state_of(f)
    return dict(meta=meta, keys=keys, shapes=shapes, state=state, x=f['x'], **{t: f[t] for t in TENSORS})


def load_online():
    f = _npz('sgn15_online.npz')
    meta, keys, shapes, state = _state_of(f)
    return dict(meta=meta, keys=keys, shapes=shapes, state=state, **{k: f[k] for k in ('record', 'draws', 'logits',
                                                                                      'scores', 'labels')})


def torch_state(state):
    import torch
    return {k: torch.from_numpy(np.array(v)) for k, v in state.items()}


def bound(ref):
    """The project's fp32 rule: 1e-4 relative to max(1, max|reference tensor|)."""
    return 1e-4 * max(1.0, float(np.abs(ref).max()))
