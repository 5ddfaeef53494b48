"""Shared by the SGN batch-statistics tests and tests/golden/make_golden_sgn_bnstats.py: the case list, the loader of
tests/golden/sgn_bnstats.npz and a numpy emulation of ``agcn_sgn_stats_finalize`` that pins its merge without a GPU."""
import json
import os

import numpy as np

from tests import sgn_util as su

BN_NAMES = ('joint_embed.cnn.0.bn', 'dif_embed.cnn.0.bn', 'gcn1.bn', 'gcn2.bn', 'gcn3.bn', 'cnn.bn1', 'cnn.bn2')
CASES = ('v15_seg20', 'v25_seg20', 'v7_seg12_nobias', 'v3_seg34', 'v15_seg20_b9')
BATCH = dict(v15_seg20=5, v25_seg20=3, v7_seg12_nobias=2, v3_seg34=3, v15_seg20_b9=9)
CHUNKED = ('v15_seg20_b9', 4)          # this case also runs in chunks of 4 clips: 4 + 4 + 1
BOUND = 1e-4                           # the project's standing fp32 bound, relative to max(1, max|ref|)

_CACHE = {}


def _file():
    if 'f' not in _CACHE:
        with np.load(os.path.join(su.GOLDEN, 'sgn_bnstats.npz')) as f:
            _CACHE['f'] = {k: f[k] for k in f.files}
    return _CACHE['f']


def load_case(case):
    """-> dict(meta, state, x): from sgn_model.npz where that file has the case, else from sgn_bnstats.npz (same format)."""
    if case in su.CASES:
        c = su.load_case(case)
        return dict(meta=c['meta'], state=c['state'], x=c['x'][:BATCH[case]])
    f = _file()
    meta = json.loads(str(f[case + '.meta']))
    keys = [str(k) for k in f[case + '.keys']]
    shapes = {k: tuple(int(d) for d in s.split('x') if d) for k, s in zip(keys, (str(s) for s in f[case + '.shapes']))}
    state = su.sgn_state(shapes, meta['seed'], meta['gscale'])
    assert np.array_equal(su.checksums(state), f[case + '.checksums']), 'the seeded recipe no longer reproduces the fixture'
    return dict(meta=meta, state=state, x=f[case + '.x'])


def load_record(case):
    """The reference's record of a case: dict(logits, g, eval_logits, floor {tensor: noise floor}, and per BatchNorm name
    mean, var, rm_none, rv_none, rm_01, rv_01 as dicts {name: array})."""
    f = _file()
    rec = dict(logits=f[case + '.logits'], g=f[case + '.g'], eval_logits=f[case + '.eval_logits'],
               floor=json.loads(str(f[case + '.floor'])))
    for kind in ('mean', 'var', 'rm_none', 'rv_none', 'rm_01', 'rv_01'):
        rec[kind] = {n: f[f'{case}.{kind}.{n}'] for n in BN_NAMES}
    return rec


def err(got, ref):
    """max |got - ref| / max(1, max|ref|), in fp64."""
    ref = np.asarray(ref, dtype=np.float64)
    got = np.asarray(got.detach().cpu().numpy() if hasattr(got, 'detach') else got, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.abs(got - ref).max() / max(1.0, float(np.abs(ref).max())))


# ---- agcn_sgn_stats_finalize in numpy ----------------------------------------------------------------------------------
def group_partials(z, counts):
    """What a pass emits: z (rows, C) split into consecutive groups of ``counts`` rows -> (sum, M2 about the group's own
    mean), each (groups, C) fp32, computed in fp32 like the kernels do."""
    sums, m2s, r0 = [], [], 0
    for n in counts:
        blk = z[r0:r0 + n].astype(np.float32)
        s = blk.sum(0, dtype=np.float32)
        d = blk - (s / np.float32(n))
        sums.append(s)
        m2s.append((d * d).sum(0, dtype=np.float32))
        r0 += n
    return np.stack(sums), np.stack(m2s)


def _merge(state, nb, meanb, m2b):
    n, mean, m2 = state
    tot = n + nb
    delta = meanb - mean
    return tot, mean + delta * (nb / tot), m2 + m2b + delta * delta * (n * nb / tot)


def finalize_emulate(sums, m2s, counts, per_clip, carry=None):
    """The merge of csrc/sgn_stats.hip (sgn_stats_clip_merge_kernel, sgn_stats_finalize_kernel): the pairwise update
    with the state (n, mean, M2) in fp64; the ``per_clip`` consecutive groups of a clip in ascending order from the zero
    state, then the clips in ascending order on top of ``carry`` -> (mean fp32, biased var fp32, carry (3, C) fp64)."""
    C = sums.shape[1]
    assert len(counts) % per_clip == 0
    state = (np.zeros(C), np.zeros(C), np.zeros(C)) if carry is None else (carry[0].copy(), carry[1].copy(), carry[2].copy())
    for g0 in range(0, len(counts), per_clip):
        clip = (np.zeros(C), np.zeros(C), np.zeros(C))
        for g in range(g0, g0 + per_clip):
            if counts[g] >= 1:
                nb = float(counts[g])
                clip = _merge(clip, nb, sums[g].astype(np.float64) / nb, m2s[g].astype(np.float64))
        if clip[0][0] >= 1:
            state = _merge(state, *clip)
    n, mean, m2 = state
    return mean.astype(np.float32), (m2 / n).astype(np.float32), np.stack([n, mean, m2])
