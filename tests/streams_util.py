"""Shared by tests/test_streams_cpu.py and tests/test_gpu_streams.py: the reference-generated fixtures
(tests/golden/make_golden_streams.py), the parent tables read out of the reference's `pairs`, and the fp64 form of the
streams' backward with the error bound that follows from its fixed summation order."""
import functools
import itertools
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
DERIVED = ('bone', 'joint_motion', 'bone_motion')
STREAMS = ('joint',) + DERIVED
SUBSETS = [c for r in (1, 2, 3) for c in itertools.combinations(DERIVED, r)]
WEIGHTS = (1.0, 0.5, -2.0, 3.0)
U = 2.0 ** -24         # unit roundoff of fp32


@functools.lru_cache(maxsize=None)
def fixture(name):
    """'ntu' / 'kinetics' -> dict of read-only arrays"""
    data = dict(np.load(os.path.join(GOLDEN, f'streams_{name}.npz')))
    for a in data.values():
        a.setflags(write=False)
    return data


def parents_from_pairs(pairs, V, one_based):
    """The reference's (joint, parent) rows -> parent per joint; a joint without a row would be its own parent."""
    parent = list(range(V))
    seen = set()
    for v1, v2 in np.asarray(pairs).tolist():
        v1, v2 = (v1 - 1, v2 - 1) if one_based else (v1, v2)
        assert v1 not in seen
        seen.add(v1)
        parent[v1] = v2
    return parent


def graph_parents(V):
    import agcn_amd  # noqa: F401
    from agcn_amd.graph import kinetics, ntu_rgb_d, openpose_b25_j15
    return {25: ntu_rgb_d, 18: kinetics, 15: openpose_b25_j15}[V].Graph().bone_parents


def motion_t64(d):
    out = np.zeros_like(d)
    out[:, :, 1:] += d[:, :, :-1]
    out[:, :, :-1] -= d[:, :, :-1]
    return out


def bone_t64(d, parent):
    out = d.copy()
    for c, p in enumerate(parent):
        out[:, :, :, p] -= d[:, :, :, c]
    return out


def backward64(cot, parent, weights=WEIGHTS):
    """cot: dict stream -> fp32 / fp64 array (absent: nothing).  -> (dx in fp64, sum |addend|, number of addends n), the
    addends being the leaves of the weighted sum: w * d for every cotangent element that reaches the dx element."""
    dx = mag = cnt = None
    for name, w in zip(STREAMS, weights):
        if cot.get(name) is None:
            continue
        d = np.asarray(cot[name], dtype=np.float64)
        a, one = np.abs(d), np.ones_like(d)
        if name.endswith('motion'):
            d = motion_t64(d)
            # |.| of the leaves: the same stencil with every sign positive
            ap, op = np.zeros_like(a), np.zeros_like(one)
            for src, dst in ((a, ap), (one, op)):
                dst[:, :, 1:] += src[:, :, :-1]
                dst[:, :, :-1] += src[:, :, :-1]
            a, one = ap, op
        if name.startswith('bone'):
            d = bone_t64(d, parent)
            ap, op = a.copy(), one.copy()
            for c, p in enumerate(parent):
                ap[:, :, :, p] += a[:, :, :, c]
                op[:, :, :, p] += one[:, :, :, c]
            a, one = ap, op
        term, tmag = w * d, abs(w) * a
        dx = term if dx is None else dx + term
        mag = tmag if mag is None else mag + tmag
        cnt = one if cnt is None else cnt + one
    return dx, mag, cnt


def backward_bound(mag, cnt):
    """|dx_fp32 - dx_exact| <= n * 2^-24 * sum |addend| per element.  Derivation: the kernel adds the n leaves of an
    element with n - g additions inside the g streams, g multiplications by the weights and g - 1 additions across them (an
    FMA only removes roundings).  Each addition errs by at most u times a partial sum, itself at most sum |addend|; the g
    multiplications err by u times their own stream's share each, together at most u * sum |addend|: (n - g) + 1 + (g - 1)
    = n roundings of at most u * sum |addend| (first order in u).  An element with no addend (motion of T = 1) is exact."""
    return cnt * U * mag
