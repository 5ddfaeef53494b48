"""Shared by the SGN input-gradient tests and tests/golden/make_golden_sgn_grad.py: the case list of
tests/golden/sgn_evalgrad.npz, what a case changes in the seeded recipe and in its input, the fixture loader, and a
numpy emulation of ``agcn_sgn_sample_bwd`` that pins its specification (fp32 adds, draws major, intervals minor)."""
import json

import numpy as np

from tests import sgn_util as su

GRAD_CASES = ('v25_seg2', 'v15_seg6', 'v7_seg12_nobias', 'v2_seg40', 'v3_seg34', 'v15_seg3_guard')
OPTIONAL_GRAD_CASES = ('v15_seg4_sharp',)          # stored only if the seed search found it
MARGIN = 2e-5
GUARD_JOINT = 3


def case_state(state, meta):
    """The recipe's state as the case runs it.  'guard': gcn3's folded bias is large and positive, so the padded joint
    rows of the fused path hold relu(bias) >> 0, which must stay out of the arg-max over the joints."""
    state = dict(state)
    if meta.get('kind') == 'guard':
        state['gcn3.bn.bias'] = np.full_like(state['gcn3.bn.bias'], 4.0)
        state['gcn3.bn.running_mean'] = np.zeros_like(state['gcn3.bn.running_mean'])
    return state


def case_input(x, meta):
    """'guard': every input of one joint is negative."""
    if meta.get('kind') != 'guard':
        return x
    v = meta['num_point']
    y = x.reshape(x.shape[0], x.shape[1], v, 3).copy()
    y[:, :, GUARD_JOINT, :] = -np.abs(y[:, :, GUARD_JOINT, :]) - 0.5
    return y.reshape(x.shape)


def stored_cases():
    f = su._npz('sgn_evalgrad.npz')
    return tuple(c for c in GRAD_CASES + OPTIONAL_GRAD_CASES if c + '.meta' in f)


def load_grad_case(case):
    """-> dict(meta, state (regenerated, checked against the stored checksums, with the case's changes), x, c, logits, g,
    grad_x, grad_x64)."""
    f = su._npz('sgn_evalgrad.npz')
    meta = json.loads(str(f[case + '.meta']))
    keys = [str(k) for k in f[case + '.keys']]
    shapes = {k: tuple(int(d) for d in s.split('x') if d) for k, s in zip(keys, (str(s) for s in f[case + '.shapes']))}
    state = su.sgn_state(shapes, meta['seed'], meta['gscale'])
    assert np.array_equal(su.checksums(state), f[case + '.checksums']), 'the seeded recipe no longer reproduces the fixture'
    out = dict(meta=meta, state=case_state(state, meta))
    out.update({k: f[f'{case}.{k}'] for k in ('x', 'c', 'logits', 'g', 'grad_x', 'grad_x64')})
    return out


def sample_bwd_emulate(win, r, dout, seg):
    """The adjoint of ``sgn_util.sample_emulate``: win (N, 3, T, V, 2), r (N, S, seg) uint32, dout (N, S, seg, V*3) fp32
    -> dwin (N, 3, T, V, 2) fp32.  Zero, then row by row dwin[source row of pick (s, k)] += dout[s, k] in fp32, s major
    and k minor; picks of the zero padding (idx >= kept rows) and empty windows add nothing."""
    N, C, T, V, K = win.shape
    assert C == 3 and K == 2 and dout.dtype == np.float32
    S = r.shape[1]
    dwin = np.zeros(win.shape, dtype=np.float32)
    for n in range(N):
        rows = np.transpose(win[n], (1, 3, 2, 0)).reshape(T * 2, V * 3)          # (t, m) major, (v, c) minor
        src = np.flatnonzero((rows != 0).any(1))
        if len(src) == 0:
            continue
        L = max(len(src), seg)
        b = su.sample_intervals(L, seg)
        for s in range(S):
            idx = b[:-1] + (r[n, s].astype(np.int64) % (b[1:] - b[:-1]))
            for k in range(seg):
                if idx[k] < len(src):
                    t, m = divmod(int(src[idx[k]]), 2)
                    dwin[n, :, t, :, m] += dout[n, s, k].reshape(V, 3).T
    return dwin
