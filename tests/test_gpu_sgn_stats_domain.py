"""GPU checks of the SGN batch-statistics kernels (csrc/sgn_stats.hip and the ``colstats`` epilogue of csrc/sgn_device.h)
over the tables of tests/sgn_stats_domain_util.py against fp64:

  each pass alone      ``ops.sgn_input_stats`` / ``sgn_frames_stats`` / ``sgn_clip_stats`` on the seeded images of
                       tests/sgn_domain_util.py, which have no BatchNorm in them: the partials group by group and the
                       finalize's mean and variance against the ReLU pre-activation of the fp64 reference
  badly centred data   the same passes on copies whose measured bias (the input pass: x) is shifted by +-512: the variance
                       per channel relative to the channel's own variance, under ``REL_VAR``
  the finalize alone   ``ops.sgn_stats_finalize`` on seeded partials, whole and in uneven chunks through the carry
  the seven passes     ``SGN.batch_statistics`` / ``recalibrate_bn`` at the domain's edges against the fp64 composition

Bound: the project's fp32 rule per tensor, 1e-4 relative to max(1, max|reference tensor|); the printed ratios are multiples
of it (measured on MI355X: profiles/sgn_stats_domain.txt).  What makes these inputs able to show an error is asserted in
tests/test_sgn_stats_domain_cpu.py."""
import copy

import numpy as np
import pytest
import torch

from tests import sgn_domain_util as du
from tests import sgn_stats_domain_util as sd

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
SENTINEL = 1024
MARK = -777.0
CASE_IDS = dict(argvalues=list(range(len(sd.CASES))), ids=du.ids('fwd'))


def _report(what, r):
    print(f'sgn_stats_domain: {what}: ' + ' '.join(f'{k} {v:.3e}' for k, v in r.items()))
    assert all(v <= 1.0 for v in r.values()), (what, r)


def _guarded(n):
    """n floats with SENTINEL marked floats behind them -> (the buffer, its first n floats)."""
    buf = torch.full((n + SENTINEL,), MARK, device=DEV)
    return buf, buf[:n]


def _untouched(buf, n):
    return bool((buf[n:] == MARK).all())


def _launch(kind, layer, d, x=None, wf=None, wc=None, clips=slice(None)):
    """Pass (kind, layer) on the case's input (or its replacements), on the clips ``clips`` -> part (groups, 2, C)."""
    from agcn_amd import ops
    V, _, nc, _ = d['case']
    if kind == sd.INPUT:
        return ops.sgn_input_stats((d['x'] if x is None else x)[clips].contiguous().to(DEV), V)
    if kind == sd.FRAMES:
        return ops.sgn_frames_stats(d['x'][clips].contiguous().to(DEV), (d['wf'] if wf is None else wf).to(DEV), layer, V)
    return ops.sgn_clip_stats(d['feat32'][clips].contiguous().to(DEV), (d['wc'] if wc is None else wc).to(DEV), layer, nc)


# ---- 1. each pass alone on the seeded images ----
@pytest.mark.parametrize('kind,layer', sd.PASSES, ids=[sd.PASS_NAMES[p] for p in sd.PASSES])
@pytest.mark.parametrize('i', **CASE_IDS)
def test_pass_alone(i, kind, layer):
    import agcn_amd  # noqa: F401
    from agcn_amd import lib, ops
    d = du.load('fwd', i)
    V, seg, nc, N = d['case']
    name = sd.PASS_NAMES[kind, layer]
    z, counts = sd.table(d, kind, layer)
    C, per = sd.channels(kind, layer, V), sd.groups_per_clip(kind, seg)
    sums, m2s = sd.group_ref(z, counts)
    part = _launch(kind, layer, d)
    assert tuple(part.shape) == (N * per, 2, C) == (len(counts), 2, z.shape[1]) and bool(torch.isfinite(part).all())
    mean, var, _ = ops.sgn_stats_finalize(part, kind, layer, N, seg, V)
    print(f'sgn_stats_domain: case {i} {d["case"]} pass {name} relative variance error {sd.rel_var(var, z.var(0)):.3e} '
          f'(variances {z.var(0).min():.3e} .. {z.var(0).max():.3e})')
    _report(f'case {i} {d["case"]} pass {name} rows {len(z)} vs fp64',
            dict(sum=sd.check(part[:, 0], sums), m2=sd.check(part[:, 1], m2s), mean=sd.check(mean, z.mean(0)), var=sd.check(var, z.var(0))))
    # exact values
    p = part.cpu().numpy()
    assert float(p[:, 1].min()) >= 0.0
    if kind == sd.CLIP and seg % sd.ROWS == 1:             # the last tile is one row: no spread, and the sum is that row
        last = p[per - 1::per]
        assert counts[per - 1] == 1 and not last[:, 1].any()
        assert sd.check(last[:, 0], z.reshape(N, seg, C)[:, -1]) <= 1.0
    if kind == sd.INPUT and seg == 1:                      # single-frame groups; dif is its zero at t = 0 alone
        assert not p[:, 1].any() and not p[:, 0, C // 2:].any()
        assert np.array_equal(p[:, 0, :C // 2], d['x'].numpy().reshape(N, C // 2))
    # the same bits again, and for clip 1 alone
    assert torch.equal(_launch(kind, layer, d), part)
    assert torch.equal(_launch(kind, layer, d, clips=slice(1, 2)), part[per:2 * per])
    # through the C entries on buffers of exactly the queried sizes
    L = lib.load()
    n = L.agcn_sgn_stats_part_floats(kind, layer, N, seg, V)
    nws = L.agcn_sgn_stats_finalize_workspace(kind, layer, N, seg, V) // 4
    assert n == part.numel() and nws == N * 3 * C * 2
    buf, own = _guarded(n)
    if kind == sd.INPUT:
        lib.call("agcn_sgn_input_stats", d['x'].to(DEV), own, n, N, seg, V)
    elif kind == sd.FRAMES:
        wf = d['wf'].to(DEV)
        lib.call("agcn_sgn_frames_stats", d['x'].to(DEV), wf, wf.numel(), own, n, layer, N, seg, V)
    else:
        wc = d['wc'].to(DEV)
        lib.call("agcn_sgn_clip_stats", d['feat32'].to(DEV), wc, wc.numel(), own, n, layer, N, seg, nc)
    wbuf, ws = _guarded(nws)
    obuf, out = _guarded(2 * C)
    lib.call("agcn_sgn_stats_finalize", own, n, kind, layer, N, seg, V, None, None, out[:C], out[C:], ws, nws * 4)
    torch.cuda.synchronize()
    assert _untouched(buf, n) and _untouched(wbuf, nws) and _untouched(obuf, 2 * C)
    assert torch.equal(own, part.view(-1)) and torch.equal(out[:C], mean) and torch.equal(out[C:], var)


# ---- 2. badly centred data through the real kernels ----
@pytest.mark.parametrize('kind,layer', sd.PASSES, ids=[sd.PASS_NAMES[p] for p in sd.PASSES])
@pytest.mark.parametrize('i', sd.OFFSET_CASES, ids=[du.ids('fwd')[i] for i in sd.OFFSET_CASES])
def test_pass_on_badly_centred_data(i, kind, layer):
    import agcn_amd  # noqa: F401
    from agcn_amd import ops
    d = du.load('fwd', i)
    V, seg, _, N = d['case']
    shifted = sd.offset_inputs(d, kind, layer)
    z, counts = sd.table(d, kind, layer, **shifted)
    assert len(z) >= 64
    part = _launch(kind, layer, d, **shifted)
    mean, var, _ = ops.sgn_stats_finalize(part, kind, layer, N, seg, V)
    rel = sd.rel_var(var, z.var(0))
    r = dict(mean=sd.check(mean, z.mean(0)), rel_var=rel / sd.REL_VAR)
    print(f'sgn_stats_domain: offset {sd.OFFSET:g} case {i} {d["case"]} pass {sd.PASS_NAMES[kind, layer]} rows {len(z)}: '
          f'relative variance error {rel:.3e} (REL_VAR {sd.REL_VAR:g}), mean {r["mean"]:.3e} bounds')
    assert float(part[:, 1].min()) >= 0.0
    assert r['mean'] <= 1.0 and rel <= sd.REL_VAR, r


# ---- 3. the finalize alone on seeded partials ----
@pytest.mark.parametrize('i', list(range(len(sd.FINALIZE))), ids=sd.finalize_ids())
def test_finalize_alone(i):
    import agcn_amd  # noqa: F401
    from agcn_amd import ops
    kind, layer, N, seg, V, chunks, recipe = sd.FINALIZE[i]
    p, counts, z = sd.finalize_inputs(i)
    per = sd.groups_per_clip(kind, seg)
    C = sd.channels(kind, layer, V)
    assert p.shape == (N * per, 2, C) and sum(chunks) == N
    part = torch.from_numpy(p).to(DEV)
    mean, var, carry = ops.sgn_stats_finalize(part, kind, layer, N, seg, V, want_carry=True)
    r_mean, r_var, r_carry = sd.merge_ref(p[:, 0], p[:, 1], counts)
    assert np.array_equal(carry[0].cpu().numpy(), np.full(C, float(sum(counts)))) and sum(counts) == r_carry[0, 0]
    _report(f'finalize {i} {sd.FINALIZE[i]} groups {len(counts)} vs the fp64 merge',
            dict(mean=sd.check(mean, r_mean), var=sd.check(var, r_var), carry_mean=sd.check(carry[1], r_carry[1]),
                 carry_m2=sd.check(carry[2], r_carry[2])))
    if recipe == 'centred50':
        rel = sd.rel_var(var, z.astype(np.float64).var(0))
        print(f'sgn_stats_domain: finalize {i} |mean| = 50 std: relative variance error {rel:.3e}')
        assert rel < 1e-4, rel
    # without the carry out; on a carry of zeros; in uneven chunks of whole clips through the carry: the same bits
    m2, v2, none = ops.sgn_stats_finalize(part, kind, layer, N, seg, V)
    assert none is None and torch.equal(m2, mean) and torch.equal(v2, var)
    zeros = torch.zeros(3, C, dtype=torch.float64, device=DEV)
    m2, v2, c2 = ops.sgn_stats_finalize(part, kind, layer, N, seg, V, carry=zeros, want_carry=True)
    assert torch.equal(m2, mean) and torch.equal(v2, var) and torch.equal(c2, carry)
    state, n0 = None, 0
    for n in chunks:
        m2, v2, state = ops.sgn_stats_finalize(part[n0 * per:(n0 + n) * per].contiguous(), kind, layer, n, seg, V, carry=state,
                                               want_carry=True)
        n0 += n
    assert torch.equal(m2, mean) and torch.equal(v2, var) and torch.equal(state, carry)


# ---- 4. the seven passes in sequence, through the model ----
_RUNS = {}


def _counters():
    from agcn_amd import ops
    return dict(ops.SGN_BNSTATS_STATS), dict(ops.SGN_STATS)


def _run(i):
    if i not in _RUNS:
        r = sd.load_model(i)
        m, x = copy.deepcopy(r['m']).to(DEV), r['x'].to(DEV)
        b0, s0 = _counters()
        logits, g, stats = m.batch_statistics(x)
        b1, s1 = _counters()
        _RUNS[i] = dict(m=m, x=x, logits=logits, g=g, stats=stats, launches={k: b1[k] - b0[k] for k in b1},
                        plain={k: s1[k] - s0[k] for k in s1})
    return _RUNS[i]


@pytest.mark.parametrize('i', list(range(len(sd.MODEL_CASES))), ids=sd.model_ids())
def test_seven_passes_through_the_model(i):
    from agcn_amd import ops
    V, seg, nc, N = sd.MODEL_CASES[i]
    run, (l64, g64, s64) = _run(i), sd.load_model(i)['ref']
    assert run['launches'] == dict(input_stats=1, frames_stats=3, clip_stats=2, stats_finalize=6)
    assert run['plain'] == dict(frames_hip=1, clip_hip=1, sample_hip=0, forward_tensor=0)
    assert tuple(run['stats']) == ops.SGN_BN_NAMES
    for k, n in enumerate(ops.SGN_BN_NAMES):
        assert run['stats'][n][2] == s64[n][2] == (N * seg * V if 2 <= k < 5 else N * seg), n
    r = sd.stats_ratios(run['stats'], s64)
    r['logits'], r['g'] = sd.check(run['logits'], l64), sd.check(run['g'], g64)
    _report(f'model {i} {sd.MODEL_CASES[i]} seven passes vs the fp64 composition', r)
    if N >= 4:                                              # uneven chunks of whole clips: the same bits
        for clips in (1, 3):
            cap = clips * ops.sgn_stats_clip_bytes(seg, V)
            assert ops.sgn_stats_chunk(N, seg, V, cap) == clips
            b0, _ = _counters()
            logits, g, stats = run['m'].batch_statistics(run['x'], max_part_bytes=cap)
            b1, _ = _counters()
            assert b1['stats_finalize'] - b0['stats_finalize'] == 6 * -(-N // clips)
            assert torch.equal(logits, run['logits']) and torch.equal(g, run['g'])
            for n in ops.SGN_BN_NAMES:
                assert torch.equal(stats[n][0], run['stats'][n][0]) and torch.equal(stats[n][1], run['stats'][n][1]), n


@pytest.mark.parametrize('momentum', [None, 0.1])
@pytest.mark.parametrize('i', sd.RECALIBRATED, ids=[sd.model_ids()[i] for i in sd.RECALIBRATED])
def test_recalibration_at_the_edges(i, momentum):
    from agcn_amd import ops
    r = sd.load_model(i)
    m = copy.deepcopy(r['m']).to(DEV)
    m.recalibrate_bn(r['x'].to(DEV), momentum=momentum)
    out = {}
    for n in ops.SGN_BN_NAMES:
        mean, var, count = r['ref'][2][n]
        unbiased = var * (count / (count - 1))
        f = 1.0 if momentum is None else momentum          # after the reset: mean 0, variance 1, one batch tracked
        want_m, want_v = torch.zeros_like(mean), torch.ones_like(var)
        bn = m.get_submodule(n)
        assert int(bn.num_batches_tracked) == 1
        out['running_mean.' + n] = sd.check(bn.running_mean, (1 - f) * want_m + f * mean)
        out['running_var.' + n] = sd.check(bn.running_var, (1 - f) * want_v + f * unbiased)
    _report(f'model {i} {sd.MODEL_CASES[i]} recalibrate_bn momentum {momentum} vs the fp64 composition', out)
