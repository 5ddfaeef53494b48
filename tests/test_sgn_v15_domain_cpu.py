"""CPU checks of the INPUTS of tests/test_gpu_sgn_v15_domain.py, with the reference alone: the table of
tests/sgn_v15_domain_util.py lies inside the kernels' domain, its seeded images condition the comparison (a softmax that
is neither flat nor one-hot, negative maxima, every token row the arg-max of some output column), the fp32 tensor
reference keeps a tenth of the bound, and every mutant of the reference -- one way each in which ``sgn15_block`` could be
subtly wrong -- misses the bound by at least 100 x.  A case that misses a condition gets another seed, never a wider
condition."""
import math

import pytest
import torch

from tests import sgn_v15_domain_util as du

CASE_IDS = list(range(len(du.CASES)))
SIDES = ('frames', 'clip')


def _block(case, side):
    """(rows, (heads, d_head, ff)) of a case's block."""
    return (case[0], case[2]) if side == 'frames' else (case[1], case[3])


def conditions(d):
    """The measured input conditions of one made case (also used when a seed is chosen)."""
    V, seg = d['case'][0], d['case'][1]
    out = {}
    for side, rows, a, y in (('frames', V, d['frames']['attn'], d['frames']['y']), ('clip', seg, d['clip']['attn'], d['clip']['z'])):
        out[side + '_rowmax'] = float(a.amax(-1).mean())
        winners = y[:, :rows].argmax(1)                                  # (token sets, columns): the row that wins a column
        out[side + '_rows_unobserved'] = sum(rows - int(torch.unique(w).numel()) for w in winners)
        out[side + '_indices_unobserved'] = rows - int(torch.unique(winners).numel())
    out['feat_negative'] = float((d['feat'] < 0).double().mean())
    out['pooled_negative'] = float((d['clip']['pooled'] < 0).double().mean())
    return out


def conditions_met(d):
    c = conditions(d)
    ok = c['feat_negative'] >= 0.1 and c['pooled_negative'] >= 0.1
    for side in SIDES:
        rows, _ = _block(d['case'], side)
        rows_seen = '_indices_unobserved' if side == 'frames' and d['case'] in du.FRAMES_ROWS_BY_INDEX else '_rows_unobserved'
        ok = ok and c[side + rows_seen] == 0 and (rows < 3 or 1.5 / rows <= c[side + '_rowmax'] <= 0.8)
    return ok, c


def fp32_ratios(d):
    """The fp32 run of the tensor reference against its fp64 run: the whole forward, and the clip half alone on feat32."""
    from agcn_amd import ops
    V, seg, sp, tp, num_class = d['case']
    with torch.no_grad():
        logits, feat, sa, ta = ops.sgn15_forward_ref(d['x'], d['wf'], d['wc'], V, seg, num_class, sp, tp)
        clip = du.clip_ref(d['feat32'], d['wc'], d['case'])
    return dict(frames=dict(feat=du.check(feat, d['feat']), spatial_attn=du.check(sa, d['spatial_attn'])),
                chained=dict(logits=du.check(logits, d['logits']), temporal_attn=du.check(ta, d['temporal_attn'])),
                clip=dict(logits=du.check(clip['logits'], d['clip']['logits']), temporal_attn=du.check(clip['attn'], d['clip']['attn'])))


def mutant_ratios(d, side, mutant):
    """The worst ratio per compared tensor of one mutant of the side's reference, on the inputs the GPU test uses."""
    with torch.no_grad():
        if side == 'frames':
            m = du.frames_ref(d['x'].double(), d['wf'].double(), d['case'], mutant)
            return dict(feat=du.check(m['feat'], d['frames']['feat']), spatial_attn=du.check(m['attn'], d['frames']['attn']))
        m = du.clip_ref(d['feat32'].double(), d['wc'].double(), d['case'], mutant)
        return dict(logits=du.check(m['logits'], d['clip']['logits']), temporal_attn=du.check(m['attn'], d['clip']['attn']))


@pytest.mark.parametrize('i', CASE_IDS, ids=du.IDS)
def test_images_fit_the_size_queries(i):
    import agcn_amd  # noqa: F401
    from agcn_amd import lib, ops
    V, seg, sp, tp, num_class = du.CASES[i]
    d = du.load(i)
    L = lib.load()
    nf, nc = L.agcn_sgn15_frames_weights(V, *sp), L.agcn_sgn15_clip_weights(seg, num_class, *tp)
    assert nf > 0 and nc > 0, 'outside sgn15_block_domain: the model would take the composition'
    assert (d['wf'].numel(), d['wc'].numel()) == (nf, nc) == ops.sgn15_weights_floats(V, seg, num_class, sp, tp)
    assert d['x'].shape == (du.N_CLIPS, seg, 3 * V) and du.N_CLIPS <= 3
    assert d['wf'].dtype == d['wc'].dtype == d['x'].dtype == torch.float32 and d['logits'].dtype == torch.float64
    assert all(bool(torch.isfinite(t).all()) for t in (d['wf'], d['wc'], d['logits'], d['feat']))


@pytest.mark.parametrize('i', CASE_IDS, ids=du.IDS)
def test_split_reference_is_the_specification(i):
    """frames_ref / clip_ref without a mutant are ops.sgn15_forward_ref cut at feat: the same bits in fp64."""
    import agcn_amd  # noqa: F401
    d = du.load(i)
    with torch.no_grad():
        chained = du.clip_ref(d['feat'], d['wc'].double(), d['case'])
    assert torch.equal(d['frames']['feat'], d['feat']) and torch.equal(d['frames']['attn'], d['spatial_attn'])
    assert torch.equal(chained['logits'], d['logits']) and torch.equal(chained['attn'], d['temporal_attn'])
    # rounding feat to fp32 moves the clip half's reference by no more than the rule allows an fp32 result to move
    assert du.check(d['feat32'], d['feat']) <= 1e-3


@pytest.mark.parametrize('i', CASE_IDS, ids=du.IDS)
def test_inputs_condition_the_comparison(i):
    import agcn_amd  # noqa: F401
    d = du.load(i)
    ok, c = conditions_met(d)
    print(f'case {i} seed {d["seed"]} q factors {d["qk_factor"][0]:.3f} {d["qk_factor"][1]:.3f}: '
          + ', '.join(f'{k} {v:.3g}' for k, v in c.items()))
    for side in SIDES:
        rows, _ = _block(d['case'], side)
        if rows >= 3:                                   # neither uniform nor one-hot
            assert 1.5 / rows <= c[side + '_rowmax'] <= 0.8, (side, c)
        # no row's feed-forward output hides behind the maximum (per row index where no seed can do better: see
        # sgn_v15_domain_util.FRAMES_ROWS_BY_INDEX and its companion cases)
        by_index = side == 'frames' and d['case'] in du.FRAMES_ROWS_BY_INDEX
        assert c[side + ('_indices_unobserved' if by_index else '_rows_unobserved')] == 0, (side, c)
    assert c['feat_negative'] >= 0.1 and c['pooled_negative'] >= 0.1, c
    assert ok


@pytest.mark.parametrize('i', CASE_IDS, ids=du.IDS)
def test_fp32_reference_has_headroom(i):
    import agcn_amd  # noqa: F401
    r = fp32_ratios(du.load(i))
    for part, v in r.items():
        print(f'case {i} {part} fp32 reference vs fp64, in bounds: ' + ' '.join(f'{k} {e:.3e}' for k, e in v.items()))
    assert all(e <= 0.1 for v in r.values() for e in v.values()), r


@pytest.mark.parametrize('i', CASE_IDS, ids=du.IDS)
def test_every_applicable_mutant_is_caught(i):
    import agcn_amd  # noqa: F401
    d = du.load(i)
    applied = 0
    for side in SIDES:
        rows, geometry = _block(d['case'], side)
        for mutant in du.MUTANTS:
            if not du.applies(mutant, side, rows, geometry):
                continue
            r = mutant_ratios(d, side, mutant)
            print(f'case {i} {side} mutant {mutant}, in bounds: ' + ' '.join(f'{k} {e:.3g}' for k, e in r.items()))
            assert max(r.values()) >= 100, (side, mutant, du.MUTANTS[mutant], r)
            applied += 1
    assert applied >= 2                                 # mutant 3 applies to both sides of every case


def test_every_mutant_is_exercised_on_both_kernels():
    for mutant in du.MUTANTS:
        for side in SIDES:
            n = sum(du.applies(mutant, side, *_block(c, side)) for c in du.CASES)
            assert n >= 1 or (mutant in (1, 2) and side == 'frames'), (mutant, side)


def test_companion_cases_observe_every_row_of_the_large_frames():
    """Each case whose frames block is held to the per-index form has a case with the same joints and spatial geometry
    that is held to the condition as stated."""
    strict = [c for c in du.CASES if c not in du.FRAMES_ROWS_BY_INDEX]
    for c in du.FRAMES_ROWS_BY_INDEX:
        assert any(s[0] == c[0] and s[2] == c[2] for s in strict), c


def test_table_walks_the_listed_geometries():
    """The gaps the table was written for, per kernel: a case that is edited away fails here, not silently."""
    assert len(du.CASES) == len(du.SEEDS) == len(du.IDS) >= 12
    for side in SIDES:
        blocks = [_block(c, side) for c in du.CASES]
        geo = [g for _, g in blocks]
        rows = {r for r, _ in blocks}
        inner = lambda g: g[0] * g[1]                               # noqa: E731
        assert {16, 32, 64, 128, 256, 384, 512} <= {g[1] for g in geo}
        assert any(g[1] == 16 and inner(g) > 128 for g in geo) and any(g[:2] == (64, 16) for g in geo)
        assert any(g[1] == 64 and inner(g) > 128 for g in geo) and any(g[1] == 32 and inner(g) >= 512 for g in geo)
        assert any(g[1] >= 128 and g[0] > 1 for g in geo) and any(g[1] == 128 and g[0] == 1 for g in geo)
        assert any(g[2] > 128 for g in geo) and any(g[2] == 1024 for g in geo)
        assert {16, 17, 31, 32} <= rows and min(rows) == (2 if side == 'frames' else 1)
    assert any(c[2][1] == 1024 for c in du.CASES)                   # 1 x 1024 at 128 -> 256
    assert {1, 4096} <= {c[4] for c in du.CASES} and any(256 < c[4] < 4096 for c in du.CASES)
    assert all(math.prod(c[2][:2]) <= 1024 and math.prod(c[3][:2]) <= 1024 for c in du.CASES)
