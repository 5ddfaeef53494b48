"""CPU checks of the INPUTS of tests/test_gpu_sgn_domain.py, with the reference alone: the tables of
tests/sgn_domain_util.py lie inside the kernels' domain, the split reference is ``ops.sgn_image_forward_ref`` bit for bit,
the calibrated images keep the adjacency softmax neither flat nor one-hot, the gradient cases meet the margin condition at
their stored seeds (never searched here), every section of the whole-route gradients has a reference maximum of at least 1,
the fp32 tensor reference keeps a tenth of the bound, and every mutant -- one way each in which a kernel could be subtly
wrong -- misses the bound by at least 100 x on every case it applies to.  A case that misses a condition gets another seed
or another recipe, never a wider condition.

"Every pooled column of the reference is won by a real row" holds by construction: the reference has no padded rows (its
gcn3 output has V joint rows and its cnn2 output seg frame rows, asserted below), so its maxima cannot be taken anywhere
else; the padded rows exist only in mutants 1 and 6."""
import re

import numpy as np
import pytest
import torch

from tests import sgn_domain_util as du

ALL = [(t, i) for t in du.TABLES for i in range(len(du.TABLES[t]))]
ALL_IDS = [f'{t}-{n}' for t in du.TABLES for n in du.ids(t)]
FWD = list(range(len(du.CASES)))


def _fmt(rep):
    out = []
    for k, v in rep.items():
        if isinstance(v, dict):
            v = {n: (tuple(f'{e:.2e}' for e in t) if isinstance(t, tuple) else f'{t:.2e}') for n, t in v.items()}
        out.append(f'{k} {v if isinstance(v, dict) else format(v, ".4g")}')
    return ', '.join(out)


@pytest.mark.parametrize('table,i', ALL, ids=ALL_IDS)
def test_cases_lie_in_the_domain_and_fit_the_size_queries(table, i):
    import agcn_amd  # noqa: F401
    from agcn_amd import lib
    V, seg, nc, N = du.TABLES[table][i]
    d = du.load(table, i)
    L = lib.load()
    assert 2 <= V <= 32 and seg >= 1 and 1 <= nc <= 4096
    assert L.agcn_sgn_frames_tape_floats(N, seg, V) == N * seg * V * du.FT['cols'] > 0
    assert L.agcn_sgn_clip_tape_floats(N, seg, nc) == N * ((seg + 2) * 256 + seg * 1024 + 512) > 0
    assert L.agcn_sgn_wgrad_workspace(N, seg, V, nc, 0) > 0
    fs, cs = du._sections(d['case'])
    assert d['wf'].numel() == fs[-1][1] + int(np.prod(fs[-1][2])) and d['wc'].numel() == cs[-1][1] + int(np.prod(cs[-1][2]))
    assert d['x'].shape == (N, seg, 3 * V) and d['x'].dtype == d['wf'].dtype == d['wc'].dtype == torch.float32
    wf_t, wc_t = du.transposed(d['wf'], d['wc'], d['case'])
    assert wf_t.numel() == 2 * 64 * 64 + 128 * 512 + 256 * 128 + 256 * 256 + 512 * 256 and wc_t.numel() == 768 * 256 + 256 * 512
    # the reference has real rows only
    assert d['frames']['y'].shape == (N, seg, V, 256) and d['clip']['y'].shape == (N, seg, 512)
    assert d['frames']['g'].shape == (N, seg, V, V)
    if table == 'frames_grad':
        assert du.frames_sites(d['case']) <= du.MAX_SITES
    if table == 'clip_grad':
        assert du.clip_sites(d['case']) <= du.MAX_SITES
    if table == 'whole':
        assert du.frames_sites(d['case']) + du.clip_sites(d['case']) <= du.WHOLE_SITES


@pytest.mark.parametrize('i', FWD, ids=du.ids('fwd'))
def test_split_reference_is_the_specification(i):
    """frames_ref / clip_ref without a mutant are ops.sgn_image_forward_ref cut at feat: the same bits in fp64."""
    import agcn_amd  # noqa: F401
    d = du.load('fwd', i)
    with torch.no_grad():
        chained = du.clip_ref(d['frames']['feat'], d['wc'].double(), d['case'])
    assert torch.equal(chained['logits'], d['logits']) and torch.equal(d['frames']['g'], d['g'])
    assert d['logits'].dtype == torch.float64
    # rounding feat to fp32 moves the clip half's reference by no more than the rule allows an fp32 result to move
    assert du.check(d['feat32'], d['frames']['feat']) <= 1e-3


@pytest.mark.parametrize('table,i', ALL, ids=ALL_IDS)
def test_inputs_condition_the_comparison(table, i):
    """The calibration range, the margins at the stored seed, the section maxima, the fp32 reference's headroom and every
    applicable mutant, per case."""
    import agcn_amd  # noqa: F401
    d = du.load(table, i)
    ok, rep = du.conditions(d)
    print(f'{table} {i} {d["case"]} seed {d["seed"]} g factor {d["factor"]:.3g}: {_fmt(rep)}')
    lo, hi = du.rowmax_range(d['case'][0])
    assert lo <= rep['rowmax'] <= hi, rep['rowmax']                      # neither uniform nor one-hot
    for side in ('frames', 'clip'):
        for name, (need, found, _) in rep.get(side + '_margins', {}).items():
            assert found >= need, (side, name, need, found)
    fp32 = rep['fp32']
    assert (max(fp32.values()) if isinstance(fp32, dict) else fp32) <= 0.1, fp32
    for k, v in rep.items():
        if k.startswith('mutant'):
            assert v >= 100, (k, du.MUTANTS[int(k[6:])], v)
    if table == 'whole':
        assert rep['section_min'] >= 1.0, rep['section_min']
        assert d['cot_scale'] >= 1 and np.log2(d['cot_scale']) % 1 == 0
    assert ok


def test_every_mutant_is_exercised():
    sides = dict(fwd=('frames', 'clip'), frames_grad=('frames',), clip_grad=('clip',))
    for mutant in du.MUTANTS:
        tables = ('fwd',) if mutant in du.FORWARD_MUTANTS else ('frames_grad', 'clip_grad')
        n = sum(du.applies(mutant, s, c) for t in tables for s in sides[t] for c in du.TABLES[t])
        assert n >= 2, (mutant, du.MUTANTS[mutant])
    for mutant in du.REDUCTION_MUTANTS:
        n = sum(du.reduction_applies(mutant, 'frames', c) for c in du.FRAMES_TAPES)
        n += sum(du.reduction_applies(mutant, 'clip', c) for c in du.CLIP_TAPES)
        assert n >= 2, (mutant, du.REDUCTION_MUTANTS[mutant])


def test_tables_walk_the_listed_geometries():
    """The gaps the tables were written for: a case that is edited away fails here, not silently."""
    V, seg, nc = ({c[k] for c in du.CASES} for k in range(3))
    assert {2, 3, 16, 17, 31, 32, 15, 25} <= V and {1, 2, 31, 32, 33, 64, 65, 97} <= seg
    assert {1, 32, 33, 60, 97, 129, 257, 4096} <= nc
    assert {c[0] for c in du.FRAMES_GRAD} >= {2, 3, 16, 17, 31, 32} and {c[1] for c in du.FRAMES_GRAD} >= {1, 32}
    assert {c[1] for c in du.CLIP_GRAD} >= {1, 31, 32, 33, 64, 65} and {c[2] for c in du.CLIP_GRAD} >= {1, 257, 4096}
    assert len(du.WHOLE) == 4 and all(len(du.SEEDS[t]) == len(du.TABLES[t]) for t in du.TABLES)


# ---- the reductions ----
def test_split_plan_is_the_header_s():
    """``du.splits`` against csrc/sgn_wgrad_plan.h through the workspace query, whose size is the largest section times
    the splits of its row count."""
    import agcn_amd  # noqa: F401
    from agcn_amd import lib
    L = lib.load()
    assert (du.split_rows(8246, 0), du.splits(8246, 0), 8246 - 31 * 258) == (258, 32, 248)
    assert (du.split_rows(8450, 0), du.splits(8450, 0), 8450 - 31 * 266) == (266, 32, 204)
    assert [du.splits(R, 0) for R in (2, 3, 255, 256, 257, 258, 297, 1280, 8192, 8193)] == [1, 1, 1, 1, 2, 2, 2, 5, 32, 32]
    assert du.splits(1000, 7) == 143 and du.splits(1500, 32) == 47
    geos = [(N, seg, V, 60, rps) for V, seg, N, rps in du.FRAMES_TAPES] + [(N, seg, 2, nc, rps) for seg, nc, N, rps in du.CLIP_TAPES]
    for N, seg, V, nc, rps in geos:
        frames, rows = N * seg, N * seg * V
        want = max([e * du.splits(rows, rps) for e in (512 * 256, 128 * 512, 2 * 3 * 64)]
                   + [e * du.splits(frames, rps) for e in (V * 64, 4 * V * 3, 256 * 512)]
                   + [e * du.splits(N, rps) for e in (seg * 256, 512 * nc)])
        assert L.agcn_sgn_wgrad_workspace(N, seg, V, nc, rps) == 4 * want, (N, seg, V, nc, rps)


def _reduction_case(side, case):
    if side == 'frames':
        x, tape = du.frames_tape_inputs(case)
        return lambda mutant=0, dtype=np.float64: du.frames_tape_ref(x, tape, case, mutant, dtype)
    tape, dfeat, dlogits = du.clip_tape_inputs(case)
    return lambda mutant=0, dtype=np.float64: du.clip_tape_ref(tape, dfeat, dlogits, case, mutant, dtype)


TAPES = [('frames', c) for c in du.FRAMES_TAPES] + [('clip', c) for c in du.CLIP_TAPES]


@pytest.mark.parametrize('side,case', TAPES, ids=[f'{s}-{"x".join(map(str, c))}' for s, c in TAPES])
def test_reduction_mutants_are_caught(side, case):
    ref_of = _reduction_case(side, case)
    ref = ref_of()
    # the fp32 evaluation of the same sums keeps a tenth of the bound
    r32 = du.reduction_ratios(ref_of(0, np.float32), ref)
    worst = max(r32, key=r32.get)
    print(f'{side} tape {case} fp32 sums vs fp64: worst {worst} {r32[worst]:.3e}')
    assert r32[worst] <= 0.1, r32
    for mutant in du.REDUCTION_MUTANTS:
        if not du.reduction_applies(mutant, side, case):
            continue
        r = du.reduction_ratios(ref_of(mutant), ref)
        worst = max(r, key=r.get)
        print(f'{side} tape {case} mutant {mutant}: {worst} {r[worst]:.4g} bounds')
        assert r[worst] >= 100, (mutant, du.REDUCTION_MUTANTS[mutant], r)


def test_tape_layout_is_the_header_s():
    """The column offsets of ``du.FT`` against the SgnFramesTape of csrc/sgn_wgrad_plan.h, read as text."""
    import os
    import agcn_amd  # noqa: F401
    from agcn_amd import lib
    with open(os.path.join(os.path.dirname(os.path.abspath(lib.__file__)), 'csrc', 'sgn_wgrad_plan.h')) as fh:
        src = fh.read()
    body = src[src.index('SGN_HD SgnFramesTape sgn_frames_tape()'):src.index('t.cols =')]
    width = {'SGN_C1': 64, 'SGN_C2': 128, 'SGN_C3': 256, '2 * SGN_C3': 512, '8': 8, '6': 6}
    o = 0
    for name, w in re.findall(r't\.(\w+) = o;\s*o \+= ([^;]+);', body):
        assert du.FT[name] == o, name
        o += width[w.strip()]
    assert o == 2638 and du.FT['cols'] == (o + 31) // 32 * 32
