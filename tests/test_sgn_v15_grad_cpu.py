"""CPU side of the SGN v15 input-gradient tests: the plan header compiled for the host, the conditions that make the
seeded table of tests/sgn_v15_grad_util.py able to show an error on the GPU (margins, maps, fp32 headroom, mutants), the
transposed images, the whole-model fixture against the composition's autograd, and the margin of the online case."""
import copy
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import sgn_v15_domain_util as du
from tests import sgn_v15_grad_util as gu
from tests import sgn_v15_util as vu

ROOT = vu.ROOT


def test_sgn_v15_bwd_plan_checker(tmp_path):
    cxx = next((c for c in (os.environ.get('CXX'), 'c++', 'g++', 'clang++') if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip('no host C++ compiler')
    exe = str(tmp_path / 'sgn_v15_bwd_plan_check')
    r = subprocess.run([cxx, '-std=c++17', '-Wall', '-Werror', '-O1', '-I', os.path.join(ROOT, '2s-agcn_amd', 'csrc'),
                        os.path.join(ROOT, 'tests', 'sgn_v15_bwd_plan_check.cpp'), '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-4000:]
    assert ' cases, 0 failures' in r.stdout and int(r.stdout.split(' cases')[0].split()[-1]) > 5000


def test_table_walks_what_it_claims():
    assert len(gu.CASES) == len(gu.SEEDS) == 10
    for i, case in enumerate(gu.CASES):
        assert sum(gu.sites(case)) <= gu.MAX_SITES, (i, gu.sites(case))
        assert 100 * i + 1 <= gu.SEEDS[i] <= 100 * i + gu.SEARCH
    c = gu.CASES
    assert c[0][2][1] == 16 and c[0][5] == 2 and c[9][1] == 1 and c[9][5] == 2          # batch cases: 0 and 9
    assert c[3][0] == 32 and c[4][1] == 32 and c[3][4] > 256 and c[8][4] == 4096
    assert c[6][2][1] == 256 and c[7][2][1] == 384 and c[7][3][1:] == (1024, 1024) and c[8][2][1:] == (1024, 1024)


@pytest.mark.parametrize('i', range(len(gu.CASES)), ids=gu.IDS)
def test_case_meets_its_conditions(i):
    """At the case's seed: the margin condition, maps neither flat nor one-hot, the fp32 tensor-code gradient within 0.1
    of the bound, every applicable mutant at least 100 bounds away; and the by-hand backward without a mutant is
    autograd's."""
    d = gu.load(i)
    case = d['case']
    ok, rep = gu.conditions(d)
    for side in ('frames', 'clip'):
        for name, (need, found, dist) in rep[side + '_margins'].items():
            print(f'case {i} {side} {name}: margin required {need:.2e}, found {found:.2e}, fp32-vs-fp64 {dist:.2e}')
            assert need >= gu.MARGIN_FLOOR and need >= 4 * dist and found >= need, (side, name, need, found)
    for side, rows in (('frames', case[0]), ('clip', case[1])):
        if rows > 1:
            lo, hi = gu.rowmax_range(rows)
            assert lo <= rep[side + '_rowmax'] <= hi, (side, rep[side + '_rowmax'])
    print(f'case {i} fp32 tensor code vs fp64, in bounds: dx {rep["dx32"]:.3e} dfeat {rep["dfeat32"]:.3e}')
    assert rep['dx32'] <= 0.1 and rep['dfeat32'] <= 0.1
    seen = {k: v for k, v in rep.items() if 'mutant' in k}
    print(f'case {i} mutants, in bounds: ' + ' '.join(f'{k} {v:.0f}' for k, v in seen.items()))
    assert all(v >= 100 for v in seen.values()), seen
    for mu in gu.MUTANTS:
        assert (f'frames_mutant{mu}' in seen) == gu.applies(mu, case[0], case[2])
        assert (f'clip_mutant{mu}' in seen) == gu.applies(mu, case[1], case[3])
    assert ok
    x, wf, wc = d['x'].double(), d['wf'].double(), d['wc'].double()
    assert du.check(gu.frames_grad_by_hand(x, wf, d['dfeat_in'].double(), case), d['dx64']) <= 1e-6
    assert du.check(gu.clip_grad_by_hand(d['feat32'].double(), wc, d['dlogits'].double(), case), d['dfeat64']) <= 1e-6


def test_every_mutant_is_reached():
    for mu in gu.MUTANTS:
        assert any(gu.applies(mu, c[0], c[2]) for c in gu.CASES) and any(gu.applies(mu, c[1], c[3]) for c in gu.CASES), mu


@pytest.mark.parametrize('i', [1, 6, 8])
def test_transposed_images_follow_the_size_queries(i):
    import agcn_amd  # noqa: F401
    from agcn_amd import ops
    V, seg, sp, tp, num_class, _ = gu.CASES[i]
    d = gu.load(i)
    fs, cs = ops.sgn15_bwd_image_sections(sp, tp)
    wf_t, wc_t = ops.sgn15_transpose_images(d['wf'], d['wc'], V, seg, num_class, sp, tp)
    assert ops.sgn15_bwd_weights_floats(V, seg, num_class, sp, tp) == (wf_t.numel(), wc_t.numel())
    fwd = [{n: (o, s) for n, o, s in secs} for secs in ops.sgn15_image_sections(V, seg, num_class, sp, tp)]
    for img, img_t, secs, at in ((d['wf'], wf_t, fs, fwd[0]), (d['wc'], wc_t, cs, fwd[1])):
        end = 0
        for name, off, shape, src in secs:
            assert off == end and name == src + '_t' and shape == at[src][1][::-1]
            end = off + shape[0] * shape[1]
            o, s = at[src]
            assert torch.equal(img_t[off:end].view(shape), img[o:o + s[0] * s[1]].view(s).t())
        assert end == img_t.numel()
    assert [n for n, *_ in fs] == ['pe2_w_t', 've2_w_t', 's_qkv_w_t', 's_o_w_t', 's_f1_w_t', 's_f2_w_t']
    assert ops.sgn15_bwd_weights_floats(V, seg, num_class, (8, 48, 128), tp) is None
    assert set(ops.SGN15_BWD_STATS) == {'clip_bwd', 'frames_bwd'}
    assert set(ops.SGN15_STATS) == {'frames_hip', 'clip_hip'}


# ---- the whole model ----
def test_gradient_fixture_is_complete():
    f = vu._npz('sgn15_evalgrad.npz')
    assert sorted({k.split('.')[0] for k in f}) == sorted(gu.GRAD_CASES)
    assert os.path.getsize(os.path.join(vu.GOLDEN, 'sgn15_evalgrad.npz')) < 1 << 20
    for case in gu.GRAD_CASES:
        c = gu.load_grad_case(case)
        m = c['meta']
        assert m['sites'] <= gu.MAX_SITES and m['grad_fp32_in_bounds'] <= 0.25
        for name, (need, found, dist) in m['margins'].items():
            assert need >= max(gu.MARGIN_FLOOR, 4 * dist) * (1 - 1e-12) and found >= need, (case, name)
        assert c['grad_x64'].dtype == np.float64 and c['grad_x'].dtype == np.float32 and c['x'].shape == c['grad_x'].shape


@pytest.mark.parametrize('case', gu.GRAD_CASES)
def test_composition_autograd_matches_the_reference_gradient(case):
    import agcn_amd  # noqa: F401
    from agcn_amd import ops
    from agcn_amd.model.sgn_v15 import SGN
    c = gu.load_grad_case(case)
    m = SGN(**c['meta']['model_args'])
    m.load_state_dict(vu.torch_state(c['state']))
    m.eval()
    assert m.fused_input_gradient is False and 'fused_input_gradient' not in m.state_dict()
    x, cot = torch.from_numpy(c['x']), torch.from_numpy(c['cot'])
    for flag in (False, True):                       # a CPU tensor takes the composition whatever the flag says
        m.fused_input_gradient = flag
        before, bwd = ops.SGN_STATS['forward_tensor'], dict(ops.SGN15_BWD_STATS)
        logits, aux, dx = m.input_gradient(x, cot)
        assert ops.SGN_STATS['forward_tensor'] == before + 1 and ops.SGN15_BWD_STATS == bwd
        r = dict(dx=du.check(dx, c['grad_x64']), logits=du.check(logits, c['logits']))
        print(f'{case} composition (flag {flag}) vs the reference, in bounds: ' + ' '.join(f'{k} {v:.3e}' for k, v in r.items()))
        assert all(v <= 1.0 for v in r.values()), r
    m.train()
    with pytest.raises(ValueError):
        m.input_gradient(x, cot)


def test_cached_images_carry_no_graph_in_grad_mode():
    """The images are folded from parameters that require grad; built with grad mode on (an ``input_gradient`` call
    outside ``no_grad``) they must still be plain tensors, or the module stops being deep-copyable and every later
    ``aux`` carries a graph into the parameters."""
    import agcn_amd  # noqa: F401
    from agcn_amd.model.sgn_v15 import SGN
    c = gu.load_grad_case('j7_seg3_nobias')
    m = SGN(**c['meta']['model_args'])
    m.load_state_dict(vu.torch_state(c['state']))
    m.eval()
    assert torch.is_grad_enabled() and all(p.requires_grad for p in m.parameters())
    cached = m._images() + m._images_t()
    assert len(cached) == 6 and all(not t.requires_grad and t.grad_fn is None for t in cached)
    assert all(not t.requires_grad for t in m._infer_cache['images'][1:])
    aux = m._fused_aux(2, None, None)
    assert not aux['tem_emb'].requires_grad and not aux['spa_emb'].requires_grad
    twin = copy.deepcopy(m)
    assert torch.equal(twin._images()[0], cached[0])


# ---- the online case: tests/golden/sgn15_online_grad.npz holds the rows the recogniser samples (recorded on the GPU; the
# GPU test asserts it samples the same) and the seed of the parameters ----
def test_online_case_keeps_its_margin():
    import agcn_amd  # noqa: F401
    c = gu.online_case()
    rows = torch.from_numpy(c['rows'])
    t64 = gu.online_margins(gu.online_model(c['meta'], torch.float64), rows.double())
    t32 = gu.online_margins(gu.online_model(c['meta']), rows)
    sites = 0
    for name, v in t64.items():
        dist = float((t32[name].double() - v).abs().max())
        need, found = max(gu.MARGIN_FLOOR, 4 * dist), float(v.abs().min())
        print(f'online {name}: margin required {need:.2e}, found {found:.2e}, fp32-vs-fp64 {dist:.2e}')
        assert found >= need, name
        sites += 0 if name.endswith('pool_gap') else v.numel()
    assert sites <= gu.MAX_SITES
