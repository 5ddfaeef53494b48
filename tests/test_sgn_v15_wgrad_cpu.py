"""CPU side of the SGN v15 parameter-gradient tests: the plan header compiled for the host, the conditions that make the
seeded table of tests/sgn_v15_wgrad_util.py able to show an error on the GPU (the fp32 tensor code within 0.1 of the bound
per section, every mutant of a hand-written weight gradient at least 100 bounds away in the section it touches), the
whole-model fixture against ``SGN.parameter_gradients`` on its composition route, and the CPU route of
``ops.SGN15FineTuneFunction``."""
import os
import shutil
import subprocess

import pytest

from tests import sgn_v15_domain_util as du
from tests import sgn_v15_grad_util as gu
from tests import sgn_v15_util as vu
from tests import sgn_v15_wgrad_util as wg

ROOT = vu.ROOT


def test_sgn_v15_wgrad_plan_checker(tmp_path):
    cxx = next((c for c in (os.environ.get('CXX'), 'c++', 'g++', 'clang++') if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip('no host C++ compiler')
    exe = str(tmp_path / 'sgn_v15_wgrad_plan_check')
    r = subprocess.run([cxx, '-std=c++17', '-Wall', '-Werror', '-O1', '-I', os.path.join(ROOT, '2s-agcn_amd', 'csrc'),
                        os.path.join(ROOT, 'tests', 'sgn_v15_wgrad_plan_check.cpp'), '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-4000:]
    assert ' cases, 0 failures' in r.stdout and int(r.stdout.split(' cases')[0].split()[-1]) > 1000


def test_plan_check_table_is_the_python_table():
    """tests/sgn_v15_wgrad_plan_check.cpp repeats ``sgn_v15_grad_util.CASES``: the same ten geometries."""
    text = open(os.path.join(ROOT, 'tests', 'sgn_v15_wgrad_plan_check.cpp')).read().replace(' ', '')
    for V, seg, sp, tp, nc, N in gu.CASES:
        row = '{%d,%d,{%d,%d,%d},{%d,%d,%d},%d,%d}' % (V, seg, *sp, *tp, nc, N)
        assert row in text, row
    assert len(wg.SEEDS) == len(gu.CASES)
    for i, s in enumerate(wg.SEEDS):
        assert s == gu.SEEDS[i] or 100 * i + 1 <= s <= 100 * i + wg.SEARCH, (i, s)


@pytest.mark.parametrize('i', range(len(gu.CASES)), ids=gu.IDS)
def test_case_meets_its_conditions(i):
    """At the case's seed: the by-hand weight gradient without a mutant is autograd's; the fp32 tensor code is within 0.1
    of the bound in every section; every mutant that applies is at least 100 bounds away in the section it touches.  A
    case whose seed is not sgn_v15_grad_util's also meets that module's margin conditions (ReLUs, maxima, maps)."""
    d = wg.load(i)
    case = d['case']
    fs, cs = wg.sections(case)
    x, wf, wc, f32 = d['x'].double(), d['wf'].double(), d['wc'].double(), d['feat32'].double()
    hand = wg.check_image(wg.frames_wgrad_by_hand(x, wf, d['dfeat_in'].double(), case), d['dwf64'], fs,
                          f'case {i} frames image gradient by hand vs autograd (fp64)')
    hand.update(wg.check_image(wg.clip_wgrad_by_hand(f32, wc, d['dlogits'].double(), case), d['dwc64'], cs,
                               f'case {i} clip image gradient by hand vs autograd (fp64)'))
    assert all(v <= 1e-6 for v in hand.values()), hand
    ok, rep = wg.conditions(d)
    for k, v in rep.items():
        print(f'case {i} seed {d["seed"]} {k}: {v:.3e}')
    for k, v in rep.items():
        if '_fp32:' in k:
            assert v <= 0.1, (k, v)
        else:
            assert v >= 100, (k, wg.MUTANTS[int(k.split('mutant')[1].split(':')[0])], v)
    assert ok
    if d['seed'] != gu.SEEDS[i]:                     # a seed of this table: the margins are asserted here
        ok, rep = wg.margin_conditions(d)
        for k, v in rep.items():
            print(f'case {i} seed {d["seed"]} {k}: {v}')
        assert ok, rep


def test_every_mutant_applies_somewhere():
    for mu in wg.MUTANTS:
        sides = [(side, i) for i, (V, seg, sp, tp, _, N) in enumerate(gu.CASES)
                 for side, sets, rows, geo in (('frames', N * seg, V, sp), ('clip', N, seg, tp))
                 if wg.applies(mu, side, sets, rows, geo)]
        assert sides, wg.MUTANTS[mu]


# ---- the whole model: the composition route against the reference class's gradients ----
@pytest.mark.parametrize('case', gu.GRAD_CASES)
def test_parameter_gradients_composition_matches_the_reference(case):
    from agcn_amd import ops
    m, x, cot, c = wg.build_model(case)
    fix = wg.load_paramgrad(case)
    assert fix['meta']['index_seed'] == wg.INDEX_SEED and all(f < wg.BOUND / 2 for f in fix['floor'].values())
    tensor, wgs = ops.SGN_STATS['forward_tensor'], dict(ops.SGN15_WGRAD_STATS)
    logits, aux, dx, grads = m.parameter_gradients(x, cot)
    assert ops.SGN_STATS['forward_tensor'] == tensor + 1 and ops.SGN15_WGRAD_STATS == wgs
    assert all(p.grad is None for p in m.parameters()) and not logits.requires_grad and not dx.requires_grad
    assert set(aux) >= {'tem_emb', 'spa_emb', 'spatial_attn_list', 'temporal_attn_list'}
    r = wg.compare(grads, fix, f'{case} parameter_gradients (composition, CPU) vs the reference in fp64')
    r.update(logits=du.check(logits, c['logits']), dx=du.check(dx, c['grad_x64']))
    print(f'{case} in bounds: logits {r["logits"]:.3e} dx {r["dx"]:.3e}')
    assert all(v <= 1.0 for v in r.values()), r
    # only the parameters that ask get a gradient
    for n, p in m.named_parameters():
        p.requires_grad_(n.startswith('fc.'))
    _, _, _, head = m.parameter_gradients(x, cot)
    assert sorted(head) == ['fc.bias', 'fc.weight']
    r = wg.compare(head, dict(fix, keys=['fc.bias', 'fc.weight']), f'{case} head-only parameter_gradients')
    assert all(v <= 1.0 for v in r.values()), r
    m.train()
    with pytest.raises(ValueError):
        m.parameter_gradients(x, cot)


CLIP_SIDE = ('temporal_mha.', 'fc.', 'semantic_embedding.tem_embedding.')      # the parameters folded into the clip image
TRAINABLE = {'all': lambda n: True, 'clip image side': lambda n: n.startswith(CLIP_SIDE),
             'frames image side': lambda n: not n.startswith(CLIP_SIDE)}


@pytest.mark.parametrize('trainable', sorted(TRAINABLE))
@pytest.mark.parametrize('case', gu.GRAD_CASES)
def test_fold_gradients_of_partial_trainable_sets(case, trainable):
    """``ops.sgn_fold_gradients`` with the image gradients from autograd of ``ops.sgn15_forward_ref``: an image none of
    whose parameters is trainable carries no graph and is skipped."""
    import torch
    from agcn_amd import ops
    m, x, cot, c = wg.build_model(case)
    pick = TRAINABLE[trainable]
    for n, p in m.named_parameters():
        p.requires_grad_(pick(n))
    wf, wc, _, _ = m._finetune_images()
    assert wf.requires_grad == (trainable != 'clip image side') and wc.requires_grad == (trainable != 'frames image side')
    leaves = [wf.detach().requires_grad_(True), wc.detach().requires_grad_(True)]
    logits = ops.sgn15_forward_ref(x, *leaves, m.num_point, m.num_segment, m.num_class, *m._geometry())[0]
    image_grads = torch.autograd.grad((logits * cot).sum(), leaves)
    named = [(n, p) for n, p in m.named_parameters() if p.requires_grad]
    got = ops.sgn_fold_gradients((wf, wc), image_grads, named)
    fix = wg.load_paramgrad(case)
    r = wg.compare(got, dict(fix, keys=[k for k in fix['keys'] if pick(k)]), f'{case}, {trainable} trainable')
    assert all(v <= 1.0 for v in r.values()), r
    for p in m.parameters():
        p.requires_grad_(False)
    assert ops.sgn_fold_gradients(m._finetune_images()[:2], image_grads, []) == {}


def test_finetune_function_cpu_route_and_flag():
    """``ops.SGN15FineTuneFunction`` on CPU tensors runs ``sgn15_forward_ref`` on the freshly folded images: the
    specification of the fold and of the image gradients' way to the parameters.  The flag is a plain attribute."""
    from agcn_amd import ops
    case = gu.GRAD_CASES[0]
    m, x, cot, c = wg.build_model(case)
    fix = wg.load_paramgrad(case)
    assert m.fused_finetune is False and 'fused_finetune' not in m.state_dict()
    m.fused_finetune = True
    assert not m._fused_finetune(x), 'a CPU tensor is not fusable'
    wf, wc, wf_t, wc_t = m._finetune_images()
    assert wf.requires_grad and wc.requires_grad and not wf_t.requires_grad and not wc_t.requires_grad
    assert 'images' not in m._infer_cache, 'the fine-tuning images are never the cached ones'
    xg = x.clone().requires_grad_(True)
    logits = ops.SGN15FineTuneFunction.apply(xg, wf, wc, wf_t, wc_t, m.num_point, m.num_class, *m._geometry())
    (logits * cot).sum().backward()
    r = wg.compare({n: p.grad for n, p in m.named_parameters()}, fix, f'{case} SGN15FineTuneFunction (CPU route)')
    r.update(logits=du.check(logits, c['logits']), dx=du.check(xg.grad, c['grad_x64']))
    assert all(v <= 1.0 for v in r.values()), r
    # chunks: whole clips under the tape cap, at least one; outside the domain an error
    sp, tp = m._geometry()
    per = 4 * (4 * 15 * (4 * sp[0] * sp[1] + 2 * sp[2] + 1120) + 4 * (4 * tp[0] * tp[1] + 2 * tp[2] + 1536) + 512)
    assert ops.sgn15_tape_chunk(64, 4, 15, 60, sp, tp, 3 * per + 5) == 3 and ops.sgn15_tape_chunk(64, 4, 15, 60, sp, tp, 1) == 1
    assert ops.sgn15_tape_chunk(2, 4, 15, 60, sp, tp, 1 << 40) == 2
    with pytest.raises(ValueError):
        ops.sgn15_tape_chunk(1, 4, 15, 60, (8, 48, 128), tp, 1 << 20)
