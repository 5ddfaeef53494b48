"""SGN parameter gradients in eval mode, the parts that need no GPU: the plan header of the kernels, the fixtures, the
composition and the image-level tensor reference against them, the image-gradient -> parameter chain through the fold,
and the routing on CPU tensors.  Bound: tests/sgn_wgrad_util.py (1e-4 relative to max(1, max |reference tensor|))."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import sgn_grad_util as gu
from tests import sgn_util as su
from tests import sgn_wgrad_util as wu

ROOT = su.ROOT
CASES = gu.stored_cases()


def _err(got, ref):
    ref = np.asarray(ref, dtype=np.float64)
    return float(np.abs(np.asarray(got, dtype=np.float64) - ref).max() / max(1.0, float(np.abs(ref).max())))


def test_sgn_wgrad_plan_checker(tmp_path):
    cxx = next((c for c in (os.environ.get('CXX'), 'c++', 'g++', 'clang++') if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip('no host C++ compiler')
    exe = str(tmp_path / 'sgn_wgrad_plan_check')
    r = subprocess.run([cxx, '-std=c++17', '-Wall', '-Werror', '-O1', '-I', os.path.join(ROOT, '2s-agcn_amd', 'csrc'),
                        os.path.join(ROOT, 'tests', 'sgn_wgrad_plan_check.cpp'), '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-4000:]
    assert ' cases, 0 failures' in r.stdout and int(r.stdout.split(' cases')[0].split()[-1]) > 1000000


def test_fixture_files():
    assert set(gu.GRAD_CASES) <= set(CASES)
    for case in CASES:
        path = os.path.join(su.GOLDEN, wu.fixture_name(case))
        assert os.path.getsize(path) < (1 << 20), path
        fix = wu.load_paramgrad(case)
        d = gu.load_grad_case(case)
        assert fix['meta']['seed'] == d['meta']['seed'] and sorted(fix['keys']) == fix['keys']
        assert all(0.0 <= f < wu.FLOOR_LIMIT for f in fix['floor'].values()), (case, max(fix['floor'].values()))
        for k in fix['keys']:
            assert (k in fix['full']) != (k in fix['samp']) and k in fix['max']
            if k in fix['samp']:
                assert fix['samp'][k].shape == (wu.SAMPLES,) and k in fix['rows'] and k in fix['cols']
        print(f"{case}: {len(fix['keys'])} tensors, worst reference floor {max(fix['floor'].values()):.2e}")


@pytest.mark.parametrize('case', CASES)
def test_composition_matches_the_reference(case):
    model, x, c, d = wu.build_model(case)
    logits, g, dx, grads = model.parameter_gradients(x, c)
    assert _err(logits, d['logits']) < wu.BOUND and _err(g, d['g']) < wu.BOUND and _err(dx, d['grad_x']) < wu.BOUND
    err, name, floor = wu.compare(grads, wu.load_paramgrad(case), case)
    print(f'{case}: composition vs reference, worst {err:.2e} ({name}, reference floor {floor:.1e})')
    assert all(p.grad is None for p in model.parameters())


@pytest.mark.parametrize('case', CASES)
def test_image_reference_matches_the_composition(case):
    from agcn_amd import ops
    model, x, c, d = wu.build_model(case)
    with torch.no_grad():
        wf, wc, _, _ = model._finetune_images()
        logits, g = ops.sgn_image_forward_ref(x, wf, wc, model.num_point, model.seg, model.num_class)
        ref_logits, ref_g = model.forward_tensor(x)
    e = (_err(logits, ref_logits), _err(g, ref_g), _err(logits, d['logits']))
    print(f'{case}: image reference vs composition: logits {e[0]:.2e}, g {e[1]:.2e}; vs the fixture {e[2]:.2e}')
    assert max(e) < wu.BOUND
    fs, cs = ops.sgn_image_sections(model.num_point, model.seg, model.num_class)
    assert fs[-1][1] + int(np.prod(fs[-1][2])) == wf.numel() and cs[-1][1] + int(np.prod(cs[-1][2])) == wc.numel()


@pytest.mark.parametrize('case', CASES)
def test_fold_chain_from_image_gradients_to_parameters(case):
    """d_wf, d_wc (here from autograd of the image reference) pushed through _folded() give the reference's gradient of
    every parameter: what the HIP path relies on for BatchNorm weight / bias, spa_embed, tem_embed and the unfolding."""
    from agcn_amd import ops
    model, x, c, d = wu.build_model(case)
    wf, wc, wf_t, wc_t = model._finetune_images()
    assert wf.requires_grad and wc.requires_grad and not wf_t.requires_grad and not wc_t.requires_grad
    wf_l, wc_l = wf.detach().requires_grad_(True), wc.detach().requires_grad_(True)
    logits, _ = ops.sgn_image_forward_ref(x, wf_l, wc_l, model.num_point, model.seg, model.num_class)
    d_wf, d_wc = torch.autograd.grad((logits * c).sum(), [wf_l, wc_l])
    named = list(model.named_parameters())
    grads = torch.autograd.grad([wf, wc], [p for _, p in named], [d_wf, d_wc])
    fix = wu.load_paramgrad(case)
    got = {n: gr for (n, _), gr in zip(named, grads)}
    err, name, floor = wu.compare(got, fix, case)
    groups = {}
    for k in fix['keys']:
        tag = next((t for t in ('.bn.weight', '.bn.bias', '.bn1.', '.bn2.', 'spa_embed', 'tem_embed') if t in k), None)
        if tag and k in fix['full']:
            groups[tag] = max(groups.get(tag, 0.0), _err(got[k], fix['full'][k]) if fix['max'][k] >= 1 else
                              float(np.abs(got[k].numpy() - fix['full'][k]).max()))
    print(f'{case}: fold chain, worst {err:.2e} ({name}, floor {floor:.1e}); ' +
          ', '.join(f'{t} {e:.1e}' for t, e in sorted(groups.items())))
    assert {'.bn.weight', '.bn.bias', 'spa_embed', 'tem_embed'} <= set(groups)


CLIP_SIDE = ('cnn.', 'fc.', 'tem_embed.')                  # the parameters folded into the clip image
TRAINABLE = {'all': lambda n: True, 'clip image side': lambda n: n.startswith(CLIP_SIDE),
             'frames image side': lambda n: not n.startswith(CLIP_SIDE)}


@pytest.mark.parametrize('trainable', sorted(TRAINABLE))
@pytest.mark.parametrize('case', CASES)
def test_fold_gradients_of_partial_trainable_sets(case, trainable):
    """``ops.sgn_fold_gradients``, what ``SGN.parameter_gradients`` does after the kernels: an image none of whose
    parameters is trainable carries no graph and must be skipped, not handed to autograd."""
    from agcn_amd import ops
    model, x, c, d = wu.build_model(case)
    pick = TRAINABLE[trainable]
    for n, p in model.named_parameters():
        p.requires_grad_(pick(n))
    wf, wc, _, _ = model._finetune_images()
    assert wf.requires_grad == (trainable != 'clip image side') and wc.requires_grad == (trainable != 'frames image side')
    leaves = [wf.detach().requires_grad_(True), wc.detach().requires_grad_(True)]
    logits, _ = ops.sgn_image_forward_ref(x, *leaves, model.num_point, model.seg, model.num_class)
    image_grads = torch.autograd.grad((logits * c).sum(), leaves)
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    got = ops.sgn_fold_gradients((wf, wc), image_grads, named)
    fix = wu.load_paramgrad(case)
    err, name, floor = wu.compare(got, dict(fix, keys=[k for k in fix['keys'] if pick(k)]), f'{case}, {trainable}')
    print(f'{case}, {trainable} trainable: worst {err:.2e} ({name}, reference floor {floor:.1e})')
    for p in model.parameters():
        p.requires_grad_(False)
    assert ops.sgn_fold_gradients(model._finetune_images()[:2], image_grads, []) == {}


def test_chunked_backward_order():
    """The chunk loop both models share: dx concatenated in clip order, the chunks' image gradients added in ascending
    chunk order -- with a triple whose fp32 sum depends on the order, the left-to-right sum bit for bit."""
    from agcn_amd import ops
    triple = [torch.tensor([1e8, 1.0]), torch.tensor([-1e8, 0.25]), torch.tensor([1.0, 1e-8])]
    left = (triple[0] + triple[1]) + triple[2]
    assert not torch.equal(left, triple[0] + (triple[1] + triple[2])), 'the triple does not tell the orders apart'
    x = torch.arange(5.0).reshape(5, 1, 1)
    feat, dlogits = x + 100, x.reshape(5, 1) + 200
    seen = []

    def step(xs, fe, dl):
        i = len(seen)
        assert torch.equal(fe, xs + 100) and torch.equal(dl, xs.reshape(-1, 1) + 200), 'the three slices differ'
        seen.append(xs.reshape(-1).tolist())
        return xs * 2, triple[i], triple[i] * 3

    dx, d_wf, d_wc = ops._sgn_chunked_backward(step, 2, x, feat, dlogits)
    assert seen == [[0.0, 1.0], [2.0, 3.0], [4.0]]
    assert torch.equal(dx, x * 2) and torch.equal(d_wf, left)
    assert torch.equal(d_wc, (triple[0] * 3 + triple[1] * 3) + triple[2] * 3)
    # one chunk: its results as they are
    one = ops._sgn_chunked_backward(lambda xs, fe, dl: (xs, triple[0], triple[1]), 5, x, feat, dlogits)
    assert torch.equal(one[0], x) and one[1] is triple[0] and one[2] is triple[1]


def test_function_cpu_route_is_the_image_reference():
    from agcn_amd import ops
    model, x, c, d = wu.build_model('v15_seg6')
    xg = x.clone().requires_grad_(True)
    logits, g = ops.SGNFineTuneFunction.apply(xg, *model._finetune_images(), model.num_point, model.num_class)
    assert not g.requires_grad
    (logits * c).sum().backward()
    assert _err(xg.grad, d['grad_x']) < wu.BOUND
    err, name, floor = wu.compare({n: p.grad for n, p in model.named_parameters()}, wu.load_paramgrad('v15_seg6'))
    print(f'SGNFineTuneFunction on the CPU: worst {err:.2e} ({name})')


def test_routing_on_the_cpu():
    from agcn_amd import ops
    stats_keys, grad_keys = set(ops.SGN_STATS), set(ops.SGN_GRAD_STATS)
    assert stats_keys == {'frames_hip', 'clip_hip', 'sample_hip', 'forward_tensor'}
    assert grad_keys == {'clip_bwd', 'frames_bwd', 'sample_bwd'}
    assert set(ops.SGN_WGRAD_STATS) == {'clip_bwd_tape', 'frames_bwd_tape', 'frames_wgrad', 'clip_wgrad'}
    model, x, c, d = wu.build_model('v15_seg6')
    assert model.fused_finetune is False and 'fused_finetune' not in model.state_dict()
    model.fused_finetune = True
    before, wbefore = dict(ops.SGN_STATS), dict(ops.SGN_WGRAD_STATS)
    logits, _ = model(x)                                   # a CPU tensor: the composition, whatever the flag
    (logits * c).sum().backward()
    assert ops.SGN_STATS['forward_tensor'] == before['forward_tensor'] + 1 and ops.SGN_WGRAD_STATS == wbefore
    wu.compare({n: p.grad for n, p in model.named_parameters()}, wu.load_paramgrad('v15_seg6'))
    model.train()
    with pytest.raises(ValueError):
        model.parameter_gradients(x, c)
    assert set(ops.SGN_STATS) == stats_keys and set(ops.SGN_GRAD_STATS) == grad_keys
