"""CPU side of the width-domain tests of unit_gcn's aggregate+project kernels (tests/gcn_width_util.py): what makes the GPU
comparison of tests/test_gpu_gcn_width.py able to fail, asserted on the fp64 reference alone, and the channel arithmetic
of the chained adjacency gradient swept on the host (tests/dadj_plan_check.cpp over csrc/dadj_plan.h)."""
import os
import shutil
import subprocess

import pytest
import torch

from tests import gcn_width_util as wu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [wu.case_id(c) for c in wu.CASES]
_REF = {}


def _case(i):
    if i not in _REF:
        p = wu.make(wu.CASES[i], wu.SEEDS[i])
        _REF[i] = (p, wu.reference(p))
    return _REF[i]


def test_table_is_what_the_issue_sets():
    assert len(wu.CASES) == len(wu.SEEDS) <= 24 and len(set(wu.CASES)) == len(wu.CASES)
    assert {c[2] for c in wu.CASES} <= {1, 3, 5, 6, 7, 9, 17} and {c[3] for c in wu.CASES} <= {15, 18, 20, 25, 32}
    assert any(c[2] == 1 for c in wu.CASES)
    assert any(c[2] > 256 // c[3] for c in wu.CASES)               # several frame tiles of the exact kernel
    widths = {c[:2] for c in wu.CASES}
    assert widths >= {(1, 1), (2, 48), (3, 100), (21, 24), (22, 24), (24, 24), (31, 33), (33, 31), (32, 40), (48, 72),
                      (63, 65), (64, 60), (64, 100), (128, 129), (64, 4), (65, 64), (80, 96), (96, 160), (192, 200),
                      (256, 24), (320, 64)}
    assert wu.fused_width(24) == 36 and wu.fused_width(40) == 60
    sub = [wu.CASES[i][0] for i in wu.F32_SUBSET]
    assert len(sub) == 6 and min(sub) < 32 and any(33 <= c <= 64 for c in sub) and any(65 <= c <= 128 for c in sub)
    assert max(sub) > 128
    assert {c[0] for c in wu.ADJ_CASES} == {1, 6, 25} and any(c[2] == 15 for c in wu.ADJ_CASES)
    assert not {c[0] for c in wu.ADJ_CASES} & {16, 32, 64}


def test_every_kernel_family_has_a_case():
    """the model of the routing puts a case of the table on every family its comments name, on both sides of every
    threshold, on 1, 2 and 3 plain stages, and on the refusals"""
    reached = set()
    for c in wu.CASES:
        reached |= {r for r in wu.routes_of(c).values() if r}
    assert reached >= set(wu.FAMILIES), sorted(set(wu.FAMILIES) - reached)
    dadj = {c[:2]: wu.route('dadj', c[0], c[1]) for c in wu.CASES}
    assert sum(r is None for r in dadj.values()) == 3 and dadj[(65, 64)] is None
    assert {wu.dadj_gpc(c[0]) for c in wu.CASES if c[0] % 64 == 0} >= {1, 2, 3}
    assert wu.dadj_gpc(192) == 3 and wu.dadj_gpc(256) == 2
    chain = [c for c in wu.CASES if c[0] % 64 == 0]
    assert any(c[1] % 8 and c[1] > 8 for c in chain) and any(c[1] < 8 for c in chain)
    infer = [wu.routes_of(c)['infer'] for c in wu.CASES]
    assert any(r is None for r in infer) and any(r for r in infer)
    assert all(wu.routes_of(c, f32=True)['fused'] is None and wu.routes_of(c, f32=True)['infer'] is None for c in wu.CASES)
    assert all('conv_' in r for c in wu.CASES for r in wu.routes_of(c, f32=True).values() if r)


@pytest.mark.parametrize('i', range(len(wu.CASES)), ids=IDS)
def test_reference_meets_the_conditions(i):
    """output scale (every channel at a quarter of its tensor at least), masks of both signs, addends of the gradient's
    order, a visible fused term -- at the recorded seed, which is the first of its range that meets them"""
    p, ref = _case(i)
    assert wu.conditions(wu.CASES[i], p, ref) == []
    assert wu.search(wu.CASES[i], i) == wu.SEEDS[i]
    assert ('dx5' in ref) == (wu.fused_width(wu.CASES[i][1]) > 0)


def test_reference_is_the_autograd_of_the_forward():
    """the hand-written einsums of dx, dw and dadj against autograd through _gcn_ref's formula"""
    p, ref = _case(6)
    x, adj, w = (p[k].clone().requires_grad_(True) for k in ('x', 'adj', 'wcat'))
    C = x.shape[1]
    y = 0
    for s in range(3):
        y = y + torch.einsum('oc,nctv->notv', w[:, s * C:(s + 1) * C], torch.einsum('nctu,nuv->nctv', x, adj[:, s]))
    y = y + p['bias'].view(1, -1, 1, 1)
    y.backward(p['dy'])
    assert wu.tensor_err(ref['y'], y) < 1e-12
    for k, t in (('dx', x), ('dw', w), ('dadj', adj)):
        assert wu.tensor_err(ref[k], t.grad) < 1e-12, k


def _mutant_err(ref, mut_out):
    worst = 0.0
    for k, keep in wu.CHANNEL_DIMS.items():
        if k in ref and k in mut_out:
            worst = max(worst, wu.channel_err(mut_out[k], ref[k], keep))
    return worst


def test_every_mutant_is_caught_wherever_it_applies():
    """each mutant models a width bug (gcn_width_util.MUTANTS); the per-channel metric must show it two decades above the
    bar at every case at which it applies: 100 % of the pairs, and every mutant applies somewhere"""
    pairs, caught, missed = 0, 0, []
    for m in wu.MUTANTS:
        assert any(wu.applies(m, c) for c in wu.CASES), m
    for i, c in enumerate(wu.CASES):
        p, ref = _case(i)
        for m in wu.MUTANTS:
            if not wu.applies(m, c):
                continue
            pairs += 1
            err = _mutant_err(ref, wu.reference(p, m))
            if err > wu.CAUGHT:
                caught += 1
            else:
                missed.append((c, m, err))
    print('%d (case, mutant) pairs, %d caught' % (pairs, caught))
    assert pairs > 100 and caught >= wu.CAUGHT_SHARE * pairs, missed


def test_the_suspected_staging_defect_is_a_mutant_of_the_table():
    """k_shift8 at dy's width: it applies to the chained adjacency gradient's cases with Cout % 8 != 0 and shows in dadj"""
    hit = [i for i, c in enumerate(wu.CASES) if c[0] % 64 == 0 and c[1] % 8 and c[1] > 8]
    assert len(hit) >= 3
    for i in hit:
        p, ref = _case(i)
        assert wu.channel_err(wu.reference(p, 'k_shift8')['dadj'], ref['dadj'], wu.CHANNEL_DIMS['dadj']) > wu.CAUGHT


def test_the_per_tensor_metric_cannot_see_one_channel():
    """why the bar is applied per channel: an error confined to the weakest channel is scaled by the tensor's maximum"""
    p, ref = _case(9)
    y = ref['y'].clone()
    cm = wu.channel_max(y, (1,))
    y[:, int(cm.argmin())] += 1.5e-4 * float(cm.min().clamp_min(1.0))
    assert wu.channel_err(y, ref['y'], (1,)) > wu.BAR
    assert wu.tensor_err(y, ref['y']) <= wu.channel_err(y, ref['y'], (1,))
    assert wu.channel_err(y, ref['y'], (1,)) <= wu.tensor_err(y, ref['y']) / wu.MIN_CHANNEL_SHARE + 1e-12


@pytest.mark.parametrize('i', range(len(wu.ADJ_CASES)))
def test_adjacency_reference_is_not_degenerate(i):
    """the softmax is neither uniform nor one-hot, so both its forward and its Jacobian are exercised"""
    ref = wu.adj_reference(wu.make_adj(wu.ADJ_CASES[i], wu.ADJ_SEEDS[i]))
    V = wu.ADJ_CASES[i][2]
    colmax = ref['P'].amax(-2)
    assert float(colmax.mean()) > 2.0 / V and float(colmax.median()) < 0.999
    assert float(ref['dtp'].abs().max()) > 0 and float(ref['db'].abs().max()) > 0


def test_dadj_plan_checker(tmp_path):
    cxx = next((c for c in (os.environ.get('CXX'), 'c++', 'g++', 'clang++') if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip('no host C++ compiler')
    exe = str(tmp_path / 'dadj_plan_check')
    r = subprocess.run([cxx, '-std=c++17', '-Wall', '-Werror', '-O2', '-I', os.path.join(ROOT, '2s-agcn_amd', 'csrc'),
                        os.path.join(ROOT, 'tests', 'dadj_plan_check.cpp'), '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-4000:]
    assert ' cases, 0 failures' in r.stdout and int(r.stdout.split(' cases')[0].split()[-1]) > 300000


def test_adjacency_bwd_names_the_refused_width():
    """ops.adjacency_bwd at a width the adjacency gradient refuses: a ValueError that names the width and the supported
    set, raised before anything is allocated or launched (the size query needs no device)"""
    from agcn_amd import ops
    C, Cout, T, V = 65, 64, 5, 25
    x, dy, w = torch.zeros(2, C, T, V), torch.zeros(2, Cout, T, V), torch.zeros(Cout, 3 * C)
    with pytest.raises(ValueError, match=r'does not support 65 input channels.*below 64 and multiples of 64'):
        ops.adjacency_bwd(dy, w, x, torch.zeros(2, 36, T, V), torch.zeros(2, 3, V, V))
    assert ops._L().agcn_dadj_num_slots(C, V, T) == 0 and ops._L().agcn_dadj_num_slots(64, V, T) > 0
