"""SGN v15 batch statistics without a GPU: the host check of csrc/sgn_v15_stats_plan.h, the fold with and without
overrides, the incremental fold against its specification, on CPU tensors ``SGN.batch_statistics`` / ``recalibrate_bn``
(the composition route) against the reference-generated fixture (tests/golden/make_golden_sgn_v15_bnstats.py), the tensor
references of the passes that the GPU tests compare the kernels with, seven mutants of them, and the argument checks of
the C entries, which return before any HIP call."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import sgn_v15_bnstats_util as bu
from tests import sgn_v15_util as vu

ROOT = vu.ROOT


def _ops():
    import agcn_amd  # noqa: F401
    from agcn_amd import ops
    return ops


def test_sgn_v15_stats_plan_checker(tmp_path):
    cxx = next((c for c in (os.environ.get('CXX'), 'c++', 'g++', 'clang++') if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip('no host C++ compiler')
    exe = str(tmp_path / 'sgn_v15_stats_plan_check')
    r = subprocess.run([cxx, '-std=c++17', '-Wall', '-Werror', '-O1', '-I', os.path.join(ROOT, '2s-agcn_amd', 'csrc'),
                        os.path.join(ROOT, 'tests', 'sgn_v15_stats_plan_check.cpp'), '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-4000:]
    assert ' cases, 0 failures' in r.stdout and int(r.stdout.split(' cases')[0].split()[-1]) > 10000


def test_names_are_the_modules_in_dependency_order():
    ops = _ops()
    _, m = bu.model('j3_seg2')
    bns = [n for n, mod in m.named_modules() if isinstance(mod, torch.nn.modules.batchnorm._BatchNorm)]
    assert tuple(bns) == ops.SGN15_BN_NAMES == bu.BN_NAMES
    assert [m.get_submodule(n).num_features for n in bns] == [9, 9, 128, 128, 256, 256]


def test_folded_with_the_running_statistics_as_override_is_the_same_bits():
    _, m = bu.model('j7_seg12_nobias')
    with torch.no_grad():
        frames, clip = m._folded()
        frames2, clip2 = m._folded({})
        running = {n: (m.get_submodule(n).running_mean, m.get_submodule(n).running_var) for n in bu.BN_NAMES}
        frames3, clip3 = m._folded(running)
        wf, wc, _, _ = m._images()
    assert len(frames) == 21 and len(clip) == 11
    for a, b, d in zip(frames + clip, frames2 + clip2, frames3 + clip3):
        assert torch.equal(a, b) and torch.equal(a, d)
    assert torch.equal(wf, torch.cat([t.reshape(-1) for t in frames])) and torch.equal(wc, torch.cat([t.reshape(-1) for t in clip]))


@pytest.mark.parametrize('case', ['j7_seg12_nobias', 'j9_seg7_h2x256'])
def test_incremental_fold_equals_the_fold_with_overrides(case):
    """``_batch_folder`` patches the working images as the statistics arrive: after each of the six steps both whole
    images are ``_batch_images(known)`` bit for bit."""
    _, m = bu.model(case)
    rng = np.random.default_rng(5)
    with torch.no_grad():
        fold = m._batch_folder()
        known = {}
        for got, want in zip(fold(known), m._batch_images(known)):
            assert torch.equal(got, want)
        for name in bu.BN_NAMES:
            C = m.get_submodule(name).num_features
            known[name] = (torch.from_numpy(rng.standard_normal(C).astype(np.float32)),
                           torch.from_numpy(rng.uniform(0.0, 2.0, C).astype(np.float32)))
            for got, want in zip(fold(known), m._batch_images(known)):
                assert torch.equal(got, want), name
    assert 'images' not in m._infer_cache


def _flags(m):
    return [(n, mod.training, getattr(mod, 'track_running_stats', None)) for n, mod in m.named_modules()]


@pytest.mark.parametrize('case', bu.CASES)
def test_batch_statistics_on_the_cpu_matches_the_reference(case):
    ops = _ops()
    c, m = bu.model(case)
    rec = bu.load_record(case)
    x = torch.from_numpy(c['x'])
    before = {k: (v.clone(), v._version) for k, v in m.state_dict().items()}
    flags = _flags(m)
    n_tensor = ops.SGN_STATS['forward_tensor']
    logits, aux, stats = m.batch_statistics(x)
    assert ops.SGN_STATS['forward_tensor'] == n_tensor + 1
    assert _flags(m) == flags and not m.training
    for k, v in m.state_dict().items():
        assert torch.equal(v, before[k][0]) and v._version == before[k][1], k
    assert tuple(stats) == bu.BN_NAMES and not logits.requires_grad
    N, seg, V = x.shape[0], x.shape[1], m.num_point
    worst = 0.0
    for i, n in enumerate(bu.BN_NAMES):
        mean, var, count = stats[n]
        assert count == (N * seg * V if 2 <= i < 4 else N * seg), (n, count)
        worst = max(worst, bu.err(mean, rec['mean'][n]), bu.err(var, rec['var'][n]))
    e_l = bu.err(logits, rec['logits'])
    print(f'{case}: composition vs reference: statistics {worst:.2e}, logits {e_l:.2e}')
    assert worst < bu.BOUND and e_l < bu.BOUND
    # the same answer from train(), with every dropout of the module (p = 0.1 and 0.2) switched off for the call
    m.train()
    flags = _flags(m)
    logits2, _, _ = m.batch_statistics(x)
    assert _flags(m) == flags and m.training and torch.equal(logits2, logits)
    for k, v in m.state_dict().items():
        assert torch.equal(v, before[k][0]) and v._version == before[k][1], k


@pytest.mark.parametrize('train', [False, True])
def test_flags_are_restored_when_the_forward_raises(train):
    c, m = bu.model('j3_seg2', train=train)
    flags = _flags(m)
    before = {k: (v.clone(), v._version) for k, v in m.state_dict().items()}

    def boom(x):
        raise RuntimeError('boom')

    m.forward_tensor = boom
    with pytest.raises(RuntimeError, match='boom'):
        m.batch_statistics(torch.from_numpy(c['x']))
    del m.forward_tensor
    assert _flags(m) == flags
    assert all(not mod._forward_pre_hooks for mod in m.modules())
    for k, v in m.state_dict().items():
        assert torch.equal(v, before[k][0]) and v._version == before[k][1], k


@pytest.mark.parametrize('case', ['j3_seg2', 'j15_deployed', 'j9_seg7_h2x256'])
@pytest.mark.parametrize('momentum', [None, 0.1])
def test_recalibrate_bn_on_the_cpu_matches_the_reference(case, momentum):
    c, m = bu.model(case)
    rec = bu.load_record(case)
    x = torch.from_numpy(c['x'])
    with torch.no_grad():
        stale, _ = m(x)
    m.recalibrate_bn(x, momentum=momentum)
    tag = 'none' if momentum is None else '01'
    worst = 0.0
    for n in bu.BN_NAMES:
        bn = m.get_submodule(n)
        assert int(bn.num_batches_tracked) == 1
        worst = max(worst, bu.err(bn.running_mean, rec['rm_' + tag][n]), bu.err(bn.running_var, rec['rv_' + tag][n]))
    print(f'{case}, momentum {momentum}: running statistics vs reference {worst:.2e}')
    assert worst < bu.BOUND
    if momentum is None:
        with torch.no_grad():
            logits, _ = m(x)
        e = bu.err(logits, rec['eval_logits'])
        print(f'{case}: eval logits after recalibrate_bn vs reference {e:.2e}')
        assert e < bu.BOUND and not torch.equal(logits, stale)
        # without reset a second call averages cumulatively: two equal batches leave the statistics where they are
        keep = {n: m.get_submodule(n).running_var.clone() for n in bu.BN_NAMES}
        m.recalibrate_bn(x, momentum=None, reset=False)
        for n in bu.BN_NAMES:
            assert int(m.get_submodule(n).num_batches_tracked) == 2
            assert bu.err(m.get_submodule(n).running_var, keep[n].numpy()) < 1e-6


def test_bad_shapes_and_one_sample_per_channel_are_refused():
    import agcn_amd  # noqa: F401
    from agcn_amd.model.sgn_v15 import SGN
    m = SGN(**vu.model_args(3, 1, 1, (8, 16, 128), (8, 16, 128), num_class=4)).eval()
    for bad in (torch.zeros(1, 1, 9), torch.zeros(2, 9), torch.zeros(2, 1, 3, 3)):
        with pytest.raises(ValueError):
            m.batch_statistics(bad)
        with pytest.raises(ValueError):
            m.recalibrate_bn(bad)
    logits, _, stats = m.batch_statistics(torch.randn(2, 1, 9))
    assert tuple(logits.shape) == (2, 4) and stats[bu.BN_NAMES[5]][2] == 2 and stats[bu.BN_NAMES[2]][2] == 6


# ---- the references the GPU tests compare the kernels with -----------------------------------------------------------------
@pytest.mark.parametrize('i', range(len(bu.PASS_CASES)), ids=bu.PASS_IDS)
def test_pass_references(i):
    """The fp64 reference of the passes continues to ``ops.sgn15_forward_ref``'s feat, and the fp32 tensor reference lies
    within 0.1 of the bound of it."""
    ops = _ops()
    p = bu.pass_case(i)
    V, seg, sp, tp = p['V'], p['seg'], p['spatial'], p['temporal']
    x, wf, wc = p['x'].double(), p['wf'].double(), p['wc'].double()
    f, _ = bu._views(x, wf, wc, V, seg, bu.PASS_NUM_CLASS, sp, tp)
    x1 = p['tile64']['frames', 2]
    y = torch.cat([torch.relu(x1 @ f['s_f1_w'] + f['s_f1_b']), x1], dim=2) @ f['s_f2_w'] + f['s_f2_b']
    feat = ops.sgn15_forward_ref(x, wf, wc, V, seg, bu.PASS_NUM_CLASS, sp, tp)[1]
    assert torch.equal(y.reshape(p['N'], seg, V, 256).amax(2), feat) and torch.equal(feat.float(), p['feat32'])
    for k in bu.PASSES:
        (m64, v64), (m32, v32) = bu.two_pass(p['tile64'][k]), bu.two_pass(p['tile32'][k])
        r = max(bu.ratio(m32, m64), bu.ratio(v32, v64))
        assert r < 0.1, (k, r)
        s64, q64 = bu.group_partials(p['tile64'][k])
        s32, q32 = bu.group_partials(p['tile32'][k])
        assert max(bu.ratio(s32, s64), bu.ratio(q32, q64)) < 0.1, k


def _known(case):
    rec = bu.load_record(case)
    return {n: (torch.from_numpy(rec['mean'][n]), torch.from_numpy(rec['var'][n])) for n in bu.BN_NAMES}


def _tiles(case, known_names=bu.BN_NAMES, **mutant):
    """The four tiles of a fixture case in fp64 on the images folded on the recorded batch statistics of ``known_names``
    (and the running ones elsewhere), and x, feat."""
    c, m = bu.model(case)
    known = {n: s for n, s in _known(case).items() if n in known_names}
    with torch.no_grad():
        wf, wc = (t.double() for t in m._batch_images(known))
        x = torch.from_numpy(c['x']).double()
        g = (m.num_point, m.num_segment, m.num_class, *m._geometry())
        feat = _ops().sgn15_forward_ref(x, wf, wc, *g)[1]
        out = {('frames', l): bu.frames_tile(x, wf, wc, *g, l) for l in (1, 2)}
        out.update({('clip', l): bu.clip_tile(feat, wf, wc, *g, l, **mutant) for l in (1, 2)})
    return out, x, feat, m


def _miss(got, ref):
    return bu.ratio(got, ref)


def test_seven_mutants_are_far_from_the_statistic_they_touch():
    """Each mutant misses the statistic it touches by at least 100 bounds, on the fixtures' seeds as they are (none needed
    a search)."""
    rec = {case: bu.load_record(case) for case in ('j3_seg2', 'j15_deployed')}
    t3, x3, feat3, m3 = _tiles('j3_seg2')
    t15, x15, feat15, m15 = _tiles('j15_deployed')
    # the tiles ARE what the reference's BatchNorms saw
    for case, t in (('j3_seg2', t3), ('j15_deployed', t15)):
        for (kind, layer), n in zip(bu.PASSES, bu.BN_NAMES[2:]):
            mean, var = bu.two_pass(t[kind, layer])
            assert bu.ratio(mean, rec[case]['mean'][n]) < 1.0 and bu.ratio(var, rec[case]['var'][n]) < 1.0, (case, n)
    miss = {}
    # 1. n_f measured on x instead of x1
    miss['n_f on x'] = min(_miss(bu.two_pass(t[k, 1])[1], bu.two_pass(t[k, 2])[1]) for t in (t3, t15) for k in ('frames', 'clip'))
    # 2. padded rows counted: the clip tile's zero rows up to 32
    z = t15['clip', 1]
    padded = torch.cat([z, z.new_zeros(z.shape[0], 32 - z.shape[1], z.shape[2])], dim=1)
    miss['padded rows'] = min(_miss(a, b) for a, b in zip(bu.two_pass(padded), bu.two_pass(z)))
    # 3. temporal n_a on feat without tem
    g15 = (m15.num_point, m15.num_segment, m15.num_class, *m15._geometry())
    with torch.no_grad():
        wf, wc = (t.double() for t in m15._batch_images(_known('j15_deployed')))
        no_tem = bu.clip_tile(feat15, wf, wc, *g15, 1, tem=False)
    miss['feat without tem'] = _miss(bu.two_pass(no_tem)[0], bu.two_pass(z)[0])
    # 4. unbiased instead of biased variance: the ten frames of j3_seg2
    z = t3['clip', 2]
    n = z.shape[0] * z.shape[1]
    var = bu.two_pass(z)[1]
    miss['unbiased variance'] = _miss(var * (n / (n - 1)), var)
    # 5. n_f under the RUNNING n_a
    running, _, _, _ = _tiles('j15_deployed', known_names=bu.BN_NAMES[:2])
    miss['n_f under the running n_a'] = _miss(bu.two_pass(running['frames', 2])[1], bu.two_pass(t15['frames', 2])[1])
    # 6. input features in c*V + v order where [v*3 + c] is due
    V = m15.num_point
    mean = torch.from_numpy(rec['j15_deployed']['mean'][bu.BN_NAMES[0]])            # the module's c*V + v
    kernel_order = mean.view(3, V).t().reshape(-1)
    miss['input feature order'] = _miss(mean, kernel_order)
    assert bu.ratio(x15.reshape(-1, 3 * V).mean(0), kernel_order) < 1.0
    # 7. a dropped group of the output projection in x1 (the temporal block of j15_deployed has two)
    dropped, _, _, _ = _tiles('j15_deployed', drop_group=1)
    miss['dropped group'] = _miss(bu.two_pass(dropped['clip', 2])[1], bu.two_pass(t15['clip', 2])[1])
    print({k: round(v) for k, v in miss.items()})
    assert len(miss) == 7 and min(miss.values()) >= 100.0, miss


def test_c_entries_refuse_bad_arguments_before_any_launch():
    """Argument errors come back before the first HIP call: no GPU needed."""
    from agcn_amd import lib
    L = lib.load()
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    sp, tp = (8, 16, 128), (8, 32, 256)
    wf, wc = L.agcn_sgn15_frames_weights(15, *sp), L.agcn_sgn15_clip_weights(20, 60, *tp)
    big = 1 << 30
    for layer in (0, 3):
        assert L.agcn_sgn15_frames_stats(p, p, wf, p, big, layer, 1, 20, 15, *sp, None) == -1
        assert L.agcn_sgn15_clip_stats(p, p, wc, p, big, layer, 1, 20, 60, *tp, None) == -1
    assert L.agcn_sgn15_frames_stats(None, p, wf, p, big, 1, 1, 20, 15, *sp, None) == -1
    assert L.agcn_sgn15_frames_stats(p, None, wf, p, big, 1, 1, 20, 15, *sp, None) == -1
    assert L.agcn_sgn15_clip_stats(p, p, wc, None, big, 1, 1, 20, 60, *tp, None) == -1
    assert L.agcn_sgn15_frames_stats(p, p, wf, p, big, 1, 1, 20, 33, *sp, None) == -1
    assert L.agcn_sgn15_frames_stats(p, p, wf + 1, p, big, 1, 1, 20, 15, *sp, None) == -1
    assert L.agcn_sgn15_clip_stats(p, p, wc - 1, p, big, 2, 1, 20, 60, *tp, None) == -1
    assert L.agcn_sgn15_frames_stats(p, p, wf, p, 16, 1, 1, 20, 15, *sp, None) == -2          # partial buffer too small
    assert L.agcn_sgn15_clip_stats(p, p, wc, p, 511, 1, 1, 20, 60, *tp, None) == -2
    assert L.agcn_sgn15_frames_stats(p, p, wf, p, big, 1, 1 << 30, 20, 15, *sp, None) == -3   # outside the forward's domain
    assert L.agcn_sgn15_frames_stats(p, p, wf, p, big, 1, 1, 20, 15, 8, 24, 128, None) == -3
    assert L.agcn_sgn15_clip_stats(p, p, wc, p, big, 1, 1, 33, 60, *tp, None) == -3
    assert L.agcn_sgn15_stats_finalize(p, big, 1, 3, 1, 20, 15, None, None, p, p, p, big, None) == -1
    assert L.agcn_sgn15_stats_finalize(p, big, 0, 1, 1, 20, 15, None, None, p, p, p, big, None) == -1
    assert L.agcn_sgn15_stats_finalize(p, big, 3, 1, 1, 20, 15, None, None, p, p, p, big, None) == -1
    assert L.agcn_sgn15_stats_finalize(p, big, 1, 1, 1, 20, 15, None, None, None, None, p, big, None) == -1
    assert L.agcn_sgn15_stats_finalize(p, big, 1, 1, 1, 20, 15, None, None, p, p, None, big, None) == -1
    assert L.agcn_sgn15_stats_finalize(p, 16, 1, 1, 1, 20, 15, None, None, p, p, p, big, None) == -2
    assert L.agcn_sgn15_stats_finalize(p, big, 1, 1, 2, 20, 15, None, None, p, p, p, 2 * 3 * 128 * 8 - 1, None) == -2
    assert L.agcn_sgn15_stats_finalize(p, big, 2, 1, 2, 33, 15, None, None, p, p, p, big, None) == -3
    assert L.agcn_sgn15_stats_finalize_workspace(1, 1, 2, 20, 15) == 2 * 3 * 128 * 8
    assert L.agcn_sgn15_stats_finalize_workspace(2, 2, 3, 20, 0) == 3 * 3 * 256 * 8
    assert L.agcn_sgn15_stats_part_floats(1, 2, 2, 20, 15) == 2 * 20 * 2 * 128
    assert L.agcn_sgn15_stats_part_floats(2, 1, 2, 20, 0) == 2 * 2 * 256
    assert L.agcn_sgn15_stats_part_floats(1, 3, 2, 20, 15) == 0 and L.agcn_sgn15_stats_part_floats(1, 1, 2, 20, 33) == 0
    assert L.agcn_sgn15_stats_part_floats(2, 1, 2, 33, 0) == 0 and L.agcn_sgn15_stats_part_floats(0, 0, 2, 20, 15) == 0
    assert L.agcn_sgn15_stats_channels(1, 1) == 128 and L.agcn_sgn15_stats_channels(2, 2) == 256
    assert L.agcn_sgn15_stats_channels(1, 0) == 0 and L.agcn_sgn15_stats_channels(3, 1) == 0
