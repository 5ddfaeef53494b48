"""SGN batch statistics without a GPU: the host check of csrc/sgn_stats_plan.h, the numpy emulation of the finalize merge
against fp64 numpy on badly centred data, and on CPU tensors ``SGN.batch_statistics`` / ``recalibrate_bn`` (the
composition route) against the reference-generated fixture (tests/golden/make_golden_sgn_bnstats.py)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import sgn_bnstats_util as bu
from tests import sgn_util as su

ROOT = su.ROOT


def _model(case):
    import agcn_amd  # noqa: F401
    from agcn_amd.model.sgn import SGN
    c = bu.load_case(case)
    m = SGN(**su.model_args(c['meta']))
    m.load_state_dict(su.torch_state(c['state']))
    return c, m.eval()


def test_sgn_stats_plan_checker(tmp_path):
    cxx = next((c for c in (os.environ.get('CXX'), 'c++', 'g++', 'clang++') if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip('no host C++ compiler')
    exe = str(tmp_path / 'sgn_stats_plan_check')
    r = subprocess.run([cxx, '-std=c++17', '-Wall', '-Werror', '-O1', '-I', os.path.join(ROOT, '2s-agcn_amd', 'csrc'),
                        os.path.join(ROOT, 'tests', 'sgn_stats_plan_check.cpp'), '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-4000:]
    assert ' cases, 0 failures' in r.stdout and int(r.stdout.split(' cases')[0].split()[-1]) > 100000


@pytest.mark.parametrize('counts,per_clip', [([7] * 60, 20), ([32, 2] * 9, 2), ([20] * 9, 1), ([1, 1, 1, 5], 2)])
def test_finalize_merge_on_badly_centred_data(counts, per_clip):
    """|mean| / std = 50: E[z^2] - mean^2 in fp32 would lose the variance; the merge must not.  The bound is the fp32
    rounding of the inputs' own scale: the group sums carry a relative 2^-24 * count of a mean of 50 std, i.e. up to
    50 * 32 * 6e-8 = 1e-4 std per group mean, averaged down by the merge; 1e-4 relative on the variance leaves a margin
    of an order of magnitude over the second-order term that error can cause."""
    rng = np.random.default_rng(77)
    rows, C = sum(counts), 48
    std = rng.uniform(0.5, 2.0, C)
    z = (50.0 * std * rng.choice([-1.0, 1.0], C) + std * rng.standard_normal((rows, C))).astype(np.float32)
    sums, m2s = bu.group_partials(z, counts)
    mean, var, carry = bu.finalize_emulate(sums, m2s, counts, per_clip)
    z64 = z.astype(np.float64)
    # a group's fp32 sum of n <= 32 terms is off by at most n * 2^-24 of itself, and so is the merged mean (plus its rounding)
    assert np.abs(mean - z64.mean(0)).max() / np.abs(z64.mean(0)).max() < 34 * 2.0 ** -24
    assert (np.abs(var - z64.var(0)) / z64.var(0)).max() < 1e-4
    assert np.array_equal(carry[0], np.full(C, float(rows)))
    # a merge in chunks of whole clips through the carry state is the same sequence of operations: equal bits
    k = per_clip * (len(counts) // per_clip // 2)
    _, _, c1 = bu.finalize_emulate(sums[:k], m2s[:k], counts[:k], per_clip)
    mean2, var2, carry2 = bu.finalize_emulate(sums[k:], m2s[k:], counts[k:], per_clip, carry=c1)
    assert np.array_equal(mean, mean2) and np.array_equal(var, var2) and np.array_equal(carry, carry2)


@pytest.mark.parametrize('case', bu.CASES)
def test_batch_statistics_on_the_cpu_matches_the_reference(case):
    c, m = _model(case)
    rec = bu.load_record(case)
    x = torch.from_numpy(c['x'])
    before = {k: (v.clone(), v._version) for k, v in m.state_dict().items()}
    from agcn_amd import ops
    n_tensor = ops.SGN_STATS['forward_tensor']
    logits, g, stats = m.batch_statistics(x)
    assert ops.SGN_STATS['forward_tensor'] == n_tensor + 1
    assert not m.training and not m.cnn.dropout.training and all(
        m.get_submodule(n).track_running_stats and not m.get_submodule(n).training for n in bu.BN_NAMES)
    for k, v in m.state_dict().items():
        assert torch.equal(v, before[k][0]) and v._version == before[k][1], k
    assert tuple(stats) == bu.BN_NAMES
    N, seg, V = x.shape[0], x.shape[1], c['meta']['num_point']
    worst = 0.0
    for i, n in enumerate(bu.BN_NAMES):
        mean, var, count = stats[n]
        assert count == (N * seg * V if 2 <= i < 5 else N * seg), (n, count)
        worst = max(worst, bu.err(mean, rec['mean'][n]), bu.err(var, rec['var'][n]))
    e_l, e_g = bu.err(logits, rec['logits']), bu.err(g, rec['g'])
    print(f'{case}: composition vs reference: statistics {worst:.2e}, logits {e_l:.2e}, g {e_g:.2e}')
    assert worst < bu.BOUND and e_l < bu.BOUND and e_g < bu.BOUND
    # the same answer from train(): the state is restored there too
    m.train()
    logits2, _, _ = m.batch_statistics(x)
    assert m.training and m.cnn.dropout.training and torch.equal(logits2, logits)


@pytest.mark.parametrize('case', ['v15_seg20', 'v3_seg34'])
@pytest.mark.parametrize('momentum', [None, 0.1])
def test_recalibrate_bn_on_the_cpu_matches_the_reference(case, momentum):
    c, m = _model(case)
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
        assert bu.err(logits, rec['eval_logits']) < bu.BOUND and not torch.equal(logits, stale)
        # without reset a second call averages cumulatively: two equal batches leave the statistics where they are
        keep = {n: m.get_submodule(n).running_var.clone() for n in bu.BN_NAMES}
        m.recalibrate_bn(x, momentum=None, reset=False)
        for n in bu.BN_NAMES:
            assert int(m.get_submodule(n).num_batches_tracked) == 2
            assert bu.err(m.get_submodule(n).running_var, keep[n].numpy()) < 1e-6


def test_folded_without_override_is_unchanged():
    """``_folded()`` element for element what the parent's fold gives: every BatchNorm on its running statistics."""
    c, m = _model('v7_seg12_nobias')
    from agcn_amd import ops
    with torch.no_grad():
        frames, clip = m._folded()
        frames2, clip2 = m._folded({})
        V = m.num_point
        s, sh = ops._fold((m.gcn2.bn.weight, m.gcn2.bn.bias, m.gcn2.bn.running_mean, m.gcn2.bn.running_var))
        sj, shj = ops._fold((m.joint_embed.cnn[0].bn.weight, m.joint_embed.cnn[0].bn.bias,
                             m.joint_embed.cnn[0].bn.running_mean, m.joint_embed.cnn[0].bn.running_var))
        running = {n: (m.get_submodule(n).running_mean, m.get_submodule(n).running_var) for n in bu.BN_NAMES}
        frames3, clip3 = m._folded(running)
        ident, _ = m._folded({'gcn2.bn': None})
    assert len(frames) == 21 and len(clip) == 7
    for a, b, d in zip(frames + clip, frames2 + clip2, frames3 + clip3):
        assert torch.equal(a, b) and torch.equal(a, d)
    wcat = torch.cat([m.gcn2.w.cnn.weight.flatten(1).t(), m.gcn2.w1.cnn.weight.flatten(1).t()])
    assert torch.equal(frames[17], wcat * s[None, :]) and torch.equal(frames[18], torch.zeros(256) * s + sh)
    assert torch.equal(frames[0], sj.reshape(3, V).t()) and torch.equal(frames[1], shj.reshape(3, V).t())
    assert torch.equal(ident[17], wcat) and torch.equal(ident[18], torch.zeros(256))
    assert all(torch.equal(a, b) for i, (a, b) in enumerate(zip(frames, ident)) if i not in (17, 18))
    assert 'images' not in m._infer_cache


def test_one_sample_per_channel_is_refused():
    import agcn_amd  # noqa: F401
    from agcn_amd.model.sgn import SGN
    m = SGN(num_class=4, num_point=3, seg=1).eval()
    with pytest.raises(ValueError):
        m.batch_statistics(torch.zeros(1, 1, 9))
    with pytest.raises(ValueError):
        m.recalibrate_bn(torch.zeros(1, 1, 9))
    logits, _, stats = m.batch_statistics(torch.randn(2, 1, 9))
    assert tuple(logits.shape) == (2, 4) and stats['cnn.bn2'][2] == 2


def test_c_entries_refuse_bad_arguments_before_any_launch():
    """Argument errors come back before the first HIP call: no GPU needed."""
    from agcn_amd import lib
    L = lib.load()
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    wf, wc = L.agcn_sgn_frames_weights(15), L.agcn_sgn_clip_weights(20, 60)
    big = 1 << 30
    for layer in (0, 4):
        assert L.agcn_sgn_frames_stats(p, p, wf, p, big, layer, 1, 20, 15, None) == -1
    for layer in (0, 3):
        assert L.agcn_sgn_clip_stats(p, p, wc, p, big, layer, 1, 20, 60, None) == -1
    assert L.agcn_sgn_frames_stats(p, p, wf, p, big, 1, 1, 20, 33, None) == -1
    assert L.agcn_sgn_input_stats(p, p, big, 1, 20, 33, None) == -1
    assert L.agcn_sgn_frames_stats(p, p, wf + 1, p, big, 1, 1, 20, 15, None) == -1
    assert L.agcn_sgn_clip_stats(p, p, wc - 1, p, big, 2, 1, 20, 60, None) == -1
    assert L.agcn_sgn_frames_stats(None, p, wf, p, big, 1, 1, 20, 15, None) == -1
    assert L.agcn_sgn_frames_stats(p, p, wf, p, 16, 1, 1, 20, 15, None) == -2          # partial buffer too small
    assert L.agcn_sgn_frames_stats(p, p, wf, p, big, 1, 1 << 30, 20, 15, None) == -3   # outside sgn_frames_domain
    assert L.agcn_sgn_clip_stats(p, p, L.agcn_sgn_clip_weights(20, 5000), p, big, 1, 1, 20, 5000, None) == -3
    assert L.agcn_sgn_stats_finalize(p, big, 1, 4, 1, 20, 15, None, None, p, p, p, big, None) == -1
    assert L.agcn_sgn_stats_finalize(p, big, 3, 1, 1, 20, 15, None, None, p, p, p, big, None) == -1
    assert L.agcn_sgn_stats_finalize(p, big, 1, 1, 1, 20, 15, None, None, None, None, p, big, None) == -1
    assert L.agcn_sgn_stats_finalize(p, big, 1, 1, 1, 20, 15, None, None, p, p, None, big, None) == -1
    assert L.agcn_sgn_stats_finalize(p, 16, 1, 1, 1, 20, 15, None, None, p, p, p, big, None) == -2
    assert L.agcn_sgn_stats_finalize(p, big, 1, 1, 2, 20, 15, None, None, p, p, p, 2 * 3 * 128 * 8 - 1, None) == -2
    assert L.agcn_sgn_stats_finalize_workspace(1, 1, 2, 20, 15) == 2 * 3 * 128 * 8
    assert L.agcn_sgn_stats_finalize_workspace(2, 2, 3, 34, 0) == 3 * 3 * 512 * 8
    assert L.agcn_sgn_stats_part_floats(1, 3, 2, 20, 15) == 2 * 20 * 2 * 256
    assert L.agcn_sgn_stats_part_floats(2, 2, 2, 34, 0) == 2 * 2 * 2 * 512
    assert L.agcn_sgn_stats_part_floats(0, 0, 3, 20, 15) == 3 * 2 * 90
    assert L.agcn_sgn_stats_part_floats(1, 4, 2, 20, 15) == 0 and L.agcn_sgn_stats_part_floats(1, 1, 2, 20, 33) == 0
    assert L.agcn_sgn_stats_channels(1, 1, 15) == 128 and L.agcn_sgn_stats_channels(2, 2, 0) == 512


@pytest.mark.parametrize('case', ['v7_seg12_nobias', 'v3_seg34'])
def test_incremental_fold_equals_the_fold_with_overrides(case):
    """``_batch_folder`` patches one working image as the statistics arrive; what a pass reads of it (everything up to and
    including the identity BatchNorm's section) must be ``_folded(override)`` bit for bit, and the final images whole."""
    import math
    from agcn_amd import ops
    c, m = _model(case)
    rng = np.random.default_rng(5)
    with torch.no_grad():
        fold = m._batch_folder()
        fs, cs = ops.sgn_image_sections(m.num_point, m.seg, m.num_class)
        end = {n: o + math.prod(s) for n, o, s in fs + cs}
        read = {'gcn1.bn': (0, 'c1_b'), 'gcn2.bn': (0, 'c2_b'), 'gcn3.bn': (0, 'c3_b'), 'cnn.bn1': (1, 't1_b'),
                'cnn.bn2': (1, 't2_b')}
        known = {}
        for name in bu.BN_NAMES:
            if name in read:
                which, last = read[name]
                got, want = fold(known, name)[which], m._batch_images(known, name)[which]
                assert torch.equal(got[:end[last]], want[:end[last]]), name
            C = m.get_submodule(name).num_features
            known[name] = (torch.from_numpy(rng.standard_normal(C).astype(np.float32)),
                           torch.from_numpy(rng.uniform(0.01, 2.0, C).astype(np.float32)))
        for got, want in zip(fold(known, None), m._batch_images(known, None)):
            assert torch.equal(got, want)
    assert 'images' not in m._infer_cache
