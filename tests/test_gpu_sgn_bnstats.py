"""GPU checks of SGN's batch statistics on the fused path (csrc/sgn_stats.hip) against the reference-generated fixture
(tests/golden/make_golden_sgn_bnstats.py): the seven means and variances, the logits and g under them, ``recalibrate_bn``
for both kinds of momentum, bitwise independence of chunking, repetition and the batch around a clip, the rebuilt fold
cache, and the error codes of the C entries.  Every comparison is within 1e-4 * max(1, max|ref|) per tensor."""
import numpy as np
import pytest
import torch

from tests import sgn_bnstats_util as bu
from tests import sgn_util as su

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
_RUNS = {}


def _model(case, train=False):
    import agcn_amd  # noqa: F401
    from agcn_amd.model.sgn import SGN
    c = bu.load_case(case)
    m = SGN(**su.model_args(c['meta']))
    m.load_state_dict(su.torch_state(c['state']))
    return c, m.to(DEV).train(train)


def _counters():
    from agcn_amd import ops
    return dict(ops.SGN_BNSTATS_STATS), dict(ops.SGN_STATS)


def _run(case):
    """One ``batch_statistics`` per case, shared by the tests: dict(c, m, x, logits, g, stats, launches, plain)."""
    if case not in _RUNS:
        c, m = _model(case)
        x = torch.from_numpy(c['x']).to(DEV)
        b0, s0 = _counters()
        logits, g, stats = m.batch_statistics(x)
        b1, s1 = _counters()
        _RUNS[case] = dict(c=c, m=m, x=x, logits=logits, g=g, stats=stats,
                           launches={k: b1[k] - b0[k] for k in b1}, plain={k: s1[k] - s0[k] for k in s1})
    return _RUNS[case]


def _chunk_cap(m, x, clips):
    from agcn_amd import ops
    cap = clips * ops.sgn_stats_clip_bytes(x.shape[1], m.num_point)
    assert ops.sgn_stats_chunk(x.shape[0], x.shape[1], m.num_point, cap) == clips
    return cap


@pytest.mark.parametrize('case', bu.CASES)
def test_batch_statistics_match_the_reference(case):
    r = _run(case)
    rec = bu.load_record(case)
    N, seg, V = r['x'].shape[0], r['x'].shape[1], r['m'].num_point
    # the HIP route ran: one input pass, three frames passes, two clip passes, a finalize each (one chunk), and the two
    # full-depth launches; nothing as tensor code
    assert r['launches'] == dict(input_stats=1, frames_stats=3, clip_stats=2, stats_finalize=6)
    assert r['plain'] == dict(frames_hip=1, clip_hip=1, sample_hip=0, forward_tensor=0)
    assert tuple(r['stats']) == bu.BN_NAMES
    errs = {}
    for i, n in enumerate(bu.BN_NAMES):
        mean, var, count = r['stats'][n]
        assert count == (N * seg * V if 2 <= i < 5 else N * seg), (n, count)
        errs['mean.' + n], errs['var.' + n] = bu.err(mean, rec['mean'][n]), bu.err(var, rec['var'][n])
    errs['logits'], errs['g'] = bu.err(r['logits'], rec['logits']), bu.err(r['g'], rec['g'])
    if case in su.TRAIN_CASES:
        errs['sgn_train logits'] = bu.err(r['logits'], su.load_train(case)['logits'])
    worst = max(errs, key=errs.get)
    print(f'{case}: fused batch statistics vs reference: logits {errs["logits"]:.2e}, g {errs["g"]:.2e}, worst {worst} '
          f'{errs[worst]:.2e} (reference noise floor {max(rec["floor"].values()):.2e})')
    assert errs[worst] < bu.BOUND, (worst, errs[worst])


@pytest.mark.parametrize('case', bu.CASES)
@pytest.mark.parametrize('momentum', [None, 0.1])
def test_recalibrate_bn_matches_the_reference(case, momentum):
    c, m = _model(case, train=(momentum is not None))          # any training state
    rec = bu.load_record(case)
    x = torch.from_numpy(c['x']).to(DEV)
    stats = m.recalibrate_bn(x, momentum=momentum)
    tag = 'none' if momentum is None else '01'
    errs = {}
    for n in bu.BN_NAMES:
        bn = m.get_submodule(n)
        assert int(bn.num_batches_tracked) == 1
        errs['running_mean.' + n] = bu.err(bn.running_mean, rec['rm_' + tag][n])
        errs['running_var.' + n] = bu.err(bn.running_var, rec['rv_' + tag][n])
        assert torch.equal(stats[n][0], _run(case)['stats'][n][0])
    worst = max(errs, key=errs.get)
    print(f'{case}, momentum {momentum}: running statistics vs reference: worst {worst} {errs[worst]:.2e}')
    assert errs[worst] < bu.BOUND, (worst, errs[worst])
    assert m.training == (momentum is not None)


def test_chunks_of_whole_clips_give_the_same_bits():
    case, clips = bu.CHUNKED
    r = _run(case)
    from agcn_amd import ops
    b0, _ = _counters()
    logits, g, stats = r['m'].batch_statistics(r['x'], max_part_bytes=_chunk_cap(r['m'], r['x'], clips))
    b1, _ = _counters()
    assert {k: b1[k] - b0[k] for k in b1} == dict(input_stats=3, frames_stats=9, clip_stats=6, stats_finalize=18)   # 4 + 4 + 1
    assert torch.equal(logits, r['logits']) and torch.equal(g, r['g'])
    for n in bu.BN_NAMES:
        assert torch.equal(stats[n][0], r['stats'][n][0]) and torch.equal(stats[n][1], r['stats'][n][1]), n
    assert ops.sgn_stats_chunk(9, 20, 15, 0) == 1


def test_two_calls_give_the_same_bits():
    r = _run('v3_seg34')
    logits, g, stats = r['m'].batch_statistics(r['x'])
    assert torch.equal(logits, r['logits']) and torch.equal(g, r['g'])
    for n in bu.BN_NAMES:
        assert torch.equal(stats[n][0], r['stats'][n][0]) and torch.equal(stats[n][1], r['stats'][n][1]), n


@pytest.mark.parametrize('case', ['v15_seg20', 'v3_seg34'])
def test_a_clips_partials_do_not_depend_on_its_batch(case):
    """Per-group partials of clip 1 alone and inside the batch, pass by pass, on the images the passes really use."""
    from agcn_amd import ops
    r = _run(case)
    m, x, V = r['m'], r['x'], r['m'].num_point
    N, seg = x.shape[0], x.shape[1]
    one = x[1:2].contiguous()
    known = {n: r['stats'][n][:2] for n in bu.BN_NAMES}
    tiles = (seg + 31) // 32
    both = ops.sgn_input_stats(x, V), ops.sgn_input_stats(one, V)
    assert tuple(both[0].shape) == (N, 2, 6 * V) and torch.equal(both[0][1:2], both[1])
    for layer in (1, 2, 3):
        wf, _ = m._batch_images(known, f'gcn{layer}.bn')
        a, b = ops.sgn_frames_stats(x, wf, layer, V), ops.sgn_frames_stats(one, wf, layer, V)
        assert tuple(a.shape) == (N * seg, 2, 128 if layer == 1 else 256) and torch.equal(a[seg:2 * seg], b), layer
        assert float(a[:, 1].min()) >= 0.0
    wf, _ = m._batch_images(known, None)
    feat, _ = ops.sgn_frames(x, wf, V)
    for layer in (1, 2):
        _, wc = m._batch_images(known, f'cnn.bn{layer}')
        a = ops.sgn_clip_stats(feat, wc, layer, m.num_class)
        b = ops.sgn_clip_stats(feat[1:2].contiguous(), wc, layer, m.num_class)
        assert tuple(a.shape) == (N * tiles, 2, 256 * layer) and torch.equal(a[tiles:2 * tiles], b), layer
    # the finalize on those partials, against the numpy emulation of its merge (fp64 state, ascending groups)
    counts = [min(32, seg - 32 * (i % tiles)) for i in range(N * tiles)]
    mean, var, carry = ops.sgn_stats_finalize(a, 2, 2, N, seg, V, want_carry=True)
    e_mean, e_var, e_carry = bu.finalize_emulate(a[:, 0].cpu().numpy(), a[:, 1].cpu().numpy(), counts, tiles)
    assert np.array_equal(carry.cpu().numpy()[0], e_carry[0]) and float(carry[0, 0]) == N * seg
    assert bu.err(mean, e_mean) < 1e-6 and bu.err(var, e_var) < 1e-6
    assert torch.equal(mean, r['stats']['cnn.bn2'][0]) and torch.equal(var, r['stats']['cnn.bn2'][1])


def test_prediction_after_recalibration_uses_rebuilt_images():
    case = 'v15_seg20'
    c, m = _model(case)
    rec = bu.load_record(case)
    x = torch.from_numpy(c['x']).to(DEV)
    with torch.no_grad():
        first, _ = m(x)
        key = m._infer_cache['images'][0]
        m.recalibrate_bn(x)
        assert m._infer_cache['images'][0] == key           # batch images never enter the cache ...
        second, _ = m(x)
        assert m._infer_cache['images'][0] != key           # ... and the in-place writes invalidate it
    assert bu.err(first, su.load_case(case)['logits']) < bu.BOUND
    e = bu.err(second, rec['eval_logits'])
    print(f'{case}: eval logits after recalibrate_bn vs reference {e:.2e}')
    assert e < bu.BOUND and not torch.equal(first, second)


def test_batch_statistics_mutates_nothing():
    c, m = _model('v7_seg12_nobias')
    x = torch.from_numpy(c['x']).to(DEV)
    with torch.no_grad():
        m(x)                                               # a warm fold cache must survive as well
    cache = dict(m._infer_cache)
    before = {k: (v.clone(), v._version) for k, v in list(m.named_parameters()) + list(m.named_buffers())}
    for train in (False, True):
        m.train(train)
        m.batch_statistics(x)
        assert m.training == train
    for k, v in list(m.named_parameters()) + list(m.named_buffers()):
        assert torch.equal(v, before[k][0]) and v._version == before[k][1], k
    assert set(m._infer_cache) == set(cache) and all(m._infer_cache[k] is cache[k] for k in cache)


def test_c_entries_return_their_error_codes():
    from agcn_amd import lib, ops
    L = lib.load()
    c, m = _model('v15_seg20')
    x = torch.from_numpy(c['x']).to(DEV)
    wf, wc = m._images()
    part = torch.empty(5 * 20 * 2 * 512, device=DEV)
    feat = torch.zeros(5, 20, 256, device=DEV)
    args = (lib.ptr(x), lib.ptr(wf), wf.numel(), lib.ptr(part), part.numel())
    cargs = (lib.ptr(feat), lib.ptr(wc), wc.numel(), lib.ptr(part), part.numel())
    assert L.agcn_sgn_frames_stats(*args, 0, 5, 20, 15, lib.stream()) == -1
    assert L.agcn_sgn_frames_stats(*args, 4, 5, 20, 15, lib.stream()) == -1
    assert L.agcn_sgn_clip_stats(*cargs, 0, 5, 20, 60, lib.stream()) == -1
    assert L.agcn_sgn_clip_stats(*cargs, 4, 5, 20, 60, lib.stream()) == -1
    assert L.agcn_sgn_frames_stats(*args, 1, 5, 20, 33, lib.stream()) == -1
    assert L.agcn_sgn_input_stats(lib.ptr(x), lib.ptr(part), part.numel(), 5, 20, 33, lib.stream()) == -1
    assert L.agcn_sgn_frames_stats(lib.ptr(x), lib.ptr(wf), wf.numel() - 1, lib.ptr(part), part.numel(), 1, 5, 20, 15,
                                   lib.stream()) == -1
    assert L.agcn_sgn_clip_stats(lib.ptr(feat), lib.ptr(wc), wc.numel() + 1, lib.ptr(part), part.numel(), 1, 5, 20, 60,
                                 lib.stream()) == -1
    assert L.agcn_sgn_frames_stats(lib.ptr(x), lib.ptr(wf), wf.numel(), lib.ptr(part), 100, 1, 5, 20, 15, lib.stream()) == -2
    assert L.agcn_sgn_stats_finalize(lib.ptr(part), part.numel(), 1, 4, 5, 20, 15, None, None, lib.ptr(part), lib.ptr(part),
                                     lib.ptr(part), part.numel() * 4, lib.stream()) == -1
    assert L.agcn_sgn_stats_finalize(lib.ptr(part), part.numel(), 1, 1, 5, 20, 15, None, None, lib.ptr(part), lib.ptr(part),
                                     lib.ptr(part), 64, lib.stream()) == -2
    with pytest.raises(ValueError):
        ops.sgn_frames_stats(x, wf, 1, 14)
    with pytest.raises(ValueError):
        ops.sgn_stats_finalize(part, 1, 1, 5, 20, 15, carry=torch.zeros(3, 64, dtype=torch.float64, device=DEV))
    torch.cuda.synchronize()
