"""GPU checks of SGN v15's batch statistics on the fused path (csrc/sgn_v15_stats.hip): each pass alone against the fp64
tensor reference on seeded images, badly centred data, bitwise independence of repetition, of the batch around a clip and
of chunking, the sections a pass must not read, the buffer contract, the whole model against the reference-generated
fixture (tests/golden/make_golden_sgn_v15_bnstats.py), routing and the error codes of the C entries.  Every comparison
is within 1e-4 * max(1, max|ref|) per tensor; the shapes are the smallest at which the kernels can still go wrong."""
import math

import numpy as np
import pytest
import torch

from tests import sgn_v15_bnstats_util as bu

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
NAN = float('nan')
_RUNS = {}


def _ops():
    import agcn_amd  # noqa: F401
    from agcn_amd import ops
    return ops


def _launch(p, kind, layer, src=None, wimg=None):
    """The partials of pass (kind, layer) of a ``bu.pass_case``; src / wimg override its input / image."""
    ops = _ops()
    if kind == 'frames':
        src = p['x'].to(DEV) if src is None else src
        return ops.sgn15_frames_stats(src, p['wf'].to(DEV) if wimg is None else wimg, layer, p['V'], *p['spatial'])
    src = p['feat32'].to(DEV) if src is None else src
    return ops.sgn15_clip_stats(src, p['wc'].to(DEV) if wimg is None else wimg, layer, bu.PASS_NUM_CLASS, *p['temporal'])


def _finalize(p, kind, layer, part, N=None):
    ops = _ops()
    k = ops.SGN15_STATS_FRAMES if kind == 'frames' else ops.SGN15_STATS_CLIP
    return ops.sgn15_stats_finalize(part, k, layer, p['N'] if N is None else N, p['seg'], p['V'])[:2]


def _pass_ratios(p, kind, layer):
    """-> {statistic: worst difference from the fp64 reference as a multiple of the bound} of one pass."""
    z = p['tile64'][kind, layer]
    part = _launch(p, kind, layer)
    s64, q64 = bu.group_partials(z)
    mean, var = _finalize(p, kind, layer, part)
    m64, v64 = bu.two_pass(z)
    assert tuple(part.shape) == (z.shape[0], 2, z.shape[2])
    assert float(part[:, 1].min()) >= 0.0
    return part, dict(sum=bu.ratio(part[:, 0], s64), m2=bu.ratio(part[:, 1], q64), mean=bu.ratio(mean, m64),
                      var=bu.ratio(var, v64))


@pytest.mark.parametrize('i', range(len(bu.PASS_CASES)), ids=bu.PASS_IDS)
def test_each_pass_alone_matches_fp64(i):
    p = bu.pass_case(i)
    worst = {}
    for kind, layer in bu.PASSES:
        part, r = _pass_ratios(p, kind, layer)
        print(f'{bu.PASS_IDS[i]} {kind} layer {layer}: ratio to the bound: ' + ', '.join(f'{k} {v:.3g}' for k, v in r.items()))
        worst[kind, layer] = max(r.values())
        if kind == 'clip' and p['seg'] == 1:
            assert float(part[:, 1].abs().max()) == 0.0          # one sample per group: M2 is exactly 0
    print(f'{bu.PASS_IDS[i]}: worst ratio to the bound {max(worst.values()):.3g}')
    assert max(worst.values()) < 1.0, worst


@pytest.mark.parametrize('i', bu.CENTRED, ids=[bu.PASS_IDS[i] for i in bu.CENTRED])
def test_badly_centred_data(i):
    """A mean of hundreds of standard deviations: an fp32 E[z^2] - mean^2 loses the variance, the kernels must not.  The
    offsets were chosen on the CPU (sgn_v15_bnstats_util.py): the first two assertions hold without a GPU."""
    p = bu.pass_case(i, centred=True)
    for kind, layer in bu.PASSES:
        z64, z32 = p['tile64'][kind, layer], p['tile32'][kind, layer]
        m64, v64 = bu.two_pass(z64)
        mutant = bu.ratio(bu.raw_moments(z32)[1], v64)
        m32, v32 = bu.two_pass(z32)
        tensor = max(bu.ratio(m32, m64), bu.ratio(v32, v64))
        assert mutant >= 100.0 and tensor <= 0.1, (kind, layer, mutant, tensor)
        _, r = _pass_ratios(p, kind, layer)
        print(f'{bu.PASS_IDS[i]} centred {kind} layer {layer}: max|mean| {float(m64.abs().max()):.0f}, max var '
              f'{float(v64.max()):.3g}; fp32 E[z^2]-mean^2 {mutant:.0f} bounds, fp32 two-pass {tensor:.3f}, kernels '
              + ', '.join(f'{k} {v:.3g}' for k, v in r.items()))
        assert max(r.values()) < 1.0, (kind, layer, r)


@pytest.mark.parametrize('i', (1, 3))
def test_partials_are_the_same_bits_again_and_alone(i):
    p = bu.pass_case(i)
    x, feat = p['x'].to(DEV), p['feat32'].to(DEV)
    keep = x.clone(), feat.clone(), p['wf'].clone(), p['wc'].clone()
    wf, wc = p['wf'].to(DEV), p['wc'].to(DEV)
    seg = p['seg']
    for kind, layer in bu.PASSES:
        src, img, per = (x, wf, seg) if kind == 'frames' else (feat, wc, 1)
        a = _launch(p, kind, layer, src, img)
        b = _launch(p, kind, layer, src, img)
        one = _launch(p, kind, layer, src[1:2].contiguous(), img)
        assert torch.equal(a, b), (kind, layer)
        assert torch.equal(a[per:2 * per], one), (kind, layer)
    assert torch.equal(x, keep[0]) and torch.equal(feat, keep[1])
    assert torch.equal(wf.cpu(), keep[2]) and torch.equal(wc.cpu(), keep[3])


def _poisoned(img, secs, keep):
    """A copy of the image with every section whose name is not in ``keep`` filled with NaN."""
    out = img.clone()
    for n, o, s in secs:
        if n not in keep:
            out[o:o + math.prod(s)] = NAN
    return out


@pytest.mark.parametrize('i', (2, 3))
def test_a_pass_does_not_read_the_sections_behind_its_batchnorm(i):
    ops = _ops()
    p = bu.pass_case(i)
    fs, cs = ops.sgn15_image_sections(p['V'], p['seg'], bu.PASS_NUM_CLASS, p['spatial'], p['temporal'])
    wf, wc = p['wf'].to(DEV), p['wc'].to(DEV)
    inputs = {n for n, _, _ in fs if not n.startswith('s_')}
    half = ('qkv_w', 'qkv_b', 'o_w', 'o_b')
    images = {('frames', 1): _poisoned(wf, fs, inputs),
              ('frames', 2): _poisoned(wf, fs, inputs | {'s_' + n for n in half}),
              ('clip', 1): _poisoned(wc, cs, {'tem'}),
              ('clip', 2): _poisoned(wc, cs, {'tem'} | {'t_' + n for n in half})}
    for (kind, layer), img in images.items():
        assert bool(torch.isnan(img).any())
        got, want = _launch(p, kind, layer, wimg=img), _launch(p, kind, layer)
        assert torch.equal(got, want) and not bool(torch.isnan(got).any()), (kind, layer)


@pytest.mark.parametrize('i', (1, 2))
def test_buffers_are_written_whole_and_not_beyond(i):
    """Partial buffers and finalize workspaces with guard floats behind the queried size: the guards stay, every float
    inside is written (pre-filled with NaN)."""
    from agcn_amd import lib
    ops = _ops()
    L = lib.load()
    p = bu.pass_case(i)
    N, seg, V = p['N'], p['seg'], p['V']
    x, feat, wf, wc = p['x'].to(DEV), p['feat32'].to(DEV), p['wf'].to(DEV), p['wc'].to(DEV)
    GUARD, MARK = 64, 12345.0
    for kind, layer in bu.PASSES:
        k = ops.SGN15_STATS_FRAMES if kind == 'frames' else ops.SGN15_STATS_CLIP
        n = L.agcn_sgn15_stats_part_floats(k, layer, N, seg, V)
        C = L.agcn_sgn15_stats_channels(k, layer)
        assert n == (N * seg if kind == 'frames' else N) * 2 * C and C == (128 if kind == 'frames' else 256)
        part = torch.full((n + GUARD,), NAN, device=DEV)
        part[n:] = MARK
        if kind == 'frames':
            rc = L.agcn_sgn15_frames_stats(lib.ptr(x), lib.ptr(wf), wf.numel(), lib.ptr(part), n, layer, N, seg, V,
                                           *p['spatial'], lib.stream())
        else:
            rc = L.agcn_sgn15_clip_stats(lib.ptr(feat), lib.ptr(wc), wc.numel(), lib.ptr(part), n, layer, N, seg,
                                         bu.PASS_NUM_CLASS, *p['temporal'], lib.stream())
        assert rc == 0
        assert not bool(torch.isnan(part[:n]).any()) and bool((part[n:] == MARK).all()), (kind, layer)
        nbytes = L.agcn_sgn15_stats_finalize_workspace(k, layer, N, seg, V)
        assert nbytes == N * 3 * C * 8
        ws = torch.full((nbytes // 8 + GUARD,), NAN, dtype=torch.float64, device=DEV)
        ws[nbytes // 8:] = MARK
        out = torch.full((2 * C + GUARD,), NAN, device=DEV)
        out[2 * C:] = MARK
        carry = torch.full((3 * C + GUARD,), NAN, dtype=torch.float64, device=DEV)
        carry[3 * C:] = MARK
        rc = L.agcn_sgn15_stats_finalize(lib.ptr(part), n, k, layer, N, seg, V, None, carry.data_ptr(), lib.ptr(out),
                                         lib.ptr(out[C:]), ws.data_ptr(), nbytes, lib.stream())
        assert rc == 0
        for buf, size in ((ws, nbytes // 8), (out, 2 * C), (carry, 3 * C)):
            assert not bool(torch.isnan(buf[:size]).any()) and bool((buf[size:] == MARK).all()), (kind, layer)
        assert float(carry[0]) == N * seg * (V if kind == 'frames' else 1)
        mean, var = _finalize(p, kind, layer, part[:n].view(-1, 2, C))
        assert torch.equal(mean, out[:C]) and torch.equal(var, out[C:2 * C])


# ---- the whole model ----------------------------------------------------------------------------------------------------
def _counters():
    ops = _ops()
    return dict(ops.SGN15_BNSTATS_STATS), dict(ops.SGN_BNSTATS_STATS), dict(ops.SGN_STATS), dict(ops.SGN15_STATS)


def _moved(before):
    return [{k: a[k] - b[k] for k in a} for a, b in zip(_counters(), before)]


def _run(case):
    """One ``batch_statistics`` per case, shared by the tests and never modified."""
    if case not in _RUNS:
        c, m = bu.model(case, DEV)
        x = torch.from_numpy(c['x']).to(DEV)
        before = _counters()
        logits, aux, stats = m.batch_statistics(x)
        _RUNS[case] = dict(c=c, m=m, x=x, logits=logits, aux=aux, stats=stats, moved=_moved(before))
    return _RUNS[case]


@pytest.mark.parametrize('case', bu.CASES)
def test_batch_statistics_match_the_reference(case):
    r = _run(case)
    rec = bu.load_record(case)
    N, seg, V = r['x'].shape[0], r['x'].shape[1], r['m'].num_point
    # the HIP route ran: the input pass, two frames passes, two clip passes, a finalize each (one chunk) and the two
    # full-depth launches; nothing as tensor code
    v15, base, plain, full = r['moved']
    assert v15 == dict(frames_stats=2, clip_stats=2, stats_finalize=4)
    assert base == dict(input_stats=1, frames_stats=0, clip_stats=0, stats_finalize=1)
    assert plain == dict(frames_hip=0, clip_hip=0, sample_hip=0, forward_tensor=0) and full == dict(frames_hip=1, clip_hip=1)
    assert tuple(r['stats']) == bu.BN_NAMES
    errs = {}
    for i, n in enumerate(bu.BN_NAMES):
        mean, var, count = r['stats'][n]
        assert count == (N * seg * V if 2 <= i < 4 else N * seg), (n, count)
        errs['mean.' + n], errs['var.' + n] = bu.err(mean, rec['mean'][n]), bu.err(var, rec['var'][n])
    errs['logits'] = bu.err(r['logits'], rec['logits'])
    worst = max(errs, key=errs.get)
    print(f'{case}: fused batch statistics vs reference: logits {errs["logits"]:.2e}, worst {worst} {errs[worst]:.2e} '
          f'(reference noise floor {max(rec["floor"].values()):.2e})')
    assert errs[worst] < bu.BOUND, (worst, errs[worst])
    assert tuple(r['aux']['spa_emb'].shape) == (N, 64, V, seg) and tuple(r['aux']['tem_emb'].shape) == (N, 256, V, seg)


@pytest.mark.parametrize('case', bu.CASES)
@pytest.mark.parametrize('momentum', [None, 0.1])
def test_recalibrate_bn_matches_the_reference(case, momentum):
    c, m = bu.model(case, DEV, train=(momentum is not None))          # any training state
    rec = bu.load_record(case)
    x = torch.from_numpy(c['x']).to(DEV)
    with torch.no_grad():
        m.eval()
        stale, _ = m(x)
        key = m._infer_cache['images'][0]
        m.train(momentum is not None)
    stats = m.recalibrate_bn(x, momentum=momentum)
    assert m.training == (momentum is not None)
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
    if momentum is None:
        with torch.no_grad():
            assert m._infer_cache['images'][0] == key            # batch images never enter the cache ...
            logits, _ = m.eval()(x)
            assert m._infer_cache['images'][0] != key            # ... and the in-place writes invalidate it
        e = bu.err(logits, rec['eval_logits'])
        print(f'{case}: eval logits after recalibrate_bn vs reference {e:.2e}')
        assert e < bu.BOUND and not torch.equal(logits, stale)


def _chunk_cap(m, x, clips):
    ops = _ops()
    cap = clips * ops.sgn15_stats_clip_bytes(x.shape[1], m.num_point)
    assert ops.sgn15_stats_chunk(x.shape[0], x.shape[1], m.num_point, cap) == clips
    return cap


@pytest.mark.parametrize('clips,chunks', [(1, 9), (4, 3)])
def test_chunks_of_whole_clips_give_the_same_bits(clips, chunks):
    case = bu.CHUNKED[0]
    r = _run(case)
    before = _counters()
    x0 = r['x'].clone()
    logits, _, stats = r['m'].batch_statistics(r['x'], max_part_bytes=_chunk_cap(r['m'], r['x'], clips))
    v15, base, plain, full = _moved(before)
    assert v15 == dict(frames_stats=2 * chunks, clip_stats=2 * chunks, stats_finalize=4 * chunks)
    assert base == dict(input_stats=chunks, frames_stats=0, clip_stats=0, stats_finalize=chunks)
    assert full == dict(frames_hip=1, clip_hip=1) and plain['forward_tensor'] == 0
    assert torch.equal(logits, r['logits']) and torch.equal(r['x'], x0)
    for n in bu.BN_NAMES:
        assert torch.equal(stats[n][0], r['stats'][n][0]) and torch.equal(stats[n][1], r['stats'][n][1]), n
    assert _ops().sgn15_stats_chunk(9, 20, 15, 0) == 1


def test_a_constant_channel_and_the_composition_on_the_gpu():
    """j3_seg2 has spa columns whose ReLU is dead for every joint: variance below 1e-12, finite logits; and the fused
    route agrees with the composition on the same device."""
    r = _run('j3_seg2')
    meta = r['c']['meta']
    assert sum(meta['constant_channels'].values()) > 0
    var = r['stats'][bu.BN_NAMES[2]][1]
    rec = bu.load_record('j3_seg2')
    dead = np.flatnonzero(rec['var'][bu.BN_NAMES[2]] < 1e-12)
    assert len(dead) == meta['constant_channels'][bu.BN_NAMES[2]] and len(dead) > 0
    assert float(var[torch.from_numpy(dead).to(DEV)].max()) < 1e-12
    assert bool(torch.isfinite(r['logits']).all())
    for case in ('j3_seg2', 'j9_seg7_h2x256'):
        r = _run(case)
        logits, _, stats = r['m']._batch_statistics_tensor(r['x'])
        errs = [bu.err(r['logits'], logits)]
        for n in bu.BN_NAMES:
            errs += [bu.err(r['stats'][n][0], stats[n][0]), bu.err(r['stats'][n][1], stats[n][1])]
            assert r['stats'][n][2] == stats[n][2]
        print(f'{case}: fused vs composition on the GPU {max(errs):.2e}')
        assert max(errs) < bu.BOUND


def test_routing(monkeypatch):
    ops = _ops()
    r = _run('j7_seg12_nobias')
    m, x = r['m'], r['x']
    state = {k: (v.clone(), v._version) for k, v in m.state_dict().items()}
    for train in (True, False):
        m.train(train)
        before = _counters()
        logits, _, _ = m.batch_statistics(x)
        v15, base, plain, full = _moved(before)
        assert m.training == train and torch.equal(logits, r['logits'])
        assert v15 == dict(frames_stats=2, clip_stats=2, stats_finalize=4) and base['input_stats'] == 1
        assert plain == dict(frames_hip=0, clip_hip=0, sample_hip=0, forward_tensor=0) and full == dict(frames_hip=1, clip_hip=1)
    for k, v in m.state_dict().items():
        assert torch.equal(v, state[k][0]) and v._version == state[k][1], k

    def tensor_route(model, inp):
        before = _counters()
        out = model.batch_statistics(inp)
        v15, base, plain, full = _moved(before)
        assert plain['forward_tensor'] == 1 and not any(v15.values()) and not any(base.values()) and not any(full.values())
        return out

    # a non-contiguous x
    wide = torch.cat([x, x], dim=2)[:, :, :x.shape[2]]
    assert not wide.is_contiguous()
    logits, _, _ = tensor_route(m, wide)
    assert bu.err(logits, r['logits']) < bu.BOUND
    # a structure outside _structure_fused(): a projected attention residual in the spatial block
    c = r['c']
    kw = dict(c['meta']['model_args'])
    kw['spatial_mha_kwargs'] = dict(kw['spatial_mha_kwargs'], res_proj=True)
    from agcn_amd.model.sgn_v15 import SGN
    other = SGN(**kw).to(DEV)
    assert not other._structure_fused()
    tensor_route(other, x)
    # the switch
    monkeypatch.setenv('AGCN_SGN_HIP', '0')
    assert not ops.sgn_hip_enabled()
    logits, _, _ = tensor_route(m, x)
    assert bu.err(logits, r['logits']) < bu.BOUND


def test_c_entries_return_their_error_codes():
    from agcn_amd import lib
    ops = _ops()
    L = lib.load()
    p = bu.pass_case(2)
    N, seg, V = p['N'], p['seg'], p['V']
    x, feat, wf, wc = p['x'].to(DEV), p['feat32'].to(DEV), p['wf'].to(DEV), p['wc'].to(DEV)
    part = torch.zeros(N * seg * 2 * 256, device=DEV)
    ws = torch.zeros(N * 3 * 256, dtype=torch.float64, device=DEV)
    s = lib.stream()
    sp, tp, nc = p['spatial'], p['temporal'], bu.PASS_NUM_CLASS
    fr = lambda **k: L.agcn_sgn15_frames_stats(*[k.get(a, d) for a, d in (                                    # noqa: E731
        ('x', lib.ptr(x)), ('w', lib.ptr(wf)), ('wn', wf.numel()), ('part', lib.ptr(part)), ('pn', part.numel()),
        ('layer', 1), ('N', N), ('seg', seg), ('V', V), ('heads', sp[0]), ('d_head', sp[1]), ('ff', sp[2]))], s)
    cl = lambda **k: L.agcn_sgn15_clip_stats(*[k.get(a, d) for a, d in (                                      # noqa: E731
        ('x', lib.ptr(feat)), ('w', lib.ptr(wc)), ('wn', wc.numel()), ('part', lib.ptr(part)), ('pn', part.numel()),
        ('layer', 1), ('N', N), ('seg', seg), ('nc', nc), ('heads', tp[0]), ('d_head', tp[1]), ('ff', tp[2]))], s)
    fin = lambda **k: L.agcn_sgn15_stats_finalize(*[k.get(a, d) for a, d in (                                 # noqa: E731
        ('part', lib.ptr(part)), ('pn', part.numel()), ('kind', 1), ('layer', 1), ('N', N), ('seg', seg), ('V', V),
        ('cin', None), ('cout', None), ('mean', lib.ptr(part)), ('var', lib.ptr(part)), ('ws', ws.data_ptr()),
        ('wsn', ws.numel() * 8))], s)
    before = _counters()
    for entry in (fr, cl):
        assert entry(x=None) == -1 and entry(w=None) == -1 and entry(part=None) == -1
        assert entry(layer=0) == -1 and entry(layer=3) == -1
        assert entry(wn=wf.numel() + wc.numel()) == -1
        assert entry(pn=100) == -2
        assert entry(d_head=24) == -3
    assert fr(V=33) == -1 and fr(wn=wf.numel() - 1) == -1 and cl(wn=wc.numel() + 1) == -1
    assert cl(seg=33) == -3
    assert fin(part=None) == -1 and fin(ws=None) == -1 and fin(mean=None) == -1
    assert fin(layer=0) == -1 and fin(layer=3) == -1 and fin(kind=0) == -1 and fin(kind=3) == -1
    assert fin(pn=100) == -2 and fin(wsn=N * 3 * 128 * 8 - 1) == -2
    assert fin(kind=2, seg=33) == -3
    assert L.agcn_sgn15_stats_part_floats(1, 0, N, seg, V) == 0 and L.agcn_sgn15_stats_part_floats(2, 1, N, 33, V) == 0
    assert L.agcn_sgn15_stats_part_floats(3, 1, N, seg, V) == 0 and L.agcn_sgn15_stats_channels(1, 3) == 0
    assert L.agcn_sgn15_stats_finalize_workspace(2, 3, N, seg, V) == 0
    assert L.agcn_sgn15_stats_finalize_workspace(2, 2, N, seg, 0) == N * 3 * 256 * 8
    with pytest.raises(ValueError):
        ops.sgn15_frames_stats(x, wf, 1, V - 1, *sp)
    with pytest.raises(ValueError):
        ops.sgn15_stats_finalize(part, 1, 1, N, seg, V, carry=torch.zeros(3, 64, dtype=torch.float64, device=DEV))
    assert not any(any(d.values()) for d in _moved(before))
    torch.cuda.synchronize()
    assert float(part.abs().max()) == 0.0 and float(ws.abs().max()) == 0.0        # nothing was launched
