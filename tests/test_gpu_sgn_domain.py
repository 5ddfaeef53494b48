"""GPU checks of the base SGN kernels (csrc/sgn.hip, csrc/sgn_bwd.hip, csrc/sgn_wgrad.hip), each ALONE, over the tables
of tests/sgn_domain_util.py against fp64 references on seeded weight images and seeded tapes: no model, no fixture.

  frames kernel        ``ops.sgn_frames`` on x                      vs the reference's feat and g
  clip kernel          ``ops.sgn_clip`` on the REFERENCE's feat rounded to fp32
                                                                    vs the reference's logits from that same input
  clip backward        ``ops.sgn_clip_bwd`` on that feat and a seeded d logits      vs fp64 autograd through ``clip_ref``
  frames backward      ``ops.sgn_frames_bwd`` on x and a seeded d feat              vs fp64 autograd through ``frames_ref``
  the taped route      ``ops.sgn_image_gradients``, section by section              vs fp64 autograd of
                                                                                       ``ops.sgn_image_forward_ref``
  the reductions       ``ops.sgn_frames_wgrad`` / ``ops.sgn_clip_wgrad`` on tapes of standard-normal floats
                                                                    vs numpy fp64 sums taken from the documented layout

so every kernel answers for its own error only.  Bound: the project's fp32 rule per tensor, 1e-4 relative to
max(1, max|reference tensor|); the printed ratios are multiples of that bound (measured on MI355X:
profiles/sgn_domain.txt).  What makes these inputs able to show an error is asserted in tests/test_sgn_domain_cpu.py."""
import re

import pytest
import torch

from tests import sgn_domain_util as du

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
SENTINEL = 1024
MARK = -777.0


def _ids(table):
    return dict(argvalues=list(range(len(du.TABLES[table]))), ids=du.ids(table))


def _report(what, r):
    print(f'sgn_domain: {what}: ' + ' '.join(f'{k} {v:.3e}' for k, v in r.items()))
    assert all(v <= 1.0 for v in r.values()), (what, r)


def _guarded(n):
    """n floats with SENTINEL marked floats behind them -> (the buffer, its first n floats)."""
    buf = torch.full((n + SENTINEL,), MARK, device=DEV)
    return buf, buf[:n]


def _untouched(buf, n):
    return bool((buf[n:] == MARK).all())


# ---- the forward kernels ----
@pytest.mark.parametrize('i', **_ids('fwd'))
def test_frames_kernel_alone(i):
    import agcn_amd  # noqa: F401
    from agcn_amd import ops
    V, seg, _, N = du.CASES[i]
    d = du.load('fwd', i)
    x, wf = d['x'].to(DEV), d['wf'].to(DEV)
    feat, g = ops.sgn_frames(x, wf, V)
    assert tuple(feat.shape) == (N, seg, 256) and bool(torch.isfinite(feat).all())
    assert tuple(g.shape) == (N, seg, V, V) and bool(torch.isfinite(g).all())       # real rows only: no padded entries exist
    rowsum = float((g.double().sum(-1) - 1).abs().max())
    assert rowsum <= 1e-5, rowsum
    _report(f'case {i} {du.CASES[i]} frames fused vs fp64', dict(feat=du.check(feat, d['frames']['feat']), g=du.check(g, d['frames']['g'])))
    # the same bits without g, and for clip 1 alone
    quiet, none = ops.sgn_frames(x, wf, V, want_g=False)
    assert none is None and torch.equal(quiet, feat)
    alone, alone_g = ops.sgn_frames(x[1:2].contiguous(), wf, V)
    assert torch.equal(alone[0], feat[1]) and torch.equal(alone_g[0], g[1])


@pytest.mark.parametrize('i', **_ids('fwd'))
def test_clip_kernel_alone(i):
    import agcn_amd  # noqa: F401
    from agcn_amd import ops
    _, _, nc, N = du.CASES[i]
    d = du.load('fwd', i)
    feat, wc = d['feat32'].to(DEV), d['wc'].to(DEV)
    logits = ops.sgn_clip(feat, wc, nc)
    assert tuple(logits.shape) == (N, nc) and bool(torch.isfinite(logits).all())
    _report(f'case {i} {du.CASES[i]} clip fused vs fp64', dict(logits=du.check(logits, d['clip']['logits'])))
    alone = ops.sgn_clip(feat[1:2].contiguous(), wc, nc)
    assert torch.equal(alone[0], logits[1])


# ---- the input-gradient kernels ----
@pytest.mark.parametrize('i', **_ids('clip_grad'))
def test_clip_backward_alone(i):
    import agcn_amd  # noqa: F401
    from agcn_amd import lib, ops
    case = du.CLIP_GRAD[i]
    _, seg, nc, N = case
    d = du.load('clip_grad', i)
    _, wc_t = du.transposed(d['wf'], d['wc'], case)
    feat, wc, wc_t, dl = d['feat32'].to(DEV), d['wc'].to(DEV), wc_t.to(DEV), d['dlogits'].to(DEV)
    dfeat = ops.sgn_clip_bwd(feat, wc, wc_t, dl)
    assert tuple(dfeat.shape) == (N, seg, 256) and bool(torch.isfinite(dfeat).all())
    _report(f'clip backward {i} {case[1:]} fused vs fp64', dict(dfeat=du.check(dfeat, d['dfeat64'])))
    # the taping variant: the same bits, and a tape of exactly the queried size
    taped, tape = ops.sgn_clip_bwd_tape(feat, wc, wc_t, dl)
    assert torch.equal(taped, dfeat)
    n = lib.load().agcn_sgn_clip_tape_floats(N, seg, nc)
    assert tape.numel() == n
    buf, own = _guarded(n)
    again = torch.empty_like(dfeat)
    lib.call("agcn_sgn_clip_bwd_tape", feat, wc, wc.numel(), wc_t, wc_t.numel(), dl, again, N, seg, nc, own, n)
    torch.cuda.synchronize()
    assert _untouched(buf, n) and torch.equal(again, dfeat) and torch.equal(own, tape)
    if N > 1:
        alone = ops.sgn_clip_bwd(feat[1:2].contiguous(), wc, wc_t, dl[1:2].contiguous())
        assert torch.equal(alone[0], dfeat[1])


@pytest.mark.parametrize('i', **_ids('frames_grad'))
def test_frames_backward_alone(i):
    import agcn_amd  # noqa: F401
    from agcn_amd import lib, ops
    case = du.FRAMES_GRAD[i]
    V, seg, _, N = case
    d = du.load('frames_grad', i)
    wf_t, _ = du.transposed(d['wf'], d['wc'], case)
    x, wf, wf_t, df = d['x'].to(DEV), d['wf'].to(DEV), wf_t.to(DEV), d['dfeat_in'].to(DEV)
    dx = ops.sgn_frames_bwd(x, wf, wf_t, df, V)
    assert tuple(dx.shape) == (N, seg, 3 * V) and bool(torch.isfinite(dx).all())
    _report(f'frames backward {i} {(V, seg, N)} fused vs fp64', dict(dx=du.check(dx, d['dx64'])))
    taped, tape = ops.sgn_frames_bwd_tape(x, wf, wf_t, df, V)
    assert torch.equal(taped, dx)
    L = lib.load()
    n, nws = L.agcn_sgn_frames_tape_floats(N, seg, V), L.agcn_sgn_frames_bwd_workspace(N, seg, V) // 4
    assert tape.numel() == n and nws > 0
    buf, own = _guarded(n)
    wbuf, ws = _guarded(nws)
    again = torch.empty_like(dx)
    lib.call("agcn_sgn_frames_bwd_tape", x, wf, wf.numel(), wf_t, wf_t.numel(), df, again, ws, nws * 4, N, seg, V, own, n)
    torch.cuda.synchronize()
    assert _untouched(buf, n) and _untouched(wbuf, nws) and torch.equal(again, dx)
    # the tape rows pad their 2638 columns to 2656: the pad is never written, everything else is the same bits
    assert torch.equal(own.reshape(-1, du.FT['cols'])[:, :2638], tape.reshape(-1, du.FT['cols'])[:, :2638])
    if N > 1:
        alone = ops.sgn_frames_bwd(x[1:2].contiguous(), wf, wf_t, df[1:2].contiguous(), V)
        assert torch.equal(alone[0], dx[1])


@pytest.mark.parametrize('i', **_ids('whole'))
def test_taped_route_per_section(i):
    import agcn_amd  # noqa: F401
    from agcn_amd import ops
    case = du.WHOLE[i]
    V, seg, nc, N = case
    d = du.load('whole', i)
    wf_t, wc_t = du.transposed(d['wf'], d['wc'], case)
    x, wf, wc, cot = (d[k].to(DEV) for k in ('x', 'wf', 'wc', 'cot'))
    logits, g, dx, d_wf, d_wc = ops.sgn_image_gradients(x, wf, wc, wf_t.to(DEV), wc_t.to(DEV), cot, V, nc)
    assert bool(torch.isfinite(d_wf).all()) and bool(torch.isfinite(d_wc).all())
    _, r = du.whole_section_ratios(d_wf.cpu(), d_wc.cpu(), d)
    r['dx'] = du.check(dx, d['dx64'])
    with torch.no_grad():                           # the chained forward: the clip half on the fp64 feat
        r['logits'] = du.check(logits, du.clip_ref(d['frames']['feat'], d['wc'].double(), case)['logits'])
    r['g'] = du.check(g, d['frames']['g'])
    _report(f'taped route {i} {case} cot x {d["cot_scale"]:g} fused vs fp64', r)


# ---- the weight-gradient reductions on seeded tapes ----
def _splits_noted():
    from agcn_amd import lib
    note = lib.load().agcn_last_kernel().decode()
    assert note.startswith('sgn_wgrad_gemm_kernel'), note
    return int(re.search(r'splits=(\d+)', note).group(1))


@pytest.mark.parametrize('case', du.FRAMES_TAPES, ids=['x'.join(map(str, c)) for c in du.FRAMES_TAPES])
def test_frames_reduction_on_a_seeded_tape(case):
    import agcn_amd  # noqa: F401
    from agcn_amd import lib, ops
    V, seg, N, rps = case
    nc = 60
    x, tape = du.frames_tape_inputs(case)
    ref = du.frames_tape_ref(x, tape, case)
    secs = ops.sgn_image_sections(V, seg, nc)[0]
    x, tape = torch.from_numpy(x).to(DEV), torch.from_numpy(tape).reshape(-1).to(DEV)
    wf = torch.zeros(secs[-1][1] + 256, device=DEV)
    got = ops.sgn_frames_wgrad(x, wf, tape, V, nc, rps)
    assert _splits_noted() == du.splits(N * seg * V, rps)
    assert got.numel() == wf.numel() and bool(torch.isfinite(got).all())
    r = du.reduction_ratios(du.image_dict(got, secs), ref)
    _report(f'frames tape {case} rows {N * seg * V} splits {du.splits(N * seg * V, rps)} vs fp64', r)
    assert torch.equal(ops.sgn_frames_wgrad(x, wf, tape, V, nc, rps), got)
    # through the C entry, with the workspace at exactly the queried size
    nws = lib.load().agcn_sgn_wgrad_workspace(N, seg, V, nc, rps) // 4
    assert nws > 0 and tape.numel() == lib.load().agcn_sgn_frames_tape_floats(N, seg, V)
    wbuf, ws = _guarded(nws)
    obuf, own = _guarded(wf.numel())
    lib.call("agcn_sgn_frames_wgrad", x, wf, tape, own, ws, nws * 4, N, seg, V, rps)
    torch.cuda.synchronize()
    assert _untouched(wbuf, nws) and _untouched(obuf, wf.numel()) and torch.equal(own, got)


@pytest.mark.parametrize('case', du.CLIP_TAPES, ids=['x'.join(map(str, c)) for c in du.CLIP_TAPES])
def test_clip_reduction_on_a_seeded_tape(case):
    import agcn_amd  # noqa: F401
    from agcn_amd import lib, ops
    seg, nc, N, rps = case
    V = 2
    tp, dfeat, dlogits = du.clip_tape_inputs(case)
    ref = du.clip_tape_ref(tp, dfeat, dlogits, case)
    secs = ops.sgn_image_sections(V, seg, nc)[1]
    tape = torch.cat([torch.from_numpy(tp[k]).reshape(-1) for k in ('h', 'y1', 'dy1', 'dy2', 'ymax')]).to(DEV)
    dfeat, dlogits = torch.from_numpy(dfeat).to(DEV), torch.from_numpy(dlogits).to(DEV)
    wc = torch.zeros(secs[-1][1] + nc, device=DEV)
    assert tape.numel() == lib.load().agcn_sgn_clip_tape_floats(N, seg, nc)
    got = ops.sgn_clip_wgrad(tape, dfeat, dlogits, wc, V, rps)
    assert _splits_noted() == du.splits(N * seg, rps)
    assert got.numel() == wc.numel() and bool(torch.isfinite(got).all())
    r = du.reduction_ratios(du.image_dict(got, secs), ref)
    _report(f'clip tape {case} rows {N * seg} splits {du.splits(N * seg, rps)} vs fp64', r)
    assert torch.equal(ops.sgn_clip_wgrad(tape, dfeat, dlogits, wc, V, rps), got)
    nws = lib.load().agcn_sgn_wgrad_workspace(N, seg, V, nc, rps) // 4
    assert nws > 0
    wbuf, ws = _guarded(nws)
    obuf, own = _guarded(wc.numel())
    lib.call("agcn_sgn_clip_wgrad", tape, dfeat, dlogits, own, ws, nws * 4, N, seg, nc, rps)
    torch.cuda.synchronize()
    assert _untouched(wbuf, nws) and _untouched(obuf, wc.numel()) and torch.equal(own, got)
