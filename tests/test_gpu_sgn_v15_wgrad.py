"""GPU checks of the SGN v15 parameter gradients (the taping instantiations of csrc/sgn_v15_bwd.hip, the reductions of
csrc/sgn_v15_wgrad.hip, ``ops.sgn15_image_gradients``, ``SGN.parameter_gradients`` and the ``fused_finetune`` route).

1. Each taping entry ALONE over the table of tests/sgn_v15_grad_util.py: the same dfeat / dx bits as the untaped entry,
   and the image gradient reduced from its tape against fp64 autograd (tests/sgn_v15_wgrad_util.py), per section.
2. Forced row splits and one clip per chunk.
3. The whole model against the reference class's parameter gradients (tests/golden/sgn15_paramgrad_*.npz).
4. Routing.   5. Argument errors of the seven C entries.

Bound: the project's fp32 rule per tensor, 1e-4 relative to max(1, max|reference tensor|); every comparison prints its
ratio, a multiple of that bound, with its section name before it asserts.  What makes the inputs able to show an error
(margins, mutants) is asserted in tests/test_sgn_v15_grad_cpu.py and tests/test_sgn_v15_wgrad_cpu.py."""
import pytest
import torch

from tests import sgn_v15_domain_util as du
from tests import sgn_v15_grad_util as gu
from tests import sgn_v15_wgrad_util as wg

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
CASE_IDS = list(range(len(gu.CASES)))


def _dev(d):
    """The case's inputs on the device, with clones to assert they are left unmodified."""
    from agcn_amd import ops
    V, seg, sp, tp, num_class, _ = d['case']
    t = {k: d[k].contiguous().to(DEV) for k in ('x', 'wf', 'wc', 'feat32', 'dfeat_in', 'dlogits')}
    t['wf_t'], t['wc_t'] = ops.sgn15_transpose_images(t['wf'], t['wc'], V, seg, num_class, sp, tp)
    return t, {k: v.clone() for k, v in t.items()}


def _unmodified(t, keep):
    assert all(torch.equal(t[k], keep[k]) for k in t), 'an input was modified'


@pytest.mark.parametrize('i', CASE_IDS, ids=gu.IDS)
def test_clip_tape_kernel_alone(i):
    import agcn_amd  # noqa: F401
    from agcn_amd import ops
    V, seg, sp, tp, num_class, N = gu.CASES[i]
    d = wg.load(i)
    t, keep = _dev(d)
    dfeat, tape = ops.sgn15_clip_bwd_tape(t['feat32'], t['wc'], t['wc_t'], t['dlogits'], *tp)
    assert torch.equal(dfeat, ops.sgn15_clip_bwd(t['feat32'], t['wc'], t['wc_t'], t['dlogits'], *tp)), 'taping changed dfeat'
    d_wc = ops.sgn15_clip_wgrad(tape, t['dlogits'], t['wc'], seg, *tp)
    assert d_wc.shape == t['wc'].shape and bool(torch.isfinite(d_wc).all())
    r = wg.check_image(d_wc.cpu(), d['dwc64'], wg.sections(d['case'])[1], f'case {i} clip image gradient vs fp64 autograd')
    assert all(v <= 1.0 for v in r.values()), r
    dfeat2, tape2 = ops.sgn15_clip_bwd_tape(t['feat32'], t['wc'], t['wc_t'], t['dlogits'], *tp)      # equal bits again
    assert torch.equal(dfeat2, dfeat) and torch.equal(ops.sgn15_clip_wgrad(tape2, t['dlogits'], t['wc'], seg, *tp), d_wc)
    _unmodified(t, keep)


@pytest.mark.parametrize('i', CASE_IDS, ids=gu.IDS)
def test_frames_tape_kernel_alone(i):
    import agcn_amd  # noqa: F401
    from agcn_amd import ops
    V, seg, sp, tp, num_class, N = gu.CASES[i]
    d = wg.load(i)
    t, keep = _dev(d)
    dx, tape = ops.sgn15_frames_bwd_tape(t['x'], t['wf'], t['wf_t'], t['dfeat_in'], V, *sp)
    assert torch.equal(dx, ops.sgn15_frames_bwd(t['x'], t['wf'], t['wf_t'], t['dfeat_in'], V, *sp)), 'taping changed dx'
    d_wf = ops.sgn15_frames_wgrad(t['x'], t['wf'], tape, V, *sp)
    assert d_wf.shape == t['wf'].shape and bool(torch.isfinite(d_wf).all())
    r = wg.check_image(d_wf.cpu(), d['dwf64'], wg.sections(d['case'])[0], f'case {i} frames image gradient vs fp64 autograd')
    assert all(v <= 1.0 for v in r.values()), r
    dx2, tape2 = ops.sgn15_frames_bwd_tape(t['x'], t['wf'], t['wf_t'], t['dfeat_in'], V, *sp)         # equal bits again
    assert torch.equal(dx2, dx) and torch.equal(ops.sgn15_frames_wgrad(t['x'], t['wf'], tape2, V, *sp), d_wf)
    _unmodified(t, keep)


# ---- 2. forced row splits and one clip per chunk ----
@pytest.mark.parametrize('rows_per_split', (2, 32, 7))
@pytest.mark.parametrize('i', (0, 9, 1), ids=[gu.IDS[i] for i in (0, 9, 1)])
def test_row_splits_and_chunks(i, rows_per_split):
    """Each kernel alone with forced splits; then the chain x -> logits with ``max_tape_bytes=1`` (one clip per chunk)
    against the chain's own fp64 gradient (autograd through ``ops.sgn15_forward_ref``)."""
    import agcn_amd  # noqa: F401
    from agcn_amd import ops
    V, seg, sp, tp, num_class, N = gu.CASES[i]
    d = wg.load(i)
    t, _ = _dev(d)
    fs, cs = wg.sections(d['case'])
    _, ctape = ops.sgn15_clip_bwd_tape(t['feat32'], t['wc'], t['wc_t'], t['dlogits'], *tp)
    _, ftape = ops.sgn15_frames_bwd_tape(t['x'], t['wf'], t['wf_t'], t['dfeat_in'], V, *sp)
    r = wg.check_image(ops.sgn15_clip_wgrad(ctape, t['dlogits'], t['wc'], seg, *tp, rows_per_split=rows_per_split).cpu(),
                       d['dwc64'], cs, f'case {i} clip image gradient, {rows_per_split} rows per split')
    r.update({'f:' + k: v for k, v in wg.check_image(
        ops.sgn15_frames_wgrad(t['x'], t['wf'], ftape, V, *sp, rows_per_split=rows_per_split).cpu(), d['dwf64'], fs,
        f'case {i} frames image gradient, {rows_per_split} rows per split').items()})
    assert all(v <= 1.0 for v in r.values()), r
    # the chain in chunks of one clip: the counters equal the chunk count
    with torch.enable_grad():
        leaves = [d[k].double().requires_grad_(True) for k in ('x', 'wf', 'wc')]
        logits64 = ops.sgn15_forward_ref(*leaves, V, seg, num_class, sp, tp)[0]
        dx64, dwf64, dwc64 = torch.autograd.grad((logits64 * d['dlogits'].double()).sum(), leaves)
    before = dict(ops.SGN15_WGRAD_STATS)
    logits, dx, d_wf, d_wc = ops.sgn15_image_gradients(t['x'], t['wf'], t['wc'], t['wf_t'], t['wc_t'], t['dlogits'], V,
                                                       num_class, sp, tp, rows_per_split=rows_per_split, max_tape_bytes=1)
    assert ops.SGN15_WGRAD_STATS == {k: v + N for k, v in before.items()}
    rc = dict(logits=du.check(logits, logits64), dx=du.check(dx, dx64))
    print(f'case {i} chain in {N} chunks, in bounds: ' + ' '.join(f'{k} {v:.3e}' for k, v in rc.items()))
    rc.update({'c:' + k: v for k, v in wg.check_image(d_wc.cpu(), dwc64, cs, f'case {i} chain, clip image').items()})
    rc.update({'f:' + k: v for k, v in wg.check_image(d_wf.cpu(), dwf64, fs, f'case {i} chain, frames image').items()})
    assert all(v <= 1.0 for v in rc.values()), rc


# ---- 3. the whole model against the reference class's gradients ----
def _counters(ops):
    return dict(ops.SGN15_STATS), dict(ops.SGN15_WGRAD_STATS), ops.SGN_STATS['forward_tensor']


@pytest.mark.parametrize('case', gu.GRAD_CASES)
def test_parameter_gradients_match_the_reference(case):
    import agcn_amd  # noqa: F401
    from agcn_amd import ops
    m, x, cot, c = wg.build_model(case, DEV)
    fix = wg.load_paramgrad(case)
    fwd, wgs, tensor = _counters(ops)
    logits, aux, dx, grads = m.parameter_gradients(x, cot)
    assert ops.SGN15_STATS == {k: v + 1 for k, v in fwd.items()}, 'two forward launches'
    assert ops.SGN15_WGRAD_STATS == {k: v + 1 for k, v in wgs.items()}, 'two taping launches, two reductions'
    assert ops.SGN_STATS['forward_tensor'] == tensor, 'parameter_gradients ran the composition'
    assert all(p.grad is None for p in m.parameters())
    assert set(aux) == {'tem_emb', 'spa_emb', 'spatial_attn_list', 'temporal_attn_list'}
    r = wg.compare(grads, fix, f'{case} parameter_gradients vs the reference in fp64')
    r.update(logits=du.check(logits, c['logits']), dx=du.check(dx, c['grad_x64']))
    print(f'{case} in bounds: logits {r["logits"]:.3e} dx {r["dx"]:.3e}')
    assert all(v <= 1.0 for v in r.values()), r
    # dx: the bits of the untaped input gradient
    m.fused_input_gradient = True
    assert torch.equal(dx, m.input_gradient(x, cot)[2])
    # fused_finetune + backward(): the same .grad
    m.fused_finetune = True
    fwd, wgs, tensor = _counters(ops)
    out, _ = m(x)
    (out * cot).sum().backward()
    assert ops.SGN15_STATS == {k: v + 1 for k, v in fwd.items()} and ops.SGN_STATS['forward_tensor'] == tensor
    assert ops.SGN15_WGRAD_STATS == {k: v + 1 for k, v in wgs.items()}
    assert torch.equal(out.detach(), logits)
    for n, p in m.named_parameters():
        assert p.grad is not None and torch.equal(p.grad, grads[n]), n
    # the cached inference images still carry no graph
    with torch.no_grad():
        m(x)
    assert all(not t.requires_grad and t.grad_fn is None for t in m._infer_cache['images'][1:])


# ---- 4. routing ----
def test_routing():
    import agcn_amd  # noqa: F401
    from agcn_amd import ops
    case = gu.GRAD_CASES[0]
    m, x, cot, c = wg.build_model(case, DEV)
    fix = wg.load_paramgrad(case)
    # flag off: the composition
    fwd, wgs, tensor = _counters(ops)
    out, _ = m(x)
    (out * cot).sum().backward()
    assert ops.SGN_STATS['forward_tensor'] == tensor + 1 and ops.SGN15_WGRAD_STATS == wgs and ops.SGN15_STATS == fwd
    comp = {n: p.grad.clone() for n, p in m.named_parameters()}
    r = wg.compare(comp, fix, f'{case} composition backward() vs the reference in fp64')
    assert all(v <= 1.0 for v in r.values()), r
    m.zero_grad(set_to_none=True)
    # head-only requires_grad, and x.requires_grad adds x.grad
    m.fused_finetune = True
    head = lambda n: n.startswith('temporal_mha.') or n.startswith('fc.')      # noqa: E731
    for n, p in m.named_parameters():
        p.requires_grad_(head(n))
    xg = x.clone().requires_grad_(True)
    fwd, wgs, tensor = _counters(ops)
    out, _ = m(xg)
    (out * cot).sum().backward()
    assert ops.SGN_STATS['forward_tensor'] == tensor and ops.SGN15_WGRAD_STATS == {k: v + 1 for k, v in wgs.items()}
    for n, p in m.named_parameters():
        assert (p.grad is not None) == head(n), n
    sub = dict(fix, keys=[k for k in fix['keys'] if head(k)])
    r = wg.compare({n: p.grad for n, p in m.named_parameters() if head(n)}, sub, f'{case} head-only fine-tuning')
    r['x.grad'] = du.check(xg.grad, c['grad_x64'])
    print(f'{case} in bounds: x.grad {r["x.grad"]:.3e}')
    assert all(v <= 1.0 for v in r.values()), r
    logits, _, dx, grads = m.parameter_gradients(x, cot)
    assert sorted(grads) == sorted(n for n, _ in m.named_parameters() if head(n)) and torch.equal(dx, xg.grad)
    # nothing requires grad: not the fine-tuning route
    for p in m.parameters():
        p.requires_grad_(False)
    wgs = dict(ops.SGN15_WGRAD_STATS)
    m(x)
    assert ops.SGN15_WGRAD_STATS == wgs
    for p in m.parameters():
        p.requires_grad_(True)
    m.zero_grad(set_to_none=True)
    # AGCN_SGN_HIP=0 and train(): the composition; parameter_gradients raises in train()
    import os
    keep = os.environ.get('AGCN_SGN_HIP')
    os.environ['AGCN_SGN_HIP'] = '0'
    try:
        fwd, wgs, tensor = _counters(ops)
        out, _ = m(x)
        (out * cot).sum().backward()
        _, _, _, g0 = m.parameter_gradients(x, cot)
        assert ops.SGN_STATS['forward_tensor'] == tensor + 2 and ops.SGN15_WGRAD_STATS == wgs and ops.SGN15_STATS == fwd
        r = wg.compare(g0, fix, f'{case} parameter_gradients with AGCN_SGN_HIP=0 (the composition)')
        assert all(v <= 1.0 for v in r.values()), r
    finally:
        if keep is None:
            del os.environ['AGCN_SGN_HIP']
        else:
            os.environ['AGCN_SGN_HIP'] = keep
    m.train()
    fwd, wgs, tensor = _counters(ops)
    m(x)
    assert ops.SGN_STATS['forward_tensor'] == tensor + 1 and ops.SGN15_WGRAD_STATS == wgs
    with pytest.raises(ValueError):
        m.parameter_gradients(x, cot)
    m.eval()
    with torch.no_grad():
        m(x)
    assert all(not t.requires_grad and t.grad_fn is None for t in m._infer_cache['images'][1:])
    assert 'fused_finetune' not in m.state_dict()


def test_parameter_gradients_frames_image_only():
    """The mirror of the head-only set of ``test_routing``: only ``spatial_mha.*`` trainable, so the CLIP image carries no
    graph.  On the smallest whole-model fixture."""
    import agcn_amd  # noqa: F401
    from agcn_amd import ops
    case = 'j5_seg3_sliced'
    m, x, cot, c = wg.build_model(case, DEV)
    fix = wg.load_paramgrad(case)
    _, _, want_dx, _ = m.parameter_gradients(x, cot)
    inside = lambda n: n.startswith('spatial_mha.')      # noqa: E731
    for n, p in m.named_parameters():
        p.requires_grad_(inside(n))
    with torch.enable_grad():
        wf, wc, _, _ = m._finetune_images()
    assert wf.requires_grad and not wc.requires_grad
    fwd, wgs, tensor = _counters(ops)
    _, _, dx, grads = m.parameter_gradients(x, cot)
    assert ops.SGN15_STATS == {k: v + 1 for k, v in fwd.items()} and ops.SGN_STATS['forward_tensor'] == tensor
    assert ops.SGN15_WGRAD_STATS == {k: v + 1 for k, v in wgs.items()}
    assert sorted(grads) == sorted(n for n, _ in m.named_parameters() if inside(n)) and grads
    assert torch.equal(dx, want_dx)
    r = wg.compare(grads, dict(fix, keys=[k for k in fix['keys'] if inside(k)]), f'{case} spatial_mha only')
    assert all(v <= 1.0 for v in r.values()), r


# ---- 5. argument errors of the seven C entries ----
def test_entries_refuse_bad_arguments():
    """The tape short by one float, the workspace short by 4 bytes, d_head 48, V = 33, num_class 0, rows_per_split -1 and
    a null tape: an error code, the outputs stay zero and no counter moves."""
    import agcn_amd  # noqa: F401
    from agcn_amd import lib, ops
    V, seg, sp, tp, num_class, N = gu.CASES[1]
    d = wg.load(1)
    t, _ = _dev(d)
    L = lib.load()
    ft, ct = L.agcn_sgn15_frames_tape_floats(N, seg, V, *sp), L.agcn_sgn15_clip_tape_floats(N, seg, num_class, *tp)
    fw, cw = L.agcn_sgn15_wgrad_workspace(N, seg, V, 0, *sp, 0), L.agcn_sgn15_wgrad_workspace(N, seg, 0, num_class, *tp, 0)
    assert ft == N * seg * V * (4 * sp[0] * sp[1] + 2 * sp[2] + 1120)
    assert ct == N * seg * (4 * tp[0] * tp[1] + 2 * tp[2] + 1536) + N * 512 and fw > 0 and cw > 0
    # the size queries return 0 outside the domain
    assert L.agcn_sgn15_frames_tape_floats(N, seg, 33, *sp) == 0 and L.agcn_sgn15_frames_tape_floats(N, seg, V, 8, 48, 128) == 0
    assert L.agcn_sgn15_clip_tape_floats(N, seg, 0, *tp) == 0 and L.agcn_sgn15_clip_tape_floats(N, seg, num_class, 8, 48, 256) == 0
    assert L.agcn_sgn15_wgrad_workspace(N, seg, V, 0, *sp, -1) == 0 and L.agcn_sgn15_wgrad_workspace(N, seg, 33, 0, *sp, 0) == 0
    assert L.agcn_sgn15_wgrad_workspace(N, seg, 0, 0, *tp, 0) == 0 and L.agcn_sgn15_wgrad_workspace(N, seg, 0, num_class, 8, 48, 256, 0) == 0
    ftape, ctape = torch.zeros(ft, device=DEV), torch.zeros(ct, device=DEV)
    dfeat, dx = torch.zeros_like(t['feat32']), torch.zeros_like(t['x'])
    d_wf, d_wc = torch.zeros_like(t['wf']), torch.zeros_like(t['wc'])
    bws = torch.zeros(L.agcn_sgn15_frames_bwd_workspace(N, seg, V) // 4, device=DEV)
    ws = torch.zeros(max(fw, cw) // 4, device=DEV)
    stats = dict(ops.SGN15_WGRAD_STATS)

    def clip_tape(tape=ctape, floats=ct, geo=tp, nc=num_class):
        return lib.status('agcn_sgn15_clip_bwd_tape', t['feat32'], t['wc'], t['wc'].numel(), t['wc_t'], t['wc_t'].numel(),
                          t['dlogits'], dfeat, N, seg, nc, *geo, tape, floats)

    def frames_tape(tape=ftape, floats=ft, geo=sp, v=V):
        return lib.status('agcn_sgn15_frames_bwd_tape', t['x'], t['wf'], t['wf'].numel(), t['wf_t'], t['wf_t'].numel(),
                          t['dfeat_in'], dx, bws, bws.numel() * 4, N, seg, v, *geo, tape, floats)

    def frames_wgrad(tape=ftape, floats=ft, ws_b=fw, geo=sp, v=V, rps=0):
        return lib.status('agcn_sgn15_frames_wgrad', t['x'], tape, floats, d_wf, d_wf.numel(), ws, ws_b, N, seg, v, *geo, rps)

    def clip_wgrad(tape=ctape, floats=ct, ws_b=cw, geo=tp, nc=num_class, rps=0):
        return lib.status('agcn_sgn15_clip_wgrad', tape, floats, t['dlogits'], d_wc, d_wc.numel(), ws, ws_b, N, seg, nc, *geo,
                          rps)

    for fn in (clip_tape, frames_tape, frames_wgrad, clip_wgrad):
        assert fn(floats=(ct if fn in (clip_tape, clip_wgrad) else ft) - 1) == lib.ERR_WORKSPACE, fn.__name__
        assert fn(geo=(8, 48, 128)) == lib.ERR_ARG and fn(tape=None) == lib.ERR_ARG, fn.__name__
    assert frames_wgrad(ws_b=fw - 4) == lib.ERR_WORKSPACE and clip_wgrad(ws_b=cw - 4) == lib.ERR_WORKSPACE
    assert frames_tape(v=33) == lib.ERR_ARG and frames_wgrad(v=33) == lib.ERR_ARG
    assert clip_tape(nc=0) == lib.ERR_ARG and clip_wgrad(nc=0) == lib.ERR_ARG
    assert frames_wgrad(rps=-1) == lib.ERR_ARG and clip_wgrad(rps=-1) == lib.ERR_ARG
    torch.cuda.synchronize()
    for name, out in (('dfeat', dfeat), ('dx', dx), ('d_wf', d_wf), ('d_wc', d_wc), ('frames tape', ftape),
                      ('clip tape', ctape), ('ws', ws)):
        assert not bool(out.any()), f'{name} was written by a refused call'
    assert ops.SGN15_WGRAD_STATS == stats
    with pytest.raises(ValueError):
        ops.sgn15_frames_wgrad(t['x'], t['wf'], ftape, V, *sp, rows_per_split=-1)
    # and the accepted calls run
    assert clip_tape() == 0 and frames_tape() == 0 and frames_wgrad() == 0 and clip_wgrad() == 0
    torch.cuda.synchronize()
