"""GPU checks of SGN's eval-mode parameter gradients on the fused path (csrc/sgn_wgrad.hip): against the reference's
gradients (tests/golden/make_golden_sgn_paramgrad.py), per section of the two weight images against fp64 autograd of the
tensor-code image reference, with forced row splits and tape chunks, reproducibility and the taped dx, the routing of
``SGN.forward`` with ``fused_finetune``, and the argument errors of the C entries.  Every shape is a fixture case.
Bound: tests/sgn_wgrad_util.py (1e-4 relative to max(1, max |reference tensor|), per tensor)."""
import os

import numpy as np
import pytest
import torch

from tests import sgn_grad_util as gu
from tests import sgn_wgrad_util as wu

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
CASES = gu.stored_cases()
ONE = dict(clip_bwd_tape=1, frames_bwd_tape=1, frames_wgrad=1, clip_wgrad=1)
_REF = {}


def _stats():
    from agcn_amd import ops
    return dict(ops.SGN_STATS), dict(ops.SGN_GRAD_STATS), dict(ops.SGN_WGRAD_STATS)


def _delta(before):
    return tuple({k: n[k] - b[k] for k in n} for n, b in zip(_stats(), before))


def _err(got, ref):
    ref = np.asarray(ref.detach().cpu() if torch.is_tensor(ref) else ref, dtype=np.float64)
    got = np.asarray(got.detach().cpu() if torch.is_tensor(got) else got, dtype=np.float64)
    return float(np.abs(got - ref).max() / max(1.0, float(np.abs(ref).max())))


def _image_reference(case):
    """fp64 autograd of ops.sgn_image_forward_ref on the CPU, once per case -> (d_wf, d_wc, dx) as float64 tensors."""
    if case not in _REF:
        from agcn_amd import ops
        model, x, c, _ = wu.build_model(case)
        with torch.no_grad():
            wf, wc, _, _ = model._finetune_images()
        leaves = [t.double().requires_grad_(True) for t in (x, wf, wc)]
        logits, _ = ops.sgn_image_forward_ref(*leaves, model.num_point, model.seg, model.num_class)
        dx, d_wf, d_wc = torch.autograd.grad((logits * c.double()).sum(), leaves)
        _REF[case] = (d_wf, d_wc, dx)
    return _REF[case]


def _sections(model, got_f, got_c, case):
    """-> (worst error, its section) of the two image gradients against the fp64 image reference, section by section."""
    from agcn_amd import ops
    d_wf, d_wc, _ = _image_reference(case)
    fs, cs = ops.sgn_image_sections(model.num_point, model.seg, model.num_class)
    worst = (0.0, '')
    for got, ref, secs in ((got_f, d_wf, fs), (got_c, d_wc, cs)):
        assert got.shape == ref.shape and bool(torch.isfinite(got).all())
        for name, o, shape in secs:
            n = int(np.prod(shape))
            worst = max(worst, (_err(got[o:o + n], ref[o:o + n]), name))
    return worst


@pytest.mark.parametrize('case', CASES)
def test_parameter_gradients_match_the_reference(case):
    model, x, c, d = wu.build_model(case, DEV)
    fix = wu.load_paramgrad(case)
    before = _stats()
    logits, g, dx, grads = model.parameter_gradients(x, c)
    fwd, bwd, wg = _delta(before)
    assert fwd == dict(frames_hip=1, clip_hip=1, sample_hip=0, forward_tensor=0)
    assert bwd == dict(clip_bwd=0, frames_bwd=0, sample_bwd=0) and wg == ONE
    assert _err(logits, d['logits']) < wu.BOUND and _err(g, d['g']) < wu.BOUND and _err(dx, d['grad_x']) < wu.BOUND
    err, name, floor = wu.compare(grads, fix, case)
    print(f'{case}: parameter_gradients vs reference: worst {err:.2e} ({name}, reference floor {floor:.1e})')
    assert all(p.grad is None for p in model.parameters())
    # the same through forward + backward() with the flag set
    model.fused_finetune = True
    before = _stats()
    out, g2 = model(x)
    assert out.requires_grad and not g2.requires_grad and torch.equal(out, logits) and torch.equal(g2, g)
    (out * c).sum().backward()
    fwd, bwd, wg = _delta(before)
    assert fwd == dict(frames_hip=1, clip_hip=1, sample_hip=0, forward_tensor=0) and wg == ONE
    err, name, floor = wu.compare({n: p.grad for n, p in model.named_parameters()}, fix, case)
    print(f'{case}: forward + backward(): worst {err:.2e} ({name}, reference floor {floor:.1e})')


@pytest.mark.parametrize('case', CASES)
def test_image_gradients_per_section(case):
    from agcn_amd import ops
    model, x, c, _ = wu.build_model(case, DEV)
    with torch.no_grad():
        images = model._finetune_images()
    logits, g, dx, d_wf, d_wc = ops.sgn_image_gradients(x, *images, c, model.num_point, model.num_class)
    assert d_wf.shape == images[0].shape and d_wc.shape == images[1].shape
    err, name = _sections(model, d_wf, d_wc, case)
    e_x = _err(dx, _image_reference(case)[2])
    print(f'{case}: image gradients vs fp64 image reference: worst section {name} {err:.2e}, dx {e_x:.2e}')
    assert err < wu.BOUND and e_x < wu.BOUND


@pytest.mark.parametrize('rows_per_split', [2, 32, 7])
@pytest.mark.parametrize('case', CASES)
def test_row_splits_and_tape_chunks(case, rows_per_split):
    """Several splits with even, tile-sized and odd tails, and one clip per tape chunk (two chunks at bs = 2): each
    against the references."""
    from agcn_amd import ops
    model, x, c, d = wu.build_model(case, DEV)
    with torch.no_grad():
        images = model._finetune_images()
    bs = x.shape[0]
    assert ops.sgn_tape_chunk(bs, model.seg, model.num_point, model.num_class, 1) == 1
    before = _stats()
    _, _, dx, d_wf, d_wc = ops.sgn_image_gradients(x, *images, c, model.num_point, model.num_class,
                                                   rows_per_split=rows_per_split, max_tape_bytes=1)
    assert _delta(before)[2] == {k: bs for k in ONE}
    err, name = _sections(model, d_wf, d_wc, case)
    _, _, _, grads = model.parameter_gradients(x, c, rows_per_split=rows_per_split, max_tape_bytes=1)
    perr, pname, floor = wu.compare(grads, wu.load_paramgrad(case), case)
    print(f'{case} rows_per_split {rows_per_split}, {bs} chunk(s): worst section {name} {err:.2e}; parameters {perr:.2e} '
          f'({pname}, reference floor {floor:.1e})')
    assert err < wu.BOUND and _err(dx, d['grad_x']) < wu.BOUND


@pytest.mark.parametrize('case', CASES)
def test_reproducible_and_same_dx_as_the_input_gradient(case):
    from agcn_amd import ops
    model, x, c, _ = wu.build_model(case, DEV)
    with torch.no_grad():
        images = model._finetune_images()
    keep = [t.clone() for t in (x,) + tuple(images)]
    a = ops.sgn_image_gradients(x, *images, c, model.num_point, model.num_class)
    b = ops.sgn_image_gradients(x, *images, c, model.num_point, model.num_class)
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    assert all(torch.equal(p, q) for p, q in zip(keep, (x,) + tuple(images)))
    logits, g, dx = model.input_gradient(x, c)
    assert torch.equal(a[2], dx) and torch.equal(a[0], logits) and torch.equal(a[1], g)
    assert float(a[3].abs().max()) > 0 and float(a[4].abs().max()) > 0


def test_routing():
    from agcn_amd import ops
    case = 'v15_seg6'
    model, x, c, d = wu.build_model(case, DEV)
    fix = wu.load_paramgrad(case)
    _, _, want_dx = model.input_gradient(x, c)
    zero = {k: 0 for k in ONE}
    tensor = dict(frames_hip=0, clip_hip=0, sample_hip=0, forward_tensor=1)

    def run(xin):
        model.zero_grad(set_to_none=True)
        before = _stats()
        logits, _ = model(xin)
        (logits * c).sum().backward()
        return _delta(before)

    # flag false, trainable parameters: the composition, as before
    assert model.fused_finetune is False
    fwd, _, wg = run(x)
    assert fwd == tensor and wg == zero
    wu.compare({n: p.grad for n, p in model.named_parameters()}, fix)
    # flag true, only the head trainable: those get gradients, everything else none; x.requires_grad adds x.grad
    model.fused_finetune = True
    head = ('cnn.', 'fc.', 'tem_embed.')
    for n, p in model.named_parameters():
        p.requires_grad_(n.startswith(head))
    xg = x.clone().requires_grad_(True)
    fwd, bwd, wg = run(xg)
    assert fwd == dict(frames_hip=1, clip_hip=1, sample_hip=0, forward_tensor=0) and wg == ONE
    assert bwd == dict(clip_bwd=0, frames_bwd=0, sample_bwd=0)
    assert torch.equal(xg.grad, want_dx)
    got = {n: p.grad for n, p in model.named_parameters() if n.startswith(head)}
    assert all(v is not None for v in got.values()) and got
    assert all(p.grad is None for n, p in model.named_parameters() if not n.startswith(head))
    sub = dict(fix, keys=[k for k in fix['keys'] if k.startswith(head)])
    err, name, floor = wu.compare(got, sub, 'head only')
    print(f'head-only fine-tuning: worst {err:.2e} ({name}, reference floor {floor:.1e})')
    # parameter_gradients with a partial trainable set: the head leaves the frames image without a graph, gcn3 alone the
    # clip image
    for tag, pick in (('head only', lambda n: n.startswith(head)), ('gcn3 only', lambda n: n.startswith('gcn3.'))):
        for n, p in model.named_parameters():
            p.requires_grad_(pick(n))
        names = [n for n, _ in model.named_parameters() if pick(n)]
        assert names
        before = _stats()
        _, _, dx, grads = model.parameter_gradients(x, c)
        fwd, bwd, wg = _delta(before)
        assert fwd == dict(frames_hip=1, clip_hip=1, sample_hip=0, forward_tensor=0) and wg == ONE
        assert sorted(grads) == sorted(names) and torch.equal(dx, want_dx)
        err, name, floor = wu.compare(grads, dict(fix, keys=[k for k in fix['keys'] if pick(k)]), tag)
        print(f'parameter_gradients, {tag}: worst {err:.2e} ({name}, reference floor {floor:.1e})')
    for p in model.parameters():
        p.requires_grad_(True)
    # the switch and train(): the composition
    os.environ['AGCN_SGN_HIP'] = '0'
    try:
        fwd, _, wg = run(x)
        assert fwd == tensor and wg == zero
        before = _stats()
        _, _, _, grads = model.parameter_gradients(x, c)
        assert _delta(before)[0] == tensor and _delta(before)[2] == zero
        wu.compare(grads, fix, 'AGCN_SGN_HIP=0')
    finally:
        del os.environ['AGCN_SGN_HIP']
    assert ops.sgn_hip_enabled()
    model.train()
    fwd, _, wg = run(x)
    assert fwd == tensor and wg == zero
    with pytest.raises(ValueError):
        model.parameter_gradients(x, c)


def test_argument_errors():
    from agcn_amd import lib, ops
    L = lib.load()
    OK_ARG, WS = -1, -2
    model, x, c, _ = wu.build_model('v15_seg6', DEV)
    V, seg, nc = model.num_point, model.seg, model.num_class
    with torch.no_grad():
        wf, wc, wf_t, wc_t = model._finetune_images()
    feat, _ = ops.sgn_frames(x, wf, V)
    before = _stats()
    p = lib.ptr
    ft, ct = L.agcn_sgn_frames_tape_floats(1, seg, V), L.agcn_sgn_clip_tape_floats(1, seg, nc)
    wsb = L.agcn_sgn_wgrad_workspace(1, seg, V, nc, 0)
    assert ft == seg * V * 2656 and ct == ((seg + 2) * 256 + seg * 1024 + 512) and wsb > 0
    assert L.agcn_sgn_frames_tape_floats(1, seg, 33) == 0 and L.agcn_sgn_clip_tape_floats(1, seg, 0) == 0
    assert L.agcn_sgn_wgrad_workspace(1, seg, 33, nc, 0) == 0 and L.agcn_sgn_wgrad_workspace(1, seg, V, 0, 0) == 0
    assert L.agcn_sgn_wgrad_workspace(1, seg, V, nc, -1) == 0
    buf = torch.zeros(max(ft, ct, wsb // 4), device=DEV)
    dfeat, dx, d_wf, d_wc = torch.zeros_like(feat), torch.zeros_like(x), torch.zeros_like(wf), torch.zeros_like(wc)
    ws = torch.zeros(max(1, L.agcn_sgn_frames_bwd_workspace(1, seg, V) // 4), device=DEV)
    s = lib.stream()
    clip = lambda nclass, tape, floats: L.agcn_sgn_clip_bwd_tape(  # noqa: E731
        p(feat), p(wc), wc.numel(), p(wc_t), wc_t.numel(), p(c), p(dfeat), 1, seg, nclass, tape, floats, s)
    frames = lambda v, wsbytes, tape, floats: L.agcn_sgn_frames_bwd_tape(  # noqa: E731
        p(x), p(wf), wf.numel(), p(wf_t), wf_t.numel(), p(feat), p(dx), ws.data_ptr(), wsbytes, 1, seg, v, tape, floats, s)
    assert clip(nc, p(buf), ct - 1) == WS and clip(0, p(buf), ct) == OK_ARG and clip(nc, None, ct) == OK_ARG
    assert frames(V, ws.numel() * 4, p(buf), ft - 1) == WS and frames(V, ws.numel() * 4 - 4, p(buf), ft) == WS
    assert frames(33, ws.numel() * 4, p(buf), ft) == OK_ARG and frames(V, ws.numel() * 4, None, ft) == OK_ARG
    fw = lambda v, wsbytes, tape: L.agcn_sgn_frames_wgrad(p(x), p(wf), tape, p(d_wf), buf.data_ptr(), wsbytes, 1, seg, v, 0, s)  # noqa: E731
    cw = lambda nclass, wsbytes, tape: L.agcn_sgn_clip_wgrad(tape, p(feat), p(c), p(d_wc), buf.data_ptr(), wsbytes, 1, seg, nclass, 0, s)  # noqa: E731
    assert fw(V, wsb - 4, p(buf)) == WS and fw(33, wsb, p(buf)) == OK_ARG and fw(V, wsb, None) == OK_ARG
    assert cw(nc, wsb - 4, p(buf)) == WS and cw(0, wsb, p(buf)) == OK_ARG and cw(nc, wsb, None) == OK_ARG
    assert L.agcn_sgn_frames_wgrad(p(x), p(wf), p(buf), p(d_wf), buf.data_ptr(), wsb, 1, seg, V, -1, s) == OK_ARG
    # the wrappers raise before a launch
    with pytest.raises(ValueError):
        ops.sgn_frames_bwd_tape(torch.zeros(1, seg, 99, device=DEV), wf, wf_t, feat, 33)
    with pytest.raises(ValueError):
        ops.sgn_clip_bwd_tape(feat, wc, wc_t, torch.zeros(1, 0, device=DEV))
    with pytest.raises(ValueError):
        ops.sgn_frames_wgrad(x, wf, buf[:ft - 1], V, nc)
    with pytest.raises(ValueError):
        ops.sgn_clip_wgrad(buf[:ct - 1], feat, c, wc, V)
    with pytest.raises(ValueError):
        ops.sgn_frames_wgrad(x, wf, buf[:ft], V, nc, rows_per_split=-1)
    with pytest.raises(RuntimeError):
        lib.check(WS, "agcn_sgn_frames_wgrad")
    torch.cuda.synchronize()
    assert _delta(before)[2] == {k: 0 for k in ONE}
    assert float(dx.abs().max()) == 0 and float(d_wf.abs().max()) == 0 and float(d_wc.abs().max()) == 0      # nothing ran
