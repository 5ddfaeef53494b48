"""unit_gcn's aggregate+project kernels and the two-kernel adjacency path across channel widths, against the fp64 reference of
tests/gcn_width_util.py (table, recipe, mutants and metric there; what makes the comparison able to fail is asserted in
tests/test_gcn_width_cpu.py).  GPU only (``-m gpu``).

Every call goes to the C entry through ``lib.status`` on outputs, slot slabs and workspaces of exactly the queried sizes
with sentinel floats behind them: every element must be written, no guard touched, and a refused call must write nothing.
Calls that take operand maxima run without them, with the true maxima and once more: bit-equal where the kernels promise
one arithmetic (forward, backward-data, adjacency gradient), and always bit-equal on the repeat.  The kernel each call
reached (``agcn_last_kernel``) must be the one gcn_width_util's model of the routing names for that width.

The bar is BAR = 1e-4 PER OUTPUT CHANNEL (row of dw, channel of y and dx, (sample, subset) of the adjacency gradient):
max |a - ref| over the channel / max(1, max |ref| over that channel).  Measured worst values: profiles/gcn_width.txt.

agcn_gcn_workspace answers for four operations at once and adds 256 bytes of slack, so its boundary is pinned as: with
257 bytes less than the query, the operation with the largest need (at least one of them) returns AGCN_ERR_WORKSPACE
and writes nothing, and no operation returns anything else than that or success."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import gcn_width_util as wu

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -7.5e30
GUARD = 64
N = wu.N
IDS = [wu.case_id(c) for c in wu.CASES]


def _gpu():
    import agcn_amd  # noqa: F401
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device('cuda:0')


def _mode():
    from agcn_amd import lib
    mode = lib.load().agcn_gemm_mode().decode()
    if mode not in ('bf16x6', 'f32'):
        pytest.skip('the routing model covers the default mode and AGCN_GEMM=f32')
    return mode == 'f32'


def _guarded(n, dev):
    buf = torch.full((n + GUARD,), SENTINEL, device=dev)
    return buf, buf[:n]


def _run(dev, name, outs, nb, args, expect=0, init=None, scratch=()):
    """One call of entry ``name``.  outs: {name: floats}; args(o, ws) -> the arguments in front of the stream; init:
    {name: tensor} copied into an output first (accumulate); scratch: outputs that need not be written everywhere.
    Returns (status, {name: copy of the output}, kernel name)."""
    from agcn_amd import lib
    bufs = {k: _guarded(n, dev) for k, n in outs.items()}
    for k, t in (init or {}).items():
        bufs[k][1].copy_(t.reshape(-1))
    nf = (nb + 3) // 4
    wsb, ws = _guarded(nf, dev)
    rc = lib.status(name, *args({k: v[1] for k, v in bufs.items()}, ws))
    torch.cuda.synchronize()
    assert rc == expect, (name, rc, expect)
    assert bool((wsb[nf:] == SENTINEL).all()), name + ': wrote behind the workspace'
    for k, (buf, view) in bufs.items():
        n = view.numel()
        assert bool((buf[n:] == SENTINEL).all()), '%s: wrote behind %s' % (name, k)
        if rc == 0 and k not in scratch:
            assert not bool((view == SENTINEL).any()), '%s: left elements of %s unwritten' % (name, k)
        if rc != 0 and k not in (init or {}):
            assert bool((view == SENTINEL).all()), '%s: refused, yet wrote into %s' % (name, k)
    if rc != 0:
        assert bool((wsb == SENTINEL).all()), name + ': refused, yet wrote into the workspace'
    return rc, {k: v[1].clone() for k, v in bufs.items()}, lib.load().agcn_last_kernel().decode()


def _pack(m):
    b = np.packbits((m.flatten() > 0).cpu().numpy(), bitorder='little')
    b = np.concatenate([b, np.zeros((-len(b)) % 4, np.uint8)])
    return torch.from_numpy(b.view(np.int32).copy()).to(m.device)


class _Report:
    def __init__(self, case):
        self.case, self.bad = wu.case_id(case), []

    def err(self, op, value, bar, kernel=''):
        print('\nGCNW %-14s %-12s %.2e  %s' % (self.case, op, value, kernel))
        if not value < bar:
            self.bad.append('%s: %.3e misses %.0e' % (op, value, bar))

    def route(self, op, kernel, want):
        if want is None or not kernel.startswith(want):
            self.bad.append('%s ran on %r, the table says %r' % (op, kernel, want))

    def same(self, what, a, b):
        if not all(torch.equal(a[k], b[k]) for k in a):
            self.bad.append(what + ': not the same bits')


@pytest.mark.parametrize('i', range(len(wu.CASES)), ids=IDS)
def test_width_case(i):
    from agcn_amd import lib, ops
    dev = _gpu()
    f32 = _mode()
    L = lib.load()
    case = wu.CASES[i]
    C, Cout, T, V = case
    p = wu.make(case, wu.SEEDS[i])
    ref = wu.reference(p)
    want = wu.routes_of(case, f32)
    d = {k: v.float().to(dev).contiguous() for k, v in p.items()}
    x, adj, w, bias, dy = d['x'], d['adj'], d['wcat'], d['bias'], d['dy']
    x_amax, dy_amax = x.abs().max().reshape(1), dy.abs().max().reshape(1)
    rep = _Report(case)
    dims = (N, C, Cout, T, V)
    nx, ny = x.numel(), dy.numel()
    nb = L.agcn_gcn_workspace(C, Cout, T, V)

    # ---- forward: y and the BatchNorm partials ----
    slots = L.agcn_gcn_stats_slots(*dims)
    assert slots > 0

    def fwd(amax, nbytes=nb, expect=0):
        return _run(dev, 'agcn_gcn_aggregate_project_fwd_ex', dict(y=ny, st=slots * 2 * Cout), nbytes,
                    lambda o, ws: (x, adj, w, bias, o['y'], o['st'], ws, nbytes) + dims + (amax,), expect)
    _, o0, k = fwd(None)
    rep.route('fwd', k, want['fwd'])
    rep.err('y', wu.channel_err(o0['y'], ref['y'], (1,)), wu.BAR, k)
    st = o0['st'].view(slots, 2, Cout).double().sum(0).cpu()
    rep.err('stats_sum', wu.tensor_err(st[0], ref['ssum']), wu.STATS_FACTOR * wu.BAR)
    rep.err('stats_sumsq', wu.tensor_err(st[1], ref['ssq']), wu.STATS_FACTOR * wu.BAR)
    _, o1, _ = fwd(x_amax)
    rep.same('fwd with max |x|', o0, o1)
    rep.same('fwd repeated', o1, fwd(x_amax)[1])

    # ---- backward-data: plain, accumulate + masked addends (float and bit masks), one addend, fused 1x1 term ----
    K2 = wu.fused_width(Cout)
    bits1, bits2 = _pack(d['mask1']), _pack(d['mask2'])      # (held here: the call takes their addresses)

    def bwd(amax, form, nbytes=nb, expect=0, bits=False, dtp_amax=None):
        a1 = d['add1'] if form in ('dx2', 'dx3') else None
        a2 = d['add2'] if form == 'dx2' else None
        m1, m2 = (d['mask1'], d['mask2']) if form == 'dx2' else (None, None)
        if bits:
            m1, m2 = lib.ptr_bits(bits1), lib.ptr_bits(bits2)
        else:
            m1, m2 = lib.ptr(m1), lib.ptr(m2)
        dtp, w2, k2 = (d['dtp'], d['wab'], K2) if form == 'dx5' else (None, None, 0)
        return _run(dev, 'agcn_gcn_aggregate_project_bwd_data_ex', dict(dx=nx), nbytes,
                    lambda o, ws: (dy, adj, w, dtp, w2, k2, o['dx'], int(form == 'dx2'), a1, m1, a2, m2, int(bits), ws,
                                   nbytes) + dims + (amax, dtp_amax),
                    expect, init=dict(dx=d['prior']) if form == 'dx2' else None)
    _, b0, k = bwd(None, 'dx')
    rep.route('bwd', k, want['bwd'])
    rep.err('dx', wu.channel_err(b0['dx'], ref['dx'], (1,)), wu.BAR, k)
    _, b1, _ = bwd(dy_amax, 'dx')
    rep.same('bwd with max |dy|', b0, b1)
    rep.same('bwd repeated', b1, bwd(dy_amax, 'dx')[1])
    _, b2, k = bwd(None, 'dx2')
    rep.err('dx_addends', wu.channel_err(b2['dx'], ref['dx2'], (1,)), wu.BAR, k)
    rep.same('bwd addends with max |dy|', b2, bwd(dy_amax, 'dx2')[1])
    rep.same('bwd addends, bit masks', b2, bwd(None, 'dx2', bits=True)[1])
    _, b3, k = bwd(None, 'dx3')
    rep.err('dx_one_addend', wu.channel_err(b3['dx'], ref['dx3'], (1,)), wu.BAR, k)
    rep.same('bwd one addend repeated', b3, bwd(None, 'dx3')[1])
    if K2 > 0:
        assert ops.fused_bwd_data_supported(C, Cout, V) == (want['fused'] is not None)
        if want['fused'] is None:                      # refused: nothing written
            bwd(None, 'dx5', expect=lib.ERR_UNSUPPORTED)
        else:
            _, b5, k = bwd(None, 'dx5')
            rep.route('fused', k, want['fused'])
            rep.err('dx_fused', wu.channel_err(b5['dx'], ref['dx5'], (1,)), wu.BAR, k)
            am = d['dtp'].abs().max().reshape(1)
            _, b6, _ = bwd(dy_amax, 'dx5', dtp_amax=am)
            rep.same('fused with the maxima', b5, b6)
            rep.same('fused repeated', b6, bwd(dy_amax, 'dx5', dtp_amax=am)[1])

    # ---- weight gradient (with both maxima: f16x3, another arithmetic) ----
    nbw = L.agcn_gcn_project_bwd_weight_workspace(*dims)

    def wgrad(amax, nbytes=nbw, expect=0):
        return _run(dev, 'agcn_gcn_project_bwd_weight_ex', dict(dw=3 * C * Cout), nbytes,
                    lambda o, ws: (dy, x, adj, o['dw'], ws, nbytes) + dims + ((dy_amax, x_amax) if amax else (None, None)),
                    expect)
    _, w0, k = wgrad(False)
    rep.route('wgrad', k, want['wgrad'])
    rep.err('dw', wu.channel_err(w0['dw'], ref['dw'], (0,)), wu.BAR, k)
    _, w1, k = wgrad(True)
    rep.route('wgrad with the maxima', k, want['wgrad'])
    rep.err('dw_maxima', wu.channel_err(w1['dw'], ref['dw'], (0,)), wu.BAR, k)
    rep.same('wgrad repeated', w1, wgrad(True)[1])
    rep.same('wgrad without the maxima repeated', w0, wgrad(False)[1])
    assert nbw > 0
    short = [lib.status('agcn_gcn_project_bwd_weight_ex', dy, x, adj, torch.empty(3 * C * Cout, device=dev),
                        torch.empty((nbw + 3) // 4, device=dev), nbw - 1, *dims, *m)
             for m in ((None, None), (dy_amax, x_amax))]
    assert lib.ERR_WORKSPACE in short and set(short) <= {0, lib.ERR_WORKSPACE}, short

    # ---- adjacency gradient: the slot partials, or the refusal ----
    nslots = L.agcn_dadj_num_slots(C, V, T)

    def dadj(amax, slots_=nslots, nbytes=nb, expect=0):
        return _run(dev, 'agcn_gcn_dadj_ex', dict(dp=N * 3 * slots_ * V * V), nbytes,
                    lambda o, ws: (dy, w, x, o['dp'], ws, nbytes) + dims + ((dy_amax, x_amax) if amax else (None, None)),
                    expect)
    if want['dadj'] is None:
        assert nslots == 0
        dadj(False, slots_=1, expect=lib.ERR_UNSUPPORTED)
        with pytest.raises(ValueError, match=r'does not support %d input channels.*below 64 and multiples of 64' % C):
            ops.adjacency_bwd(dy, w, x, torch.zeros(N, 6, T, V, device=dev), torch.zeros(N, 3, V, V, device=dev))
    else:
        assert nslots > 0
        _, a0, k = dadj(False)
        rep.route('dadj', k, want['dadj'])
        rep.err('dadj', wu.channel_err(a0['dp'].view(N, 3, nslots, V, V).double().sum(2), ref['dadj'], (0, 1)), wu.BAR, k)
        _, a1, _ = dadj(True)
        rep.same('dadj with the maxima', a0, a1)
        rep.same('dadj repeated', a1, dadj(True)[1])

    # ---- the shared workspace query's boundary (see the module docstring) ----
    need = nb - 256
    if need > 0:
        codes = [lib.status('agcn_gcn_aggregate_project_fwd_ex', x, adj, w, bias, torch.empty_like(dy), None,
                            torch.empty((nb + 3) // 4, device=dev), need - 1, *dims, None)]
        codes.append(lib.status('agcn_gcn_aggregate_project_bwd_data_ex', dy, adj, w, None, None, 0, torch.empty_like(x), 0,
                                None, None, None, None, 0, torch.empty((nb + 3) // 4, device=dev), need - 1, *dims, None,
                                None))
        if K2 > 0 and want['fused'] is not None:
            codes.append(lib.status('agcn_gcn_aggregate_project_bwd_data_ex', dy, adj, w, d['dtp'], d['wab'], K2,
                                    torch.empty_like(x), 0, None, None, None, None, 0,
                                    torch.empty((nb + 3) // 4, device=dev), need - 1, *dims, None, None))
        if want['dadj'] is not None:
            codes.append(lib.status('agcn_gcn_dadj_ex', dy, w, x, torch.empty(N * 3 * nslots * V * V, device=dev),
                                    torch.empty((nb + 3) // 4, device=dev), need - 1, *dims, None, None))
        torch.cuda.synchronize()
        assert lib.ERR_WORKSPACE in codes and set(codes) <= {0, lib.ERR_WORKSPACE}, codes
        # the refused call writes nothing: once more on guarded buffers, for the forward or the backward-data
        if codes[0] == lib.ERR_WORKSPACE:
            fwd(None, nbytes=need - 1, expect=lib.ERR_WORKSPACE)
        if codes[1] == lib.ERR_WORKSPACE:
            bwd(None, 'dx', nbytes=need - 1, expect=lib.ERR_WORKSPACE)
    else:
        fwd(None, nbytes=0)

    # ---- folded inference: act(y [+ res] [+ w2 . x2]) ----
    for res, x2, relu in ((False, False, False), (True, False, True), (False, True, True), (True, True, False)):
        k2 = wu.X2_WIDTH if x2 else 0
        nbi = L.agcn_gcn_unit_infer_workspace(C, Cout, k2, T, V)
        key = 'infer_x2' if x2 else 'infer'

        def infer(nbytes=nbi, expect=0):
            return _run(dev, 'agcn_gcn_unit_infer', dict(y=ny), nbytes,
                        lambda o, ws: (x, adj, w, bias, d['res'] if res else None, d['x2'] if x2 else None,
                                       d['w2'] if x2 else None, k2, int(relu), o['y'], ws, nbytes) + dims, expect)
        if want[key] is None:
            infer(expect=lib.ERR_UNSUPPORTED)
            continue
        _, y0, k = infer()
        rep.route(key, k, want[key])
        tag = 'infer' + ('+res' if res else '') + ('+x2' if x2 else '') + ('+relu' if relu else '')
        rep.err(tag, wu.channel_err(y0['y'], wu.infer_reference(p, ref['y'], res, x2, relu), (1,)), wu.BAR, k)
        rep.same(tag + ' repeated', y0, infer()[1])
        if nbi > 257:
            infer(nbytes=nbi - 257, expect=lib.ERR_WORKSPACE)
    assert not rep.bad, '\n'.join(rep.bad)


@pytest.mark.parametrize('i', range(len(wu.ADJ_CASES)), ids=[wu.case_id(c) for c in wu.ADJ_CASES])
def test_adjacency_two_kernel_path(i):
    """agcn_adjacency_fwd, agcn_adjacency_bwd_softmax and agcn_adjacency_bwd_scores at Ci outside {16, 32, 64}, V = 15 (below
    the fused kernel's V >= 16: such a model always takes this path) among the cases"""
    from agcn_amd import lib, ops
    dev = _gpu()
    L = lib.load()
    case = wu.ADJ_CASES[i]
    Ci, T, V = case
    p = wu.make_adj(case, wu.ADJ_SEEDS[i])
    ref = wu.adj_reference(p)
    tp, A, PA = (p[k].float().to(dev).contiguous() for k in ('tp', 'A', 'PA'))
    rep = _Report(case)
    assert not ops.adjacency_fused_supported(64, Ci, T, V)
    nt = L.agcn_scores_num_tiles(V, T)
    VV = V * V

    def fwd():
        return _run(dev, 'agcn_adjacency_fwd', dict(sp=N * 3 * nt * VV, P=N * 3 * VV, adj=N * 3 * VV), 0,
                    lambda o, ws: (tp, A, PA, None, o['sp'], o['P'], o['adj'], N, Ci, T, V))
    _, f0, _ = fwd()
    rep.err('P', wu.channel_err(f0['P'], ref['P'], (0, 1)), wu.BAR)
    rep.err('adj', wu.channel_err(f0['adj'], ref['adj'], (0, 1)), wu.BAR)
    rep.same('adjacency_fwd repeated', f0, fwd()[1])
    # backward from the reference's P (rounded to fp32) and a one-slot partial slab holding the seeded dadj
    P32 = ref['P'].float().to(dev).contiguous()
    dpart = p['dadj'].float().to(dev).contiguous()

    def soft():
        return _run(dev, 'agcn_adjacency_bwd_softmax', dict(dadj=N * 3 * VV, dS=N * 3 * VV, dPA=3 * VV), 0,
                    lambda o, ws: (dpart, P32, None, o['dadj'], o['dS'], o['dPA'], None, N, Ci, T, V, 1))
    _, s0, _ = soft()
    rep.err('dPA', wu.channel_err(s0['dPA'], ref['dPA'], (0,)), wu.BAR)
    rep.same('bwd_softmax repeated', s0, soft()[1])
    dS = s0['dS'].contiguous()
    scratch = ops._scratch(6 * Ci, tp)

    def scores():
        return _run(dev, 'agcn_adjacency_bwd_scores', dict(dtp=tp.numel(), dbp=N * nt * 6 * Ci, db=6 * Ci), 0,
                    lambda o, ws: (tp, dS, o['dtp'], o['dbp'], scratch, o['db'], N, Ci, T, V), scratch=('dbp',))
    _, g0, _ = scores()
    gmax = float(ref['dtp'].abs().max())
    rep.err('dtp', float((g0['dtp'].double().cpu().view_as(ref['dtp']) - ref['dtp']).abs().max()) / gmax, wu.DTP_BAR)
    bmax = float(ref['db'].abs().max())
    rep.err('db', float((g0['db'].double().cpu() - ref['db']).abs().max()) / bmax, wu.DB_BAR)
    rep.same('bwd_scores repeated', g0, scores()[1])
    assert not rep.bad, '\n'.join(rep.bad)


def test_width_cases_on_the_exact_kernels_subprocess():
    """AGCN_GEMM is read once per process: six cases of the table (C < 32, 33..64, 65..128 and > 128 among them) once more
    in a fresh process under AGCN_GEMM=f32, where every width takes the exact kernels.  The same bar."""
    _gpu()
    if _mode():
        pytest.skip('already the exact-f32 mode')
    ids = ' or '.join(IDS[i] for i in wu.F32_SUBSET)
    r = subprocess.run([sys.executable, '-m', 'pytest', os.path.join(ROOT, 'tests', 'test_gpu_gcn_width.py'), '-q', '-s',
                        '-m', 'gpu', '-p', 'no:cacheprovider', '-k', 'test_width_case and (%s)' % ids],
                       env=dict(os.environ, AGCN_GEMM='f32'), cwd=ROOT, capture_output=True, text=True, timeout=600)
    print('\n'.join('GCNW-f32' + ln.split('GCNW', 1)[1] for ln in r.stdout.splitlines() if 'GCNW' in ln))
    assert r.returncode == 0, r.stdout[-6000:] + r.stderr[-2000:]
    assert '6 passed' in r.stdout and ' skipped' not in r.stdout, r.stdout[-2000:]
