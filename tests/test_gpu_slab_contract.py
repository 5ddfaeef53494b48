"""The slab contract of the C boundary on the GPU: a launch writes exactly the slots its size query reports.  ``-m gpu``.

The caller allocates the partial-sum slabs (BatchNorm partials ``stats_part``, adjacency-gradient partials ``dadj_part``)
from a size query and hands the launcher a raw pointer; the kernel writes as many slots as ITS geometry says.  The queries
are dry runs of the launch ladders, so the two cannot disagree.  Through ctypes, with buffers of the test's own, per case:
the slab gets the queried slots plus three times as many guard slots, all filled with one NaN bit pattern; after the call
no queried slot holds the pattern (compared as int32), every guard slot does, and the slab's sums match fp64 tensor code
at the tolerance tests/test_gpu_tconv.py uses for partial sums (1e-3 of max(1, max|ref|); 0.2 in AGCN_GEMM=bf16).  In the
default mode the rung that ran is checked through agcn_last_kernel.  The shapes are the smallest that reach each rung of
the ladders; AGCN_GEMM is fixed per process, so one test runs this file again under f32 and bf16.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATTERN = 0x7FC0DEAD            # a quiet NaN no kernel produces
GUARD = 3


def _gpu():
    import agcn_amd  # noqa: F401
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device('cuda:0')


def _lib():
    from agcn_amd import lib
    return lib, lib.load()


def _tol(L):
    return (2e-2 if L.agcn_gemm_mode().decode() == 'bf16' else 1e-4) * 10


def rel(a, ref):
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    return float((a - ref).abs().max() / max(1.0, float(ref.abs().max())))


def rnd(gen, *shape, scale=1.0):
    return torch.randn(*shape, generator=gen, dtype=torch.float64) * scale


def _slab(slots, slot_floats, dev):
    """(1 + GUARD) * slots slots of slot_floats floats, every word the pattern."""
    return torch.full(((1 + GUARD) * slots, slot_floats), PATTERN, dtype=torch.int32, device=dev)


def _check_slab(slab, slots):
    """No queried slot keeps the pattern, every guard slot does; returns the queried part as fp32."""
    assert slots > 0
    torch.cuda.synchronize()
    assert not bool((slab[:slots] == PATTERN).any()), "a queried slot was not written"
    assert bool((slab[slots:] == PATTERN).all()), "the launch wrote past the queried slots"
    return slab[:slots].view(torch.float32)


def _ws(nbytes, dev):
    return torch.empty((int(nbytes) + 3) // 4, dtype=torch.float32, device=dev)


TCONV_CASES = [
    # Cin, Cout, T, V, taps, stride, pad, kernel of the default mode (prefix; None: not checked), slots per sample there
    # (ceil(T_out / frames per tile): 512 // 25 = 20 frames on the wide tile, 256 // 25 = 10 on every other)
    (64, 64, 24, 25, 9, 1, 4, 'conv_gemm_bf16_kernel<9, 2, 3, 2, 2, true>', 2),     # wide 512-position tile
    (64, 64, 48, 25, 9, 2, 4, 'conv_gemm_bf16_kernel<9, 2, 3, 2, 1, true>', 3),     # wide refused: the narrow tile
    (64, 128, 24, 25, 9, 1, 4, 'conv_pc_kernel<9', 3),                              # producer / consumer
    (64, 96, 24, 25, 9, 1, 4, 'conv_gemm_bf16_kernel<9, 2, 2, 2, 1, true>', 3),     # narrow
    (64, 64, 23, 25, 3, 1, 1, 'conv_gemm_bf16_kernel<3, 2, 3, 2, 2, true>', 2),     # wide, 3 taps
    (32, 48, 17, 25, 6, 4, 2, 'conv_gemm_kernel<6', 1),                             # exact-f32 kernel
    (64, 64, 20, 25, 1, 1, 0, None, 2),
]


@pytest.mark.parametrize('case', TCONV_CASES)
def test_tconv_fwd_writes_the_queried_stats_slots(case):
    dev = _gpu()
    lib, L = _lib()
    Cin, Cout, T, V, taps, stride, pad, kernel, per_sample = case
    N = 2
    g = torch.Generator().manual_seed(11 + taps + Cout)
    x = rnd(g, N, Cin, T, V)
    w = rnd(g, Cout, Cin, taps, 1, scale=1.0 / np.sqrt(Cin * taps))
    b = rnd(g, Cout, scale=0.1)
    y_ref = F.conv2d(x, w, b, stride=(stride, 1), padding=(pad, 0))
    T_out = y_ref.shape[2]
    xg, wg, bg = x.float().to(dev), w.float().to(dev).contiguous(), b.float().to(dev)
    slots = N * L.agcn_tconv_stats_tiles(Cin, Cout, T_out, V, taps, stride, pad)
    default = L.agcn_gemm_mode().decode() == 'bf16x6'
    if default and per_sample:
        assert slots == N * per_sample
    slab = _slab(slots, 2 * Cout, dev)
    y = torch.empty((N, Cout, T_out, V), dtype=torch.float32, device=dev)
    nb = L.agcn_tconv_workspace(Cin, Cout, T, V, taps, stride, pad)
    ws = _ws(nb, dev)
    lib.check(L.agcn_tconv_fwd(lib.ptr(xg), lib.ptr(wg), lib.ptr(bg), lib.ptr(y), slab.data_ptr(), ws.data_ptr(), nb, N,
                               Cin, Cout, T, V, taps, stride, pad, None, lib.stream()), 'agcn_tconv_fwd')
    part = _check_slab(slab, slots).reshape(slots, 2, Cout)
    if default and kernel:
        assert L.agcn_last_kernel().decode().startswith(kernel), L.agcn_last_kernel().decode()
    s = part.double().sum(0).cpu()
    assert rel(s[0], y_ref.sum((0, 2, 3))) < _tol(L)
    assert rel(s[1], (y_ref ** 2).sum((0, 2, 3))) < _tol(L)


GCN_CASES = [
    # N, C, Cout, T, V, kernel of the default mode (prefix)
    (2, 64, 64, 20, 25, 'gcn_ws_kernel<2, 2, 0>'),      # persistent kernel, 64 streamed channels
    (5, 64, 64, 20, 25, 'gcn_ws_kernel<2, 2, 0>'),      # (its slot count depends on N)
    (2, 128, 128, 20, 18, 'gcn_ws_kernel<2, 4, 0>'),    # persistent kernel, 128 streamed channels
    (5, 128, 128, 20, 18, 'gcn_ws_kernel<2, 4, 0>'),
    (2, 256, 256, 10, 25, 'gcn_chain_kernel'),          # tile-per-workgroup chain
    (2, 3, 64, 20, 25, 'conv_gemm_kernel'),             # first layer: exact-f32 kernel
]


def _gcn_operands(g, N, C, Cout, T, V):
    x = rnd(g, N, C, T, V)
    adj = rnd(g, N, 3, V, V, scale=1.0 / np.sqrt(V))
    wcat = rnd(g, Cout, 3 * C, scale=1.0 / np.sqrt(3 * C))
    return x, adj, wcat


@pytest.mark.parametrize('case', GCN_CASES)
def test_gcn_fwd_writes_the_queried_stats_slots(case):
    dev = _gpu()
    lib, L = _lib()
    N, C, Cout, T, V, kernel = case
    assert 'AGCN_WS_SPLIT' not in os.environ
    g = torch.Generator().manual_seed(5 + C + N)
    x, adj, wcat = _gcn_operands(g, N, C, Cout, T, V)
    b = rnd(g, Cout, scale=0.1)
    z = torch.einsum('nctu,niuv->nictv', x, adj)
    y_ref = torch.einsum('oic,nictv->notv', wcat.reshape(Cout, 3, C), z) + b.view(1, -1, 1, 1)
    xg, ag, wg, bg = (t.float().to(dev).contiguous() for t in (x, adj, wcat, b))
    slots = L.agcn_gcn_stats_slots(N, C, Cout, T, V)
    slab = _slab(slots, 2 * Cout, dev)
    y = torch.empty((N, Cout, T, V), dtype=torch.float32, device=dev)
    nb = L.agcn_gcn_workspace(C, Cout, T, V)
    ws = _ws(nb, dev)
    lib.check(L.agcn_gcn_aggregate_project_fwd_ex(lib.ptr(xg), lib.ptr(ag), lib.ptr(wg), lib.ptr(bg), lib.ptr(y),
                                                  slab.data_ptr(), ws.data_ptr(), nb, N, C, Cout, T, V, None,
                                                  lib.stream()), 'agcn_gcn_aggregate_project_fwd_ex')
    part = _check_slab(slab, slots).reshape(slots, 2, Cout)
    if L.agcn_gemm_mode().decode() == 'bf16x6':
        assert L.agcn_last_kernel().decode().startswith(kernel), L.agcn_last_kernel().decode()
    s = part.double().sum(0).cpu()
    assert rel(s[0], y_ref.sum((0, 2, 3))) < _tol(L)
    assert rel(s[1], (y_ref ** 2).sum((0, 2, 3))) < _tol(L)


@pytest.mark.parametrize('C,Cout', [(3, 64), (64, 64), (128, 128)])
def test_gcn_dadj_writes_the_queried_slots(C, Cout):
    dev = _gpu()
    lib, L = _lib()
    N, T, V = 2, 20, 25
    g = torch.Generator().manual_seed(3 + C)
    x, _, wcat = _gcn_operands(g, N, C, Cout, T, V)
    dy = rnd(g, N, Cout, T, V)
    h = torch.einsum('oic,notv->nictv', wcat.reshape(Cout, 3, C), dy)
    ref = torch.einsum('nctu,nictv->niuv', x, h)
    xg, wg, dyg = (t.float().to(dev).contiguous() for t in (x, wcat, dy))
    nslots = L.agcn_dadj_num_slots(C, V, T)
    slots = N * 3 * nslots
    slab = _slab(slots, V * V, dev)
    nb = L.agcn_gcn_workspace(C, Cout, T, V)
    ws = _ws(nb, dev)
    lib.check(L.agcn_gcn_dadj_ex(lib.ptr(dyg), lib.ptr(wg), lib.ptr(xg), slab.data_ptr(), ws.data_ptr(), nb, N, C, Cout,
                                 T, V, None, None, lib.stream()), 'agcn_gcn_dadj_ex')
    part = _check_slab(slab, slots).reshape(N, 3, nslots, V, V)
    assert rel(part.double().sum(2), ref) < _tol(L)


TAP_WGRAD_CASES = [
    # Cin, Cout, T, V, taps, stride, pad, kernel of the default mode (the smallest shape that reaches each instantiation class)
    (64, 64, 20, 25, 9, 1, 4, 'wgrad9_f16_kernel<2, 2, 1>'),
    (128, 128, 20, 25, 9, 2, 4, 'wgrad9_f16_kernel<4, 1, 2>'),
    (64, 64, 20, 18, 3, 1, 1, 'wgrad9_f16_kernel<2, 2, 1, 3, 3>'),
]
GUARD_BYTES = 4096


@pytest.mark.parametrize('case', TAP_WGRAD_CASES)
def test_tap_wgrad_writes_inside_the_queried_workspace(case):
    """The tap weight gradients keep their slabs, transposed copies and the two maxima they take themselves (no maxima
    are passed) inside the bytes agcn_tconv_bwd_weight_workspace reports: a guard behind them keeps its pattern."""
    dev = _gpu()
    lib, L = _lib()
    Cin, Cout, T, V, taps, stride, pad, kernel = case
    N = 2
    g = torch.Generator().manual_seed(17 + taps + stride + Cout)
    x = rnd(g, N, Cin, T, V)
    w = torch.zeros(Cout, Cin, taps, 1, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x, w, None, stride=(stride, 1), padding=(pad, 0))
    dy = rnd(g, *y.shape)
    y.backward(dy)
    dw_ref = w.grad.reshape(Cout, Cin, taps)
    xg, dyg = x.float().to(dev), dy.float().to(dev)
    nb = L.agcn_tconv_bwd_weight_workspace(N, Cin, Cout, T, V, taps, stride, pad)
    assert nb > 0
    words = (nb + 3) // 4
    ws = torch.full((words + GUARD_BYTES // 4,), PATTERN, dtype=torch.int32, device=dev)
    dw = torch.empty((Cout, Cin, taps), dtype=torch.float32, device=dev)
    lib.check(L.agcn_tconv_bwd_weight(lib.ptr(dyg), lib.ptr(xg), lib.ptr(dw), ws.data_ptr(), nb, N, Cin, Cout, T, V, taps,
                                      stride, pad, None, None, lib.stream()), 'agcn_tconv_bwd_weight')
    torch.cuda.synchronize()
    assert bool((ws[words:] == PATTERN).all()), "the launch wrote past the queried workspace"
    if L.agcn_gemm_mode().decode() == 'bf16x6':
        assert L.agcn_last_kernel().decode() == kernel, L.agcn_last_kernel().decode()
    err = rel(dw, dw_ref)
    print(f"tap wgrad {case[:7]}: rel err {err:.3e} (tol {_tol(L):.1e})")
    assert err < _tol(L)


@pytest.mark.parametrize('mode', ['f32', 'bf16'])
def test_slab_contract_other_gemm_modes_subprocess(mode):
    """The contract holds in every arithmetic mode: this file once more in a process with AGCN_GEMM=<mode>."""
    _gpu()
    r = subprocess.run([sys.executable, '-m', 'pytest', os.path.abspath(__file__), '-q', '-x', '-m', 'gpu',
                        '-p', 'no:cacheprovider', '-k', 'not other_gemm_modes'],
                       env=dict(os.environ, AGCN_GEMM=mode), cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert ' passed' in r.stdout and ' skipped' not in r.stdout, r.stdout[-2000:]
