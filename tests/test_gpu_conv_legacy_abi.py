"""The agcn_conv_* entry points are argument checks in front of the agcn_tconv_* routes with pad = (taps-1)/2: on the same
inputs both names must launch the same kernels and write the same bits (y, the BatchNorm partials, dx plain and
accumulated with a masked addend, dw).  Straight through ctypes, one call per entry point.  ``-m gpu``."""
import pytest
import torch

pytestmark = pytest.mark.gpu

CASES = [
    # N, Cin, Cout, T, V, taps, stride
    (2, 64, 64, 11, 25, 9, 2),      # odd T: 6 + 5 output slots in the two backward passes
    (2, 64, 128, 9, 25, 9, 1),      # 128-row blocks
    (2, 3, 64, 7, 18, 1, 2),        # ragged K; the odd frames' pass is empty
    (2, 64, 64, 1, 25, 9, 2),       # T = 1: a single residue pass
]


@pytest.mark.parametrize('case', CASES)
def test_conv_entry_points_are_tconv_at_same_padding(case):
    import agcn_amd  # noqa: F401
    from agcn_amd import lib
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    dev = torch.device('cuda:0')
    L = lib.load()
    N, Cin, Cout, T, V, taps, stride = case
    pad = (taps - 1) // 2
    To = (T + 2 * pad - taps) // stride + 1
    g = torch.Generator().manual_seed(41 + T + taps)
    x = torch.randn(N, Cin, T, V, generator=g).to(dev)
    w = (torch.randn(Cout, Cin, taps, 1, generator=g) / (Cin * taps) ** 0.5).to(dev)
    b = (0.1 * torch.randn(Cout, generator=g)).to(dev)
    dy = torch.randn(N, Cout, To, V, generator=g).to(dev)
    base, add, mask = (torch.randn(N, Cin, T, V, generator=g).to(dev) for _ in range(3))
    p, st = lib.ptr, lib.stream()

    nb = L.agcn_tconv_workspace(Cin, Cout, T, V, taps, stride, pad)
    assert L.agcn_conv_workspace(Cin, Cout, T, V, taps, stride) == nb
    nt = L.agcn_tconv_stats_tiles(Cin, Cout, To, V, taps, stride, pad)
    assert nt > 0 and L.agcn_conv_stats_tiles(Cin, Cout, To, V, taps, stride) == nt
    nbw = L.agcn_tconv_bwd_weight_workspace(N, Cin, Cout, T, V, taps, stride, pad)
    assert L.agcn_conv_bwd_weight_workspace(N, Cin, Cout, T, V, taps, stride) == nbw
    ws = torch.empty((max(nb, nbw) + 3) // 4, device=dev)

    def kernel():
        torch.cuda.synchronize()
        return L.agcn_last_kernel().decode()

    def run(legacy):
        tail = (taps, stride) if legacy else (taps, stride, pad)
        y = torch.full((N, Cout, To, V), float('nan'), device=dev)
        stats = torch.full((N * nt, 2, Cout), float('nan'), device=dev)
        fwd = L.agcn_conv_fwd_ex if legacy else L.agcn_tconv_fwd
        lib.check(fwd(p(x), p(w), p(b), p(y), p(stats), ws.data_ptr(), nb, N, Cin, Cout, T, V, *tail, None, st), 'fwd')
        k_fwd = kernel()
        bwd = L.agcn_conv_bwd_data_ex if legacy else L.agcn_tconv_bwd_data
        dx = torch.full((N, Cin, T, V), float('nan'), device=dev)
        lib.check(bwd(p(dy), p(w), p(dx), 0, None, None, None, None, ws.data_ptr(), nb, N, Cin, Cout, T, V, *tail, None, st),
                  'bwd_data')
        k_bwd = kernel()
        dx2 = base.clone()
        lib.check(bwd(p(dy), p(w), p(dx2), 1, p(add), p(mask), None, None, ws.data_ptr(), nb, N, Cin, Cout, T, V, *tail,
                      None, st), 'bwd_data (accumulate)')
        assert kernel() == k_bwd
        wg = L.agcn_conv_bwd_weight_ex if legacy else L.agcn_tconv_bwd_weight
        dw = torch.full((Cout, Cin, taps, 1), float('nan'), device=dev)
        lib.check(wg(p(dy), p(x), p(dw), ws.data_ptr(), nbw, N, Cin, Cout, T, V, *tail, None, None, st), 'bwd_weight')
        torch.cuda.synchronize()
        return (y, stats, dx, dx2, dw), (k_fwd, k_bwd)

    old, k_old = run(True)
    new, k_new = run(False)
    assert k_old == k_new and all(k_old), (k_old, k_new)
    for name, a, c in zip(('y', 'stats', 'dx', 'dx accumulated', 'dw'), old, new):
        assert not torch.isnan(a).any(), name
        assert torch.equal(a, c), name
    # the accumulated form is the plain one plus what was there plus the addend where its mask passes
    ref = old[2].double() + base.double() + add.double() * (mask > 0)
    assert float((old[3].double() - ref).abs().max()) <= 1e-5 * max(1.0, float(ref.abs().max()))
