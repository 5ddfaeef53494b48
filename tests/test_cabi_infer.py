"""CPU checks of the folded-inference boundary: ``agcn_tconv_infer`` is exported and bound, rejects bad arguments and
shapes outside its domain on the host (nothing is launched, no GPU is touched), and the BatchNorm folding arithmetic
behind ``ops.unit_infer`` / ``ops.tcn_infer`` equals ``nn.BatchNorm2d.eval()`` for a plain and a GhostBatchNorm
module.  The kernels themselves are tested on the GPU (tests/test_gpu_infer_aagcn.py)."""
import ctypes

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

ERR_ARG, ERR_UNSUPPORTED = -1, -3


def _lib():
    import agcn_amd  # noqa: F401
    from agcn_amd import lib
    return lib


def test_tconv_infer_is_exported_and_bound():
    lib = _lib()
    assert 'agcn_tconv_infer' in lib.SIGNATURES
    handle = ctypes.CDLL(lib.LIB_PATH)
    assert hasattr(handle, 'agcn_tconv_infer')
    assert lib.load().agcn_tconv_infer.argtypes == lib.SIGNATURES['agcn_tconv_infer'][1]


def _call(L, x, w, y, ws, ws_bytes, N=2, Cin=64, Cout=64, T=30, V=25, taps=9, stride=1, pad=4):
    return L.agcn_tconv_infer(x, w, None, None, None, None, None, 1, y, ws, ws_bytes, N, Cin, Cout, T, V, taps, stride, pad,
                              None, None)


def test_null_pointers_and_bad_sizes_are_argument_errors():
    L = _lib().load()
    buf = ctypes.create_string_buffer(64)        # host memory: never dereferenced, the checks come first
    p = ctypes.addressof(buf)
    assert _call(L, None, p, p, p, 1 << 30) == ERR_ARG
    assert _call(L, p, None, p, p, 1 << 30) == ERR_ARG
    assert _call(L, p, p, None, p, 1 << 30) == ERR_ARG
    assert _call(L, p, p, p, None, 1 << 30) == ERR_ARG
    assert _call(L, p, p, p, p, 1 << 30, N=0) == ERR_ARG
    assert _call(L, p, p, p, p, 1 << 30, V=33) == ERR_ARG


@pytest.mark.parametrize('kw', [dict(taps=10, pad=4), dict(stride=10), dict(taps=5, pad=3), dict(taps=1, pad=1),
                                dict(taps=0, pad=0), dict(stride=0), dict(pad=-1), dict(taps=9, pad=0, T=8)])
def test_outside_the_domain_is_unsupported_without_a_launch(kw):
    L = _lib().load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    assert _call(L, p, p, p, p, 1 << 30, **kw) == ERR_UNSUPPORTED


def _random_bn_stats(bn, gen):
    with torch.no_grad():
        bn.weight.copy_(torch.rand(bn.weight.shape, generator=gen) + 0.5)
        bn.bias.copy_(torch.randn(bn.bias.shape, generator=gen))
        bn.running_mean.copy_(torch.randn(bn.running_mean.shape, generator=gen))
        bn.running_var.copy_(torch.rand(bn.running_var.shape, generator=gen) + 0.25)


@pytest.mark.parametrize('ghost', [False, True])
def test_fold_equals_eval_batchnorm(ghost):
    _lib()
    from agcn_amd import ops
    from agcn_amd.model.agcn import _bn_args
    from agcn_amd.model.ghostbatchnorm import GhostBatchNorm2d
    gen = torch.Generator().manual_seed(3 + int(ghost))
    cin, cout, k = 6, 10, 3
    conv = nn.Conv2d(cin, cout, (k, 1), padding=(1, 0), stride=(2, 1)).double()
    bn = (GhostBatchNorm2d(cout, 2) if ghost else nn.BatchNorm2d(cout)).double()
    _random_bn_stats(bn, gen)
    bn.train()
    bn.eval()                                    # GhostBatchNorm collates its 2*cout running statistics here
    before = [t.clone() for t in _bn_args(bn)]
    if ghost:
        assert bn.running_mean.numel() == 2 * cout
        assert torch.equal(bn.running_mean[:cout], bn.running_mean[cout:])
    x = torch.randn(4, cin, 11, 5, generator=gen, dtype=torch.float64)
    with torch.no_grad():
        ref = bn(conv(x))
        s, sh = ops._fold(_bn_args(bn))
        assert s.shape == (cout,) and sh.shape == (cout,)
        assert torch.allclose(conv(x) * s[None, :, None, None] + sh[None, :, None, None], ref, rtol=0, atol=1e-12)
        wf, bf = ops._fold_conv(conv.weight, conv.bias, _bn_args(bn))
        got = F.conv2d(x, wf, bf, stride=(2, 1), padding=(1, 0))
    assert float((got - ref).abs().max()) < 1e-12
    for a, b in zip(before, _bn_args(bn)):       # folding reads, never writes
        assert torch.equal(a, b)


@pytest.mark.parametrize('ghost', [False, True])
def test_fold_unit_equals_eval_unit(ghost):
    """``ops._fold_unit`` of a unit with a conv `down` and a stride-2 convolutional residual, in fp64 on the CPU: the
    folded unit_gcn equals bn(sum_i conv_d_i(x . adj_i)) + down_bn(down(x)) of the eval-mode modules, the temporal and
    residual pairs are ``_fold_conv`` of the same inputs, and nothing it reads is written."""
    _lib()
    from agcn_amd import ops
    from agcn_amd.model.agcn import _bn_args, unit_params
    from agcn_amd.model.aagcn import TCNGCNUnit
    gen = torch.Generator().manual_seed(11 + int(ghost))
    N, C, Cout, T, V = 2, 6, 10, 5, 4
    A = torch.rand(3, V, V, generator=gen).numpy()
    unit = TCNGCNUnit(C, Cout, A, stride=2, gbn_split=2 if ghost else None).double()
    gcn, tcn, res = unit.gcn1, unit.tcn1, unit.residual
    bns = (gcn.bn, gcn.down[1], tcn.bn, res.bn)
    with torch.no_grad():
        for conv in (*gcn.conv_d, gcn.down[0], tcn.conv, res.conv):
            conv.bias.copy_(torch.randn(conv.bias.shape, generator=gen))
    for bn in bns:
        _random_bn_stats(bn, gen)
    unit.train()
    unit.eval()                                  # GhostBatchNorm collates its 2*Cout running statistics here
    if ghost:
        assert all(bn.running_mean.numel() == 2 * Cout for bn in bns)
    p = unit_params(unit, gcn.params(), gcn.attn_params())
    assert p['down'] is not None and p['res'] is not None and p['res_mode'] == 2 and p['stride'] == 2
    srcs = [t for wb in p['conv_d'] for t in wb] + [t for q in p['ab'] for t in q]
    srcs += [*p['gbn'], *p['down'], p['tw'], p['tb'], *p['tbn'], *p['res']]
    before = [t.clone() for t in srcs]
    x = torch.randn(N, C, T, V, generator=gen, dtype=torch.float64)
    adj = torch.randn(N, 3, V, V, generator=gen, dtype=torch.float64)
    with torch.no_grad():
        wdf, bias, w2, twf, tbf, rwf, rbf, wab, bab = ops._fold_unit(p)
        xa = [torch.einsum('nctu,nuv->nctv', x, adj[:, i]) for i in range(3)]
        ref = gcn.bn(sum(gcn.conv_d[i](xa[i]) for i in range(3))) + gcn.down(x)
        got = bias.view(1, -1, 1, 1) + torch.einsum('ok,nktv->notv', wdf, torch.cat(xa, 1)) \
            + torch.einsum('oc,nctv->notv', w2, x)
        assert float((got - ref).abs().max()) < 1e-12
        for (wf, bf), (conv, bn) in (((twf, tbf), (tcn.conv, tcn.bn)), ((rwf, rbf), (res.conv, res.bn))):
            we, be = ops._fold_conv(conv.weight, conv.bias, _bn_args(bn))
            assert torch.equal(wf, we) and torch.equal(bf, be)
    assert wab.shape == (6 * (Cout // 4), C, 1, 1) and bab.shape == (6 * (Cout // 4),)
    for a, b in zip(before, srcs):               # folding reads, never writes
        assert torch.equal(a, b)
