"""lib.call on the GPU: it reaches the library with the same addresses and stream as a direct ctypes call, and refuses
a tensor of the wrong element type or layout on the host, before anything is launched.  (int32 draws and row counts, the
int64 index, the float64 carry and the uint8 masks travel through lib.call in the ops-level tests.)"""
import pytest
import torch

import agcn_amd  # noqa: F401
from agcn_amd import lib

pytestmark = pytest.mark.gpu


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def test_call_writes_the_bits_of_the_direct_ctypes_call():
    dev = _gpu()
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(1024, generator=g) * 37.0).to(dev)
    direct, checked = torch.full((1,), -1.0, device=dev), torch.full((1,), -2.0, device=dev)
    assert lib.load().agcn_absmax(lib.ptr(x), 1024, lib.ptr(direct), lib.stream()) == 0
    lib.call("agcn_absmax", x, 1024, checked)
    assert lib.status("agcn_absmax", x, 1024, checked) == 0
    torch.cuda.synchronize()
    assert torch.equal(direct.view(torch.int32), checked.view(torch.int32))
    assert float(checked) == float(x.abs().max())


def test_wrong_element_type_or_layout_is_refused_before_the_launch():
    dev = _gpu()
    out = torch.full((1,), -3.0, device=dev)
    x64 = torch.ones(1024, dtype=torch.float64, device=dev)
    with pytest.raises(RuntimeError, match=r'agcn_absmax\(x\).*fp32 GPU tensor'):
        lib.call("agcn_absmax", x64, 1024, out)
    strided = torch.ones(2048, device=dev)[::2]                     # a non-contiguous view
    with pytest.raises(RuntimeError, match=r'agcn_absmax\(x\).*GPU tensor'):
        lib.call("agcn_absmax", strided, 1024, out)
    # the int64 sample index of the SGN collate, handed an fp32 tensor; every other argument is valid
    N, S, seg, T, V, P = 2, 1, 4, 6, 5, 3
    pool = torch.ones(P, 3, T, V, 2, device=dev)
    r = torch.zeros(N, S, seg, dtype=torch.int32, device=dev)
    clips = torch.full((N, S, seg, V * 3), -3.0, device=dev)
    L = torch.full((N,), -3, dtype=torch.int32, device=dev)
    index = torch.zeros(N, device=dev)
    with pytest.raises(RuntimeError, match=r'agcn_sgn_collate\(index\).*int64 GPU tensor'):
        lib.call("agcn_sgn_collate", pool, index, r, None, clips, None, L, P, N, T, V, 2, S, seg)
    torch.cuda.synchronize()
    assert float(out) == -3.0 and bool((clips == -3.0).all()) and bool((L == -3).all())     # nothing was launched
