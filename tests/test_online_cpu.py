"""CPU checks of the online-recognition path: the 15-joint OpenPose graph against the reference's (fixture), the
argument checks of ``agcn_skel_append`` / ``agcn_prenorm`` (on the host, before any launch: no GPU is touched) and the
``infer.inference`` shim.  The kernels themselves are tested on the GPU (tests/test_gpu_online.py)."""
import ctypes
import os

import numpy as np
import pytest

ERR_ARG = -1
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _lib():
    import agcn_amd  # noqa: F401
    from agcn_amd import lib
    return lib


def test_openpose_graph_equals_the_reference_bit_for_bit():
    import agcn_amd  # noqa: F401
    from agcn_amd.graph.openpose_b25_j15 import Graph
    import graph.openpose_b25_j15 as shim
    ref = np.load(os.path.join(GOLDEN, 'graph_openpose_b25_j15.npz'))['A']
    A = Graph(labeling_mode='spatial').A
    assert A.shape == (3, 15, 15) and A.dtype == ref.dtype
    assert np.array_equal(A, ref)
    assert shim.Graph is Graph and shim.num_node == 15 and len(shim.inward) == 14


def test_new_entry_points_are_exported_and_bound():
    lib = _lib()
    handle = ctypes.CDLL(lib.LIB_PATH)
    for name in ('agcn_skel_append', 'agcn_prenorm', 'agcn_prenorm_max_frames'):
        assert name in lib.SIGNATURES and hasattr(handle, name)
    assert lib.load().agcn_prenorm_max_frames() >= 300


def _prenorm(L, p, **kw):
    a = dict(inp=p, out=p, sel=p, energy=p, N=1, M=4, K=2, T=24, Tmax=24, origin=0, V=15, select=1, pad=1, center=1,
             z0=8, z1=1, x0=2, x1=5, zz0=-1, zz1=-1)
    a.update(kw)
    return L.agcn_prenorm(a['inp'], a['out'], a['sel'], a['energy'], a['N'], a['M'], a['K'], a['T'], a['Tmax'],
                          a['origin'], a['V'], a['select'], a['pad'], a['center'], a['z0'], a['z1'], a['x0'], a['x1'],
                          a['zz0'], a['zz1'], None)


@pytest.mark.parametrize('kw', [
    dict(inp=None), dict(out=None), dict(sel=None), dict(energy=None),      # null pointers
    dict(z1=15), dict(x0=15), dict(zz0=0, zz1=15), dict(z0=-1),            # an axis joint >= V, a half-given pair
    dict(V=33, z0=0, z1=1), dict(V=1, z0=0, z1=0, x0=0, x1=0),             # V > 32, V < 2
    dict(K=5), dict(K=0), dict(M=9, K=2),                                   # K > M, no body, more bodies than planned
    dict(T=0, Tmax=24), dict(T=25, Tmax=24), dict(origin=24), dict(origin=-1), dict(center=3), dict(N=0),
])
def test_prenorm_argument_errors(kw):
    L = _lib().load()
    buf = ctypes.create_string_buffer(64)        # host memory: never dereferenced, the checks come first
    assert _prenorm(L, ctypes.addressof(buf), **kw) == ERR_ARG


def test_prenorm_frames_above_the_lds_plan_are_an_argument_error():
    L = _lib().load()
    buf = ctypes.create_string_buffer(64)
    t = L.agcn_prenorm_max_frames() + 1
    assert _prenorm(L, ctypes.addressof(buf), T=t, Tmax=t) == ERR_ARG


@pytest.mark.parametrize('args', [
    (None, 1, 4, 24, 15, 0, 1, 1), (1, None, 4, 24, 15, 0, 1, 1),           # null pointers
    (1, 1, 4, 24, 33, 0, 1, 1), (1, 1, 0, 24, 15, 0, 1, 1),                # V > 32, no body
    (1, 1, 4, 24, 15, 24, 24, 1), (1, 1, 4, 24, 15, -1, 1, 1),             # slot outside the ring
    (1, 1, 4, 24, 15, 3, 2, 1),                                            # while filling the slot is count - 1
    (1, 1, 4, 24, 15, 0, 25, 1), (1, 1, 4, 24, 15, 0, 0, 1),               # count outside 1..Tmax
    (1, 1, 4, 24, 15, 0, 1, 0), (1, 1, 4, 24, 15, 0, 1, 25),               # moving average outside 1..Tmax
])
def test_skel_append_argument_errors(args):
    L = _lib().load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    frame, ring, *ints = args
    assert L.agcn_skel_append(p if frame else None, p if ring else None, *ints, None) == ERR_ARG


def test_infer_shim_resolves():
    import agcn_amd  # noqa: F401
    from agcn_amd.online import ActionRecognition
    from agcn_amd.processor import import_class
    import infer.inference
    assert infer.inference.ActionRecognition is ActionRecognition
    assert import_class('infer.inference.ActionRecognition') is ActionRecognition


def test_python_layer_rejects_cpu_tensors_and_bad_options():
    import torch
    import agcn_amd  # noqa: F401
    from agcn_amd import ops, preprocess
    x = torch.zeros(1, 3, 7, 15, 2)
    with pytest.raises(RuntimeError, match='GPU tensor'):
        preprocess.pre_normalization(x, zaxis=[8, 1], xaxis=[2, 5])
    with pytest.raises(RuntimeError, match='GPU tensor'):
        ops.skel_append(torch.zeros(4, 24, 15, 3), torch.zeros(4, 15, 3), 0, 1)
    with pytest.raises(ValueError):
        ops.prenorm(torch.zeros(1, 2, 7, 15, 3), center=True, center_firstframe=True)
    with pytest.raises(ValueError):
        ops.skel_append(torch.zeros(4, 24, 15, 3), torch.zeros(3, 15, 3), 0, 1)       # fewer bodies than the ring tracks
