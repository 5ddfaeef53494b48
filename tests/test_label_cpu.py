"""CPU checks of recording labelling and multi-stream recognition: the window plan against a plain sliding-window
emulation, the recording readers of tools/label_recording.py, the argument checks of ``agcn_prenorm_windows`` /
``agcn_skel_smooth`` / ``agcn_skel_append_many`` (on the host, before any launch: no GPU is touched) and the shape checks
of their Python wrappers.  The kernels themselves are tested on the GPU (tests/test_gpu_label.py)."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

ERR_ARG = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    import agcn_amd  # noqa: F401
    from agcn_amd import lib
    return lib


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, 'tools', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- window_plan -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('L', [40, 24, 9])                   # above, equal to and below the window
@pytest.mark.parametrize('interval', [1, 3, 7])
def test_window_plan_against_a_sliding_window(L, interval):
    import agcn_amd  # noqa: F401
    from agcn_amd.online import window_plan
    T = 24
    ends = list(range(0, L, interval))
    start, length = window_plan(L, T, ends)
    assert start.dtype == length.dtype == np.int32 and start.shape == length.shape == (len(ends),)
    window, at = [], {}
    for f in range(L):                                       # the frames a window of T holds after appending frame f
        window.append(f)
        if len(window) > T:
            window.pop(0)
        at[f] = list(window)
    for s, n, e in zip(start, length, ends):
        assert list(range(s, s + n)) == at[e], e


def test_window_plan_takes_any_order_and_rejects_frames_outside():
    import torch
    import agcn_amd  # noqa: F401
    from agcn_amd.online import window_plan, window_plan_device
    start, length = window_plan(100, 30, [99, 0, 29, 30, 99])
    assert start.tolist() == [70, 0, 0, 1, 70] and length.tolist() == [30, 1, 30, 30, 30]
    for bad in ([100], [-1], [3, 100]):
        with pytest.raises(ValueError):
            window_plan(100, 30, bad)
    # the variant that builds the plan with tensor ops (here on the CPU) agrees
    for interval, first in ((1, 0), (7, 3)):
        s, n, e = window_plan_device(100, 30, torch.device('cpu'), interval, first)
        ws, wn = window_plan(100, 30, e.tolist())
        assert e.tolist() == list(range(first, 100, interval)) and s.dtype == n.dtype == torch.int32
        assert s.tolist() == ws.tolist() and n.tolist() == wn.tolist()
    with pytest.raises(ValueError):
        window_plan_device(100, 30, torch.device('cpu'), 0)


# ---- the recording readers -------------------------------------------------------------------------------------------------
def test_directory_reader(tmp_path):
    tool = _tool('label_recording')
    rng = np.random.default_rng(0)
    v, tracked = 5, 3
    rows = {
        'frame_010.txt': rng.standard_normal((2, 3 * v)),           # fewer bodies than tracked
        'frame_002.txt': rng.standard_normal((5, 3 * v)),           # more bodies than tracked
        'frame_001.txt': rng.standard_normal((3, 3 * (v + 2))),     # more joints than the model takes
    }
    for name, a in rows.items():
        np.savetxt(tmp_path / name, a, delimiter=',')
    (tmp_path / 'frame_003.txt').write_text('1.5,2.5,3.5,4.5\n\n')  # a short row, then an empty line
    (tmp_path / 'frame_004.txt').write_text('')                      # nobody in the frame
    rec = tool.read_directory(str(tmp_path), tracked, v)
    assert rec.shape == (5, tracked, v, 3) and rec.dtype == np.float32      # sorted by name: 001, 002, 003, 004, 010
    assert np.array_equal(rec[0], rows['frame_001.txt'][:, :3 * v].reshape(3, v, 3).astype(np.float32))
    assert np.array_equal(rec[1], rows['frame_002.txt'][:3].reshape(3, v, 3).astype(np.float32))
    assert rec[2, 0].reshape(-1)[:4].tolist() == [1.5, 2.5, 3.5, 4.5] and not rec[2].reshape(-1)[4:].any()
    assert not rec[3].any()
    assert np.array_equal(rec[4, :2], rows['frame_010.txt'].reshape(2, v, 3).astype(np.float32)) and not rec[4, 2].any()


def test_npy_reader_and_csv(tmp_path):
    tool = _tool('label_recording')
    a = np.random.default_rng(1).standard_normal((6, 2, 7, 3)).astype(np.float32)
    np.save(tmp_path / 'rec.npy', a)
    rec = tool.read_recording(str(tmp_path / 'rec.npy'), 4, 5)             # bodies padded, joints dropped
    assert rec.shape == (6, 4, 5, 3) and np.array_equal(rec[:, :2], a[:, :, :5]) and not rec[:, 2:].any()
    with pytest.raises(SystemExit):
        np.save(tmp_path / 'bad.npy', a[..., :2])
        tool.read_recording(str(tmp_path / 'bad.npy'), 4, 5)
    out = tmp_path / 'labels.csv'
    scores = np.array([[0.1, 0.9], [0.75, 0.25]], dtype=np.float32)
    tool.write_csv(str(out), np.array([4, 9]), np.array([1, 0]), scores)
    assert out.read_text().splitlines() == ['frame,label,score', '4,1,0.900000', '9,0,0.750000']


# ---- argument errors of the C entry points ---------------------------------------------------------------------------------
def test_entry_points_are_exported_and_bound():
    lib = _lib()
    handle = ctypes.CDLL(lib.LIB_PATH)
    for name in ('agcn_prenorm_windows', 'agcn_skel_smooth', 'agcn_skel_append_many'):
        assert name in lib.SIGNATURES and hasattr(handle, name)


def _windows(L, p, **kw):
    a = dict(inp=p, out=p, sel=p, energy=p, block=p, start=p, len=p, N=2, nblocks=1, M=4, K=2, T=24, Tmax=29, V=15,
             select=1, pad=1, center=1, z0=8, z1=1, x0=2, x1=5, zz0=-1, zz1=-1)
    a.update(kw)
    return L.agcn_prenorm_windows(a['inp'], a['out'], a['sel'], a['energy'], a['block'], a['start'], a['len'], a['N'],
                                  a['nblocks'], a['M'], a['K'], a['T'], a['Tmax'], a['V'], a['select'], a['pad'],
                                  a['center'], a['z0'], a['z1'], a['x0'], a['x1'], a['zz0'], a['zz1'], None)


@pytest.mark.parametrize('kw', [
    dict(inp=None), dict(out=None), dict(sel=None), dict(energy=None), dict(start=None), dict(len=None),
    dict(z1=15), dict(x0=15), dict(zz0=0, zz1=15), dict(z0=-1),            # an axis joint >= V, a half-given pair
    dict(V=33, z0=0, z1=1), dict(V=1, z0=0, z1=0, x0=0, x1=0),             # V > 32, V < 2
    dict(K=5), dict(K=0), dict(M=9, K=2),                                   # K > M, no body, more bodies than planned
    dict(T=0), dict(T=30), dict(T=2049, Tmax=4096), dict(center=3), dict(N=0), dict(nblocks=0),
])
def test_prenorm_windows_argument_errors(kw):
    L = _lib().load()
    buf = ctypes.create_string_buffer(64)        # host memory: never dereferenced, the checks come first
    assert _windows(L, ctypes.addressof(buf), **kw) == ERR_ARG


@pytest.mark.parametrize('args', [
    (None, 1, 4, 29, 15, 1), (1, None, 4, 29, 15, 1),                       # null pointers
    (1, 1, 0, 29, 15, 1), (1, 1, 4, 0, 15, 1), (1, 1, 4, 29, 0, 1), (1, 1, 4, 29, 33, 1),     # no body, no frame, V
    (1, 1, 4, 29, 15, 0), (1, 1, 4, 29, 15, 30),                            # moving average outside 1..L
])
def test_skel_smooth_argument_errors(args):
    L = _lib().load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    raw, out, *ints = args
    assert L.agcn_skel_smooth(p if raw else None, p if out else None, *ints, None) == ERR_ARG


@pytest.mark.parametrize('args', [
    (0, 1, 1, 1, 3, 4, 24, 15, 1), (1, 0, 1, 1, 3, 4, 24, 15, 1), (1, 1, 0, 1, 3, 4, 24, 15, 1),
    (1, 1, 1, 0, 3, 4, 24, 15, 1),                                          # null pointers
    (1, 1, 1, 1, 0, 4, 24, 15, 1), (1, 1, 1, 1, 65536, 4, 24, 15, 1),      # no stream, more than one launch holds
    (1, 1, 1, 1, 3, 0, 24, 15, 1), (1, 1, 1, 1, 3, 4, 0, 15, 1), (1, 1, 1, 1, 3, 4, 24, 33, 1),
    (1, 1, 1, 1, 3, 4, 24, 15, 0), (1, 1, 1, 1, 3, 4, 24, 15, 25),         # moving average outside 1..Tmax
])
def test_skel_append_many_argument_errors(args):
    L = _lib().load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    ptrs, ints = args[:4], args[4:]
    assert L.agcn_skel_append_many(*(p if x else None for x in ptrs), *ints, None) == ERR_ARG


# ---- the Python wrappers -----------------------------------------------------------------------------------------------------
def test_wrappers_reject_wrong_shapes():
    import torch
    import agcn_amd  # noqa: F401
    from agcn_amd import ops
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)          # noqa: E731
    pool = torch.zeros(1, 4, 29, 15, 3)
    for bad in (dict(pool=torch.zeros(4, 29, 15, 3)), dict(pool=torch.zeros(1, 4, 29, 15, 2)),
                dict(length=i32(1)), dict(block=i32(0, 0, 0)), dict(start=torch.zeros(2, dtype=torch.int64)),
                dict(start=torch.zeros(2, 1, dtype=torch.int32)), dict(start=None), dict(frames=30), dict(frames=0),
                dict(start=i32(), length=i32()), dict(center=True, center_firstframe=True)):
        kw = dict(pool=pool, start=i32(0, 5), length=i32(10, 24), frames=24)
        kw.update(bad)
        with pytest.raises(ValueError):
            ops.prenorm_windows(**kw)
    for raw, k in ((torch.zeros(29, 4, 15), 1), (torch.zeros(29, 4, 15, 2), 1), (torch.zeros(29, 4, 15, 3), 0),
                   (torch.zeros(29, 4, 15, 3), 30)):
        with pytest.raises(ValueError):
            ops.skel_smooth(raw, k)
    rings, frames = torch.zeros(3, 4, 24, 15, 3), torch.zeros(3, 4, 15, 3)
    for bad in (dict(rings=rings[0]), dict(frames=frames[:2]), dict(frames=torch.zeros(3, 4, 1, 15, 3)),
                dict(slot=i32(0, 0)), dict(count=torch.ones(3, dtype=torch.int64))):
        kw = dict(rings=rings, frames=frames, slot=i32(0, 0, -1), count=i32(1, 1, 0))
        kw.update(bad)
        with pytest.raises(ValueError):
            ops.skel_append_many(**kw)
    # right shapes on the wrong device get as far as the pointer check: there is no CPU path
    with pytest.raises(RuntimeError, match='GPU tensor'):
        ops.skel_smooth(torch.zeros(29, 4, 15, 3), 3)
    with pytest.raises(RuntimeError, match='GPU tensor'):
        ops.prenorm_windows(pool, i32(0, 5), i32(10, 24), frames=24)


def test_infer_shim_exports_the_new_classes():
    import agcn_amd  # noqa: F401
    from agcn_amd import online
    import infer.inference as shim
    assert shim.RecordingRecognition is online.RecordingRecognition
    assert shim.MultiStreamRecognition is online.MultiStreamRecognition and shim.window_plan is online.window_plan
