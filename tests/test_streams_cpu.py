"""CPU checks of the bone / motion input streams: the graphs' parent tables and the tensor-code form against fixtures
written by the reference's own dataset scripts, the autograd node's CPU route against finite differences, the C entries'
host-side refusals (no device call), the index arithmetic of the kernels on the host (tests/streams_plan_check.cpp) and
the Processor's stream argument."""
import ctypes
import os
import random
import shutil
import subprocess
import types

import numpy as np
import pytest
import torch
import yaml

from tests import streams_util as su

ROOT = su.ROOT
ERR_ARG, ERR_UNSUPPORTED = -1, -3


def _ops():
    import agcn_amd  # noqa: F401
    from agcn_amd import ops
    return ops


# ---- tables --------------------------------------------------------------------------------------------------------------
def test_bone_parents_equal_the_reference_tables():
    ntu, kin = su.fixture('ntu'), su.fixture('kinetics')
    assert su.graph_parents(25) == su.parents_from_pairs(ntu['pairs_ntu'], 25, one_based=True)
    assert su.graph_parents(18) == su.parents_from_pairs(ntu['pairs_kinetics'], 18, one_based=False)
    assert np.array_equal(ntu['pairs_kinetics'], kin['pairs_kinetics'])
    # NTU, compared after subtracting 1, row by row; every joint has exactly one row
    assert sorted((int(a) - 1, int(b) - 1) for a, b in ntu['pairs_ntu']) == list(enumerate(su.graph_parents(25)))
    assert sorted((int(a), int(b)) for a, b in kin['pairs_kinetics']) == list(enumerate(su.graph_parents(18)))


def test_kinetics_table_is_not_the_graphs_inward_list():
    from agcn_amd.graph import kinetics
    inward = dict(kinetics.inward)
    g = kinetics.Graph()
    assert g.bone_parents[0] == 0 and g.bone_parents[1] == 0 and inward[0] == 1 and 1 not in inward
    assert all(g.bone_parents[v] == inward[v] for v in range(2, 18))


def test_b25_j15_parents_come_from_its_own_edges():
    from agcn_amd.graph import openpose_b25_j15 as g15
    parents = g15.Graph().bone_parents
    assert len(parents) == 15 and parents[1] == 1
    assert all(parents[c] == p for c, p in g15.inward) and len(g15.inward) == 14


@pytest.mark.parametrize('module', ['ntu_rgb_d', 'kinetics', 'openpose_b25_j15'])
def test_graph_exposes_bone_parents(module):
    import importlib
    import agcn_amd  # noqa: F401
    m = importlib.import_module(f'agcn_amd.graph.{module}')
    g = m.Graph()
    assert g.bone_parents == list(m.bone_parents) and len(g.bone_parents) == g.num_node
    assert all(0 <= p < g.num_node for p in g.bone_parents)
    top = importlib.import_module(f'graph.{module}')                 # the reference's import path
    assert top.Graph().bone_parents == g.bone_parents


# ---- the tensor-code form against the reference's files ------------------------------------------------------------------
@pytest.mark.parametrize('name,V', [('ntu', 25), ('kinetics', 18)])
def test_streams_ref_reproduces_the_reference_files(name, V):
    ops, f = _ops(), su.fixture(name)
    x = torch.from_numpy(f['x'].copy())
    got = ops.streams_ref(x, su.graph_parents(V), su.DERIVED)
    for s in su.DERIVED:
        assert got[s].dtype == torch.float32 and np.array_equal(got[s].numpy(), f[s]), s
    # the route skeleton_streams takes for a CPU tensor, and every subset
    for want in su.SUBSETS:
        got = ops.skeleton_streams(x, su.graph_parents(V), want)
        assert tuple(got) == want
        for s in want:
            assert np.array_equal(got[s].numpy(), f[s]), (want, s)


def test_fixture_is_what_the_generator_promises():
    f = su.fixture('ntu')
    assert f['x'].shape == (2, 3, 5, 25, 2) and not f['x'][1, :, 3:].any() and not f['x'][0, :, :, :, 1].any()
    assert f['x'][1, :, :3].all() and f['x'][0, :, :, :, 0].all()
    # the padded zero frames are frames like any other: the last real frame's motion is -x[t]
    assert np.array_equal(f['joint_motion'][1, :, 2], -f['x'][1, :, 2])
    assert not f['bone'][:, :, :, 20].any()                           # the spine is its own parent: exactly 0
    for name in ('streams_ntu.npz', 'streams_kinetics.npz'):
        assert os.path.getsize(os.path.join(su.GOLDEN, name)) < 512 << 10


@pytest.mark.parametrize('V', [15, 18, 25])
def test_gradcheck_of_the_cpu_route(V):
    ops = _ops()
    parent = tuple(su.graph_parents(V))
    x = torch.randn(1, 2, 3, V, 2, dtype=torch.float64, generator=torch.Generator().manual_seed(V)).requires_grad_(True)
    for want in (su.DERIVED, ('bone',), ('joint_motion',), ('bone_motion',)):
        assert torch.autograd.gradcheck(lambda t: ops.StreamsFunction.apply(t, parent, want, None), (x,))
    # and through the public function, against the fp64 form the GPU test compares the kernel with
    out = ops.skeleton_streams(x, parent, su.DERIVED)
    cot = {s: torch.randn(x.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(i))
           for i, s in enumerate(su.DERIVED)}
    dx, = torch.autograd.grad(sum((out[s] * cot[s]).sum() for s in su.DERIVED), x)
    want, _, _ = su.backward64({s: c.numpy() for s, c in cot.items()}, parent, (0.0, 1.0, 1.0, 1.0))
    assert np.abs(dx.numpy() - want).max() < 1e-13
    got = ops.streams_bwd_ref({'joint': cot['bone'], **cot}, parent, su.WEIGHTS)
    want, mag, cnt = su.backward64({'joint': cot['bone'].numpy(), **{s: c.numpy() for s, c in cot.items()}}, parent)
    assert np.abs(got.numpy() - want).max() < 1e-13 and cnt.max() >= 10 and (mag > 0).all()


def test_host_refusals_of_ops():
    ops = _ops()
    x = torch.randn(2, 3, 4, 25, 2)
    parent = su.graph_parents(25)
    with pytest.raises(ValueError, match='contiguous'):
        ops.skeleton_streams(x.transpose(1, 2), parent)
    with pytest.raises(ValueError, match='25 joints'):
        ops.skeleton_streams(x, parent[:-1])
    with pytest.raises(ValueError, match='parent'):
        ops.skeleton_streams(x, [25] + parent[1:])
    with pytest.raises(ValueError, match='parent'):
        ops.skeleton_streams(x, [-1] + parent[1:])
    with pytest.raises(ValueError, match='want'):
        ops.skeleton_streams(x, parent, ())
    with pytest.raises(ValueError, match='want'):
        ops.skeleton_streams(x, parent, ('joint',))
    with pytest.raises(ValueError, match='floating'):
        ops.skeleton_streams(x.to(torch.int32), parent)
    with pytest.raises(ValueError, match='5-D'):
        ops.skeleton_streams(x[0], parent)
    with pytest.raises(ValueError, match='cotangent'):
        ops.streams_bwd({}, parent)


# ---- the C entries refuse on the host, without a GPU ------------------------------------------------------------------------
def _table(values):
    return (ctypes.c_int * len(values))(*values)


def test_c_entries_return_the_stated_codes_before_any_device_call():
    import agcn_amd  # noqa: F401
    from agcn_amd import lib
    L = lib.load()
    p = 16          # any non-null address: the checks must return before touching it
    ok = list(range(25))

    def fwd(table, V, bone=p, x=p, N=1, C=3, T=4, M=2):
        return L.agcn_streams_fwd(x, bone, None, None, table, N, C, T, V, M, None)

    def bwd(table, V, d=p, dx=p, N=1, C=3, T=4, M=2):
        return L.agcn_streams_bwd(None, d, None, None, dx, table, 1.0, 1.0, 1.0, 1.0, N, C, T, V, M, None)

    for call in (fwd, bwd):
        assert call(_table(ok), 0) == ERR_ARG                                    # V = 0
        assert call(_table(list(range(33))), 33) == ERR_UNSUPPORTED              # V = 33
        assert call(_table([25] + ok[1:]), 25) == ERR_ARG                        # parent[v] = V
        assert call(_table(ok[:24] + [-1]), 25) == ERR_ARG                       # parent[v] = -1
        assert call(None, 25) == ERR_ARG                                         # no table
        assert call(_table(ok), 25, N=0) == ERR_ARG and call(_table(ok), 25, T=-1) == ERR_ARG
        assert call(_table(ok), 25, N=1 << 15, C=1 << 10, T=64, M=2) == ERR_UNSUPPORTED      # 2^31 * 25 * 2 elements
    assert fwd(_table(ok), 25, bone=None) == ERR_ARG                             # no output pointer
    assert fwd(_table(ok), 25, x=None) == ERR_ARG
    assert bwd(_table(ok), 25, d=None) == ERR_ARG and bwd(_table(ok), 25, dx=None) == ERR_ARG


def test_lib_call_passes_a_host_int_array_and_nothing_else_there(monkeypatch):
    import agcn_amd  # noqa: F401
    from agcn_amd import lib
    monkeypatch.setattr(lib, 'stream', lambda: None)       # no GPU here; every check below returns before a HIP call
    assert lib.DECLARATIONS['agcn_streams_fwd'][1][4] == ('const int*', 'host_parent')
    assert lib.status('agcn_streams_fwd', None, None, None, None, list(range(25)), 1, 3, 4, 25, 2) == lib.ERR_ARG
    assert lib.status('agcn_streams_fwd', 16, 16, None, None, [25] + list(range(1, 25)), 1, 3, 4, 25, 2) == lib.ERR_ARG
    assert lib.status('agcn_streams_fwd', 16, 16, None, None, np.arange(33), 1, 3, 4, 33, 2) == lib.ERR_UNSUPPORTED
    assert lib.status('agcn_streams_fwd', 16, 16, None, None, torch.arange(25), 0, 3, 4, 25, 2) == lib.ERR_ARG
    with pytest.raises(RuntimeError, match=r'agcn_streams_fwd\(host_parent\)'):
        lib.status('agcn_streams_fwd', 16, 16, None, None, [0.5] * 25, 1, 3, 4, 25, 2)
    with pytest.raises(RuntimeError, match=r'agcn_streams_fwd\(host_parent\)'):
        lib.status('agcn_streams_fwd', 16, 16, None, None, torch.zeros(25), 1, 3, 4, 25, 2)
    # the only host arrays of the header are the two tables
    hosts = [(n, p) for n, (_, ps) in lib.DECLARATIONS.items() for _, p in ps if p.startswith('host_')]
    assert sorted(hosts) == [('agcn_streams_bwd', 'host_parent'), ('agcn_streams_fwd', 'host_parent')]


def test_streams_plan_checker(tmp_path):
    cxx = next((c for c in (os.environ.get('CXX'), 'c++', 'g++', 'clang++') if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip('no host C++ compiler')
    exe = str(tmp_path / 'streams_plan_check')
    r = subprocess.run([cxx, '-std=c++17', '-Wall', '-Werror', '-O2', '-I', os.path.join(ROOT, '2s-agcn_amd', 'csrc'),
                        os.path.join(ROOT, 'tests', 'streams_plan_check.cpp'), '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-4000:]
    assert ' cases, 0 failures' in r.stdout and int(r.stdout.split(' cases')[0].split()[-1]) > 1000000


# ---- Processor ---------------------------------------------------------------------------------------------------------------
def _args(tmp_path, **cfg):
    from agcn_amd.processor import load_args
    base = dict(work_dir=str(tmp_path / 'work'), feeder='agcn_amd.feeders.feeder.Feeder', stream='bone',
                train_feeder_args=dict(data_path='none.npy', label_path='none.pkl'),
                model_args=dict(graph='graph.ntu_rgb_d.Graph'))
    base.update(cfg)
    path = tmp_path / 'cfg.yaml'
    path.write_text(yaml.safe_dump(base))
    return load_args(['--config', str(path)])


def test_stream_argument_surface(tmp_path):
    from agcn_amd.processor import load_args
    a = load_args([])
    assert a.stream == 'joint' and a.stream_parents is None
    b = load_args(['--stream', 'bone_motion', '--stream-parents', '0', '0', '1'])
    assert b.stream == 'bone_motion' and b.stream_parents == [0, 0, 1]
    with pytest.raises(SystemExit):
        load_args(['--stream', 'limb'])
    for name, phase in (('train_bone.yaml', 'train'), ('test_bone.yaml', 'test')):
        c = load_args(['--config', os.path.join(ROOT, 'config', 'nturgbd-cross-view', name)])
        j = load_args(['--config', os.path.join(ROOT, 'config', 'nturgbd-cross-view', 'train_joint.yaml')])
        assert c.stream == 'bone' and c.phase == phase and c.model_args == j.model_args
        assert c.test_feeder_args == j.test_feeder_args          # the bone configs point at the joint data
    assert load_args(['--config', os.path.join(ROOT, 'config', 'nturgbd-cross-view', 'test_bone.yaml')]).save_score is True


@pytest.mark.parametrize('cfg,match', [
    (dict(device_augment=False, train_feeder_args=dict(random_move=True)), 'device-augment'),
    (dict(train_feeder_args=dict(random_rotation=True, stretch=True)), 'stretch'),
    (dict(train_feeder_args=dict(random_subsample=100)), 'random_subsample'),
    (dict(train_feeder_args=dict(normalization=True)), 'normalization'),
    (dict(train_feeder_args=dict(), test_feeder_args=dict(normalization=True)), 'test_feeder_args.normalization'),
    (dict(feeder='agcn_amd.processor.NpyFeeder', train_feeder_args=dict(random_shift=True)), 'random_shift'),
])
def test_processor_refuses_what_breaks_the_transform_order(tmp_path, cfg, match):
    """Raised by Processor itself, first thing: before a device, a model or a dataset file is touched."""
    from agcn_amd.processor import Processor
    arg = _args(tmp_path, **cfg)
    for stream in ('bone', 'joint_motion', 'bone_motion'):
        arg.stream = stream
        with pytest.raises(ValueError, match=match) as e:
            Processor(arg)
        assert f'--stream {stream}' in str(e.value)


def test_check_stream_lets_the_supported_configurations_through():
    from agcn_amd.feeders.feeder import Feeder
    from agcn_amd.processor import SyntheticFeeder, check_stream
    every = dict(random_choose=True, random_shift=True, random_move=True, random_zaxis_flip=True, random_xaxis_scale=True,
                 random_yaxis_scale=True, random_rotation=True, window_size=64)
    check_stream('bone', Feeder, every, True)                      # all of them, on the device: after the stream
    check_stream('bone', Feeder, dict(window_size=64), False)      # nothing random on the host
    check_stream('bone_motion', SyntheticFeeder, dict(num_samples=4), True)
    check_stream('joint', Feeder, dict(normalization=True, random_move=True), False)     # the joint stream: as before
    with pytest.raises(ValueError, match='--stream'):
        check_stream('limb', Feeder, {}, True)
    from agcn_amd.sgn_processor import SGNProcessor
    with pytest.raises(ValueError, match='--stream bone'):
        SGNProcessor(types.SimpleNamespace(stream='bone', world_size=1))


def test_prepare_batch_derives_the_stream_before_the_transforms():
    from agcn_amd.feeders import DeviceAugment
    from agcn_amd.processor import prepare_batch
    f = su.fixture('ntu')
    parents = su.graph_parents(25)
    x = torch.from_numpy(f['x'].copy())
    aug = DeviceAugment(window_size=8, random_move=True, random_rotation=True, rotation_theta=0.3)

    def seeded(fn):
        random.seed(5)
        np.random.seed(5)
        return fn()
    for s in su.DERIVED:
        want = seeded(lambda: aug(torch.from_numpy(f[s].copy())))
        got = seeded(lambda: prepare_batch(x.double(), aug, s, parents))
        assert got.dtype == torch.float32 and tuple(got.shape) == (2, 3, 8, 25, 2)
        assert np.array_equal(got.numpy(), want.numpy()), s
        assert np.array_equal(prepare_batch(x, None, s, parents).numpy(), f[s])
    # the translation of random_move does not commute with the bone difference: the other order is different data
    other = ops_bone_after(aug, x, parents, seeded)
    assert not np.array_equal(other.numpy(), seeded(lambda: prepare_batch(x, aug, 'bone', parents)).numpy())
    assert np.array_equal(seeded(lambda: prepare_batch(x, aug)).numpy(), seeded(lambda: aug(x)).numpy())      # joint
    with pytest.raises(ValueError, match='parent'):
        prepare_batch(x, None, 'bone')


def ops_bone_after(aug, x, parents, seeded):
    return _ops().streams_ref(seeded(lambda: aug(x)), parents, ('bone',))['bone']
