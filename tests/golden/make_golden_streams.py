"""Generate the bone / motion stream fixtures by running the REFERENCE's dataset scripts on the CPU:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_streams.py

  streams_ntu.npz        seeded joint files (N = 2, C = 3, T = 5, V = 25, M = 2; clip 1 is zero from frame 3 on, body 1 of
                         clip 0 is absent) are written into a temporary tree and the reference's
                         data_gen/gen_bone_data.py and data_gen/gen_motion_data.py are EXECUTED UNMODIFIED on it
                         (runpy.run_path).  The first resolves ./data/..., the second ../data/..., so the working directory
                         differs between the two.  Stored: x (the ntu/xview train joint file), bone, joint_motion,
                         bone_motion (the files the scripts wrote next to it) and the scripts' own `pairs` tables
                         (pairs_ntu: 1-based (joint, parent) rows, pairs_kinetics: 0-based rows).
  streams_kinetics.npz   the scripts only loop over the two NTU datasets, so no script run can produce a Kinetics file.
                         This fixture is made with the script's own statement, `x[..., v1, :] - x[..., v2, :]` per pair
                         of its pairs['kinetics'] (no index shift: that table is 0-based), and the motion script's own
                         statement `data[:, :, t + 1] - data[:, :, t]`, last frame 0, on a seeded (2, 3, 5, 18, 2) tensor.

Needs the reference checkout and tqdm (the scripts import it).  Only data is stored."""
import os
import runpy
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

import make_golden as mg  # noqa: E402

LIMIT = 512 << 10
N, C, T, M = 2, 3, 5, 2


def joint_file(rng, V):
    x = rng.standard_normal((N, C, T, V, M)).astype(np.float32)
    x[1, :, 3:] = 0            # the dataset's zero padding behind a short clip
    x[0, :, :, :, 1] = 0       # an absent second body
    return x


def run_scripts(root):
    """Joint files for both NTU datasets and both sets -> run the two scripts -> the xview train files and `pairs`."""
    rng = np.random.default_rng(2100)
    for dataset in ('xview', 'xsub'):
        os.makedirs(os.path.join(root, 'data', 'ntu', dataset))
        for part in ('train', 'val'):
            np.save(os.path.join(root, 'data', 'ntu', dataset, f'{part}_data_joint.npy'), joint_file(rng, 25))
    os.makedirs(os.path.join(root, 'sub'))
    cwd = os.getcwd()
    try:
        os.chdir(root)
        pairs = runpy.run_path(os.path.join(mg.REF, 'data_gen', 'gen_bone_data.py'))['pairs']
        os.chdir(os.path.join(root, 'sub'))
        runpy.run_path(os.path.join(mg.REF, 'data_gen', 'gen_motion_data.py'))
    finally:
        os.chdir(cwd)

    def load(name):
        return np.load(os.path.join(root, 'data', 'ntu', 'xview', f'train_data_{name}.npy'))
    return load('joint'), load('bone'), load('joint_motion'), load('bone_motion'), pairs


def motion(data):
    out = np.zeros_like(data)
    for t in range(data.shape[2] - 1):
        out[:, :, t, :, :] = data[:, :, t + 1, :, :] - data[:, :, t, :, :]
    return out


def save(name, **arrays):
    path = os.path.join(HERE, name)
    np.savez_compressed(path, **arrays)
    assert os.path.getsize(path) < LIMIT, os.path.getsize(path)
    print(path, os.path.getsize(path))


if __name__ == '__main__':
    with tempfile.TemporaryDirectory() as root:
        x, bone, jm, bm, pairs = run_scripts(root)
    assert x.dtype == bone.dtype == jm.dtype == bm.dtype == np.float32 and x.shape == (N, C, T, 25, M)
    assert pairs['ntu/xview'] == pairs['ntu/xsub']
    assert np.array_equal(jm, motion(x)) and np.array_equal(bm, motion(bone))      # the scripts ran on these files
    save('streams_ntu.npz', x=x, bone=bone, joint_motion=jm, bone_motion=bm,
         pairs_ntu=np.asarray(pairs['ntu/xview'], dtype=np.int64),
         pairs_kinetics=np.asarray(pairs['kinetics'], dtype=np.int64))

    xk = joint_file(np.random.default_rng(2101), 18)
    bk = xk.copy()
    for v1, v2 in pairs['kinetics']:
        bk[:, :, :, v1, :] = xk[:, :, :, v1, :] - xk[:, :, :, v2, :]
    save('streams_kinetics.npz', x=xk, bone=bk, joint_motion=motion(xk), bone_motion=motion(bk),
         pairs_kinetics=np.asarray(pairs['kinetics'], dtype=np.int64))
