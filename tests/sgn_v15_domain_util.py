"""Shared by tests/test_sgn_v15_domain_cpu.py and tests/test_gpu_sgn_v15_domain.py: the table of geometries that walks the
domain of the SGN v15 kernels (csrc/sgn_v15.hip, csrc/sgn_v15_device.h), a seeded recipe for the two flat weight images
(no model, no fixture), the calibration of the query scale, the fp64 reference and a set of mutants of that reference.

Which case reaches which code of ``sgn15_block`` (F = the frames kernel, 128 -> 256; C = the clip kernel, 256 -> 512):

  whole-head groups    d_head 16: F 0 1 2, C 0 1 2 (the ``r >= 16`` select in both kernels); more than one group of 16-wide
                       heads (``sgn15_group_first_head(g) = 8 g``): F 1 2, C 0 2; the 64-head limit: F 2, C 2
                       d_head 32 up to group 7: F 10, C 10;  d_head 64 with 2 groups: F 3, C 3, with 8 groups: F 11, C 11
  sliced heads         d_head 128 (hs = 1): F 4 5, C 4 5;  256: F 6, C 6 9;  384 (odd hs): F 7, C 7;  512: F 8, C 8;
                       1024: F 9;  more than one sliced head (``head * hs + sl``, the per-head map offset, P slot 0 reused):
                       F 5 6 8, C 5 6 7 8 9
  group walk of Wo     inner > 128: every case but F 0 4 and C 1 4
  chunk walk of the FFN  ff > 128: F 1 4 5 7 10, C 1 3 5 6 9 10 (ff 1024: F 4, C 3)
  rows                 V 2 16 17 31 32 and seg 1 16 17 31 32: cases 0 1 2 3 4 (and 3 4 5 9 13 25 joints, 2 3 5 7 9 20 frames)
  num_class            1 (case 0), 257 and 400 (the fc loop's second trip: 3, 6), 4096 (the limit: 9)
  cases 12 - 14        the frames geometry and joint count of 3, 4, 7 on one-frame clips (see FRAMES_ROWS_BY_INDEX), with
                       a 1 x 1024, an 8 x 32 and a 2 x 64 clip block on a single row

The frames kernel is compared with the reference on x; the clip kernel is fed the REFERENCE's feat rounded to fp32 and
compared with the reference recomputed from that same input, so that each kernel answers for its own error only.  The
conditions that make the comparison meaningful (a softmax that is neither flat nor one-hot, negative maxima, every token
row the arg-max of some output column, fp32 headroom, every mutant caught) are asserted on the CPU."""
import math

import numpy as np
import torch

from tests import sgn_v15_util as vu

N_CLIPS = 2
ROWS = 32          # the height of the kernels' token tile: a clip's frames are padded with zero rows up to it

# V, seg, spatial (heads, d_head, ff), temporal (heads, d_head, ff), num_class
CASES = (
    (2, 1, (8, 16, 128), (16, 16, 128), 1),
    (16, 17, (16, 16, 256), (8, 16, 384), 60),
    (17, 16, (64, 16, 128), (64, 16, 128), 33),
    (31, 31, (4, 64, 128), (4, 64, 1024), 257),
    (32, 32, (1, 128, 1024), (1, 128, 128), 60),
    (5, 3, (2, 128, 256), (3, 128, 256), 60),
    (9, 7, (2, 256, 128), (2, 256, 384), 400),
    (25, 20, (1, 384, 384), (2, 384, 128), 60),
    (4, 32, (2, 512, 128), (2, 512, 128), 60),
    (32, 2, (1, 1024, 128), (4, 256, 512), 4096),
    (13, 9, (32, 32, 256), (32, 32, 256), 60),
    (3, 5, (16, 64, 128), (16, 64, 128), 60),
    (31, 1, (4, 64, 128), (1, 1024, 128), 60),
    (32, 1, (1, 128, 1024), (8, 32, 128), 60),
    (25, 1, (1, 384, 384), (2, 64, 128), 60),
)
# Cases 12 - 14 repeat the frames geometry and the joint count of cases 3, 4 and 7 on two one-frame clips.  "Every real
# row of every token set is the arg-max of some output column" cannot be met by a seed for the frames block of 3, 4 and 7:
# a frame has 256 output columns for 25 - 32 rows, so even with equally likely rows a given row wins no column with
# probability (1 - 1/32)^256 = 3e-4, and the 62 / 64 / 40 token sets of those cases hold 1922 / 2048 / 1000 rows; measured
# at seeds 301 / 401 / 701, 106 / 68 / 17 (set, row) pairs win no column, and no seed of 60 tried brought case 7 under 10.
# There the condition is asserted per row INDEX (every joint wins a column in some token set), and as stated, for every
# row of every token set, on the two token sets of the companion case and on every other block of the table.
FRAMES_ROWS_BY_INDEX = tuple(CASES[i] for i in (3, 4, 7))
# one seed per case: the first of 100 * case + 1, + 2, ... (case 9: of 9001, ...) at which the case meets every condition
# of the CPU test
SEEDS = (1, 101, 202, 301, 401, 501, 601, 701, 804, 9246, 1001, 1101, 1209, 1328, 1404)
IDS = [f'{i}-j{c[0]}s{c[1]}-{"x".join(map(str, c[2]))}-{"x".join(map(str, c[3]))}-c{c[4]}' for i, c in enumerate(CASES)]

MUTANTS = {
    1: 'padded rows treated as real tokens, as keys and in the maximum',
    2: 'padded rows masked as keys but included in the maximum',
    3: 'the maximum clamped at 0, the neutral element of a ReLU',
    4: 'd_head 16: the odd head of a pair uses the even head\'s probabilities in a . v',
    5: 'the maps of two heads swapped in the stored attention output',
    6: 'the last 128 columns of q and k dropped from the scores',
    7: 'the last 128 hidden columns of the feed-forward dropped',
    8: 'group g > 0 projected with group 0\'s rows of o_w',
}
TARGET_STD = 1.5   # of the logits q k^T after the calibration


def applies(mutant, side, rows, geometry):
    """Whether ``mutant`` changes the block ``geometry`` = (heads, d_head, ff) of ``side`` ('frames' / 'clip') on ``rows``
    token rows.  With a single row every head's map is the 1 x 1 matrix [1] whatever the scores: mutants 4, 5 and 6 are
    then the reference itself."""
    heads, d_head, ff = geometry
    return {1: side == 'clip' and rows < ROWS, 2: side == 'clip' and rows < ROWS, 3: True, 4: d_head == 16 and rows > 1,
            5: heads > 1 and rows > 1, 6: d_head >= 256 and rows > 1, 7: ff >= 256, 8: heads * d_head >= 256}[mutant]


def check(got, ref):
    """The project's fp32 rule per tensor, max|got - ref| <= 1e-4 max(1, max|ref|) (sgn_v15_util.bound) -> the measured
    worst difference as a multiple of that bound: the tensor passes iff the ratio is <= 1."""
    got = np.asarray(got.detach().cpu().numpy() if torch.is_tensor(got) else got, dtype=np.float64)
    ref = np.asarray(ref.detach().cpu().numpy() if torch.is_tensor(ref) else ref, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.abs(got - ref).max()) / vu.bound(ref)


# ---- the seeded images ----
def _sections(case):
    from agcn_amd import ops
    V, seg, sp, tp, num_class = case
    return ops.sgn15_image_sections(V, seg, num_class, sp, tp)


def seeded_images(case, seed):
    """-> (x (N, seg, 3V), frames image, clip image) as fp32 numpy arrays; section i (counted through both images) and x
    each draw from a generator of their own."""
    V, seg = case[0], case[1]
    images, i = [], 0
    for secs in _sections(case):
        img = np.zeros(secs[-1][1] + math.prod(secs[-1][2]), dtype=np.float32)
        for name, off, shape in secs:
            rng = np.random.default_rng([int(seed), i])
            i += 1
            if name == 'aff':                           # (4, V, 3): scale, shift of the position; scale, shift of the velocity
                v = np.stack([rng.uniform(0.5, 1.5, shape[1:]), 0.2 * rng.standard_normal(shape[1:]),
                              rng.uniform(0.5, 1.5, shape[1:]), 0.2 * rng.standard_normal(shape[1:])])
            elif name in ('spa', 'tem'):
                v = 0.5 * rng.standard_normal(shape)
            elif name.endswith('_b'):
                v = 0.1 * rng.standard_normal(shape)
            else:                                       # a (K, N) matrix
                v = math.sqrt(2.0 / shape[0]) * rng.standard_normal(shape)
            img[off:off + math.prod(shape)] = v.astype(np.float32).reshape(-1)
        images.append(img)
    x = np.random.default_rng([int(seed), i]).standard_normal((N_CLIPS, seg, 3 * V)).astype(np.float32)
    return x, images[0], images[1]


def _views(img, secs):
    return {n: img[o:o + math.prod(s)].reshape(s) for n, o, s in secs}


# ---- the reference, split at feat, with the mutants.  mutant = 0 is ops.sgn15_forward_ref operation for operation (the
# CPU test asserts equal bits in fp64). ----
def tokens(x, f, V, seg):
    """The input of the spatial block (N * seg, V, 128) = [pos + vel | spa]."""
    relu = torch.relu
    N = x.shape[0]
    xr = x.reshape(N, seg, V, 3)
    dif = torch.cat([xr.new_zeros(N, 1, V, 3), xr[:, 1:] - xr[:, :-1]], dim=1)

    def emb(v, p):
        return relu(relu(v @ f[p + '1_w'] + f[p + '1_b']) @ f[p + '2_w'] + f[p + '2_b'])

    h = torch.cat([emb(xr * f['aff'][0] + f['aff'][1], 'pe') + emb(dif * f['aff'][2] + f['aff'][3], 've'),
                   f['spa'].expand(N, seg, V, 64)], dim=3)
    return h.reshape(N * seg, V, 128)


def scores(t, w, p, heads, d_head):
    """q k^T of the block (B, heads, R, R)."""
    B, R, _ = t.shape
    q, k, _ = ((t @ w[p + 'qkv_w'] + w[p + 'qkv_b']).reshape(B, R, 3, heads, d_head).permute(2, 0, 3, 1, 4))
    return q @ k.transpose(-1, -2)


def block(t, w, p, heads, d_head, mutant=0):
    """t (B, R, din) -> (y (B, R or 32, dout), the stored map (B, heads, R, R)).  Mutants 1 and 2 run on the 32-row tile."""
    B, real, din = t.shape
    inner = heads * d_head
    if mutant in (1, 2):
        t = torch.cat([t, t.new_zeros(B, ROWS - real, din)], dim=1)
    R = t.shape[1]
    q, k, v = ((t @ w[p + 'qkv_w'] + w[p + 'qkv_b']).reshape(B, R, 3, heads, d_head).permute(2, 0, 3, 1, 4))
    if mutant == 6:
        q, k = q[..., :-128], k[..., :-128]
    s = q @ k.transpose(-1, -2)
    if mutant == 2:
        s = s.clone()
        s[..., real:] = -math.inf
    a = torch.softmax(s, dim=-1)
    used = a
    if mutant == 4:
        used = a.clone()
        used[:, 1::2] = a[:, 0::2]
    o_w = w[p + 'o_w']
    if mutant == 8:
        o_w = o_w[:128].repeat(inner // 128, 1)
    t1 = (used @ v).transpose(1, 2).reshape(B, R, inner) @ o_w + w[p + 'o_b'] + t
    hid = torch.relu(t1 @ w[p + 'f1_w'] + w[p + 'f1_b'])
    if mutant == 7:
        hid = hid.clone()
        hid[..., -128:] = 0
    y = torch.cat([hid, t1], dim=2) @ w[p + 'f2_w'] + w[p + 'f2_b']
    stored = a[:, :, :real, :real]
    if mutant == 5:
        stored = stored.clone()
        stored[:, [heads - 2, heads - 1]] = stored[:, [heads - 1, heads - 2]]
    return y, stored


def _pool(y, dim, mutant):
    m = y.amax(dim)
    return m.clamp(min=0) if mutant == 3 else m


def frames_ref(x, wf, case, mutant=0):
    """-> dict(feat (N, seg, 256) without tem, as ``ops.sgn15_frames`` returns it, attn (N * seg, heads, V, V), y)."""
    V, seg, sp = case[0], case[1], case[2]
    f = _views(wf, _sections(case)[0])
    y, sa = block(tokens(x, f, V, seg), f, 's_', sp[0], sp[1], mutant)
    return dict(feat=_pool(y.reshape(x.shape[0], seg, V, 256), 2, mutant), attn=sa, y=y)


def clip_ref(feat, wc, case, mutant=0):
    """feat (N, seg, 256) -> dict(logits, attn (N, heads, seg, seg), pooled (N, 512), z)."""
    tp = case[3]
    c = _views(wc, _sections(case)[1])
    z, ta = block(feat + c['tem'], c, 't_', tp[0], tp[1], mutant)
    pooled = _pool(z, 1, mutant)
    return dict(logits=pooled @ c['fc_w'] + c['fc_b'], attn=ta, pooled=pooled, z=z)


# ---- calibration ----
def _calibrate(img, secs, p, t64, heads, d_head):
    """Scale the q columns of the block ``p`` in the fp32 image so that std(q k^T) over the token sets ``t64`` is
    TARGET_STD (in fp64, from the image alone); nothing to do for a single row.  -> the factor."""
    if t64.shape[1] == 1:
        return 1.0
    w = {n: torch.from_numpy(v).double() for n, v in _views(img, secs).items() if n.startswith(p + 'qkv')}
    factor = TARGET_STD / float(scores(t64, w, p, heads, d_head).std())
    inner = heads * d_head
    v = _views(img, secs)
    v[p + 'qkv_w'][:, :inner] = (v[p + 'qkv_w'][:, :inner].astype(np.float64) * factor).astype(np.float32)
    v[p + 'qkv_b'][:inner] = (v[p + 'qkv_b'][:inner].astype(np.float64) * factor).astype(np.float32)
    return factor


def make(case, seed):
    """The calibrated inputs and the fp64 reference of one case, all from the seed and the reference alone -> dict:
    x, wf, wc (fp32 tensors); logits, feat, spatial_attn, temporal_attn = ``ops.sgn15_forward_ref`` in fp64; feat32 = feat
    rounded to fp32; frames / clip = ``frames_ref`` on x / ``clip_ref`` on feat32 in fp64."""
    from agcn_amd import ops
    V, seg, sp, tp, num_class = case
    x, wf, wc = seeded_images(case, seed)
    fs, cs = _sections(case)
    x64 = torch.from_numpy(x).double()
    f64 = {n: torch.from_numpy(v).double() for n, v in _views(wf, fs).items()}
    qk = [_calibrate(wf, fs, 's_', tokens(x64, f64, V, seg), sp[0], sp[1])]
    feat = frames_ref(x64, torch.from_numpy(wf).double(), case)['feat']
    tem = torch.from_numpy(_views(wc, cs)['tem']).double()
    qk.append(_calibrate(wc, cs, 't_', feat + tem, tp[0], tp[1]))
    x, wf, wc = torch.from_numpy(x), torch.from_numpy(wf), torch.from_numpy(wc)
    logits, feat, sa, ta = ops.sgn15_forward_ref(x.double(), wf.double(), wc.double(), V, seg, num_class, sp, tp)
    feat32 = feat.float()
    return dict(case=case, seed=seed, qk_factor=tuple(qk), x=x, wf=wf, wc=wc, logits=logits, feat=feat, spatial_attn=sa,
                temporal_attn=ta, feat32=feat32, frames=frames_ref(x.double(), wf.double(), case),
                clip=clip_ref(feat32.double(), wc.double(), case))


_MADE = {}


def load(i):
    """Case i of the table at its seed, made once and never modified by a test."""
    if i not in _MADE:
        with torch.no_grad():
            _MADE[i] = make(CASES[i], SEEDS[i])
    return _MADE[i]
