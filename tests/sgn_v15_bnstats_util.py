"""Shared by the SGN v15 batch-statistics tests and tests/golden/make_golden_sgn_v15_bnstats.py: the case table, the
loader of tests/golden/sgn15_bnstats.npz, the fp64 / fp32 tensor references of every pass (``ops.sgn15_forward_ref``'s
views cut at the token tile) and the seven mutants of the CPU test."""
import json
import os

import numpy as np

from tests import sgn_v15_util as vu

BN_NAMES = ('feature_extractor.pos_embed.norm.bn', 'feature_extractor.vel_embed.norm.bn',
            'spatial_mha.transformer.layers.l1.attn.norm.fn', 'spatial_mha.transformer.layers.l1.ffn.norm.fn',
            'temporal_mha.transformer.layers.l1.attn.norm.fn', 'temporal_mha.transformer.layers.l1.ffn.norm.fn')
# name: the geometry of the eval fixture of that name (tests/sgn_v15_util.py::CASES) with this many clips and this seed
CASES = {'j3_seg2': (5, 2311), 'j15_deployed': (9, 2321), 'j25_yaml': (3, 2331), 'j7_seg12_nobias': (4, 2341),
         'j9_seg7_h2x256': (2, 2351)}
CHUNKED = ('j15_deployed', 4)          # this case also runs in chunks of 4 clips: 4 + 4 + 1
BOUND = 1e-4                           # the project's standing fp32 bound, relative to max(1, max|ref|)
KINDS = ('mean', 'var', 'rm_none', 'rv_none', 'rm_01', 'rv_01')

_CACHE = {}


def case_args(case):
    return vu.case_args(case)


def _file():
    if 'f' not in _CACHE:
        with np.load(os.path.join(vu.GOLDEN, 'sgn15_bnstats.npz')) as f:
            _CACHE['f'] = {k: f[k] for k in f.files}
    return _CACHE['f']


def load_case(case):
    """-> dict(meta, state, x): the parameters from the seeded recipe, checked against the stored checksums."""
    f = _file()
    meta = json.loads(str(f[case + '.meta']))
    keys = [str(k) for k in f[case + '.keys']]
    shapes = {k: tuple(int(d) for d in s.split('x') if d) for k, s in zip(keys, (str(s) for s in f[case + '.shapes']))}
    state = vu.sgn15_state(shapes, meta['seed'], tuple(meta['qk_scale']))
    assert np.array_equal(vu.checksums(state), f[case + '.checksums']), 'the seeded recipe no longer reproduces the fixture'
    return dict(meta=meta, state=state, x=f[case + '.x'])


def load_record(case):
    """The reference's record of a case: dict(logits, eval_logits, floor {tensor: noise floor}, and per BatchNorm name
    mean, var, rm_none, rv_none, rm_01, rv_01 as dicts {name: array})."""
    f = _file()
    rec = dict(logits=f[case + '.logits'], eval_logits=f[case + '.eval_logits'], floor=json.loads(str(f[case + '.floor'])))
    for kind in KINDS:
        rec[kind] = {n: f[f'{case}.{kind}.{n}'] for n in BN_NAMES}
    return rec


def err(got, ref):
    """max |got - ref| / max(1, max|ref|), in fp64."""
    ref = np.asarray(ref.detach().cpu().numpy() if hasattr(ref, 'detach') else ref, dtype=np.float64)
    got = np.asarray(got.detach().cpu().numpy() if hasattr(got, 'detach') else got, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.abs(got - ref).max() / max(1.0, float(np.abs(ref).max())))


def model(case, device='cpu', train=False):
    import torch  # noqa: F401
    import agcn_amd  # noqa: F401
    from agcn_amd.model.sgn_v15 import SGN
    c = load_case(case)
    m = SGN(**c['meta']['model_args'])
    m.load_state_dict(vu.torch_state(c['state']))
    return c, m.to(device).train(train)


# ---- the tensor reference of every pass: ops.sgn15_forward_ref's views, cut at the token tile ------------------------------
def _views(x, wf, wc, V, seg, num_class, spatial, temporal):
    from agcn_amd import ops
    return ops._sgn_ref_views("sgn15 pass reference", "csrc/sgn_v15_plan.h", x, wf, wc, V, seg,
                              ops.sgn15_image_sections(V, seg, num_class, spatial, temporal))


def attention_half(t, w, p, heads, d_head, drop_group=None):
    """x1 = concat_h(a . v) Wo + bo + x of tokens t (B, R, din) on the folded views w; ``drop_group``: a mutant that
    leaves one group of 128 inner columns out of the output projection."""
    import torch
    B, R, _ = t.shape
    q, k, v = ((t @ w[p + 'qkv_w'] + w[p + 'qkv_b']).reshape(B, R, 3, heads, d_head).permute(2, 0, 3, 1, 4))
    a = torch.softmax(q @ k.transpose(-1, -2), dim=-1)
    o = (a @ v).transpose(1, 2).reshape(B, R, heads * d_head)
    if drop_group is not None:
        o = o.clone()
        o[..., drop_group * 128:(drop_group + 1) * 128] = 0
    return o @ w[p + 'o_w'] + w[p + 'o_b'] + t


def frames_tile(x, wf, wc, V, seg, num_class, spatial, temporal, layer, **mutant):
    """The tile the spatial pass ``layer`` measures, (N * seg, V, 128), in the dtype of x and the images."""
    import torch
    from agcn_amd import ops
    f, _ = _views(x, wf, wc, V, seg, num_class, spatial, temporal)
    N = x.shape[0]
    h = torch.cat([ops._sgn_ref_input(x, f, V, seg, 'pe', 've'), f['spa'].expand(N, seg, V, 64)], dim=3).reshape(N * seg, V, 128)
    return h if layer == 1 else attention_half(h, f, 's_', spatial[0], spatial[1], **mutant)


def clip_tile(feat, wf, wc, V, seg, num_class, spatial, temporal, layer, tem=True, **mutant):
    """The tile the temporal pass ``layer`` measures, (N, seg, 256); feat as ``sgn15_frames`` returns it (without tem)."""
    x0 = feat.new_zeros(feat.shape[0], seg, 3 * V)
    _, c = _views(x0, wf, wc, V, seg, num_class, spatial, temporal)
    h = feat + c['tem'] if tem else feat
    return h if layer == 1 else attention_half(h, c, 't_', temporal[0], temporal[1], **mutant)


def two_pass(z):
    """(mean, biased variance) per channel of z (..., C) by the two-pass formula in z's dtype."""
    z = z.reshape(-1, z.shape[-1])
    mean = z.sum(0) / z.shape[0]
    d = z - mean
    return mean, (d * d).sum(0) / z.shape[0]


def raw_moments(z):
    """The E[z^2] - mean^2 mutant in z's dtype."""
    z = z.reshape(-1, z.shape[-1])
    mean = z.sum(0) / z.shape[0]
    return mean, (z * z).sum(0) / z.shape[0] - mean * mean


def group_partials(z):
    """What a pass emits for the tiles z (groups, rows, C): (sum, M2 about the group's own mean), each (groups, C), in fp64."""
    s = z.sum(1)
    d = z - (s / z.shape[1])[:, None, :]
    return s, (d * d).sum(1)


# ---- each pass alone: seeded images (tests/sgn_v15_domain_util.py's recipe), no model, no fixture ---------------------------
# V, seg, N, spatial (heads, d_head, ff), temporal (heads, d_head, ff)
PASS_CASES = (
    (2, 1, 3, (8, 16, 128), (8, 16, 128)),            # one-frame clips: every clip group has count 1 and M2 exactly 0
    (3, 2, 4, (4, 32, 128), (2, 64, 128)),
    (15, 20, 5, (8, 16, 128), (8, 32, 256)),          # the deployed heads
    (17, 17, 2, (1, 128, 128), (1, 256, 128)),        # sliced heads
    (31, 31, 2, (2, 256, 512), (64, 16, 1024)),
    (32, 32, 2, (1, 512, 512), (1, 1024, 1024)),      # no padded row
)
PASS_IDS = [f'j{c[0]}s{c[1]}n{c[2]}-{"x".join(map(str, c[3]))}-{"x".join(map(str, c[4]))}' for c in PASS_CASES]
PASS_NUM_CLASS = 7
PASSES = (('frames', 1), ('frames', 2), ('clip', 1), ('clip', 2))
CENTRED = (2, 3)                       # the cases of PASS_CASES that also run badly centred
# chosen on the CPU (test_gpu_sgn_v15_bnstats.py asserts both conditions before it looks at a kernel): the E[z^2] - mean^2
# mutant's miss grows with the square of the tile's mean M (about 3 M^2 2^-24), the fp32 rounding of the tile itself with
# M / sqrt(samples); an offset of 1000 on x left the fp32 two-pass reference at 0.2 - 0.35 of the bound, one of 500 on
# feat the mutant of the clip passes at 36 - 59 bounds (the well centred columns have a variance of 15 - 22)
X_OFFSET, FEAT_OFFSET, FEAT_COLUMNS = 250.0, 1000.0, 64
_PASS = {}


def _pass_inputs(i, centred):
    """Seeded, calibrated images and x of PASS_CASES[i], and feat32 = the fp64 reference's feat rounded to fp32.
    ``centred``: the badly centred variant.  Frames passes: the position's DataNorm scale is 1 for every joint and
    x -> 0.3 x + X_OFFSET, so the embedding columns of the spatial tile get a large common mean, and the rows of the spatial
    qkv_w under those 64 columns are zero: the offset reaches x1 through the residual only.  Clip passes: the well centred
    feat plus FEAT_OFFSET on its first FEAT_COLUMNS columns, with the rows of the temporal qkv_w under them zero."""
    import torch
    from tests import sgn_v15_domain_util as du
    V, seg, N, sp, tp = PASS_CASES[i]
    case = (V, seg, sp, tp, PASS_NUM_CLASS)
    seed = 7100 + 10 * i
    _, wf, wc = du.seeded_images(case, seed)
    x = np.random.default_rng([seed, 99]).standard_normal((N, seg, 3 * V)).astype(np.float32)
    fs, cs = du._sections(case)

    def calibrated_frames(x, wf):
        x64 = torch.from_numpy(x).double()
        f64 = {n: torch.from_numpy(v).double() for n, v in du._views(wf, fs).items()}
        du._calibrate(wf, fs, 's_', du.tokens(x64, f64, V, seg), sp[0], sp[1])
        return du.frames_ref(x64, torch.from_numpy(wf).double(), case)['feat']

    feat = calibrated_frames(x, wf) if not centred else calibrated_frames(x.copy(), wf.copy())
    if centred:
        x = (0.3 * x + np.float32(X_OFFSET)).astype(np.float32)
        du._views(wf, fs)['aff'][0] = 1.0
        du._views(wf, fs)['s_qkv_w'][:64] = 0.0
        calibrated_frames(x, wf)
        du._views(wc, cs)['t_qkv_w'][:FEAT_COLUMNS] = 0.0
        feat = feat.clone()
        feat[..., :FEAT_COLUMNS] += FEAT_OFFSET
    feat32 = feat.float()
    tem = torch.from_numpy(du._views(wc, cs)['tem']).double()
    du._calibrate(wc, cs, 't_', feat32.double() + tem, tp[0], tp[1])
    return torch.from_numpy(x), torch.from_numpy(wf), torch.from_numpy(wc), feat32


def pass_case(i, centred=False):
    """-> dict(x, wf, wc, feat32 (the fp64 reference's feat rounded to fp32: what the clip passes are fed), geometry,
    tile64 / tile32 {(kind, layer): the tile the pass measures, from the fp64 / fp32 tensor reference}); made once."""
    import torch
    key = (i, centred)
    if key not in _PASS:
        V, seg, N, sp, tp = PASS_CASES[i]
        with torch.no_grad():
            x, wf, wc, feat32 = _pass_inputs(i, centred)
            g = (V, seg, PASS_NUM_CLASS, sp, tp)
            tiles = {}
            for name, cast in (('tile64', lambda t: t.double()), ('tile32', lambda t: t)):
                tiles[name] = {}
                for kind, layer in PASSES:
                    tiles[name][kind, layer] = (frames_tile(cast(x), cast(wf), cast(wc), *g, layer) if kind == 'frames'
                                                else clip_tile(cast(feat32), cast(wf), cast(wc), *g, layer))
        _PASS[key] = dict(x=x, wf=wf, wc=wc, feat32=feat32, V=V, seg=seg, N=N, spatial=sp, temporal=tp, **tiles)
    return _PASS[key]


def ratio(got, ref):
    """max |got - ref| as a multiple of the bound 1e-4 max(1, max|ref|)."""
    return err(got, ref) / BOUND
