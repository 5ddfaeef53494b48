"""Shared by tests/test_sgn_stats_domain_cpu.py and tests/test_gpu_sgn_stats_domain.py: the SGN batch-statistics passes
(csrc/sgn_stats.hip, the ``colstats`` epilogue of csrc/sgn_device.h; geometry: csrc/sgn_stats_plan.h), each alone over the
seeded images of tests/sgn_domain_util.py, on badly centred copies of them, the finalize alone on seeded partials, and the
seven passes in sequence through the model at the domain's edges.  No fixture, no model file: everything is seeded.

A seeded image has no BatchNorm in it, so a pass run on it measures a ReLU pre-activation that the fp64 reference of
sgn_domain_util already returns:

  input pass              x | dif (zero at t = 0 of every clip), features [v*3 + c]         groups: clips of seg frames
  frames pass L = 1..3    frames_ref(x)['pre']['c<L>']       (N, seg, V, C)                 groups: frames of V joints
  clip pass L = 1..2      clip_ref(feat32)['pre']['t<L>']    (N, seg, C)                    groups: (clip, tile) of
                                                                                            min(32, seg - 32 tile) frames

``table`` returns such a tensor as z (rows, C) with its rows in group order and the group counts; everything else here is
numpy on (z, counts).  The group geometry below is written from the text of csrc/sgn_stats_plan.h:

  channels        input 2 * 3 * V; frames 128, 256, 256; clip 256, 512
  groups / clip   input 1; frames seg; clip ceil(seg / 32)
  count of g      input seg; frames V; clip min(32, seg - 32 * (g mod tiles))
  partial buffer  (groups, 2, C): the sum, then M2 = the sum of squares about the group's own mean
  carry           (3, C) doubles: count, mean, M2

Bounds.  ``check`` is the project's fp32 rule, a tensor's worst difference as a multiple of 1e-4 max(1, max|ref|).  On the
offset cases the variance is held per channel, relative to the channel's own variance, by ``REL_VAR``."""
import copy
import math

import numpy as np
import torch

from tests import sgn_bnstats_util as bu
from tests import sgn_domain_util as du
from tests import sgn_util as su

check = du.check
ROWS = du.ROWS
INPUT, FRAMES, CLIP = 0, 1, 2
# (kind, layer) of the six passes, and the name each goes by
PASSES = ((INPUT, 0), (FRAMES, 1), (FRAMES, 2), (FRAMES, 3), (CLIP, 1), (CLIP, 2))
PASS_NAMES = {(INPUT, 0): 'input', (FRAMES, 1): 'c1', (FRAMES, 2): 'c2', (FRAMES, 3): 'c3', (CLIP, 1): 't1', (CLIP, 2): 't2'}
CASES = du.CASES


# ---- csrc/sgn_stats_plan.h, restated ----
def channels(kind, layer, V):
    return 2 * 3 * V if kind == INPUT else (128 if layer == 1 else 256) if kind == FRAMES else (256 if layer == 1 else 512)


def groups_per_clip(kind, seg):
    return 1 if kind == INPUT else seg if kind == FRAMES else (seg + ROWS - 1) // ROWS


def group_count(kind, g, seg, V):
    if kind == INPUT:
        return seg
    if kind == FRAMES:
        return V
    return min(ROWS, seg - ROWS * (g % groups_per_clip(kind, seg)))


def counts_of(kind, N, seg, V):
    return [group_count(kind, g, seg, V) for g in range(N * groups_per_clip(kind, seg))]


# ---- the measured tensor of a pass as a table ----
def input_table(x, seg, V, mutant=0):
    """x (N, seg, 3V) -> z (N * seg, 2 * 3V) fp64: x, then dif.  Mutant 3: dif at t = 0 takes the previous clip's last
    frame."""
    x = np.asarray(x, dtype=np.float64)
    N = x.shape[0]
    dif = np.concatenate([np.zeros((N, 1, 3 * V)), x[:, 1:] - x[:, :-1]], axis=1)
    if mutant == 3:
        flat = x.reshape(N * seg, 3 * V)
        dif = np.concatenate([np.zeros((1, 3 * V)), flat[1:] - flat[:-1]]).reshape(N, seg, 3 * V)
    return np.concatenate([x, dif], axis=2).reshape(N * seg, 6 * V)


def table(d, kind, layer, x=None, wf=None, wc=None, mutant=0):
    """The tensor pass (kind, layer) measures on case ``d`` as z (rows, C) fp64 in group order -> (z, counts).  ``x`` /
    ``wf`` / ``wc``: fp32 replacements of the case's own input and images (the offset copies); with none of them and no
    mutant the case's stored reference is used."""
    V, seg, _, N = d['case']
    if kind == INPUT:
        return input_table((d['x'] if x is None else x).numpy(), seg, V, mutant), counts_of(kind, N, seg, V)
    with torch.no_grad():
        if kind == FRAMES:
            r = d['frames'] if wf is None and not mutant else du.frames_ref(d['x'].double(), (d['wf'] if wf is None else wf).double(),
                                                                            d['case'], mutant)
            z = r['pre'][f'c{layer}'].numpy()
            return z.reshape(N * seg * V, z.shape[-1]), counts_of(kind, N, seg, V)
        r = d['clip'] if wc is None and not mutant else du.clip_ref(d['feat32'].double(), (d['wc'] if wc is None else wc).double(),
                                                                    d['case'], mutant)
        z = r['pre'][f't{layer}'].numpy()
        return z.reshape(-1, z.shape[-1]), counts_of(kind, N, seg, V)


def group_ref(z, counts):
    """-> (sums, M2s about each group's own mean), each (groups, C) fp64."""
    sums, m2s, r0 = [], [], 0
    for n in counts:
        blk = z[r0:r0 + n]
        sums.append(blk.sum(0))
        m2s.append(np.square(blk - blk.mean(0)).sum(0))
        r0 += n
    assert r0 == len(z)
    return np.stack(sums), np.stack(m2s)


def merge_ref(sums, m2s, counts, carry=None):
    """The fp64 merge of group partials in one step, not in the kernel's order: mean = sum of sums / n, M2 = sum of M2s +
    sum of count (group mean - mean)^2 -> (mean, biased var, carry (3, C))."""
    cnt = np.asarray(counts, dtype=np.float64)[:, None]
    sums, m2s = np.asarray(sums, dtype=np.float64), np.asarray(m2s, dtype=np.float64)
    if carry is not None:
        cnt = np.concatenate([carry[0][:1, None], cnt])
        sums, m2s = np.concatenate([(carry[0] * carry[1])[None], sums]), np.concatenate([carry[2][None], m2s])
    n = cnt.sum()
    mean = sums.sum(0) / n
    m2 = m2s.sum(0) + (cnt * np.square(sums / cnt - mean)).sum(0)
    return mean, m2 / n, np.stack([np.full_like(mean, n), mean, m2])


def emulate(z, counts, per_clip):
    """The project's fp32 emulation of a pass and its finalize on z rounded to fp32 -> (sums, M2s, mean, var)."""
    sums, m2s = bu.group_partials(np.asarray(z, dtype=np.float32), counts)
    mean, var, _ = bu.finalize_emulate(sums, m2s, counts, per_clip)
    return sums, m2s, mean, var


def one_pass(z, counts):
    """The mutant the header rules out: per group sum z and sum z^2 in fp32, the variance as E[z^2] - mean^2 -> var fp32."""
    z = np.asarray(z, dtype=np.float32)
    s = z.sum(0, dtype=np.float32)
    q = (z * z).sum(0, dtype=np.float32)
    n = np.float32(len(z))
    return q / n - (s / n) * (s / n)


def rel_var(var, ref):
    """max over the channels of |var - ref| / ref (nan: a reference variance of 0 among them)."""
    var = np.asarray(var.detach().cpu().numpy() if torch.is_tensor(var) else var, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    if not (ref > 0).all():
        return math.nan
    return float((np.abs(var - ref) / ref).max())


# ---- section 2: badly centred copies ----
OFFSET_CASES = (3, 4, 5, 6, 7)     # >= 64 rows in every pass; V 17, 31, 32, 25, 15; seg 32, 33, 64, 65, 20
OFFSET = 512.0                     # S: a power of two
# 10 x the emulation's worst relative variance error over the offset cases and passes (4.1e-5, case 3's c3 pass),
# rounded up to one significant digit; the kernels' worst on MI355X is in profiles/sgn_stats_domain.txt
REL_VAR = 5e-4
_BIAS = {(FRAMES, 1): 'c1_b', (FRAMES, 2): 'c2_b', (FRAMES, 3): 'c3_b', (CLIP, 1): 't1_b', (CLIP, 2): 't2_b'}


def offset_inputs(d, kind, layer, S=OFFSET):
    """-> dict(x=, wf= or wc=): the fp32 copy of the case's input with the bias section of the measured layer shifted by
    +S on even and -S on odd channels (the input pass: x itself by +S), rounded to fp32 -- what the kernel AND the fp64
    reference read."""
    if kind == INPUT:
        return dict(x=(d['x'] + np.float32(S)).float())
    which = 0 if kind == FRAMES else 1
    img = (d['wf'] if kind == FRAMES else d['wc']).clone()
    sec = {n: (o, s) for n, o, s in du._sections(d['case'])[which]}[_BIAS[kind, layer]]
    C = sec[1][0]
    sign = torch.where(torch.arange(C) % 2 == 0, 1.0, -1.0).float()
    img[sec[0]:sec[0] + C] += np.float32(S) * sign
    return dict(wf=img) if kind == FRAMES else dict(wc=img)


# ---- the mutants: 1 - 11 are what a wrong pass or merge would report, 12 and 13 what a wrong sequence would ----
MUTANTS = {
    1: 'padded joint rows, which hold z = bias, are summed with count 32',
    2: 'g\'s softmax runs over 32 columns, seen in c1..c3',
    3: 'dif at t = 0 takes the previous clip\'s last frame (input pass; frames passes)',
    4: 'the input pass takes dif\'s statistics over seg - 1 frames, leaving out the zero at t = 0',
    5: 'the convolution reads across the clip boundary',
    6: 'the halo at a 32-frame tile boundary reads as zero',
    7: 'the padded rows of the last tile are included in the sums',
    8: 'the last tile is merged with count 32',
    9: 'the between-group term of the merge is dropped: var = sum of M2 / n',
    10: 'groups are weighted equally in the mean',
    11: 'the variance is divided by n - 1',
    12: 'a later pass sees an earlier BatchNorm on its running statistics, not the batch\'s',
    13: 'the input statistics are not permuted from [v*3 + c] to the module\'s c*V + v',
}
PASS_MUTANTS = tuple(range(1, 12))
MODEL_MUTANTS = (12, 13)
MUTANT11_ROWS = 64


def applies(mutant, kind, case):
    """Whether ``mutant`` changes what pass ``kind`` reports on ``case`` = (V, seg, num_class, N) by an amount the bound can
    see.  The reasons where it does not:
      1, 2    V = 32: a frame tile has no padded joint row
      3, 5    N = 1: no previous clip (every case of the table has N >= 2)
      4       seg = 1: dif is the zero at t = 0 alone, there is nothing to leave out but everything
      6       seg <= 32: one tile, no tile boundary
      7, 8    seg % 32 = 0: the last tile is full
      9       the input pass at seg > 65: its groups are whole clips, whose means over seg standard-normal frames differ
              by about var (N - 1) / (N seg) -- at seg = 97 half a percent of a variance, under 100 bounds; every other
              pass of every case has it (each case has at least two groups)
      10      seg <= 32 or seg % 32 = 0: all groups of a clip pass have the same count (as those of the input and frames
              passes always have), and equal weights are then the right ones
      11      more than MUTANT11_ROWS rows: var / (n - 1) is then below 100 x 1e-4 max(1, max var); the tables of
              at most 64 rows keep the mutant in"""
    V, seg, _, N = case
    rows = N * seg * (V if kind == FRAMES else 1)
    return {1: kind == FRAMES and V < ROWS, 2: kind == FRAMES and V < ROWS, 3: kind != CLIP and N > 1,
            4: kind == INPUT and seg > 1, 5: kind == CLIP and N > 1, 6: kind == CLIP and seg > ROWS,
            7: kind == CLIP and seg % ROWS != 0, 8: kind == CLIP and seg % ROWS != 0, 9: kind != INPUT or seg <= 65,
            10: kind == CLIP and seg > ROWS and seg % ROWS != 0, 11: rows <= MUTANT11_ROWS}[mutant]


def mutant_stats(d, kind, layer, mutant):
    """What pass (kind, layer) and its finalize report on case ``d`` under ``mutant`` -> {tensor: fp64 array} with 'mean',
    'var' and, where the mutant acts inside the pass and keeps its groups, the partials 'sum' and 'm2'; the caller has
    asked ``applies``."""
    V, seg, _, N = d['case']
    z, counts = table(d, kind, layer)
    C = z.shape[1]

    def of_table(zm, cm):
        sums, m2s = group_ref(zm, cm)
        return dict(sum=sums, m2=m2s, mean=zm.mean(0), var=zm.var(0))

    if mutant == 1:
        sec = {n: (o, s) for n, o, s in du._sections(d['case'])[0]}[_BIAS[kind, layer]]
        b = d['wf'][sec[0]:sec[0] + C].double().numpy()
        zm = np.concatenate([z.reshape(N * seg, V, C), np.broadcast_to(b, (N * seg, ROWS - V, C))], axis=1).reshape(-1, C)
        return of_table(zm, [ROWS] * len(counts))
    if mutant in (2, 3):
        return of_table(*table(d, kind, layer, mutant=mutant))
    if mutant == 4:
        dif = z.reshape(N, seg, C)[:, 1:, C // 2:].reshape(-1, C // 2)
        return dict(mean=np.concatenate([z[:, :C // 2].mean(0), dif.mean(0)]), var=np.concatenate([z[:, :C // 2].var(0), dif.var(0)]))
    if mutant in (5, 6):
        return of_table(*table(d, kind, layer, mutant={5: 4, 6: 5}[mutant]))      # clip_ref's numbering
    if mutant == 7:
        zm, _ = table(d, kind, layer, mutant=6)
        return of_table(zm, [ROWS] * len(counts))
    sums, m2s = group_ref(z, counts)
    n = float(sum(counts))
    mean, var, _ = merge_ref(sums, m2s, counts)
    if mutant == 8:
        tiles = groups_per_clip(kind, seg)
        # the sums are what the kernel wrote; only the count the merge divides and weights by is wrong
        cnt = np.asarray([ROWS if g % tiles == tiles - 1 else c for g, c in enumerate(counts)], dtype=np.float64)[:, None]
        gm = sums / cnt
        m = (cnt * gm).sum(0) / cnt.sum()
        return dict(mean=m, var=(m2s.sum(0) + (cnt * np.square(gm - m)).sum(0)) / cnt.sum())
    if mutant == 9:
        return dict(mean=mean, var=m2s.sum(0) / n)
    if mutant == 10:
        cnt = np.asarray(counts, dtype=np.float64)[:, None]
        gm = sums / cnt
        m = gm.mean(0)
        return dict(mean=m, var=(m2s.sum(0) + (cnt * np.square(gm - m)).sum(0)) / n)
    if mutant == 11:
        return dict(mean=mean, var=var * n / (n - 1))
    raise ValueError(mutant)


def mutant_ratio(d, kind, layer, mutant):
    """The worst ratio of ``mutant`` over the tensors the GPU test compares (partials, mean, variance)."""
    z, counts = table(d, kind, layer)
    sums, m2s = group_ref(z, counts)
    ref = dict(sum=sums, m2=m2s, mean=z.mean(0), var=z.var(0))
    return max(check(v, ref[k]) for k, v in mutant_stats(d, kind, layer, mutant).items())


# ---- section 3: the finalize alone on seeded partials ----
# (kind, layer, N, seg, V, chunks of whole clips, recipe)
FINALIZE = ((INPUT, 0, 3, 5, 2, (2, 1), 'normal'),            # C = 12: a fraction of one 64-thread block
            (INPUT, 0, 2, 7, 32, (1, 1), 'normal'),           # C = 192: exactly three blocks
            (FRAMES, 1, 1, 1, 2, (1,), 'normal'),             # a single group
            (FRAMES, 3, 5, 20, 15, (2, 2, 1), 'centred50'),   # the badly centred recipe: |mean| / std = 50
            (CLIP, 2, 257, 33, 2, (128, 128, 1), 'normal'),   # 514 groups of 32 and 1 rows; 257 = 4 * 64 + 1
            (CLIP, 1, 2, 97, 2, (1, 1), 'normal'))            # four tiles per clip
FINALIZE_SEED = 52000


def finalize_ids():
    return [f'{i}-{PASS_NAMES[c[0], c[1]]}-n{c[2]}s{c[3]}v{c[4]}' for i, c in enumerate(FINALIZE)]


def finalize_inputs(i):
    """-> (part (groups, 2, C) fp32, counts, z or None).  'normal': standard-normal sums and |normal| M2s; 'centred50':
    the recipe of test_finalize_merge_on_badly_centred_data (|mean| = 50 std per channel) through ``group_partials``."""
    kind, layer, N, seg, V, _, recipe = FINALIZE[i]
    C, counts = channels(kind, layer, V), counts_of(kind, N, seg, V)
    rng = np.random.default_rng([FINALIZE_SEED, i])
    if recipe == 'normal':
        part = np.stack([rng.standard_normal((len(counts), C)), np.abs(rng.standard_normal((len(counts), C)))], axis=1)
        part = part.astype(np.float32)
        one = np.asarray(counts) == 1
        part[one, 1] = 0.0                                  # a group of one row has no spread
        return part, counts, None
    std = rng.uniform(0.5, 2.0, C)
    z = (50.0 * std * rng.choice([-1.0, 1.0], C) + std * rng.standard_normal((sum(counts), C))).astype(np.float32)
    sums, m2s = bu.group_partials(z, counts)
    return np.stack([sums, m2s], axis=1), counts, z


# ---- section 4: the seven passes through the model ----
# (V, seg, num_class, N)
MODEL_CASES = ((2, 1, 1, 8), (3, 2, 32, 4), (32, 2, 64, 4), (16, 31, 33, 2), (17, 33, 60, 2), (31, 32, 97, 2), (5, 65, 129, 2),
               (25, 64, 257, 2), (15, 20, 400, 5), (4, 97, 4096, 2))
# per case the first seed of 7100 + i, 7200 + i, ... at which the mean row maximum of the fp64 g lies inside
# ``du.rowmax_range(V)`` shrunk by 2 % at either end (cases 0, 1 and 9 moved on; the narrow range of two joints took 13 steps)
MODEL_SEEDS = (8400, 7301, 7102, 7103, 7104, 7105, 7106, 7107, 7108, 7209)
MODEL_GSCALE = 0.35
RECALIBRATED = (3, 4)              # seg 31 <= 32, seg 33 > 32


def search_model_seed(i, tries=40):
    """The rule behind ``MODEL_SEEDS[i]``: the first seed of 7100 + i + 100 k whose fp64 g keeps its mean row maximum inside
    the range shrunk by 2 % (None: none of ``tries``)."""
    import agcn_amd  # noqa: F401
    from agcn_amd.model.sgn import SGN
    V, seg, nc, N = MODEL_CASES[i]
    lo, hi = du.rowmax_range(V)
    m = SGN(num_class=nc, num_point=V, seg=seg).double().eval()
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    for seed in range(7100 + i, 7100 + i + 100 * tries, 100):
        m.load_state_dict(su.torch_state(su.sgn_state(shapes, seed, MODEL_GSCALE)))
        x = np.random.default_rng([seed, 9000]).standard_normal((N, seg, 3 * V)).astype(np.float32)
        with torch.no_grad():
            g = m._batch_statistics_tensor(torch.from_numpy(x).double())[1]
        if 1.02 * lo <= float(g.amax(-1).mean()) <= 0.98 * hi:
            return seed
    return None


def model_ids():
    return [f'{i}-j{c[0]}s{c[1]}c{c[2]}n{c[3]}' for i, c in enumerate(MODEL_CASES)]


def build_model(i):
    """-> (SGN in eval mode on the CPU in fp32 with the seeded state of case i, x (N, seg, 3V) fp32 standard normal)."""
    import agcn_amd  # noqa: F401
    from agcn_amd.model.sgn import SGN
    V, seg, nc, N = MODEL_CASES[i]
    m = SGN(num_class=nc, num_point=V, seg=seg)
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    m.load_state_dict(su.torch_state(su.sgn_state(shapes, MODEL_SEEDS[i], MODEL_GSCALE)))
    x = np.random.default_rng([MODEL_SEEDS[i], 9000]).standard_normal((N, seg, 3 * V)).astype(np.float32)
    return m.eval(), torch.from_numpy(x)


def composition(m, x, frozen=None, unpermuted=False):
    """``SGN._batch_statistics_tensor`` in the dtype of ``m`` -> (logits, g, {name: (mean, var, count)}).  The model
    mutants: ``frozen`` names a BatchNorm that stays on its running statistics (12); ``unpermuted`` hands the two input
    BatchNorms their batch statistics in the kernels' feature order [v*3 + c] as if that were the module's c*V + v (13)."""
    from agcn_amd import ops
    V = m.num_point
    with torch.no_grad():
        if frozen is None and not unpermuted:
            return m._batch_statistics_tensor(x)
        m = copy.deepcopy(m)
        names = (frozen,) if frozen else ops.SGN_BN_NAMES[:2]
        if unpermuted:
            _, _, right = m._batch_statistics_tensor(x)
            for n in names:
                bn = m.get_submodule(n)
                mean, var, _ = right[n]
                bn.running_mean.copy_(mean.reshape(3, V).t().reshape(-1))        # [v*3 + c], read as c*V + v
                bn.running_var.copy_(var.reshape(3, V).t().reshape(-1))
        # _batch_statistics_tensor flips every BatchNorm to batch mode: keep these on their running statistics
        keep = {n: m.get_submodule(n) for n in names}
        for bn in keep.values():
            bn.__class__ = _Frozen
        return m._batch_statistics_tensor(x)


class _Frozen(torch.nn.BatchNorm1d):
    """A BatchNorm that normalises by its running statistics whatever its flags say."""

    def forward(self, a):
        shape = [1, -1] + [1] * (a.dim() - 2)
        return ((a - self.running_mean.reshape(shape)) / torch.sqrt(self.running_var.reshape(shape) + self.eps)
                * self.weight.reshape(shape) + self.bias.reshape(shape))


def stats_ratios(stats, ref):
    """{'mean.<name>' / 'var.<name>': ratio} of a statistics dict against the fp64 one."""
    out = {}
    for n in ref:
        out['mean.' + n], out['var.' + n] = check(stats[n][0], ref[n][0]), check(stats[n][1], ref[n][1])
    return out


_MODELS = {}


def load_model(i):
    """Case i of ``MODEL_CASES``, built once: dict(m, x, ref = the fp64 composition (logits, g, stats))."""
    if i not in _MODELS:
        m, x = build_model(i)
        m64 = copy.deepcopy(m).double()
        _MODELS[i] = dict(m=m, x=x, m64=m64, ref=composition(m64, x.double()))
    return _MODELS[i]


def model_mutant_ratios(i):
    """-> {12: weakest ratio over the six BatchNorms that have one behind them, on the statistics of the next BatchNorm in
    dependency order, 13: the weaker of the reported input statistics left in [v*3 + c] order (on those) and of the fold
    fed unpermuted (on gcn1.bn's)}."""
    from agcn_amd import ops
    r = load_model(i)
    V = r['m'].num_point
    names, ref = ops.SGN_BN_NAMES, r['ref'][2]
    out12 = []
    for k in range(1, 6):
        frozen = names[k]
        _, _, st = composition(r['m64'], r['x'].double(), frozen=frozen)
        nxt = names[k + 1]
        out12.append(max(check(st[nxt][0], ref[nxt][0]), check(st[nxt][1], ref[nxt][1])))
    _, _, st = composition(r['m64'], r['x'].double(), frozen=names[0])
    out12.append(max(check(st[names[2]][0], ref[names[2]][0]), check(st[names[2]][1], ref[names[2]][1])))
    _, _, st = composition(r['m64'], r['x'].double(), unpermuted=True)
    fed = max(check(st[names[2]][0], ref[names[2]][0]), check(st[names[2]][1], ref[names[2]][1]))
    mean, var, _ = ref[names[0]]
    rep = max(check(mean.reshape(3, V).t().reshape(-1), mean), check(var.reshape(3, V).t().reshape(-1), var))
    return {12: min(out12), 13: min(fed, rep)}
