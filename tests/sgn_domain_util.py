"""Shared by tests/test_sgn_domain_cpu.py and tests/test_gpu_sgn_domain.py: the tables of geometries that walk the domain
of the base SGN kernels (csrc/sgn.hip, csrc/sgn_bwd.hip, csrc/sgn_wgrad.hip; domain: csrc/sgn_plan.h), a seeded recipe for
the two flat weight images (no model, no fixture), the calibration of the adjacency softmax, the fp64 reference split at
feat, its mutants, the margin condition of the gradient cases, and the numpy reductions of seeded tapes.

Which case of ``CASES`` (V, seg, num_class, N) reaches which code (F = sgn_frames_kernel, C = sgn_clip_kernel):

  0  (2, 1, 1, 3)       smallest of everything: 30 padded joint rows, dif zero everywhere, both conv halos are padding, one class
  1  (3, 2, 32, 2)      odd V; the dif term's clip boundary; fc over exactly 32 classes
  2  (16, 31, 33, 2)    half a joint tile; one frame short of a frame tile; one class into a second 32-wide column group
  3  (17, 32, 60, 2)    row 16; a full frame tile (no padded frame row); the deployed class count
  4  (31, 33, 97, 2)    one padded joint row at the tile's edge; a second frame tile of one row (its left halo is tile 0's
                        last row)
  5  (32, 64, 129, 2)   no padded joint row (Kg = 32); two full frame tiles
  6  (25, 65, 257, 2)   the NTU skeleton; a third frame tile of one row; the fc loop's second trip (classes >= 256)
  7  (15, 20, 400, 5)   the deployed skeleton and frame count on five clips
  8  (5, 97, 4096, 2)   four frame tiles; the class limit
  9  (32, 2, 64, 2)     no padded joint row on two-frame clips

The frames kernel is compared with the reference on x; the clip kernel is fed the REFERENCE's feat rounded to fp32 and
compared with the reference recomputed from that same input, so that each kernel answers for its own error only.  The
gradient kernels are held the same way (``FRAMES_GRAD``, ``CLIP_GRAD``), the taped route as a whole on ``WHOLE``, and the
weight-gradient reductions alone on tapes of standard-normal floats (``FRAMES_TAPES``, ``CLIP_TAPES``): they are linear in
their tapes.  What makes these inputs able to show an error is asserted in tests/test_sgn_domain_cpu.py.

The margin condition of the gradient cases is ``sgn_v15_grad_util``'s: a condition on the INPUTS, not a tolerance.  Every
x-dependent ReLU pre-activation (frames: the four embedding layers -- not the dif branch at t = 0, which does not depend on
x -- and gcn1..3; clip: cnn1 and cnn2) is at least MARGIN away from 0, and wherever top-1 > 0 the top-1 minus top-2 gap of
the maximum is at least MARGIN, with MARGIN = max(2e-5, 4 x the reference's own fp32-vs-fp64 distance on that tensor)."""
import math

import numpy as np
import torch

from tests import sgn_v15_domain_util as v15
from tests import sgn_v15_grad_util as v15g

ROWS = 32                    # joint rows of a frame tile and frame rows of a clip tile (SGN_VP)
TARGET_STD = v15.TARGET_STD  # of g1(x0) . g2(x0)^T after the calibration
MARGIN_FLOOR = v15g.MARGIN_FLOOR
MAX_SITES = v15g.MAX_SITES
WHOLE_SITES = 120000
SEARCH = v15g.SEARCH
SEARCH_HEADROOM = 1.5        # on the margins, when a seed is chosen
check = v15.check
rowmax_range = v15g.rowmax_range

# ---- the tables.  A case is (V, seg, num_class, N) everywhere. ----
CASES = ((2, 1, 1, 3), (3, 2, 32, 2), (16, 31, 33, 2), (17, 32, 60, 2), (31, 33, 97, 2), (32, 64, 129, 2), (25, 65, 257, 2),
         (15, 20, 400, 5), (5, 97, 4096, 2), (32, 2, 64, 2))
# the frames backward kernel alone: the clip image is not used (one class)
FRAMES_GRAD = tuple((V, seg, 1, N) for V, seg, N in (
    (2, 1, 2), (3, 2, 2), (16, 4, 1), (17, 3, 1), (31, 2, 1), (32, 2, 1), (2, 32, 1), (15, 4, 1), (25, 2, 1)))
# the clip backward kernel alone, on the feat of a five-joint skeleton
CLIP_V = 5
CLIP_GRAD = tuple((CLIP_V, seg, nc, N) for seg, nc, N in (
    (1, 1, 2), (2, 32, 2), (31, 33, 2), (32, 60, 2), (33, 97, 2), (64, 129, 1), (65, 257, 1), (20, 400, 3), (3, 4096, 2)))
WHOLE = ((32, 2, 33, 1), (17, 3, 129, 1), (3, 2, 4096, 2), (2, 33, 97, 1))
TABLES = dict(fwd=CASES, frames_grad=FRAMES_GRAD, clip_grad=CLIP_GRAD, whole=WHOLE)
# one seed per case: the first of BASE[table] + 100 * case + 1, + 2, ... at which the case meets ``conditions`` with 1.5 x
# the required margins (``search``)
BASE = dict(fwd=0, frames_grad=10000, clip_grad=20000, whole=30000)
SEEDS = dict(
    fwd=(4, 101, 201, 301, 401, 501, 601, 701, 801, 901),
    frames_grad=(10006, 10103, 10201, 10301, 10404, 10501, 10696, 10703, 10803),
    clip_grad=(20001, 20101, 20203, 20301, 20402, 20502, 20601, 20701, 20801),
    whole=(30011, 30106, 30201, 30358),
)
# {case: shift of c3_b}: a case whose padded-row mutant could not reach 100 bounds at any seed would get +1 here, as the
# v15_seg3_guard fixture does.  No case of these tables needed it.
C3B_SHIFT = {}


def ids(table):
    return [f'{i}-j{c[0]}s{c[1]}c{c[2]}n{c[3]}' for i, c in enumerate(TABLES[table])]


MUTANTS = {
    1: 'F padded joint rows, which hold relu(c3_b), are included in the maximum over the joints',
    2: 'F g\'s softmax runs over 32 columns, the padded ones included',
    3: 'F dif at t = 0 takes the previous clip\'s last frame',
    4: 'C the temporal convolution reads across the clip boundary',
    5: 'C the temporal convolution\'s halo at a 32-frame tile boundary reads as zero',
    6: 'C the frame maximum includes the padded rows of the last tile',
    7: 'C classes >= 256 are left out of fc',
    11: 'B the maxima are routed to the first index among the rows within 1.0 of the top',
    12: 'B the softmax backward lacks the row-sum term',
    13: 'B the dd[t + 1] -> x[t] coupling is dropped',
    14: 'B the convolution\'s backward halo at a tile boundary is dropped',
    15: 'B fc^T is truncated at 256 classes',
}
FORWARD_MUTANTS = (1, 2, 3, 4, 5, 6, 7)
BACKWARD_MUTANTS = (11, 12, 13, 14, 15)


def applies(mutant, side, case):
    """Whether ``mutant`` changes what ``side`` ('frames' / 'clip') computes on ``case``."""
    V, seg, nc, N = case
    if side == 'frames':
        return {1: V < ROWS, 2: V < ROWS, 3: N > 1, 11: True, 12: True, 13: seg > 1}.get(mutant, False)
    return {4: N > 1, 5: seg > ROWS, 6: seg % ROWS != 0, 7: nc > 256, 11: seg > 1, 14: seg > ROWS, 15: nc > 256}.get(mutant, False)


def frames_sites(case):
    V, seg, _, N = case
    return N * V * (seg * 896 - 128)          # 4 x 64 + 128 + 256 + 256 per joint row, less the dif branch at t = 0


def clip_sites(case):
    return case[3] * case[1] * 768


# ---- the seeded images ----
def _sections(case):
    from agcn_amd import ops
    return ops.sgn_image_sections(case[0], case[1], case[2])


def _views(img, secs):
    return {n: img[o:o + math.prod(s)].reshape(s) for n, o, s in secs}


def seeded_images(case, seed):
    """-> (x (N, seg, 3V), frames image, clip image) as fp32 numpy arrays; section i (counted through both images) and x
    each draw from a generator of their own."""
    V, seg, _, N = case
    images, i = [], 0
    for secs in _sections(case):
        img = np.zeros(secs[-1][1] + math.prod(secs[-1][2]), dtype=np.float32)
        for name, off, shape in secs:
            rng = np.random.default_rng([int(seed), i])
            i += 1
            if name == 'aff':                           # (4, V, 3): scale, shift of the position; scale, shift of the velocity
                v = np.stack([rng.uniform(0.5, 1.5, shape[1:]), 0.2 * rng.standard_normal(shape[1:]),
                              rng.uniform(0.5, 1.5, shape[1:]), 0.2 * rng.standard_normal(shape[1:])])
            elif name in ('spa1', 'tem1'):
                v = 0.5 * rng.standard_normal(shape)
            elif name.endswith('_b'):
                v = 0.1 * rng.standard_normal(shape) + (C3B_SHIFT.get(case, 0.0) if name == 'c3_b' else 0.0)
            else:                                       # a (K, N) matrix
                v = math.sqrt(2.0 / shape[0]) * rng.standard_normal(shape)
            img[off:off + math.prod(shape)] = v.astype(np.float32).reshape(-1)
        images.append(img)
    x = np.random.default_rng([int(seed), i]).standard_normal((N, seg, 3 * V)).astype(np.float32)
    return x, images[0], images[1]


def transposed(wf, wc, case):
    """The two images of the backward from the flat forward images, through the model's own ``SGN._transposed``."""
    from agcn_amd.model.sgn import SGN
    fs, cs = _sections(case)
    f, c = _views(wf, fs), _views(wc, cs)
    frames = list(f['aff']) + [f[n] for n, _, _ in fs[1:]]
    # the folded list holds cnn1 as (tap, in, out); the image section is its (3 * 256, 256) view
    return SGN._transposed(frames, [c[n].reshape(3, 256, 256) if n == 't1_w' else c[n] for n, _, _ in cs])


# ---- the reference, split at feat, with the mutants.  mutant = 0 is ops.sgn_image_forward_ref operation for operation
# (the CPU test asserts equal bits in fp64).  The backward mutants (11 - 15) leave every value as it is and change what
# autograd sends back. ----
class _SoftmaxNoRowsum(torch.autograd.Function):
    @staticmethod
    def forward(ctx, s):
        a = torch.softmax(s, dim=-1)
        ctx.save_for_backward(a)
        return a

    @staticmethod
    def backward(ctx, da):
        a, = ctx.saved_tensors
        return a * da


def _pool(y, dim, mutant):
    """The maximum of y over ``dim``; mutant 11 picks the first row within 1.0 of the top instead."""
    if mutant != 11:
        return y.amax(dim)
    R = y.shape[dim]
    near = y.detach() >= y.detach().amax(dim, keepdim=True) - 1.0
    order = torch.arange(R, 0, -1).reshape([R if d == dim else 1 for d in range(y.dim())])
    return y.gather(dim, (near * order).argmax(dim, keepdim=True)).squeeze(dim)


def frames_ref(x, wf, case, mutant=0):
    """-> dict(feat (N, seg, 256) without tem1, as ``ops.sgn_frames`` returns it, g (N, seg, V, V), pre {layer: ReLU
    pre-activation}, y = gcn3's output (N, seg, V, 256))."""
    V, seg = case[0], case[1]
    f = _views(wf, _sections(case)[0])
    relu = torch.relu
    N = x.shape[0]
    xr = x.reshape(N, seg, V, 3)
    dif = torch.cat([xr.new_zeros(N, 1, V, 3), xr[:, 1:] - (xr[:, :-1].detach() if mutant == 13 else xr[:, :-1])], dim=1)
    if mutant == 3:
        flat = xr.reshape(N * seg, V, 3)
        dif = torch.cat([flat.new_zeros(1, V, 3), flat[1:] - flat[:-1]]).reshape(N, seg, V, 3)
    pre = {}

    def emb(v, p):
        pre[p + '1'] = v @ f[p + '1_w'] + f[p + '1_b']
        pre[p + '2'] = relu(pre[p + '1']) @ f[p + '2_w'] + f[p + '2_b']
        return relu(pre[p + '2'])

    dy = emb(xr * f['aff'][0] + f['aff'][1], 'je') + emb(dif * f['aff'][2] + f['aff'][3], 'de')
    h = torch.cat([dy, f['spa1'].expand(N, seg, V, 64)], dim=3)
    gg = h @ f['g_w'] + f['g_b']
    s = gg[..., :256] @ gg[..., 256:].transpose(-1, -2)
    if mutant == 2:                                     # a padded row of x0 is zero: its g2 is the bias
        pad = (gg[..., :256] @ f['g_b'][256:])[..., None].expand(N, seg, V, ROWS - V)
        g = torch.softmax(torch.cat([s, pad], dim=-1), dim=-1)[..., :V]
    elif mutant == 12:
        g = _SoftmaxNoRowsum.apply(s)
    else:
        g = torch.softmax(s, dim=-1)
    for l in ('c1', 'c2', 'c3'):
        pre[l] = torch.cat([g @ h, h], dim=3) @ f[l + '_w'] + f[l + '_b']
        h = relu(pre[l])
    feat = _pool(h, 2, mutant)
    if mutant == 1 and V < ROWS:
        feat = torch.maximum(feat, relu(f['c3_b']).expand_as(feat))
    return dict(feat=feat, g=g, pre=pre, y=h)


def clip_ref(feat, wc, case, mutant=0):
    """feat (N, seg, 256) -> dict(logits (N, num_class), pooled (N, 512), pre {layer: ReLU pre-activation}, y = cnn2's
    output (N, seg, 512))."""
    seg = case[1]
    c = _views(wc, _sections(case)[1])
    relu = torch.relu
    N = feat.shape[0]
    H = feat + c['tem1']
    rows = seg
    if mutant == 6:                                     # the padded rows of the last tile are zero rows of H
        rows = (seg + ROWS - 1) // ROWS * ROWS
        H = torch.cat([H, H.new_zeros(N, rows - seg, 256)], dim=1)
    Hp = torch.nn.functional.pad(H, (0, 0, 1, 1))
    taps = [Hp[:, dt:dt + rows] for dt in range(3)]
    if mutant == 4:
        Fp = torch.nn.functional.pad(H.reshape(N * seg, 256), (0, 0, 1, 1))
        taps = [Fp[dt:dt + N * seg].reshape(N, seg, 256) for dt in range(3)]
    if mutant in (5, 14):                               # the left halo of a tile's first row, the right one of its last row
        t = torch.arange(rows)
        for dt, edge in ((0, 0), (2, ROWS - 1)):
            inner = (t % ROWS != edge).to(H.dtype)[None, :, None]
            taps[dt] = taps[dt] * inner if mutant == 5 else taps[dt] * inner + taps[dt].detach() * (1 - inner)
    taps = torch.cat(taps, dim=2)
    pre = {'t1': taps @ c['t1_w'] + c['t1_b']}
    pre['t2'] = relu(pre['t1']) @ c['t2_w'] + c['t2_b']
    y2 = relu(pre['t2'])
    pooled = _pool(y2, 1, mutant)
    if mutant == 15:
        logits = torch.cat([pooled @ c['fc_w'][:, :256], pooled.detach() @ c['fc_w'][:, 256:]], dim=1) + c['fc_b']
    else:
        logits = pooled @ c['fc_w'] + c['fc_b']
    if mutant == 7:
        logits = torch.cat([logits[:, :256], torch.zeros_like(logits[:, 256:])], dim=1)
    return dict(logits=logits, pooled=pooled, pre=pre, y=y2)


# ---- calibration ----
def calibrate(wf, x, case):
    """Scale g_w and g_b in the fp32 image ``wf`` (in place) by sqrt(TARGET_STD / std) so that std(g1(x0) . g2(x0)^T)
    over the frames of x is TARGET_STD (in fp64, from the image alone) -> the factor on the product."""
    V, seg = case[0], case[1]
    secs = _sections(case)[0]
    with torch.no_grad():
        x64 = torch.from_numpy(x).double()
        f = {n: torch.from_numpy(v).double() for n, v in _views(wf, secs).items()}
        N = x64.shape[0]
        xr = x64.reshape(N, seg, V, 3)
        dif = torch.cat([xr.new_zeros(N, 1, V, 3), xr[:, 1:] - xr[:, :-1]], dim=1)
        emb = lambda v, p: torch.relu(torch.relu(v @ f[p + '1_w'] + f[p + '1_b']) @ f[p + '2_w'] + f[p + '2_b'])  # noqa: E731
        x0 = torch.cat([emb(xr * f['aff'][0] + f['aff'][1], 'je') + emb(dif * f['aff'][2] + f['aff'][3], 'de'),
                        f['spa1'].expand(N, seg, V, 64)], dim=3)
        gg = x0 @ f['g_w'] + f['g_b']
        factor = TARGET_STD / float((gg[..., :256] @ gg[..., 256:].transpose(-1, -2)).std())
    v = _views(wf, secs)
    for n in ('g_w', 'g_b'):
        v[n][...] = (v[n].astype(np.float64) * math.sqrt(factor)).astype(np.float32)
    return factor


# ---- the margin condition ----
def _gap(y, dim):
    """The smallest top-1 minus top-2 gap of the maxima of y over ``dim`` among the columns whose top-1 is > 0 (inf: none,
    or a single row)."""
    if y.shape[dim] < 2:
        return math.inf
    top = y.topk(2, dim=dim).values
    a, b = top.select(dim, 0), top.select(dim, 1)
    live = a > 0
    return float((a - b)[live].min()) if bool(live.any()) else math.inf


def margins(side, inp32, img32, case):
    """-> {tensor: (margin required, smallest distance found, the reference's fp32-vs-fp64 distance)}: the margin condition
    of ``side`` holds iff found >= required for every tensor."""
    ref = frames_ref if side == 'frames' else clip_ref
    with torch.no_grad():
        r64, r32 = ref(inp32.double(), img32.double(), case), ref(inp32, img32, case)
    out = {}
    for name, v in r64['pre'].items():
        w = r32['pre'][name]
        if name.startswith('de'):                       # the dif branch at t = 0 does not depend on x
            v, w = v[:, 1:], w[:, 1:]
        if v.numel():
            dist = float((w.double() - v).abs().max())
            out[name] = (max(MARGIN_FLOOR, 4 * dist), float(v.abs().min()), dist)
    dist = float((r32['y'].double() - r64['y']).abs().max())
    out['max_gap'] = (max(MARGIN_FLOOR, 4 * dist), _gap(r64['y'], 2 if side == 'frames' else 1), dist)
    return out


# ---- the reference gradients: autograd through the reference ----
def frames_grad(x, wf, dfeat, case, mutant=0):
    """d sum(feat * dfeat) / dx through ``frames_ref`` in the dtype of x."""
    with torch.enable_grad():
        xg = x.detach().clone().requires_grad_(True)
        g, = torch.autograd.grad((frames_ref(xg, wf, case, mutant)['feat'] * dfeat).sum(), xg)
    return g


def clip_grad(feat, wc, dlogits, case, mutant=0):
    """d sum(logits * dlogits) / dfeat through ``clip_ref`` in the dtype of feat."""
    with torch.enable_grad():
        fg = feat.detach().clone().requires_grad_(True)
        g, = torch.autograd.grad((clip_ref(fg, wc, case, mutant)['logits'] * dlogits).sum(), fg)
    return g


def whole_grads(x, wf, wc, cot, case):
    """(dx, d_wf, d_wc) of sum(logits * cot) through ``ops.sgn_image_forward_ref`` in the dtype of x."""
    from agcn_amd import ops
    with torch.enable_grad():
        leaves = [t.detach().clone().requires_grad_(True) for t in (x, wf, wc)]
        logits, _ = ops.sgn_image_forward_ref(*leaves, *case[:3])
        return torch.autograd.grad((logits * cot).sum(), leaves)


def section_maxima(d_wf, d_wc, case):
    """{section: max |gradient|} over both images."""
    out = {}
    for img, secs in zip((d_wf, d_wc), _sections(case)):
        for n, o, s in secs:
            out[n] = float(img[o:o + math.prod(s)].abs().max())
    return out


# ---- one case ----
def make(table, case, seed):
    """The calibrated inputs and the fp64 references of one case of ``table``, from the seed and the reference alone ->
    dict of x, wf, wc, feat32 (the reference's feat rounded) as fp32 tensors, frames / clip = ``frames_ref`` on x /
    ``clip_ref`` on feat32 in fp64, and per table: 'fwd' logits, g = ``ops.sgn_image_forward_ref``; the gradient tables
    dfeat_in, dlogits seeded ~ N(0, 1) and dx64 / dfeat64; 'whole' cot (a power of two times N(0, 1)) and dx64, d_wf64,
    d_wc64."""
    from agcn_amd import ops
    V, seg, nc, N = case
    x, wf, wc = seeded_images(case, seed)
    factor = calibrate(wf, x, case)
    x, wf, wc = torch.from_numpy(x), torch.from_numpy(wf), torch.from_numpy(wc)
    d = dict(table=table, case=case, seed=seed, factor=factor, x=x, wf=wf, wc=wc)
    with torch.no_grad():
        d['frames'] = frames_ref(x.double(), wf.double(), case)
        d['feat32'] = d['frames']['feat'].float()
        d['clip'] = clip_ref(d['feat32'].double(), wc.double(), case)
        if table == 'fwd':
            d['logits'], d['g'] = ops.sgn_image_forward_ref(x.double(), wf.double(), wc.double(), V, seg, nc)
    rng = np.random.default_rng([int(seed), 1000])
    d['dfeat_in'] = torch.from_numpy(rng.standard_normal((N, seg, 256)).astype(np.float32))
    d['dlogits'] = torch.from_numpy(rng.standard_normal((N, nc)).astype(np.float32))
    if table == 'frames_grad':
        d['dx64'] = frames_grad(x.double(), wf.double(), d['dfeat_in'].double(), case)
    if table == 'clip_grad':
        d['dfeat64'] = clip_grad(d['feat32'].double(), wc.double(), d['dlogits'].double(), case)
    if table == 'whole':
        # the cotangent is scaled by a power of two so that every section's reference maximum is at least 1: the bound
        # 1e-4 max(1, max|ref|) is then relative on every section
        g = whole_grads(x.double(), wf.double(), wc.double(), d['dlogits'].double(), case)
        low = min(section_maxima(g[1], g[2], case).values())
        d['cot_scale'] = 2.0 ** max(0, math.ceil(-math.log2(low)))
        d['cot'] = d['dlogits'] * d['cot_scale']
        d['dx64'], d['d_wf64'], d['d_wc64'] = (t * d['cot_scale'] for t in g)
    return d


def forward_mutant_ratios(d, mutant):
    """The ratio per compared tensor of a forward mutant, on the inputs the GPU test uses ({}: it does not apply)."""
    case, out = d['case'], {}
    with torch.no_grad():
        if applies(mutant, 'frames', case):
            m = frames_ref(d['x'].double(), d['wf'].double(), case, mutant)
            out.update(feat=check(m['feat'], d['frames']['feat']), g=check(m['g'], d['frames']['g']))
        if applies(mutant, 'clip', case):
            out.update(logits=check(clip_ref(d['feat32'].double(), d['wc'].double(), case, mutant)['logits'], d['clip']['logits']))
    return out


def conditions(d, headroom=1.0):
    """Everything the CPU test asserts about a made case that a seed can miss -> (ok, report).  ``headroom``: the factor on
    the required margins (``search`` asks for 1.5 of what the test asserts, so that another BLAS's fp32 summation order,
    which moves the reference's fp32-vs-fp64 distance a little, does not unseat a stored seed)."""
    table, case = d['table'], d['case']
    V, seg, nc, N = case
    rep, ok = {}, True
    lo, hi = rowmax_range(V)
    rep['rowmax'] = float(d['frames']['g'].amax(-1).mean())
    ok = ok and lo <= rep['rowmax'] <= hi
    x, wf, wc, f32 = d['x'], d['wf'], d['wc'], d['feat32']
    if table == 'fwd':
        from agcn_amd import ops
        with torch.no_grad():
            logits, g = ops.sgn_image_forward_ref(x, wf, wc, V, seg, nc)
            fr, cl = frames_ref(x, wf, case), clip_ref(f32, wc, case)
        rep['fp32'] = dict(feat=check(fr['feat'], d['frames']['feat']), g=check(g, d['g']), chained_logits=check(logits, d['logits']),
                           logits=check(cl['logits'], d['clip']['logits']))
        ok = ok and max(rep['fp32'].values()) <= 0.1
        for mu in FORWARD_MUTANTS:
            r = forward_mutant_ratios(d, mu)
            if r:
                rep[f'mutant{mu}'] = max(r.values())
                ok = ok and rep[f'mutant{mu}'] >= 100
        return ok, rep
    sides = dict(frames_grad=('frames',), clip_grad=('clip',), whole=('frames', 'clip'))[table]
    for side in sides:
        m = margins(side, x if side == 'frames' else f32, wf if side == 'frames' else wc, case)
        rep[side + '_margins'] = m
        ok = ok and all(found >= headroom * need for need, found, _ in m.values())
    if table == 'frames_grad':
        rep['fp32'] = check(frames_grad(x, wf, d['dfeat_in'], case), d['dx64'])
        for mu in BACKWARD_MUTANTS:
            if applies(mu, 'frames', case):
                rep[f'mutant{mu}'] = check(frames_grad(x.double(), wf.double(), d['dfeat_in'].double(), case, mu), d['dx64'])
    elif table == 'clip_grad':
        rep['fp32'] = check(clip_grad(f32, wc, d['dlogits'], case), d['dfeat64'])
        for mu in BACKWARD_MUTANTS:
            if applies(mu, 'clip', case):
                rep[f'mutant{mu}'] = check(clip_grad(f32.double(), wc.double(), d['dlogits'].double(), case, mu), d['dfeat64'])
    else:
        g32 = whole_grads(x, wf, wc, d['cot'], case)
        rep['fp32'] = max(check(g32[0], d['dx64']), whole_section_ratios(g32[1], g32[2], d)[0])
        rep['section_min'] = min(section_maxima(d['d_wf64'], d['d_wc64'], case).values())
        ok = ok and rep['section_min'] >= 1.0
    ok = ok and rep['fp32'] <= 0.1 and all(v >= 100 for k, v in rep.items() if k.startswith('mutant'))
    return ok, rep


def whole_section_ratios(d_wf, d_wc, d):
    """The image gradients against the fp64 ones of a 'whole' case, section by section -> (worst ratio, {section: ratio})."""
    out = {}
    for got, ref, secs in zip((d_wf, d_wc), (d['d_wf64'], d['d_wc64']), _sections(d['case'])):
        assert got.shape == ref.shape
        for n, o, s in secs:
            out[n] = check(got[o:o + math.prod(s)], ref[o:o + math.prod(s)])
    return max(out.values()), out


_MADE = {}


def load(table, i):
    """Case i of ``table`` at its seed, made once and never modified by a test."""
    if (table, i) not in _MADE:
        _MADE[table, i] = make(table, TABLES[table][i], SEEDS[table][i])
    return _MADE[table, i]


def search(table, i, tries=SEARCH):
    """The first seed of BASE[table] + 100 * i + 1, ... at which the case meets ``conditions`` with SEARCH_HEADROOM on its
    margins (None: none of ``tries``)."""
    first = BASE[table] + 100 * i + 1
    for seed in range(first, first + tries):
        ok, rep = conditions(make(table, TABLES[table][i], seed), headroom=SEARCH_HEADROOM)
        if ok:
            return seed, rep
    return None, rep


# ---- the weight-gradient reductions on seeded tapes (csrc/sgn_wgrad_plan.h) ----
# (V, seg, N, rows_per_split): R = N * seg * V joint rows
FRAMES_TAPES = ((2, 1, 1, 0),        # R = 2
                (3, 1, 1, 0),        # R = 3: an odd last row
                (32, 8, 1, 0),       # R = 256: exactly one split
                (2, 43, 3, 0),       # R = 258: 256 + 2
                (5, 17, 3, 0),       # R = 255
                (31, 19, 14, 0),     # R = 8246 > 8192: 32 splits of 258 rows, the last of 248; 266 frames: 256 + 10
                (25, 20, 2, 7),      # 143 splits of 7 rows, the last of 6
                (15, 20, 5, 32))     # 47 splits of 32 rows, the last of 28
# (seg, num_class, N, rows_per_split): R = N * seg frames
CLIP_TAPES = ((1, 1, 257, 0),        # R = 257: 256 + 1; tap groups of one row; 257 clips split tem1, fc_w, fc_b; the <1> strip
              (33, 33, 9, 0),        # R = 297: the split boundary falls inside a clip; the <2> strip with a tail
              (32, 97, 8, 0),        # R = 256; the <4> strip with a guarded tail
              (20, 60, 64, 0),       # R = 1280: five splits, a training batch
              (65, 129, 130, 0),     # R = 8450: the 32-split cap (266 rows, the last of 204); a second strip of one column
              (2, 4096, 2, 0),       # the class limit
              (3, 31, 5, 7),         # forced odd splits
              (64, 257, 3, 32))
TAPE_SEED = 41000
FT = dict(gx3=0, x2=256, dz3=512, gx2=768, x1=896, dz2=1024, gx1=1280, x0=1408, dz1=1536, dg=1664, e1=2176, de2=2304,
          de1=2432, dspa=2560, xn=2624, dxn=2632, cols=2656)          # SgnFramesTape
REDUCTION_MUTANTS = {
    1: 'the last odd row of a split is dropped',
    2: 'the last partial column tile of fc_w is zero',
    3: 'splits beyond the 32nd are dropped',
    4: 'tap dt reads H with group stride seg instead of seg + 2',
    5: 'aff\'s dif at t = 0 uses the previous frame',
}


def split_rows(R, rows_per_split):
    """Rows per split: the forced count, else ceil(R / 32) rounded up to even and at least 256."""
    if rows_per_split > 0:
        return rows_per_split
    return max(256, (-(-R // 32) + 1) & ~1)


def splits(R, rows_per_split):
    return max(1, -(-R // split_rows(R, rows_per_split)))


def reduction_applies(mutant, side, case):
    a, b, N, rps = case
    if side == 'frames':
        V, seg = a, b
        Rs = (N * seg * V, N * seg)
        return {1: any(_odd_split(R, rps) for R in Rs[:1]), 3: any(splits(R, rps) > 32 for R in Rs), 5: N > 1}.get(mutant, False)
    seg, nc = a, b
    Rs = (N * seg, N)
    return {1: any(_odd_split(R, rps) for R in Rs), 2: nc % 32 != 0, 3: any(splits(R, rps) > 32 for R in Rs),
            4: N > 1}.get(mutant, False)


def _odd_split(R, rps):
    rows = split_rows(R, rps)
    return rows % 2 == 1 or R % rows % 2 == 1


def _keep(R, rps, mutant):
    """The rows of a reduction over R rows that mutants 1 and 3 leave in the sum -> a boolean mask."""
    keep = np.ones(R, dtype=bool)
    rows = split_rows(R, rps)
    if mutant == 1:
        for b in range(0, R, rows):
            e = min(R, b + rows)
            if (e - b) % 2:
                keep[e - 1] = False
    if mutant == 3:
        keep[32 * rows:] = False
    return keep


def frames_tape_inputs(case, seed=TAPE_SEED):
    """-> (x (N, seg, 3V), tape (N * seg * V, 2656)) of standard-normal floats."""
    V, seg, N, _ = case
    rng = np.random.default_rng([seed, V, seg, N])
    return (rng.standard_normal((N, seg, 3 * V), dtype=np.float32),
            rng.standard_normal((N * seg * V, FT['cols']), dtype=np.float32))


def frames_tape_ref(x, tape, case, mutant=0, dtype=np.float64):
    """The gradient of the frames image from a frames tape in ``dtype``, taken from the documented layout -> {section:
    array}.  Mutants 1 and 3 act on the matrix products and column sums over the joint rows (and 3 on the per-frame
    sections)."""
    V, seg, N, rps = case
    R = N * seg * V
    t = tape.astype(dtype)
    k = _keep(R, rps, mutant)[:, None]
    col = lambda name, w, o=0: t[:, FT[name] + o:FT[name] + o + w]  # noqa: E731
    mm = lambda X, Z: (X * k).T @ Z                                  # noqa: E731
    out = {'c3_w': mm(col('gx3', 512), col('dz3', 256)), 'c3_b': (col('dz3', 256) * k).sum(0),
           'c2_w': mm(col('gx2', 256), col('dz2', 256)), 'c2_b': (col('dz2', 256) * k).sum(0),
           'c1_w': mm(col('gx1', 256), col('dz1', 128)), 'c1_b': (col('dz1', 128) * k).sum(0),
           'g_w': mm(col('x0', 128), col('dg', 512)), 'g_b': (col('dg', 512) * k).sum(0)}
    for p, o, xo in (('je', 0, 0), ('de', 64, 4)):
        out[p + '2_w'] = mm(col('e1', 64, o), col('de2', 64, o))
        out[p + '2_b'] = (col('de2', 64, o) * k).sum(0)
        out[p + '1_w'] = mm(col('xn', 3, xo), col('de1', 64, o))
        out[p + '1_b'] = (col('de1', 64, o) * k).sum(0)
    kf = _keep(N * seg, rps, 3 if mutant == 3 else 0)[:, None, None]          # the per-frame sections split over the frames
    out['spa1'] = (col('dspa', 64).reshape(N * seg, V, 64) * kf).sum(0)
    xr = x.astype(dtype).reshape(N, seg, V, 3)
    dif = np.concatenate([np.zeros((N, 1, V, 3), dtype), xr[:, 1:] - xr[:, :-1]], axis=1)
    if mutant == 5:
        flat = xr.reshape(N * seg, V, 3)
        dif = np.concatenate([np.zeros((1, V, 3), dtype), flat[1:] - flat[:-1]]).reshape(N, seg, V, 3)
    dxn = col('dxn', 6).reshape(N * seg, V, 6) * kf
    dj, dd = dxn[..., :3], dxn[..., 3:]
    out['aff'] = np.stack([(dj * xr.reshape(N * seg, V, 3)).sum(0), dj.sum(0), (dd * dif.reshape(N * seg, V, 3)).sum(0), dd.sum(0)])
    return out


def clip_tape_inputs(case, seed=TAPE_SEED):
    """-> (tape {h (N (seg + 2), 256), y1, dy1 (N seg, 256), dy2 (N seg, 512), ymax (N, 512)}, dfeat (N, seg, 256),
    dlogits (N, num_class)) of standard-normal floats; the flat tape is the five matrices one after the other."""
    seg, nc, N, _ = case
    rng = np.random.default_rng([seed, seg, nc, N])
    n = lambda *s: rng.standard_normal(s, dtype=np.float32)          # noqa: E731
    tape = dict(h=n(N * (seg + 2), 256), y1=n(N * seg, 256), dy1=n(N * seg, 256), dy2=n(N * seg, 512), ymax=n(N, 512))
    return tape, n(N, seg, 256), n(N, nc)


def clip_tape_ref(tape, dfeat, dlogits, case, mutant=0, dtype=np.float64):
    """The gradient of the clip image from a clip tape in ``dtype`` -> {section: array}."""
    seg, nc, N, rps = case
    R = N * seg
    t = {n: v.astype(dtype) for n, v in tape.items()}
    dfeat, dlogits = dfeat.astype(dtype), dlogits.astype(dtype)
    k = _keep(R, rps, mutant)[:, None]
    kn = _keep(N, rps, mutant)[:, None]
    r = np.arange(R)
    stride = seg if mutant == 4 else seg + 2
    t1 = [(t['h'][r // seg * stride + r % seg + dt] * k).T @ t['dy1'] for dt in range(3)]
    fc_w = (t['ymax'] * kn).T @ dlogits
    if mutant == 2 and nc % 32:
        fc_w[:, nc // 32 * 32:] = 0
    return {'tem1': (dfeat * kn[:, :, None]).sum(0), 't1_w': np.concatenate(t1), 't1_b': (t['dy1'] * k).sum(0),
            't2_w': (t['y1'] * k).T @ t['dy2'], 't2_b': (t['dy2'] * k).sum(0), 'fc_w': fc_w,
            'fc_b': (dlogits * kn).sum(0)}


def reduction_ratios(got, ref):
    """{section: ratio}; ``got`` is a flat image in the layout ``secs`` or a {section: array} dict."""
    return {n: check(np.asarray(got[n]).reshape(ref[n].shape), ref[n]) for n in ref}


def image_dict(img, secs):
    """A flat image (tensor or array) -> {section: array}."""
    img = img.detach().cpu().numpy() if torch.is_tensor(img) else img
    return {n: img[o:o + math.prod(s)].reshape(s) for n, o, s in secs}


if __name__ == '__main__':
    import sys
    import agcn_amd  # noqa: F401
    for table in (sys.argv[1:] or TABLES):
        found = []
        for i in range(len(TABLES[table])):
            seed, rep = search(table, i)
            found.append(seed)
            print(table, i, TABLES[table][i], seed, {k: (v if not isinstance(v, dict) else {
                n: (tuple(f'{e:.2e}' for e in t) if isinstance(t, tuple) else f'{t:.2e}') for n, t in v.items()})
                for k, v in rep.items()}, flush=True)
        print(table, 'SEEDS', tuple(found), flush=True)
