"""Shared by tests/test_sgn_v15_wgrad_cpu.py, tests/test_gpu_sgn_v15_wgrad.py and
tests/golden/make_golden_sgn_v15_paramgrad.py: the fp64 reference of the SGN v15 IMAGE gradients (the gradient of a loss on
the logits with respect to the two folded weight images, csrc/sgn_v15_wgrad.hip), a hand-written weight gradient of the
block that carries the mutants, and the whole-model fixture's format.

The cases, seeds and inputs are those of tests/sgn_v15_grad_util.py (``CASES``, ``SEEDS``, ``load``): the clip side is fed
the reference's feat rounded to fp32 and a seeded d logits, the frames side x and a seeded d feat, so each kernel answers
for its own error only.  Their ReLU and maximum margins are asserted in tests/test_sgn_v15_grad_cpu.py, and a weight
gradient switches at the same sites as the input gradient.

Reference: torch autograd through ``du.frames_ref`` / ``du.clip_ref`` with the image as the leaf.  Bound: the project's
fp32 rule per tensor (``du.check``), here per SECTION of an image."""
import json
import math

import numpy as np
import torch

from tests import sgn_v15_domain_util as du
from tests import sgn_v15_grad_util as gu
from tests import sgn_v15_util as vu
from tests import sgn_wgrad_util as wu

MUTANTS = {
    1: 'dk columns missing from d qkv_w',
    2: 'd_head 16: the odd head\'s dv taken with the even head\'s P',
    3: 'the Wr half of d f2_w dropped',
    4: 'the last FFN chunk dropped from d f1_w',
    5: 'the last 128-column slice of o dropped from d o_w',
    6: 'a bias taken over padded rows too: 32 rows of the packed tape per token set, into the next set\'s rows',
    7: 'd spa from the first frame only',
    8: 'd tem from the first clip only',
}
# the section a mutant touches, without the block's prefix
MUTANT_SECTION = {1: 'qkv_w', 2: 'qkv_w', 3: 'f2_w', 4: 'f1_w', 5: 'o_w', 6: 'f2_b', 7: 'spa', 8: 'tem'}


def applies(mutant, side, sets, rows, geometry):
    """Whether ``mutant`` changes the image gradient of ``side`` ('frames' / 'clip') with ``sets`` token sets of ``rows``
    rows and the block ``geometry``.  One row: dS = 0, so dk = 0 already (1) and both heads of a pair hold the map [1]
    (2).  One 128-column slice of o is all of o (5).  Mutant 6 needs a padded row and a following token set."""
    heads, d_head, ff = geometry
    return {1: rows > 1, 2: d_head == 16 and rows > 1, 3: True, 4: ff >= 256, 5: heads * d_head >= 256,
            6: rows < du.ROWS and sets > 1, 7: side == 'frames' and sets > 1, 8: side == 'clip' and sets > 1}[mutant]


def sections(case):
    """(frames, clip) sections of the images of a six-field case of sgn_v15_grad_util."""
    return du._sections(gu.dcase(case))


def views(img, secs):
    return {n: img[o:o + math.prod(s)].reshape(s) for n, o, s in secs}


# ---- the reference: autograd with the image as the leaf ----
def frames_wgrad(x, wf, dfeat, case):
    """d sum(feat * dfeat) / d wf through ``du.frames_ref`` in the dtype of the inputs."""
    with torch.enable_grad():
        w = wf.detach().clone().requires_grad_(True)
        g, = torch.autograd.grad((du.frames_ref(x, w, gu.dcase(case))['feat'] * dfeat).sum(), w)
    return g


def clip_wgrad(feat, wc, dlogits, case):
    """d sum(logits * dlogits) / d wc through ``du.clip_ref`` in the dtype of the inputs."""
    with torch.enable_grad():
        w = wc.detach().clone().requires_grad_(True)
        g, = torch.autograd.grad((du.clip_ref(feat, w, gu.dcase(case))['logits'] * dlogits).sum(), w)
    return g


# one seed per case: sgn_v15_grad_util's where every mutant of this module that applies reaches 100 bounds there (cases 2
# and 9); otherwise the first seed of 100 * case + 1, ... + SEARCH that meets ``margin_conditions`` AND ``conditions``
# below.  What misses at sgn_v15_grad_util's seeds is mutant 1: dk = dS^T q carries the d_head^-1/2 folded into q, so the
# k columns of d qkv_w are small against the v columns that set the section's scale (23 to 92 bounds at those seeds).
# Case 7 (one 1024-wide temporal head, the smallest q) needed 2916 seeds: none of 701 .. 3615 passes 100 bounds there.
SEARCH = 3000
SEEDS = (71, 109, 201, 404, 742, 507, 1113, 3616, 825, 901)

_REF = {}


def load(i):
    """Case i of sgn_v15_grad_util at its seed of ``SEEDS`` with the fp64 image gradients added (dwf64, dwc64), made once
    and never modified by a test."""
    if i not in _REF:
        d = dict(gu.load(i) if SEEDS[i] == gu.SEEDS[i] else gu.make(gu.CASES[i], SEEDS[i]))
        case = d['case']
        d['dwf64'] = frames_wgrad(d['x'].double(), d['wf'].double(), d['dfeat_in'].double(), case)
        d['dwc64'] = clip_wgrad(d['feat32'].double(), d['wc'].double(), d['dlogits'].double(), case)
        _REF[i] = d
    return _REF[i]


def check_image(got, ref, secs, what):
    """Per section of an image: print and return {name: ratio} (``du.check``: a multiple of the bound, passing iff <= 1)."""
    got, ref = views(got, secs), views(ref, secs)
    out = {n: du.check(got[n], ref[n]) for n, _, _ in secs}
    print(f'{what}, in bounds: ' + ' '.join(f'{n} {v:.3e}' for n, v in out.items()))
    return out


# ---- the block's weight gradient by hand, with the mutants.  mutant = 0 is autograd's result (asserted on the CPU). ----
def _window_sum(z, rows=du.ROWS):
    """Column sums over ``rows`` rows of the PACKED rows from every token set's first row on (mutant 6)."""
    B, R, C = z.shape
    flat = z.reshape(B * R, C)
    return sum(flat[b * R:b * R + rows].sum(0) for b in range(B))


def block_wgrad(t, w, p, heads, d_head, d, mutant=0):
    """t (B, R, din), d (B, dout) the gradient of the block's pooled output -> ({section: gradient}, dt)."""
    B, R, din = t.shape
    inner = heads * d_head
    ff = w[p + 'f1_w'].shape[1]
    q, k, v = ((t @ w[p + 'qkv_w'] + w[p + 'qkv_b']).reshape(B, R, 3, heads, d_head).permute(2, 0, 3, 1, 4))
    a = torch.softmax(q @ k.transpose(-1, -2), dim=-1)
    o = (a @ v).transpose(1, 2).reshape(B, R, inner)
    t1 = o @ w[p + 'o_w'] + w[p + 'o_b'] + t
    pre = t1 @ w[p + 'f1_w'] + w[p + 'f1_b']
    hid = torch.relu(pre)
    y = torch.cat([hid, t1], dim=2) @ w[p + 'f2_w'] + w[p + 'f2_b']
    dy = gu._route(y, d, 0)
    dpre = (dy @ w[p + 'f2_w'][:ff].t()) * (pre > 0)
    dt1 = dpre @ w[p + 'f1_w'].t() + dy @ w[p + 'f2_w'][ff:].t()
    do = (dt1 @ w[p + 'o_w'].t()).reshape(B, R, heads, d_head).transpose(1, 2)
    dP = do @ v.transpose(-1, -2)
    used = a
    if mutant == 2:
        used = a.clone()
        used[:, 1::2] = a[:, 0::2]
    dv = used.transpose(-1, -2) @ do
    dS = a * (dP - (dP * a).sum(-1, keepdim=True))
    dq, dk = dS @ k, dS.transpose(-1, -2) @ q
    dqkv = torch.stack([dq, torch.zeros_like(dk) if mutant == 1 else dk, dv]).permute(1, 3, 0, 2, 4).reshape(B, R, 3 * inner)
    true_dqkv = torch.stack([dq, dk, dv]).permute(1, 3, 0, 2, 4).reshape(B, R, 3 * inner)
    xt = lambda a_, b_: torch.einsum('brk,brn->kn', a_, b_)      # noqa: E731
    bias = _window_sum if mutant == 6 else (lambda z: z.sum((0, 1)))
    dpre_w, o_w = dpre, o
    if mutant == 4:
        dpre_w = dpre.clone()
        dpre_w[..., -128:] = 0
    if mutant == 5:
        o_w = o.clone()
        o_w[..., -128:] = 0
    f2x = torch.cat([hid, torch.zeros_like(t1) if mutant == 3 else t1], dim=2)
    g = {p + 'qkv_w': xt(t, dqkv), p + 'qkv_b': bias(true_dqkv), p + 'o_w': xt(o_w, dt1), p + 'o_b': bias(dt1),
         p + 'f1_w': xt(t1, dpre_w), p + 'f1_b': bias(dpre), p + 'f2_w': xt(f2x, dy), p + 'f2_b': bias(dy)}
    return g, true_dqkv @ w[p + 'qkv_w'].t() + dt1


def _flat(grads, secs):
    return torch.cat([grads[n].reshape(-1) for n, _, _ in secs])


def frames_wgrad_by_hand(x, wf, dfeat, case, mutant=0):
    """The frames image gradient: the block by hand, the input side (aff, the embeddings, spa) by autograd through
    ``du.tokens`` with the block's d tokens as the cotangent."""
    V, seg, sp = case[0], case[1], case[2]
    fs = sections(case)[0]
    with torch.enable_grad():
        w = wf.detach().clone().requires_grad_(True)
        f = views(w, fs)
        tok = du.tokens(x, f, V, seg)
        fd = {n: v.detach() for n, v in f.items()}
        g, dtok = block_wgrad(tok.detach(), fd, 's_', sp[0], sp[1], dfeat.reshape(-1, 256), mutant)
        if mutant == 7:
            dtok = dtok.clone()
            dtok[1:, :, 64:] = 0
        gin, = torch.autograd.grad((tok * dtok).sum(), w)
    gin = views(gin, fs)
    return _flat({n: g.get(n, gin[n]) for n, _, _ in fs}, fs)


def clip_wgrad_by_hand(feat, wc, dlogits, case, mutant=0):
    tp = case[3]
    cs = sections(case)[1]
    c = views(wc, cs)
    dpool = dlogits @ c['fc_w'].t()
    g, dt = block_wgrad(feat + c['tem'], c, 't_', tp[0], tp[1], dpool, mutant)
    g['tem'] = dt[0] if mutant == 8 else dt.sum(0)
    pooled = du.clip_ref(feat, wc, gu.dcase(case))['pooled']
    g['fc_w'] = pooled.t() @ dlogits
    g['fc_b'] = dlogits.sum(0)
    return _flat(g, cs)


# ---- the whole-model fixture (tests/golden/make_golden_sgn_v15_paramgrad.py), in the scheme of sgn_wgrad_util ----
BOUND = wu.BOUND
FULL, SAMPLES, INDEX_SEED = wu.FULL, wu.SAMPLES, 7150
sample_index = wu.sample_index


def compare(grads, fix, what=''):
    """grads {name: tensor} against a loaded fixture, ``sgn_wgrad_util.compare``'s arithmetic (full tensors entry by
    entry; larger ones by their samples and by row and column sums at n times the bound for a sum over n entries) as a
    multiple of the bound 1e-4 max(1, max|reference tensor|), printed per tensor before anything is asserted
    -> {name: ratio}."""
    assert sorted(grads) == sorted(fix['keys']), (sorted(set(grads) ^ set(fix['keys'])), what)
    out = {}
    for k in fix['keys']:
        a = np.asarray(grads[k].detach().cpu())
        assert np.isfinite(a).all(), (k, what)
        scale = BOUND * max(1.0, fix['max'][k])
        if k in fix['full']:
            assert a.shape == fix['full'][k].shape, (k, a.shape, what)
            out[k] = float(np.abs(a.astype(np.float64) - fix['full'][k]).max() / scale)
        else:
            m = a.reshape(a.shape[0], -1).astype(np.float64)
            assert m.shape == (fix['rows'][k].size, fix['cols'][k].size), (k, a.shape, what)
            out[k] = float(max(
                np.abs(a.reshape(-1)[sample_index(k, a.size, fix['meta']['index_seed'])] - fix['samp'][k]).max() / scale,
                np.abs(m.sum(1) - fix['rows'][k]).max() / (scale * m.shape[1]),
                np.abs(m.sum(0) - fix['cols'][k]).max() / (scale * m.shape[0])))
    print(f'{what}, in bounds: ' + ' '.join(f'{k} {v:.3e}' for k, v in out.items()))
    return out


def fixture_name(case):
    return f'sgn15_paramgrad_{case}.npz'


def load_paramgrad(case):
    """-> dict(meta, keys, full, samp, rows, cols, max, floor) as ``sgn_wgrad_util.load_paramgrad``."""
    f = vu._npz(fixture_name(case))
    meta = json.loads(str(f['meta']))
    keys = [str(k) for k in f['keys']]
    pick = lambda p: {k: f[p + k] for k in keys if p + k in f}  # noqa: E731
    return dict(meta=meta, keys=keys, full=pick('full.'), samp=pick('samp.'), rows=pick('rows.'), cols=pick('cols.'),
                max={k: float(v) for k, v in pick('max.').items()}, floor={k: float(v) for k, v in pick('floor.').items()})


def build_model(case, device=None):
    """-> (model in eval mode with the case's state, x, cot as torch tensors, the evalgrad case dict)."""
    from agcn_amd.model.sgn_v15 import SGN
    c = gu.load_grad_case(case)
    m = SGN(**c['meta']['model_args'])
    m.load_state_dict(vu.torch_state(c['state']))
    m.eval()
    x, cot = torch.from_numpy(c['x']), torch.from_numpy(c['cot'])
    if device is not None:
        m, x, cot = m.to(device), x.to(device), cot.to(device)
    return m, x, cot, c


# ---- what the CPU test asserts about a case, and the seed search ----
def _name(side, sec):
    return sec if sec in ('spa', 'tem') else ('s_' if side == 'frames' else 't_') + sec


def conditions(d):
    """Everything tests/test_sgn_v15_wgrad_cpu.py asserts about a made case (a dict of ``sgn_v15_grad_util.make`` with
    dwf64 / dwc64 added) -> (ok, report): the fp32 tensor code within 0.1 of the bound in every section, and every mutant
    that applies at least 100 bounds away in the section it touches."""
    case = d['case']
    V, seg, sp, tp, _, N = case
    fs, cs = sections(case)
    rep, ok = {}, True
    for side, got, ref, secs in (('frames', frames_wgrad(d['x'], d['wf'], d['dfeat_in'], case), d['dwf64'], fs),
                                 ('clip', clip_wgrad(d['feat32'], d['wc'], d['dlogits'], case), d['dwc64'], cs)):
        g, r = views(got, secs), views(ref, secs)
        for n, _, _ in secs:
            rep[f'{side}_fp32:{n}'] = du.check(g[n], r[n])
            ok = ok and rep[f'{side}_fp32:{n}'] <= 0.1
    x, wf, wc, f32 = d['x'].double(), d['wf'].double(), d['wc'].double(), d['feat32'].double()
    for mu, sec in MUTANT_SECTION.items():
        if applies(mu, 'frames', N * seg, V, sp):
            n = _name('frames', sec)
            got = views(frames_wgrad_by_hand(x, wf, d['dfeat_in'].double(), case, mu), fs)[n]
            rep[f'frames_mutant{mu}:{n}'] = du.check(got, views(d['dwf64'], fs)[n])
            ok = ok and rep[f'frames_mutant{mu}:{n}'] >= 100
        if applies(mu, 'clip', N, seg, tp):
            n = _name('clip', sec)
            got = views(clip_wgrad_by_hand(f32, wc, d['dlogits'].double(), case, mu), cs)[n]
            rep[f'clip_mutant{mu}:{n}'] = du.check(got, views(d['dwc64'], cs)[n])
            ok = ok and rep[f'clip_mutant{mu}:{n}'] >= 100
    return ok, rep


def margin_conditions(d):
    """The conditions of sgn_v15_grad_util that a NEW seed must meet for the comparison with fp64 to mean something: every
    ReLU pre-activation and every pooled column's top-1 minus top-2 gap at least the margin away from its switch, and
    attention maps that are neither flat nor one-hot -> (ok, report)."""
    case = d['case']
    V, seg = case[0], case[1]
    rep, ok = {}, True
    for side, inp, img, rows, a in (('frames', d['x'], d['wf'], V, d['spatial_attn']),
                                    ('clip', d['feat32'], d['wc'], seg, d['temporal_attn'])):
        for name, (need, found, dist) in gu.margins(side, inp, img, case).items():
            rep[f'{side}_margin:{name}'] = (need, found, dist)
            ok = ok and need >= gu.MARGIN_FLOOR and found >= need
        if rows > 1:
            lo, hi = gu.rowmax_range(rows)
            rep[f'{side}_rowmax'] = float(a.amax(-1).mean())
            ok = ok and lo <= rep[f'{side}_rowmax'] <= hi
    return ok, rep


def with_refs(d):
    d = dict(d)
    d['dwf64'] = frames_wgrad(d['x'].double(), d['wf'].double(), d['dfeat_in'].double(), d['case'])
    d['dwc64'] = clip_wgrad(d['feat32'].double(), d['wc'].double(), d['dlogits'].double(), d['case'])
    return d


def search(i, tries=SEARCH):
    """The first seed of 100 * i + 1, ... at which case i meets ``margin_conditions`` and ``conditions``."""
    rep = None
    for seed in range(100 * i + 1, 100 * i + 1 + tries):
        d = with_refs(gu.make(gu.CASES[i], seed))
        ok, rep = conditions(d)
        if ok and margin_conditions(d)[0]:
            return seed, rep
    return None, rep


if __name__ == '__main__':
    import sys
    for i in ([int(a) for a in sys.argv[1:]] or range(len(gu.CASES))):
        seed, rep = search(i)
        print(i, seed, {k: f'{v:.2e}' for k, v in rep.items() if 'mutant' in k}, flush=True)
