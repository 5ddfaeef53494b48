"""The aagcn_v24 fixture cases and the seeded recipes of their parameters and inputs, shared by the generator
(tests/golden/make_golden_v24.py) and the tests: the fixture files hold inputs and results only."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
NUM_CLASS = 60
N, M = 2, 2
STRESS = 2.0
ALPHA = 0.8
KERNEL = 3
NULLS = [(0, 24), (1, 18)]                  # (sample, first null frame): all persons, to the end of the clip
MUTANT_MOVE = 100 * 1e-4                    # every stored mutant moves the logits by at least 100 x the 1e-4 rule

_NTU = dict(num_point=25, graph='graph.ntu_rgb_d.Graph', T=30, model_layers=101)
_COMMON = dict(num_class=NUM_CLASS, num_person=M, graph_args=dict(labeling_mode='spatial'), kernel_size=KERNEL, pad=False)
_CFG = dict(model_dim=24, num_heads=3, ffn_dim=96, num_layers=2, dropout=0.0, activation='gelu', prenorm=False)

# name -> (seed, constructor arguments beside _COMMON (T is the clip length), s_trans_cfg entries beside _CFG)
CASES = {
    # the shipped configuration at width 24: 10 windows a sample, L = 51, the masked mean of CLS_MASK
    'tv24_shipped': (2401, dict(_NTU, add_A='single', pos_enc='cossin', classifier_type='CLS_MASK'), {}),
    'tv24_triple': (2402, dict(_NTU, add_A='triple', pos_enc='True', classifier_type='CLS'),
                    dict(prenorm=True, activation='relu')),
    # two windowing layers: 27 frames -> 9 -> 3 windows
    'tv24_two_windows': (2403, dict(_NTU, add_A='single', pos_enc='True', classifier_type='CLS', model_layers=102,
                                    T=27), {}),
    # no bias (alpha gets no gradient), no positional table, Kinetics graph: L = 37
    'tv24_plain_kinetics': (2404, dict(num_point=18, graph='graph.kinetics.Graph', T=30, model_layers=101,
                                       add_A='False', pos_enc='False', classifier_type='CLS'), {}),
}
NAMES = list(CASES)


def model_kwargs(name, **cfg_over):
    kw = dict(_COMMON, **CASES[name][1])
    kw.pop('T')
    kw['s_trans_cfg'] = dict(_CFG, **CASES[name][2], **cfg_over)
    return kw


def has_bias(name):
    return CASES[name][1]['add_A'] in ('single', 'triple')


def mutants(name):
    """The mutants of a case with a bias whose logits the fixture stores (``mut.<mutant>``)."""
    if not has_bias(name):
        return []
    return ['alpha0', 'pa_t'] + (['heads_rolled'] if CASES[name][1]['add_A'] == 'triple' else [])


def mutate(sd, mutant):
    sd = dict(sd)
    for k in sd:
        if mutant == 'alpha0' and k == 'alpha':
            sd[k] = torch.zeros_like(sd[k])
        elif mutant == 'pa_t' and k.startswith('s_trans_enc_layers.') and k.endswith('.PA'):
            sd[k] = sd[k].transpose(-1, -2).contiguous()
        elif mutant == 'heads_rolled' and k.startswith('s_trans_enc_layers.') and k.endswith('.PA'):
            sd[k] = torch.roll(sd[k], 1, 0)
    return sd


def inputs(name):
    """x (N, 3, T, V, M) ~ N(0, 1) with the null frames of NULLS, r (N, num_class) ~ N(0, 1)."""
    seed, kw, _ = CASES[name]
    rng = np.random.default_rng(seed + 7000)
    x = rng.standard_normal((N, 3, kw['T'], kw['num_point'], M)).astype(np.float32)
    r = rng.standard_normal((N, NUM_CLASS)).astype(np.float32)
    for n, t0 in NULLS:
        x[n, :, t0:] = 0.0
    return x, r


def window_mask(x):
    """(N, ceil(T / KERNEL)) uint8: 1 where frame t*KERNEL is all zero (the vector CLS_MASK multiplies by)."""
    null = ~(x != 0).any(axis=(1, 3, 4))
    return null[:, ::KERNEL].astype(np.uint8)


def windows(name):
    """T': the frame windows the backbone leaves of the case's clip."""
    kw = CASES[name][1]
    tp = kw['T']
    for _ in range(kw['model_layers'] - 100):
        tp = (tp - KERNEL) // KERNEL + 1
    return tp


def attn_sequences(name):
    """The sequences n*T' + t whose attention maps the fixture stores (all N*T' maps of L x L would not fit a fixture):
    one per case, alternately the last window of the last sample (null) and the first window of the first (valid)."""
    return [N * windows(name) - 1] if NAMES.index(name) % 2 == 0 else [0]


def pa_init(name):
    """The value the reference initialises every layer's PA with (aagcn_v24.py:233-243), from the stored graph."""
    from tests import golden_util as gu
    A = gu.graph_A(25).numpy().astype(np.float64)
    if CASES[name][1]['add_A'] == 'triple':
        P = np.ones((3, 51, 51))
        P[:, 1:26, 1:26] = A
        P[:, 26:, 26:] = A
    else:
        P = np.ones((51, 51))
        P[1:26, 1:26] = A[0]
        P[26:, 26:] = A[0]
    return P.astype(np.float32)


def cossin_table(shape):
    """sin / cos positional table (1, rows, d) with base 10000 (reference aagcn_v24.py:42-47)."""
    _, rows, d = shape
    pos = torch.arange(rows).unsqueeze(1)
    div = torch.exp(torch.arange(0, d, 2) * (-np.log(10000.0) / d))
    pe = torch.zeros(1, rows, d)
    pe[0, :, 0::2] = torch.sin(pos * div)
    pe[0, :, 1::2] = torch.cos(pos * div)
    return pe


def state(shapes, name):
    """oracle.agcn_oracle.aagcn_randomized_state(stress=2), then from a child generator: alpha = 0.8, every layer's PA =
    its initial value + 0.5 * N(0, 1), the CLS token and a learned positional table = 0.5 * N(0, 1), the LayerNorm
    weights in (0.5, 1.5)."""
    from oracle import agcn_oracle as orc
    seed = CASES[name][0]
    sd = orc.aagcn_randomized_state(shapes, seed, stress=STRESS)
    rng = np.random.default_rng([seed, 24])
    for k in sorted(sd):
        if '.norm1.weight' in k or '.norm2.weight' in k:
            sd[k] = torch.from_numpy(rng.uniform(0.5, 1.5, shapes[k])).float()
        elif k == 's_pos_encoder.pe' and CASES[name][1]['pos_enc'] == 'cossin':
            sd[k] = cossin_table(shapes[k])          # a buffer: the table itself (the generator checks it)
        elif k in ('s_cls_token', 's_pos_encoder.pe'):
            sd[k] = torch.from_numpy(0.5 * rng.standard_normal(shapes[k])).float()
        elif k == 'alpha':
            sd[k] = torch.full((1,), ALPHA)
        elif k.startswith('s_trans_enc_layers.') and k.endswith('.PA'):
            sd[k] = torch.from_numpy(pa_init(name) + (0.5 * rng.standard_normal(shapes[k])).astype(np.float32))
    return sd


def shapes_of(gold):
    return {k[len('shape.'):]: tuple(int(d) for d in v) for k, v in gold.items() if k.startswith('shape.')}


def load(name):
    return dict(np.load(os.path.join(GOLDEN, name + '.npz')))
