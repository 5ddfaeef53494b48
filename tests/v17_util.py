"""The aagcn_v17 fixture cases and the seeded recipes of their parameters and inputs, shared by the generator
(tests/golden/make_golden_v17.py) and the tests: the fixture files hold inputs and results only."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
NUM_CLASS = 60
N, M = 2, 2
STRESS = 2.0

_NTU = dict(num_point=25, graph='graph.ntu_rgb_d.Graph', T=30, model_layers=101)
_COMMON = dict(num_class=NUM_CLASS, num_person=M, graph_args=dict(labeling_mode='spatial'), kernel_size=3, pad=False,
               trans_dropout=0.0, trans_num_layers=2, trans_model_dim=16, trans_ffn_dim=64)

# name -> (seed, constructor arguments beside _COMMON, T, frames nulled: [(sample or None, person or None, first frame)])
CASES = {
    # the shipped configuration: L = 21, D = 400, H = 2
    'tv17_shipped': (701, dict(_NTU, pos_enc='False', classifier_type='CLS', attn_masking='False',
                               trans_activation='gelu', trans_prenorm=False), []),
    'tv17_frame': (702, dict(_NTU, pos_enc='True', classifier_type='CLS', attn_masking='True', trans_prenorm=True,
                             need_attn=True), [(1, None, 18), (None, 1, 24)]),
    'tv17_forward': (703, dict(_NTU, pos_enc='cossin', classifier_type='CLS', attn_masking='forward',
                               trans_num_heads=8, trans_activation='relu', need_attn=True), []),
    'tv17_backward': (704, dict(_NTU, pos_enc='False', classifier_type='CLS', attn_masking='backward'), []),
    # Kinetics graph, two windowing layers, token mean: L = 6, dh = 144
    'tv17_gap': (705, dict(num_point=18, graph='graph.kinetics.Graph', T=27, model_layers=102, pos_enc='True',
                           classifier_type='GAP', attn_masking='False', need_attn=True), []),
}
NAMES = list(CASES)


def model_kwargs(name):
    kw = dict(_COMMON, **CASES[name][1])
    kw.pop('T')
    return kw


def frames(name):
    return CASES[name][1]['T']


def inputs(name):
    """x (N, 3, T, V, M) ~ N(0, 1) with the case's null frames, r (N, num_class) ~ N(0, 1)."""
    seed, kw, nulls = CASES[name]
    rng = np.random.default_rng(seed + 7000)
    x = rng.standard_normal((N, 3, kw['T'], kw['num_point'], M)).astype(np.float32)
    r = rng.standard_normal((N, NUM_CLASS)).astype(np.float32)
    for n, m, t0 in nulls:
        x[slice(None) if n is None else n, :, t0:, :, slice(None) if m is None else m] = 0.0
    return x, r


def state(shapes, name):
    """oracle.agcn_oracle.aagcn_randomized_state, with the LayerNorm weights in (0.5, 1.5) and the CLS token and the
    positional table at 0.5 * N(0, 1) from a child generator (the stock recipe scales them by their fan-in, ~1e-3,
    which no comparison would see)."""
    from oracle import agcn_oracle as orc
    seed = CASES[name][0]
    sd = orc.aagcn_randomized_state(shapes, seed, stress=STRESS)
    rng = np.random.default_rng([seed, 17])
    for k in sorted(sd):
        if '.norm1.weight' in k or '.norm2.weight' in k:
            sd[k] = torch.from_numpy(rng.uniform(0.5, 1.5, shapes[k])).float()
        elif k in ('cls_token', 'pos_encoder.pe'):
            sd[k] = torch.from_numpy(0.5 * rng.standard_normal(shapes[k])).float()
    return sd


def shapes_of(gold):
    return {k[len('shape.'):]: tuple(int(d) for d in v) for k, v in gold.items() if k.startswith('shape.')}


def load(name):
    return dict(np.load(os.path.join(GOLDEN, name + '.npz')))
