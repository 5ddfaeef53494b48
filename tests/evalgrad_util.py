"""Shared cases and fp64-oracle plumbing of the eval-mode gradient tests (tests/test_eval_grad_cpu.py on the CPU,
tests/test_gpu_eval_grad.py on the GPU).  Eval mode = BatchNorm on its frozen running statistics, gradients enabled.

Every case is the smallest one that reaches a route of its own in the HIP backward; states come from the oracle's
seeded ``randomized_state`` recipes (running mean 0.1*N(0,1), running variance U(0.5, 1.5): away from (0, 1)); the
ten-layer model alone takes its running statistics from a calibration pass (``_calibrated`` says why).
The seeds were kept after checking, on the CPU, that the oracle run in fp32 with the ReLU patterns pinned stays inside
the stated tolerances of its own fp64 run for every case (test_eval_grad_cpu.py repeats that check)."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import agcn_oracle as orc
from tests import golden_util as gu

TOL_Y, TOL_G, TOL_SCALAR, ZERO_ABS = 1e-4, 2e-4, 5e-3, 1e-5      # the project's stated tolerances

# kind, then the constructor facts.  n = person-samples in the batch.
CASES = {
    'agcn_unit_64_64_s1_v25': dict(kind='agcn_unit', cin=64, cout=64, stride=1, res=True, v=25, t=16, n=2, seed=711,
                                   stress=2.0),                      # identity residual
    'agcn_unit_64_128_s2_v18_oddT': dict(kind='agcn_unit', cin=64, cout=128, stride=2, res=True, v=18, t=15, n=2,
                                         seed=712, stress=2.0),      # conv residual and `down`, odd T
    'agcn_unit_3_64_nores': dict(kind='agcn_unit', cin=3, cout=64, stride=1, res=False, v=25, t=16, n=2, seed=713,
                                 stress=1.0),                        # first-layer kernel
    'aagcn_unit_64_64_attn': dict(kind='aagcn_unit', cin=64, cout=64, stride=1, res=True, v=25, t=16, n=2, seed=714,
                                  stress=3.0, gbn=None),
    'aagcn_unit_64_64_gbn2': dict(kind='aagcn_unit', cin=64, cout=64, stride=1, res=True, v=25, t=16, n=4, seed=715,
                                  stress=3.0, gbn=2),                # GhostBatchNorm: plain BN after .eval()
    'unit_tcn_k3s3p0': dict(kind='unit_tcn', cin=16, cout=16, k=3, stride=3, v=25, t=30, n=2, seed=716),
    'agcn_model_ntu_b1_t32': dict(kind='agcn_model', v=25, t=32, n=1, seed=717, stress=3.0, num_class=60,
                                  calibrate=True),
    'aagcn_model_l3_t32': dict(kind='aagcn_model', v=25, t=32, n=1, seed=718, stress=3.0, num_class=60, layers=3),
}
UNIT_CASES = [k for k, c in CASES.items() if c['kind'].endswith('unit') or c['kind'] == 'unit_tcn']
MODEL_CASES = [k for k, c in CASES.items() if c['kind'].endswith('model')]


def state_and_inputs(name):
    """(fp32 state dict, x, r): r is the cotangent, the loss is (output * r).sum()."""
    c = CASES[name]
    rng = np.random.default_rng(c['seed'] + 5000)
    if c['kind'] == 'agcn_unit':
        sd = orc.randomized_state(orc.unit_param_shapes('', c['cin'], c['cout'], c['v'], c['stride'], c['res']),
                                  c['seed'], stress=c['stress'])
    elif c['kind'] == 'aagcn_unit':
        shapes = orc.aagcn_unit_param_shapes('', c['cin'], c['cout'], c['v'], c['stride'], c['res'], True, True, c['gbn'])
        sd = orc.aagcn_randomized_state(shapes, c['seed'], stress=c['stress'])
    elif c['kind'] == 'unit_tcn':
        shapes = {'conv.weight': (c['cout'], c['cin'], c['k'], 1), 'conv.bias': (c['cout'],)}
        for s in ('weight', 'bias', 'running_mean', 'running_var'):
            shapes['bn.' + s] = (c['cout'],)
        shapes['bn.num_batches_tracked'] = ()
        sd = orc.randomized_state(shapes, c['seed'])
    elif c['kind'] == 'agcn_model':
        sd = orc.randomized_state(orc.model_param_shapes(c['num_class'], c['v']), c['seed'], stress=c['stress'])
    else:
        sd = orc.aagcn_randomized_state(orc.aagcn_model_param_shapes(c['num_class'], c['v'], model_layers=c['layers']),
                                        c['seed'], stress=c['stress'])
    if c['kind'].endswith('model'):
        x = rng.standard_normal((c['n'], 3, c['t'], c['v'], 2)).astype(np.float32)
        r = rng.standard_normal((c['n'], c['num_class'])).astype(np.float32)
        if c.get('calibrate'):
            sd = _calibrated(c, sd, rng.standard_normal((2,) + x.shape[1:]).astype(np.float32))
    else:
        x = rng.standard_normal((c['n'], c['cin'], c['t'], c['v'])).astype(np.float32)
        if c['kind'] == 'unit_tcn':
            tout = (c['t'] - c['k']) // c['stride'] + 1
        else:
            tout = (c['t'] + 2 * 4 - 9) // c['stride'] + 1
        r = rng.standard_normal((c['n'], c['cout'], tout, c['v'])).astype(np.float32)
    return sd, x, r


def _calibrated(c, sd, xcal):
    """Running statistics of a trained checkpoint rather than of the recipe: ten stacked units on statistics that have
    nothing to do with their inputs let the activations grow to ~1e4, the adjacency softmax saturates, and the oracle's
    own fp32 run (ReLU patterns pinned) lands 1e-3 .. O(1) of max|g| from its fp64 run -- no fp32 implementation can be
    held to 2e-4 there (measured on the CPU for seeds 717-719 at stress 1 and 2).  So the statistics are taken from ONE
    train-mode pass of the fp64 oracle over a seeded calibration batch with momentum 1: still away from (0, 1), and not
    the batch statistics of the test clip."""
    sd = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    keep, orc.BN_MOMENTUM = orc.BN_MOMENTUM, 1.0
    try:
        with torch.no_grad():
            orc.model_forward(torch.from_numpy(xcal).double(), sd, gu.graph_A(c['v']).double(), training=True)
    finally:
        orc.BN_MOMENTUM = keep
    return {k: (v.float() if v.is_floating_point() else torch.zeros_like(v)) for k, v in sd.items()}


def make_module(name):
    """The HIP module of the case (on the CPU, parameters not loaded yet)."""
    c = CASES[name]
    if c['kind'] == 'agcn_unit':
        from agcn_amd.model.agcn import TCN_GCN_unit
        return TCN_GCN_unit(c['cin'], c['cout'], gu.graph_A(c['v']).numpy(), stride=c['stride'], residual=c['res'])
    if c['kind'] == 'aagcn_unit':
        from agcn_amd.model.aagcn import AdaptiveGCN, TCNGCNUnit
        return TCNGCNUnit(c['cin'], c['cout'], gu.graph_A(c['v']).numpy(), stride=c['stride'], residual=c['res'],
                          adaptive=AdaptiveGCN, attention=True, gbn_split=c['gbn'])
    if c['kind'] == 'unit_tcn':
        from agcn_amd.model.aagcn import TCNUnit
        return TCNUnit(c['cin'], c['cout'], kernel_size=c['k'], stride=c['stride'], pad=False)
    kw = dict(num_class=c['num_class'], num_point=c['v'], num_person=2, graph='graph.ntu_rgb_d.Graph',
              graph_args=dict(labeling_mode='spatial'))
    if c['kind'] == 'agcn_model':
        from model.agcn import Model
        return Model(**kw)
    from model.aagcn import Model
    return Model(model_layers=c['layers'], **kw)


def layer_keys(name):
    c = CASES[name]
    if c['kind'] == 'agcn_model':
        return list(range(1, 11))
    if c['kind'] == 'aagcn_model':
        return list(orc.AAGCN_LAYER_SUBSETS[c['layers']])
    return []


def _oracle_state(name, sd0, dtype):
    """State dict of the oracle: eval statistics of a GhostBatchNorm collated as ``.eval()`` does, conv_d aliases of
    the AAGCN state dict sharing one tensor, leaves requiring a gradient."""
    sd = {k: (v.to(dtype) if v.is_floating_point() else v.clone()) for k, v in sd0.items()}
    sd = orc.with_grad(orc.ghost_collate(sd))
    for k in list(sd):
        if gu.is_alias_key(k):
            sd[k] = sd[gu.canonical_key(k)]
    return sd


def _no_attention(sd):
    return {k: v for k, v in sd.items() if 'attn_' not in k}


def _unit_forward(c, x, sd, prefix, A, stride, res, masks):
    if c['kind'].startswith('agcn'):
        return orc.tcn_gcn_unit_forward(x, sd, prefix, A, stride, res, training=False, masks=masks)
    return orc.aagcn_unit_forward(x, sd, prefix, None, stride, res, training=False, masks=masks)


def _gcn_pattern(c, x, sd, prefix, A):
    """ReLU pattern of the unit's GCN core (before the attention gates) at input x."""
    with torch.no_grad():
        if c['kind'].startswith('agcn'):
            g = orc.unit_gcn_forward(x, sd, prefix + 'gcn1.', A, training=False)
        else:
            g = orc.aagcn_gcn_unit_forward(x, _no_attention(sd), prefix + 'gcn1.', None, training=False)
    return (g > 0).to(x.dtype)


def _layers(c, name):
    if c['kind'] == 'agcn_model':
        return [(k,) + tuple(orc.LAYERS[k - 1][2:]) for k in layer_keys(name)]
    return [(k,) + tuple(orc.AAGCN_LAYER_CFG[k][2:]) for k in layer_keys(name)]


def oracle_own_masks(name, sd0, xn, dtype=torch.float64):
    """The ReLU patterns of the oracle's own (unpinned) eval forward at ``dtype``: what the CPU pre-check pins."""
    c = CASES[name]
    sd = _oracle_state(name, sd0, dtype)
    A = gu.graph_A(c['v']).to(dtype)
    x = torch.from_numpy(xn).to(dtype)
    with torch.no_grad():
        if c['kind'] == 'unit_tcn':
            return None
        if c['kind'].endswith('unit'):
            mg = _gcn_pattern(c, x, sd, '', A)
            y = _unit_forward(c, x, sd, '', A, c['stride'], c['res'], None)
            return (mg, (y > 0).to(dtype))
        n, ch, t, v, m = x.shape
        h = orc._bn(x.permute(0, 4, 3, 1, 2).reshape(n, m * v * ch, t), sd, 'data_bn.', False)
        h = h.reshape(n, m, v, ch, t).permute(0, 1, 3, 4, 2).reshape(n * m, ch, t, v)
        masks = {}
        for k, stride, res in _layers(c, name):
            mg = _gcn_pattern(c, h, sd, f'l{k}.', A)
            h = _unit_forward(c, h, sd, f'l{k}.', A, stride, res, None)
            masks[k] = (mg, (h > 0).to(dtype))
        return masks


def oracle_run(name, sd0, xn, rn, masks, dtype=torch.float64):
    """Eval-mode forward + backward of the oracle at ``dtype`` with the given ReLU patterns imposed.
    Returns (output, dx, {parameter name: gradient})."""
    c = CASES[name]
    sd = _oracle_state(name, sd0, dtype)
    A = gu.graph_A(c['v']).to(dtype)
    x = torch.from_numpy(xn).to(dtype).requires_grad_(True)
    cast = lambda mk: None if mk is None else tuple(t.to(dtype) for t in mk)  # noqa: E731
    if c['kind'] == 'unit_tcn':
        y = orc._bn(F.conv2d(x, sd['conv.weight'], sd['conv.bias'], stride=(c['stride'], 1)), sd, 'bn.', False)
    elif c['kind'].endswith('unit'):
        y = _unit_forward(c, x, sd, '', A, c['stride'], c['res'], cast(masks))
    elif c['kind'] == 'agcn_model':
        y = orc.model_forward(x, sd, A, training=False, masks={k: cast(v) for k, v in masks.items()})
    else:
        y = orc.aagcn_model_forward(x, sd, A, training=False, layers=layer_keys(name),
                                    masks={k: cast(v) for k, v in masks.items()})
    (y * torch.from_numpy(rn).to(dtype)).sum().backward()
    grads = {k: v.grad for k, v in sd.items() if not orc.is_buffer(k) and v.grad is not None}
    return y.detach(), x.grad, grads


def is_conv_a_bias(k):
    return k.endswith(('conv_a.0.bias', 'conv_a.1.bias', 'conv_a.2.bias'))


def is_bn_conv_bias(k):
    """Biases of the convolutions in front of a BatchNorm: zero gradient in train mode, NOT in eval mode."""
    return gu.is_zero_grad_bias(k) and not is_conv_a_bias(k)


def compare(name, y, dx, grads, ref, bf16=False):
    """Worst error of EVERY tensor against ``ref`` = (y, dx, grads) of the fp64 oracle, on the project's criteria;
    returns the list of violations (empty = pass) and a printable record."""
    y_ref, dx_ref, g_ref = ref
    tol_y, tol_g, tol_s = (2e-2, 2e-2, 6e-2) if bf16 else (TOL_Y, TOL_G, TOL_SCALAR)
    bad, rec = [], {}

    def note(k, e, tol):
        rec[k] = e
        if not e <= tol:
            bad.append((k, e, tol))
    note('y', gu.rel_err(y, y_ref.numpy()), tol_y)
    if dx is not None:
        note('dx', float(np.abs(np.asarray(dx, dtype=np.float64) - dx_ref.numpy()).max()) /
             max(1e-30, float(dx_ref.abs().max())), tol_g)
    for k, g in grads.items():
        r = g_ref[gu.canonical_key(k)] if gu.canonical_key(k) in g_ref else g_ref[k]
        g = np.asarray(g, dtype=np.float64)
        if is_conv_a_bias(k):          # the softmax cancels it in either mode: absolute floor
            if not bf16:
                note(k, float(np.abs(g).max()), ZERO_ABS)
            continue
        den = float(r.abs().max())
        scalar = g.size == 1
        if scalar and bf16:            # tests/bf16_check.py: a single-scalar parameter on its sibling tensor's scale
            sib = k[:-4] + 'weight' if k.endswith('bias') else k.replace('alpha', 'PA')
            den = max(den, float(g_ref[sib].abs().max()))
        note(k, float(np.abs(g - r.numpy()).max()) / max(1e-30, den), tol_s if scalar else tol_g)
    return bad, rec
