"""aagcn_v24: a per-frame spatial transformer head with a learned adjacency bias on the windowed AAGCN backbone.

Same public surface as the reference ``model/architecture/aagcn/aagcn_v24.py``: ``PositionalEncoding`` /
``CosSinPositionalEncoding`` (:18-55), ``TransformerEncoderLayerExt`` (:58-104), ``TransformerEncoderLayerExtV2(cfg, A)``
(:107-123), ``TransformerEncoderExt`` (:126-147), ``transformer_config_checker`` (:150-163) and ``Model`` (:175-324) with
its constructor arguments, ``forward(x) -> (logits, attn_list)`` and the identical state_dict (``alpha``,
``s_cls_token``, ``s_pos_encoder.pe``, ``s_trans_enc_layers.<i>.{PA, self_attn.*, linear1/2.*, norm1/2.*}``, ``fc.*``).

What runs where: the backbone is ``aagcn.TCNGCNUnit`` with ``stride = kernel_size``.  Its output (N*M, C, T', V) becomes
one sequence per frame window, (N*T', [CLS +] M*V, C) (``ops.SpatialTokensFunction``); every layer's attention core
takes the logits ``q k^T / sqrt(dh) + alpha * PA`` (``ops.MHABiasFunction``; ``alpha * PA`` is formed in torch, so
autograd carries the kernel's ``dbias`` to ``PA`` and ``alpha``); residual add + LayerNorm is
``ops.AddLayerNormFunction``.  All three are gfx950 kernels of ``csrc/encoder.hip``; the four projections of a layer and
its activation are ``F.linear`` / ATen.  ``AGCN_ENCODER_HIP=0`` runs the same maths as tensor code and counts in
``ops.ENCODER_STATS``.

Behaviour kept from the reference as it is:
  * ``classifier_type='CLS_MASK'`` multiplies the per-window CLS outputs by a mask that is TRUE FOR NULL WINDOWS
    (:278-280, :317-318) and then takes ``mean(1)`` over all T' windows: the valid windows are zeroed, and a sample
    without null frames yields ``fc.bias``.  The shipped yaml trains with it.
  * The bias applies to every layer; each layer owns its ``PA`` (deep copies, :250-252), all layers share the one
    ``alpha`` (:208, :300-303).
  * ``need_attn`` returns the head-averaged maps (N*T', L, L) of every layer.
  * pre-norm takes the residual from the normed tensor (:85-94).
Deviations: a frame is null when ALL its values are zero (the reference tests ``sum() == 0``), as elsewhere in the
project.  Every ``classifier_type`` other than ``CLS`` / ``CLS_MASK`` raises ``ValueError`` at construction (the reference
raises in forward).  Combinations on which the reference dies of a shape error inside ``MultiheadAttention`` raise
``ValueError`` at construction: ``add_A`` in (``single``, ``triple``) unless ``num_point == 25``, ``num_person == 2`` and a
CLS token is present (the reference hard-codes 51 tokens), ``triple`` with ``num_heads != 3``, and a positional table
shorter than the token count.
"""
import copy
import math
from typing import Optional

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from .. import ops
from . import aagcn_v17
from .aagcn import BaseModel, TCNGCNUnit

MAX_LEN = 100                  # rows of the spatial positional table (reference :256-260)


class PositionalEncoding(aagcn_v17.PositionalEncoding):
    pass


class CosSinPositionalEncoding(aagcn_v17.PositionalEncodingBase):
    def __init__(self, d_model: int, dropout: float = 0.0, max_len: int = 601):
        super().__init__(d_model, dropout, max_len)
        position = torch.arange(max_len).unsqueeze(1)
        div_term = torch.exp(torch.arange(0, d_model, 2) * (-math.log(10000.0) / d_model))
        pe = torch.zeros(1, max_len, d_model)
        pe[0, :, 0::2] = torch.sin(position * div_term)
        pe[0, :, 1::2] = torch.cos(position * div_term)
        self.register_buffer('pe', pe)


class TransformerEncoderLayerExt(aagcn_v17.TransformerEncoderLayerExt):
    """aagcn_v17's layer (same pre- / post-norm handling, the dropout keep mask drawn once for either route) with the
    parameter ``PA`` (from ``A``, or None) and an additive ``bias`` (Hb, L, L), Hb in {1, nhead}, on the logits.  The
    reference passes the bias as ``src_mask``; here it has an argument of its own and ``src_mask`` is refused."""

    def __init__(self, d_model: int, nhead: int, dim_feedforward: int = 2048, dropout: float = 0.1,
                 activation: str = "relu", layer_norm_eps: float = 1e-5, batch_first: bool = False,
                 pre_norm: bool = False, A: Optional[np.ndarray] = None) -> None:
        super().__init__(d_model, nhead, dim_feedforward, dropout, activation, layer_norm_eps, batch_first, pre_norm)
        if A is None:
            self.register_parameter('PA', None)
        else:
            self.PA = nn.Parameter(torch.from_numpy(A.astype(np.float32)))

    def forward(self, src: torch.Tensor, src_mask: Optional[torch.Tensor] = None,
                src_key_padding_mask: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None,
                need_attn: bool = True):
        if src_mask is not None or src_key_padding_mask is not None:
            raise ValueError("agcn_amd.aagcn_v24.TransformerEncoderLayerExt: pass the additive mask as bias, not as "
                             "src_mask / src_key_padding_mask tensors")
        hip = ops.encoder_hip_enabled()
        if hip and not src.is_cuda:
            raise RuntimeError("agcn_amd.aagcn_v24: the encoder kernels need a GPU tensor (AGCN_ENCODER_HIP=0 runs the "
                               "tensor-code composition)")
        ops.ENCODER_STATS['layers_hip' if hip else 'layers_tensor'] += 1
        add_ln = ops.AddLayerNormFunction.apply if hip else ops.add_ln_ref
        att, H = self.self_attn, self.self_attn.num_heads
        n1, n2 = self.norm1, self.norm2
        x = add_ln(src, None, n1.weight, n1.bias, n1.eps) if self.pre_norm else src
        qkv = F.linear(x, att.in_proj_weight, att.in_proj_bias)
        keep, keep_scale = None, 1.0
        if self.training and att.dropout > 0.0:
            # dropout of the attention probabilities: the keep mask is drawn here, once, for either path
            N, L = x.shape[0], x.shape[1]
            keep = (torch.rand(N, H, L, L, device=x.device) >= att.dropout).to(torch.uint8)
            keep_scale = 1.0 / (1.0 - att.dropout)
        if hip:
            ctx, attn = ops.MHABiasFunction.apply(qkv, H, bias, None, 0, keep, keep_scale, need_attn)
        else:
            ctx, attn = ops.mha_ref(qkv, H, None, 0, keep, keep_scale, need_attn, bias=bias)
            attn = None if attn is None else attn.detach()
        sa = self.dropout1(F.linear(ctx, att.out_proj.weight, att.out_proj.bias))
        if self.pre_norm:
            x = add_ln(x, sa, n2.weight, n2.bias, n2.eps)
            return x + self.dropout2(self.linear2(self.dropout(self.activation(self.linear1(x))))), attn
        x = add_ln(x, sa, n1.weight, n1.bias, n1.eps)
        ff = self.dropout2(self.linear2(self.dropout(self.activation(self.linear1(x)))))
        return add_ln(x, ff, n2.weight, n2.bias, n2.eps), attn


class TransformerEncoderLayerExtV2(TransformerEncoderLayerExt):
    def __init__(self, cfg: dict, A: Optional[np.ndarray] = None) -> None:
        super().__init__(d_model=cfg['model_dim'], nhead=cfg['num_heads'], dim_feedforward=cfg['ffn_dim'],
                         dropout=cfg['dropout'], activation=cfg['activation'], layer_norm_eps=cfg['layer_norm_eps'],
                         batch_first=cfg['batch_first'], pre_norm=cfg['prenorm'], A=A)


class TransformerEncoderExt(nn.TransformerEncoder):
    """A stack of ``TransformerEncoderLayerExt`` returning (output, attention list) (reference :126-147; the reference
    model does not use it either).  ``bias`` goes to every layer."""

    def __init__(self, encoder_layer, num_layers, norm=None, need_attn: bool = False):
        super().__init__(encoder_layer, num_layers, norm)
        self.need_attn = need_attn

    def forward(self, src: torch.Tensor, mask: Optional[torch.Tensor] = None,
                src_key_padding_mask: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None):
        output, attn_list = src, []
        for mod in self.layers:
            output, attn = mod(output, src_mask=mask, src_key_padding_mask=src_key_padding_mask, bias=bias,
                               need_attn=self.need_attn)
            if self.need_attn:
                attn_list.append(attn)
        if self.norm is not None:
            output = self.norm(output)
        return output, attn_list


TRANS_CFG_NAMES = ('num_heads', 'model_dim', 'ffn_dim', 'dropout', 'activation', 'prenorm', 'batch_first',
                   'layer_norm_eps', 'num_layers')


def transformer_config_checker(cfg: dict):
    for x in cfg:
        assert f'{x}' in TRANS_CFG_NAMES, f'{x} not in transformer config'


def window_null_mask(x: torch.Tensor, kernel_size: int) -> torch.Tensor:
    """(N, ceil(T / kernel_size), 1) bool from the raw input (N, C, T, V, M): True where frame t*kernel_size is null for
    every person (reference :278-280).  A frame is null when all its values are zero."""
    null = ~(x != 0).any(dim=4).any(dim=3).any(dim=1)             # N, T
    return null[:, ::kernel_size].unsqueeze(-1).detach()


class Model(BaseModel):
    def __init__(self, num_class: int = 60, num_point: int = 25, num_person: int = 2, num_subset: int = 3,
                 graph: Optional[str] = None, graph_args: dict = dict(), in_channels: int = 3, drop_out: int = 0,
                 adaptive: bool = True, attention: bool = True, gbn_split: Optional[int] = None, kernel_size: int = 9,
                 pad: bool = True, need_attn: bool = False, s_trans_cfg: Optional[dict] = None, add_A: str = 'False',
                 pos_enc: str = 'True', classifier_type: str = 'CLS', model_layers: int = 10):
        super().__init__(num_class, num_point, num_person, in_channels, drop_out, adaptive, gbn_split)
        if s_trans_cfg is None:
            raise ValueError("agcn_amd.aagcn_v24.Model: s_trans_cfg is required")
        s_trans_cfg = dict(s_trans_cfg, layer_norm_eps=1e-5, batch_first=True)
        transformer_config_checker(s_trans_cfg)
        if classifier_type not in ('CLS', 'CLS_MASK'):
            raise ValueError(f"agcn_amd.aagcn_v24.Model: unknown classifier_type {classifier_type!r}")
        add_A, pos_enc = str(add_A), str(pos_enc)
        tokens = 1 + num_person * num_point                      # both classifier types carry a CLS token
        if add_A in ('single', 'triple') and (num_point != 25 or num_person != 2):
            raise ValueError(f"agcn_amd.aagcn_v24.Model: add_A={add_A!r} needs num_point=25, num_person=2 and a CLS token "
                             f"(got num_point={num_point}, num_person={num_person}): the bias has 51 x 51 entries")
        if add_A == 'triple' and s_trans_cfg['num_heads'] != 3:
            raise ValueError(f"agcn_amd.aagcn_v24.Model: add_A='triple' needs num_heads=3 (got "
                             f"{s_trans_cfg['num_heads']}): one slice of the bias per head")
        has_pe = pos_enc in ('True', 'original', 'cossin')
        if has_pe and tokens > MAX_LEN:
            raise ValueError(f"agcn_amd.aagcn_v24.Model: {tokens} tokens per sequence, the positional table has "
                             f"{MAX_LEN} rows")
        self.need_attn = need_attn
        self.kernel_size = kernel_size
        self.attn_mask = None                    # the null flags of the windows of the last forward (CLS_MASK)
        self.alpha = nn.Parameter(torch.zeros(1))
        self.init_graph(graph, graph_args)

        def _unit(_in, _out, stride=kernel_size, padding=pad, residual=True):
            return TCNGCNUnit(_in, _out, self.graph.A, num_subset=num_subset, kernel_size=kernel_size, stride=stride,
                              pad=padding, residual=residual, adaptive=self.adaptive_fn, attention=attention,
                              gbn_split=gbn_split)

        self.init_model_backbone(model_layers=model_layers, tcngcn_unit=_unit, output_channel=s_trans_cfg['model_dim'])
        if add_A == 'triple':
            A = np.ones((3, 51, 51))
            A[:, 1:26, 1:26] = self.graph.A
            A[:, 26:, 26:] = self.graph.A
        elif add_A == 'single':
            A = np.ones((51, 51))
            A[1:26, 1:26] = self.graph.A[0, :, :]
            A[26:, 26:] = self.graph.A[0, :, :]
        else:
            A = None
        dim = s_trans_cfg['model_dim']
        layer = TransformerEncoderLayerExtV2(cfg=s_trans_cfg, A=A)
        self.s_trans_enc_layers = nn.ModuleList([copy.deepcopy(layer) for _ in range(s_trans_cfg['num_layers'])])
        if pos_enc in ('True', 'original'):
            self.s_pos_encoder = PositionalEncoding(dim, max_len=MAX_LEN)
        elif pos_enc == 'cossin':
            self.s_pos_encoder = CosSinPositionalEncoding(dim, max_len=MAX_LEN)
        else:
            self.s_pos_encoder = lambda x: x
        self.classifier_type = classifier_type
        self.s_cls_token = nn.Parameter(torch.randn(1, 1, dim))
        self.init_fc(dim, num_class)

    def forward_preprocess(self, x, size):
        self.attn_mask = window_null_mask(x, self.kernel_size) if self.classifier_type == 'CLS_MASK' else None
        return super().forward_preprocess(x, size)

    def forward_postprocess(self, x, size):
        N, M = size[0], size[4]
        C, Tp = x.size(1), x.size(2)
        pe = self.s_pos_encoder.pe if isinstance(self.s_pos_encoder, aagcn_v17.PositionalEncodingBase) else None
        if ops.encoder_hip_enabled():
            x = ops.SpatialTokensFunction.apply(x, self.s_cls_token, pe, M)
        else:
            x = ops.tokens_spatial_ref(x, self.s_cls_token, pe, M)
        attn = []
        for layer in self.s_trans_enc_layers:
            bias = None
            if layer.PA is not None:
                bias = (layer.PA if layer.PA.dim() == 3 else layer.PA.unsqueeze(0)) * self.alpha
            x, a = layer(x, bias=bias, need_attn=self.need_attn)
            if self.need_attn:
                attn.append(a)
        x = x[:, 0, :].reshape(N, Tp, C)
        if self.classifier_type == 'CLS_MASK':
            if self.attn_mask.size(1) != Tp:
                raise ValueError(f"agcn_amd.aagcn_v24.Model: the window mask has {self.attn_mask.size(1)} entries for "
                                 f"{Tp} windows (kernel_size, pad and model_layers must give T/kernel_size windows)")
            x = x * self.attn_mask                               # True for NULL windows: kept as the reference has it
        return x.mean(1), attn

    def forward_classifier(self, x, size):
        return self.fc(self.drop_out(x))
