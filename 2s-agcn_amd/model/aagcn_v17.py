"""aagcn_v17: a transformer-encoder head on the windowed AAGCN backbone, on the MI355X-native hot path.

Same public surface as the reference ``model/architecture/aagcn/aagcn_v17.py``: ``PositionalEncoding`` /
``CosSinPositionalEncoding`` (:19-57), ``TransformerEncoderLayerExt`` (:60-101), ``generate_square_subsequent_mask``
(:132-137) and ``Model`` (:145-318) with its constructor arguments, ``forward(x) -> (logits, attn_list)`` and the
identical state_dict (``trans_enc.<i>.self_attn.in_proj_weight`` ..., ``cls_token``, ``pos_encoder.pe``, ``fc.*``).

What runs where: the backbone is ``aagcn.TCNGCNUnit`` with ``kernel_size = stride`` (the windowed temporal convolution
kernels).  The head's tokens, the attention core of every layer (logits, mask, softmax, dropout of the probabilities,
context, head-averaged weights) and the residual add + LayerNorm are the gfx950 kernels of ``csrc/encoder.hip``
(``ops.TokensFunction`` / ``ops.MHAFunction`` / ``ops.AddLayerNormFunction``); the four projections of a layer and its
activation are ``F.linear`` / ATen.  ``AGCN_ENCODER_HIP=0`` runs the same maths as tensor code.

Behaviour kept from the reference as it is: the attention mask applies to the LAST encoder layer only (:303-307); pre-norm
takes the residual from the normed tensor (:82-91); the frame mask is built from the raw input, subsampled
``[::kernel_size]``, flattened in (t, m) order although the tokens are in (m, t) order, and masks (i, j) where both are
null (:255-273).  Deviation: a frame is null when ALL its values are zero (the reference tests ``sum() == 0``), as
``pre_normalization`` here already does.  Combinations on which the reference dies of a shape error inside
``MultiheadAttention`` raise ``ValueError`` instead.  Not supported: ``data_norm='ln'``.
"""
import copy
import math
from typing import Optional

import torch
import torch.nn.functional as F
from torch import nn

from .. import ops
from .aagcn import BaseModel, TCNGCNUnit


class PositionalEncodingBase(nn.Module):
    def __init__(self, d_model: int, dropout: float = 0.0, max_len: int = 601):
        super().__init__()
        self.dropout = nn.Dropout(p=dropout)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self.dropout(x + self.pe[:, :x.size(1), :])


class PositionalEncoding(PositionalEncodingBase):
    def __init__(self, d_model: int, dropout: float = 0.0, max_len: int = 601):
        super().__init__(d_model, dropout, max_len)
        _pe = torch.empty(1, max_len, d_model)
        nn.init.normal_(_pe, std=0.02)
        self.pe = nn.Parameter(_pe)


class CosSinPositionalEncoding(PositionalEncodingBase):
    def __init__(self, d_model: int, dropout: float = 0.0, max_len: int = 601):
        super().__init__(d_model, dropout, max_len)
        position = torch.arange(max_len).unsqueeze(1)
        div_term = torch.exp(torch.arange(0, d_model, 2) * (-math.log(100.0) / d_model))
        pe = torch.zeros(1, max_len, d_model)
        pe[0, :, 0::2] = torch.sin(position * div_term)
        pe[0, :, 1::2] = torch.cos(position * div_term)
        self.register_buffer('pe', pe)


def generate_square_subsequent_mask(sz: int, device: str) -> torch.Tensor:
    """0 where j <= i, -inf elsewhere (reference :132-137, from nn.Transformer)."""
    keep = torch.tril(torch.ones(sz, sz, device=device, dtype=torch.bool))
    return torch.zeros(sz, sz, device=device).masked_fill(~keep, float('-inf'))


CAUSAL = {'forward': 1, 'backward': 2}          # ops.MHAFunction's causal argument: keeps j <= i / j >= i


class TransformerEncoderLayerExt(nn.TransformerEncoderLayer):
    """nn.TransformerEncoderLayer with the choice of pre- or post-norm, returning (output, head-averaged attention).

    The mask arrives as what it is made of instead of an (N*H, L, L) tensor: ``null_tok`` (N, L) uint8, logit (i, j)
    masked where both tokens are null, and ``causal`` (0 none, 1 keeps j <= i, 2 keeps j >= i).  ``need_attn=False``
    skips the head average and returns None for it."""

    def __init__(self, d_model: int, nhead: int, dim_feedforward: int = 2048, dropout: float = 0.1,
                 activation: str = "relu", layer_norm_eps: float = 1e-5, batch_first: bool = False,
                 pre_norm: bool = False) -> None:
        super().__init__(d_model, nhead, dim_feedforward, dropout, activation, layer_norm_eps, batch_first)
        if not batch_first:
            raise ValueError("agcn_amd.aagcn_v17.TransformerEncoderLayerExt: batch_first must be True")
        self.pre_norm = pre_norm

    def forward(self, src: torch.Tensor, src_mask: Optional[torch.Tensor] = None,
                src_key_padding_mask: Optional[torch.Tensor] = None, null_tok: Optional[torch.Tensor] = None,
                causal: int = 0, need_attn: bool = True):
        if src_mask is not None or src_key_padding_mask is not None:
            raise ValueError("agcn_amd.aagcn_v17.TransformerEncoderLayerExt: pass the mask as null_tok / causal, not as "
                             "src_mask / src_key_padding_mask tensors")
        hip = ops.encoder_hip_enabled()
        if hip and not src.is_cuda:
            raise RuntimeError("agcn_amd.aagcn_v17: the encoder kernels need a GPU tensor (AGCN_ENCODER_HIP=0 runs the "
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
            ctx, attn = ops.MHAFunction.apply(qkv, H, null_tok, causal, keep, keep_scale, need_attn)
        else:
            ctx, attn = ops.mha_ref(qkv, H, null_tok, causal, keep, keep_scale, need_attn)
            attn = None if attn is None else attn.detach()
        sa = self.dropout1(F.linear(ctx, att.out_proj.weight, att.out_proj.bias))
        if self.pre_norm:
            x = add_ln(x, sa, n2.weight, n2.bias, n2.eps)
            return x + self.dropout2(self.linear2(self.dropout(self.activation(self.linear1(x))))), attn
        x = add_ln(x, sa, n1.weight, n1.bias, n1.eps)
        ff = self.dropout2(self.linear2(self.dropout(self.activation(self.linear1(x)))))
        return add_ln(x, ff, n2.weight, n2.bias, n2.eps), attn


def frame_null_tokens(x: torch.Tensor, kernel_size: int) -> torch.Tensor:
    """The null flags of the tokens, (N, 1 + (T/kernel_size)*M) uint8, from the raw input (N, C, T, V, M): frame
    t*kernel_size of person m at position 1 + t*M + m (the reference's (t, m) flattening, :261-264), 0 for CLS.
    A frame is null when all its values are zero."""
    null = ~(x != 0).any(dim=3).any(dim=1)                      # N, T, M
    null = null[:, ::kernel_size, :].reshape(x.size(0), -1)
    zeros = torch.zeros(x.size(0), 1, dtype=torch.bool, device=x.device)
    return torch.cat((zeros, null), dim=1).to(torch.uint8).contiguous()


class Model(BaseModel):
    def __init__(self, num_class: int = 60, num_point: int = 25, num_person: int = 2, num_subset: int = 3,
                 graph: Optional[str] = None, graph_args: dict = dict(), in_channels: int = 3, drop_out: int = 0,
                 adaptive: bool = True, attention: bool = True, gbn_split: Optional[int] = None, data_norm: str = 'bn',
                 kernel_size: int = 9, pad: bool = True, need_attn: bool = False, attn_masking: str = 'False',
                 trans_num_heads: int = 2, trans_model_dim: int = 16, trans_ffn_dim: int = 64,
                 trans_dropout: float = 0.2, trans_activation: str = "gelu", trans_prenorm: bool = False,
                 trans_num_layers: int = 1, pos_enc: str = 'True', classifier_type: str = 'CLS',
                 model_layers: int = 10):
        super().__init__(num_class=num_class, num_point=num_point, num_person=num_person, in_channels=in_channels,
                         drop_out=drop_out, adaptive=adaptive, gbn_split=gbn_split, data_norm=data_norm)
        attn_masking = str(attn_masking)
        if classifier_type not in ('CLS', 'GAP'):
            raise ValueError(f"agcn_amd.aagcn_v17.Model: unknown classifier_type {classifier_type!r}")
        if attn_masking in ('True', 'frame', 'forward', 'backward') and (classifier_type != 'CLS' or model_layers != 101):
            raise ValueError(f"agcn_amd.aagcn_v17.Model: attn_masking={attn_masking!r} needs classifier_type='CLS' and "
                             f"model_layers=101 (got classifier_type={classifier_type!r}, model_layers={model_layers}): "
                             f"the mask has 1 + T*M/kernel_size rows, which is the token count only with a CLS token "
                             f"and one windowing layer")
        self.attn_masking = attn_masking
        self.attn_mask = None                    # the token null flags of the last forward (frame masking)
        self.trans_num_heads = trans_num_heads
        self.kernel_size = kernel_size
        self.need_attn = need_attn
        self.init_graph(graph, graph_args)

        def _unit(_in, _out, stride=1, residual=True):
            return TCNGCNUnit(_in, _out, self.graph.A, num_subset=num_subset, kernel_size=kernel_size,
                              stride=kernel_size, pad=pad, residual=residual, adaptive=self.adaptive_fn,
                              attention=attention, gbn_split=gbn_split)

        self.init_model_backbone(model_layers=model_layers, tcngcn_unit=_unit, output_channel=trans_model_dim)
        trans_dim = trans_model_dim * num_point
        pos_enc = str(pos_enc)
        if pos_enc in ('True', 'original'):
            self.pos_encoder = PositionalEncoding(trans_dim)
        elif pos_enc == 'cossin':
            self.pos_encoder = CosSinPositionalEncoding(trans_dim)
        else:
            self.pos_encoder = lambda x: x
        self.classifier_type = classifier_type
        self.cls_token = nn.Parameter(torch.randn(1, 1, trans_dim)) if classifier_type == 'CLS' else None
        layer = TransformerEncoderLayerExt(d_model=trans_dim, nhead=trans_num_heads,
                                           dim_feedforward=trans_ffn_dim * num_point, dropout=trans_dropout,
                                           activation=trans_activation, layer_norm_eps=1e-5, batch_first=True,
                                           pre_norm=trans_prenorm)
        self.trans_enc = nn.ModuleList([copy.deepcopy(layer) for _ in range(trans_num_layers)])
        self.init_fc(trans_dim, num_class)

    def forward_preprocess(self, x, size):
        N, C, T, V, M = size
        self.attn_mask = None
        if self.attn_masking in ('True', 'frame', 'forward', 'backward') and T % self.kernel_size != 0:
            raise ValueError(f"agcn_amd.aagcn_v17.Model: attn_masking={self.attn_masking!r} needs T % kernel_size == 0 "
                             f"(got T={T}, kernel_size={self.kernel_size})")
        if self.attn_masking in ('True', 'frame'):
            self.attn_mask = frame_null_tokens(x, self.kernel_size)
        return super().forward_preprocess(x, size)

    def forward_postprocess(self, x, size):
        M = size[4]
        pe = self.pos_encoder.pe if isinstance(self.pos_encoder, PositionalEncodingBase) else None
        if ops.encoder_hip_enabled():
            x = ops.TokensFunction.apply(x, self.cls_token, pe, M)
        else:
            x = ops.tokens_ref(x, self.cls_token, pe, M)
        if self.attn_mask is not None and self.attn_mask.size(1) != x.size(1):
            raise ValueError(f"agcn_amd.aagcn_v17.Model: the frame mask has {self.attn_mask.size(1)} entries for "
                             f"{x.size(1)} tokens (kernel_size, pad and model_layers must give T/kernel_size tokens "
                             f"per person)")
        attn = []
        last = len(self.trans_enc) - 1
        for i, layer in enumerate(self.trans_enc):
            masked = i == last                                   # the reference masks its last layer only (:303-307)
            x, a = layer(x, null_tok=self.attn_mask if masked else None,
                         causal=CAUSAL.get(self.attn_masking, 0) if masked else 0, need_attn=self.need_attn)
            if self.need_attn:
                attn.append(a)
        x = x[:, 0, :] if self.classifier_type == 'CLS' else x.mean(1)
        return x, attn

    def forward_classifier(self, x, size):
        return self.fc(self.drop_out(x))
