"""SGN v15, the attention SGN (reference model/architecture/sgn/sgn_v15.py): the base SGN's input side -- two DataNorm +
1x1 embeddings of position and velocity, the one-hot joint and frame embeddings, maximum over joints, maximum over frames,
fc -- with one pre-norm multi-head-attention block (reference model/layers/attention/crossattention.py::Transformer) over
the joints of a frame in place of the three adaptive graph convolutions and the same block over the frames of a clip in
place of the temporal CNN.  Constructor arguments, module tree and state_dict keys are the reference's, so a trained
``sgn-*.pt`` loads as it is; the class constructs without a GPU and needs neither einops nor torchinfo.

Two routes:

* eval mode under ``no_grad`` on the GPU in the structure of the reference's experiment yaml (``_fusable``): two HIP
  launches (csrc/sgn_v15.hip) on weight images with every BatchNorm folded -- ``ops.sgn15_frames`` (input side + the
  spatial block + maximum over joints) and ``ops.sgn15_clip`` (+ tem_emb, the temporal block, maximum over frames, fc).
  The images are cached under ``ops._cache_key`` and rebuilt after any parameter or running statistic changes; a batch
  of more than ``ops.SGN15_MAX_CLIPS`` clips goes through in chunks of whole clips with the same bits.  With
  ``fused_attention = True`` (a plain attribute, off by default, not in the state_dict) the kernels also store the
  attention maps.
* everything else (grad mode, ``train()``, a CPU tensor, any other supported configuration, ``AGCN_SGN_HIP=0``): the
  tensor-code composition ``forward_tensor``, channels last, a complete ``nn.Module`` in every mode.  It is the
  comparison of the fused path, NOT the hot path, and is counted in ``ops.SGN_STATS['forward_tensor']``.

``input_gradient`` (what ``explain()`` of an online recogniser asks for) has the same two routes: with
``fused_input_gradient = True`` (a plain attribute, off by default, not in the state_dict) the fused forward followed by
``ops.sgn15_clip_bwd`` and ``ops.sgn15_frames_bwd`` (csrc/sgn_v15_bwd.hip) on transposed weight images cached with the
forward ones, otherwise torch autograd on the composition.

Frozen-BatchNorm fine-tuning: with ``fused_finetune = True`` (a plain attribute, off by default, not in the state_dict),
eval mode, grad mode and some parameter that requires grad, ``forward`` is ``ops.SGN15FineTuneFunction``: the two forward
launches, and in ``backward()`` the two taping backward launches and the fixed-order reductions of
csrc/sgn_v15_wgrad.hip, which give the gradients of the two folded images; torch autograd takes them through the fold
(``_finetune_images``, a fresh fold per call) to the parameters.  ``parameter_gradients`` is the same route without
autograd state.  Nothing of the forward is stored but feat; the tapes are capped by ``ops.SGN_MAX_TAPE_BYTES``.

``batch_statistics(x)`` / ``recalibrate_bn(x)`` in any ``training`` state: the batch statistics of the six BatchNorms of x
as one batch and the logits under them (the forward half of train-mode BatchNorm, every dropout off), on the fused
structure as the base SGN's input pass, four truncated passes of the fused forward (csrc/sgn_v15_stats.hip) on freshly
folded images and the two full-depth launches; otherwise the composition with its BatchNorms in batch mode.  The
backward of batch-mode BatchNorm is not built in HIP.

One block, with n_a, n_f the two per-channel BatchNorms: a = softmax_j((n_a(x) Wq)(n_a(x) Wk)^T d_head^-1/2) per head,
x1 = concat_h(a . n_a(x) Wv) Wo + bo + res_a(x), y = relu(n_f(x1) W1 + b1) W2 + b2 + res_f(x1): both residuals take the
un-normalised input, and a residual is a Linear where the widths differ (crossattention.py:297-304)."""
import math
from collections import OrderedDict

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops

_EMB_MODES = (0, 1)


def _unsupported(what):
    raise NotImplementedError(f"agcn_amd.sgn_v15: {what}")


class DataNorm(nn.Module):
    """BatchNorm1d over the C*V features of a frame, feature c*V + v (reference blocks/semantic.py:21-31), on
    channels-last x (bs, step, V, C)."""

    def __init__(self, dim):
        super().__init__()
        self.bn = nn.BatchNorm1d(dim)

    def forward(self, x):
        bs, step, V, C = x.shape
        y = self.bn(x.permute(0, 3, 2, 1).reshape(bs, C * V, step))
        return y.reshape(bs, C, V, step).permute(0, 3, 2, 1)


class _Conv1x1(nn.Module):
    """reference block.py::Conv1xN at kernel size 1: the Conv2d holds the parameters, applied as a linear map."""

    def __init__(self, cin, cout, bias):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, kernel_size=(1, 1), bias=bool(bias))

    def forward(self, x):
        return F.linear(x, self.conv.weight.flatten(1), self.conv.bias)


class Conv(nn.Module):
    """reference block.py::Conv as Embedding builds it: conv + activation under ``block``."""

    def __init__(self, cin, cout, bias):
        super().__init__()
        self.block = nn.Sequential(OrderedDict(conv=_Conv1x1(cin, cout, bias), act=nn.ReLU()))

    def forward(self, x):
        return self.block(x)


class Embedding(nn.Module):
    """Mode 1 of the reference's Embedding (blocks/semantic.py:34-125): [DataNorm,] two 1x1 convs with ReLU."""

    def __init__(self, in_channels, out_channels, bias, num_point, in_norm):
        super().__init__()
        self.norm = DataNorm(in_channels * num_point) if in_norm else nn.Identity()
        self.cnn1 = Conv(in_channels, out_channels, bias)
        self.cnn2 = Conv(out_channels, out_channels, bias)

    def forward(self, x):
        return self.cnn2(self.cnn1(self.norm(x)))


class FeatureExtractor(nn.Module):
    def __init__(self, in_pos, in_vel, in_channels, out_channels, bias, num_point, fusion):
        super().__init__()
        self.fusion, self.in_pos, self.in_vel = fusion, in_pos, in_vel
        if in_pos > 0:
            self.pos_embed = Embedding(in_channels, out_channels, bias, num_point, True)
        if in_vel > 0:
            self.vel_embed = Embedding(in_channels, out_channels, bias, num_point, True)
        if in_pos == 0 and in_vel == 0:
            raise ValueError("Input args are faulty...")

    def forward(self, x):
        """x (bs, step, V, C); velocity is x[t] - x[t - 1] with a zero at t = 0."""
        if self.in_vel > 0:
            dif = torch.cat([x.new_zeros(x.shape[0], 1, *x.shape[2:]), x[:, 1:] - x[:, :-1]], dim=1)
        if self.in_pos > 0 and self.in_vel > 0:
            pos, vel = self.pos_embed(x), self.vel_embed(dif)
            return torch.cat([pos, vel], dim=3) if self.fusion == 0 else pos + vel
        return self.pos_embed(x) if self.in_pos > 0 else self.vel_embed(dif)


class OneHotTensor(nn.Module):
    """The reference's persistent one-hot buffer, in its shape: mode 0 (1, V, V, seg) one-hot over the joint, mode 1
    (1, seg, V, seg) one-hot over the frame (blocks/semantic.py:128-146)."""

    def __init__(self, dim_eye, dim_length, mode):
        super().__init__()
        eye = torch.eye(dim_eye)[None, None].repeat(1, dim_length, 1, 1)
        self.register_buffer('onehot', (eye.permute(0, 3, 2, 1) if mode == 0 else eye.permute(0, 3, 1, 2)).contiguous())


class SemanticEmbedding(nn.Module):
    def __init__(self, num_point, num_segment, sem_spa, sem_tem, spa_out, tem_out, bias):
        super().__init__()
        self.sem_spa, self.sem_tem = sem_spa, sem_tem
        if sem_spa > 0:
            self.spa_onehot = OneHotTensor(num_point, num_segment, 0)
            self.spa_embedding = Embedding(num_point, spa_out, bias, num_point, False)
        if sem_tem > 0:
            self.tem_onehot = OneHotTensor(num_segment, num_point, 1)
            self.tem_embedding = Embedding(num_segment, tem_out, bias, num_point, False)

    def spa(self):
        """(V, C): the input-independent joint embedding, or None."""
        return self.spa_embedding(self.spa_onehot.onehot[0, :, :, 0].t()) if self.sem_spa > 0 else None

    def tem(self):
        """(seg, C): the input-independent frame embedding, or None."""
        return self.tem_embedding(self.tem_onehot.onehot[0, :, 0, :].t()) if self.sem_tem > 0 else None


class Normalize(nn.Module):
    """BatchNorm1d over the channels of (b, n, c) tokens (crossattention.py:37-43)."""

    def __init__(self, fn):
        super().__init__()
        self.fn = fn

    def forward(self, x):
        return self.fn(x.transpose(1, 2)).transpose(1, 2)


class PreNorm(nn.Module):
    def __init__(self, dim, fn):
        super().__init__()
        self.norm = Normalize(nn.BatchNorm1d(dim))
        self.fn = fn

    def forward(self, x):
        return self.fn(self.norm(x))


def _residual(dim, output_dim, force=False):
    return nn.Linear(dim, output_dim) if force or dim != output_dim else nn.Identity()


class Attention(nn.Module):
    def __init__(self, dim, heads, dim_head, dropout, res_proj, output_dim):
        super().__init__()
        inner = dim_head * heads
        self.heads, self.dim_head, self.scale = heads, dim_head, dim_head ** -0.5
        self.to_q = nn.Linear(dim, inner, bias=False)
        self.to_k = nn.Linear(dim, inner, bias=False)
        self.to_v = nn.Linear(dim, inner, bias=False)
        self.to_out = nn.Sequential(OrderedDict(linear=nn.Linear(inner, output_dim), dropout=nn.Dropout(dropout)))
        self.residual = _residual(dim, output_dim, res_proj)

    def forward(self, x):
        b, n, _ = x.shape
        q, k, v = (t(x).reshape(b, n, self.heads, self.dim_head).transpose(1, 2) for t in (self.to_q, self.to_k, self.to_v))
        attn = torch.softmax(q.matmul(k.transpose(-1, -2)) * self.scale, dim=-1)
        out = attn.matmul(v).transpose(1, 2).reshape(b, n, self.heads * self.dim_head)
        return self.to_out(out), attn


class FeedForward(nn.Module):
    def __init__(self, dim, hidden_dim, dropout, output_dim):
        super().__init__()
        output_dim = output_dim or dim
        self.net = nn.Sequential(OrderedDict(linear1=nn.Linear(dim, hidden_dim), relu=nn.ReLU(), dropout1=nn.Dropout(dropout),
                                             linear2=nn.Linear(hidden_dim, output_dim), dropout2=nn.Dropout(dropout)))
        self.residual = _residual(dim, output_dim)

    def forward(self, x):
        return self.net(x)


def _per_layer(v, depth, kind):
    v = [v] * depth if isinstance(v, kind) else v
    assert isinstance(v, list) and len(v) >= depth
    return v


class Transformer(nn.Module):
    """The pre-norm BatchNorm / relu branch of crossattention.py::Transformer."""

    def __init__(self, dim, depth, heads, dim_head, mlp_dim, dropout, mlp_out_dim, global_norm, d_out=None, res_proj=False):
        super().__init__()
        dim, heads, dim_head, mlp_dim, mlp_out_dim = (_per_layer(v, depth, int) for v in (dim, heads, dim_head, mlp_dim,
                                                                                            mlp_out_dim))
        dropout = _per_layer(float(dropout) if isinstance(dropout, (int, float)) else dropout, depth, float)
        d_out = dim if d_out is None else _per_layer(d_out, depth, int)
        self.layers = nn.ModuleDict()
        for i in range(depth):
            attn = Attention(dim[i], heads[i], dim_head[i], dropout[i], res_proj, d_out[i])
            ffn = FeedForward(d_out[i], mlp_dim[i], dropout[i], mlp_out_dim[i])
            self.layers[f'l{i + 1}'] = nn.ModuleDict(OrderedDict(attn=PreNorm(dim[i], attn), ffn=PreNorm(d_out[i], ffn)))
        self.norm = Normalize(nn.BatchNorm1d(mlp_out_dim[-1] or dim[-1])) if global_norm else nn.Identity()

    def forward(self, x):
        attn_list = []
        for layer in self.layers.values():
            x1, attn = layer['attn'](x)
            x = x1 + layer['attn'].fn.residual(x)
            x = layer['ffn'](x) + layer['ffn'].fn.residual(x)
            attn_list.append(attn)
        return self.norm(x), attn_list


class MHA(nn.Module):
    def __init__(self, name, kwargs):
        super().__init__()
        kw = dict(kwargs or {})
        if 'norm' not in kw:
            _unsupported(f"{name} without 'norm' selects the reference's nn.TransformerEncoderLayer branch")
        if kw.get('post_norm', False):
            _unsupported(f"{name}: post_norm")
        if 'bn' not in str(kw['norm']):
            _unsupported(f"{name}: norm {kw['norm']!r} (only 'bn')")
        if kw.get('activation', 'gelu') != 'relu':
            _unsupported(f"{name}: activation {kw.get('activation', 'gelu')!r} (only 'relu')")
        self.transformer = Transformer(dim=kw['d_model'], depth=kw['num_layers'], heads=kw['nhead'], dim_head=kw['d_head'],
                                       mlp_dim=kw['dim_feedforward'], dropout=kw['dropout'],
                                       mlp_out_dim=kw['dim_feedforward_output'], global_norm=kw['global_norm'],
                                       d_out=kw.get('d_out'), res_proj=kw.get('res_proj', False))

    def forward(self, x):
        """x (bs, step, V, C) -> (y, [attn per layer]): tokens are the joints of a frame (spatial) or the frames of a clip
        with the joints' channels side by side (temporal)."""
        raise NotImplementedError


class SpatialMHA(MHA):
    def forward(self, x):
        bs, step, V, C = x.shape
        y, attn = self.transformer(x.reshape(bs * step, V, C))
        return y.reshape(bs, step, V, -1), attn


class TemporalMHA(MHA):
    def forward(self, x):
        bs, step, V, C = x.shape
        y, attn = self.transformer(x.reshape(bs, step, V * C))
        return y.reshape(bs, step, V, -1), attn


def _cf(x):
    """(bs, step, V, C) -> the reference's (bs, C, V, step), as a view."""
    return x.permute(0, 3, 2, 1)


_t = ops._sgn_t


class SGN(nn.Module):
    def __init__(self, num_class=60, num_point=25, num_segment=20, in_channels=3, bias=1, dropout=0.0, dropout2d=0.0,
                 c_multiplier=1, norm_type='bn-pre', act_type='relu', input_position=1, input_velocity=1, semantic_joint=1,
                 semantic_frame=1, semantic_class=0, input_emb_fusion=1, semantic_joint_fusion=0, semantic_frame_fusion=1,
                 semantic_frame_location=0, spatial_maxpool=1, temporal_maxpool=1, spatial_mha_kwargs=None,
                 temporal_mha_kwargs=None):
        super().__init__()
        for name, mode in (('input_position', input_position), ('input_velocity', input_velocity),
                           ('semantic_joint', semantic_joint), ('semantic_frame', semantic_frame)):
            if mode not in _EMB_MODES:
                _unsupported(f"{name} = {mode}: only the embedding modes 0 and 1 are built")
        if semantic_class != 0:
            _unsupported(f"semantic_class = {semantic_class}")
        if 'bn' not in str(norm_type):
            _unsupported(f"norm_type {norm_type!r} (only 'bn')")
        if act_type != 'relu':
            _unsupported(f"act_type {act_type!r} (only 'relu')")
        for name, v in (('spatial_maxpool', spatial_maxpool), ('temporal_maxpool', temporal_maxpool)):
            if v not in (0, 1):
                _unsupported(f"{name} = {v}")
        for name, v in (('input_emb_fusion', input_emb_fusion), ('semantic_joint_fusion', semantic_joint_fusion)):
            if v not in (0, 1):
                raise ValueError(f"agcn_amd.sgn_v15: {name} must be 0 (concat) or 1 (sum)")
        if input_position == 0 and semantic_joint > 0:
            raise ValueError("input_position is 0 but semantic_joint is not")
        assert semantic_frame_location in (0, 1)
        if isinstance(c_multiplier, (int, float)):
            c_multiplier = [c_multiplier] * 4
        elif not isinstance(c_multiplier, list):
            raise ValueError("Unknown c_multiplier type")
        self.c1, self.c2, self.c3, self.c4 = (int(c * m) for c, m in zip((64, 128, 256, 512), c_multiplier))
        self.num_class, self.num_point, self.num_segment, self.in_channels = num_class, num_point, num_segment, in_channels
        self.bias = bias
        self.input_position, self.input_velocity = input_position, input_velocity
        self.semantic_joint, self.semantic_frame, self.semantic_class = semantic_joint, semantic_frame, semantic_class
        self.input_emb_fusion, self.semantic_joint_fusion = input_emb_fusion, semantic_joint_fusion
        self.semantic_frame_fusion, self.semantic_frame_location = semantic_frame_fusion, semantic_frame_location
        self.spatial_maxpool, self.temporal_maxpool = spatial_maxpool, temporal_maxpool
        self.fc_dropout = nn.Dropout(dropout)

        self.feature_extractor = FeatureExtractor(input_position, input_velocity, in_channels, self.c1, bias, num_point,
                                                  input_emb_fusion)
        sem_out = self.c2 if input_emb_fusion == 0 else self.c1
        self.semantic_embedding = SemanticEmbedding(num_point, num_segment, semantic_joint, semantic_frame, sem_out,
                                                    self.c3, bias)
        self.spatial_mha = SpatialMHA('spatial_mha_kwargs', spatial_mha_kwargs)
        self.temporal_mha = TemporalMHA('temporal_mha_kwargs', temporal_mha_kwargs)
        self._mha_args = tuple({k: kw.get(k) for k in ('d_model', 'nhead', 'd_head', 'dim_feedforward', 'num_layers',
                                                       'dim_feedforward_output', 'global_norm', 'd_out', 'res_proj')}
                               for kw in (spatial_mha_kwargs, temporal_mha_kwargs))

        fc_in = self.c4                    # the reference's arithmetic (sgn_v15.py:234-238)
        if spatial_maxpool == 0 and temporal_maxpool == 0:
            fc_in = fc_in * num_segment * num_point
        if temporal_maxpool == 0:
            fc_in = fc_in * num_segment
        self.fc = nn.Linear(fc_in, num_class)

        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                n = m.kernel_size[0] * m.kernel_size[1] * m.out_channels
                m.weight.data.normal_(0, math.sqrt(2. / n))
        self._infer_cache = {}
        self.fused_attention = False       # opt in: the fused route also stores and returns the attention maps
        self.fused_input_gradient = False  # opt in: input_gradient through the HIP backward (csrc/sgn_v15_bwd.hip)
        self.fused_finetune = False        # opt in: eval-mode backward() to the parameters on the HIP kernels

    @property
    def seg(self):
        """The name the base SGN and the online recognisers use for ``num_segment``."""
        return self.num_segment

    # ---- tensor-code composition ----
    def _forward_tensor(self, x):
        """-> (logits, aux, feat): feat is the input of the temporal block (bs, step, V or 1, C)."""
        bs, step, dim = x.shape
        V = dim // self.in_channels
        x = x.reshape(bs, step, V, self.in_channels)
        h = self.feature_extractor(x)
        spa, tem = self.semantic_embedding.spa(), self.semantic_embedding.tem()
        if spa is not None:
            spa_x = spa[None, None].expand(bs, step, V, spa.shape[1])
            h = torch.cat([h, spa_x], dim=3) if self.semantic_joint_fusion == 0 else h + spa_x
        if tem is not None and self.semantic_frame_location == 1:
            h = h + tem[None, :, None, :]
        spatial, spatial_attn = self.spatial_mha(h)
        h = spatial
        if tem is not None and self.semantic_frame_location == 0:
            h = h + tem[None, :, None, :]
        if self.spatial_maxpool == 1:                          # plain maxima: no ReLU in front
            h = h.amax(2, keepdim=True)
        feat = h
        temporal, temporal_attn = self.temporal_mha(h)
        y = temporal.amax((1, 2), keepdim=True) if self.temporal_maxpool == 1 else temporal
        y = self.fc(self.fc_dropout(_cf(y).flatten(1)))
        aux = dict(tem_emb=None if tem is None else tem.t()[None, :, None, :].expand(bs, tem.shape[1], V, step),
                   spa_emb=None if spa is None else spa.t()[None, :, :, None].expand(bs, spa.shape[1], V, step),
                   spatial_attn_list=spatial_attn, temporal_attn_list=temporal_attn,
                   spatial_featuremap=_cf(spatial), temporal_featuremap=_cf(temporal))
        return y, aux, feat

    def forward_tensor(self, x):
        logits, aux, _ = self._forward_tensor(x)
        return logits, aux

    # ---- folded weight images of the HIP path ----
    def _structure_fused(self):
        """The structure of the reference's experiment yaml at sizes inside the kernels' domain."""
        s, t = self._mha_args
        if not (self.input_position == self.input_velocity == self.semantic_joint == self.semantic_frame == 1
                and self.input_emb_fusion == 1 and self.semantic_joint_fusion == 0 and self.semantic_frame_location == 0
                and self.spatial_maxpool == self.temporal_maxpool == 1 and self.in_channels == 3
                and (self.c1, self.c2, self.c3, self.c4) == (64, 128, 256, 512)):
            return False
        for a, din, dout in ((s, 128, 256), (t, 256, 512)):
            one = lambda v: v[0] if isinstance(v, list) else v      # noqa: E731
            if (a['num_layers'] != 1 or a['global_norm'] or a['res_proj'] or one(a['d_model']) != din
                    or one(a['dim_feedforward_output']) != dout or (a['d_out'] is not None and one(a['d_out']) != din)):
                return False
        return True

    def _geometry(self):
        """((heads, d_head, ff) of the spatial block, of the temporal block)."""
        out = []
        for m in (self.spatial_mha, self.temporal_mha):
            l1 = m.transformer.layers['l1']
            out.append((l1['attn'].fn.heads, l1['attn'].fn.dim_head, l1['ffn'].fn.net.linear1.out_features))
        return tuple(out)

    @staticmethod
    def _block_base(layer):
        """The unfolded matrices the two BatchNorms of a block are folded into -> ([Wq d_head^-1/2 | Wk | Wv] (DIN, 3 inner),
        W1 (DIN, ff), b1)."""
        att, ffn = layer['attn'].fn, layer['ffn'].fn
        wqkv = torch.cat([att.to_q.weight.t() * att.scale, att.to_k.weight.t(), att.to_v.weight.t()], dim=1)
        return wqkv, ffn.net.linear1.weight.t(), ffn.net.linear1.bias

    @staticmethod
    def _running(bn):
        return ops._fold((bn.weight, bn.bias, bn.running_mean, bn.running_var))

    @classmethod
    def _fold_block(cls, layer, fold=None):
        """One block's sections in the order of csrc/sgn_v15_plan.h::Sgn15BlockW; ``fold(bn)`` -> (scale, shift), by
        default on the running statistics."""
        fold = fold or cls._running
        a, f = layer['attn'], layer['ffn']
        att, ffn = a.fn, f.fn
        sa, sha = fold(a.norm.fn)
        sf, shf = fold(f.norm.fn)
        wqkv, w1, b1 = cls._block_base(layer)
        return [wqkv * sa[:, None], sha @ wqkv,
                att.to_out.linear.weight.t(), att.to_out.linear.bias,
                w1 * sf[:, None], shf @ w1 + b1,
                torch.cat([ffn.net.linear2.weight.t(), ffn.residual.weight.t()]), ffn.net.linear2.bias + ffn.residual.bias]

    def _folded(self, override=None):
        """The folded tensors in the order of the two weight images -> (frames list, clip list).  ``override``:
        {BatchNorm module name: (mean, var)} folds that BatchNorm on the given statistics (in the module's own feature
        order) instead of its running ones: the images of the batch-statistics passes.  Without it every BatchNorm is
        folded on its running statistics."""
        V, like = self.num_point, self.fc.weight
        fe = self.feature_extractor
        names = {m: n for n, m in self.named_modules()} if override else {}

        def fold(bn):
            if override and names[bn] in override:
                mean, var = override[names[bn]]
                return ops._fold((bn.weight, bn.bias, mean, var))
            return self._running(bn)

        def emb(e):
            a, b = e.cnn1.block.conv.conv, e.cnn2.block.conv.conv
            bias = lambda c: c.bias if c.bias is not None else like.new_zeros(c.out_channels)      # noqa: E731
            return [_t(a.weight), bias(a), _t(b.weight), bias(b)]

        aff = []
        for e in (fe.pos_embed, fe.vel_embed):              # BatchNorm feature c*V + v -> [v*3 + c]
            aff += [c.reshape(3, V).t() for c in fold(e.norm.bn)]
        frames = (aff + emb(fe.pos_embed) + emb(fe.vel_embed) + [self.semantic_embedding.spa()]
                  + self._fold_block(self.spatial_mha.transformer.layers['l1'], fold))
        clip = ([self.semantic_embedding.tem()] + self._fold_block(self.temporal_mha.transformer.layers['l1'], fold)
                + [self.fc.weight.t(), self.fc.bias])
        return frames, clip

    @staticmethod
    def _flatten(frames, clip):
        """The two folded lists -> (frames image, clip image), each one flat tensor."""
        return torch.cat([t.reshape(-1) for t in frames]), torch.cat([t.reshape(-1) for t in clip])

    def _images(self):
        """-> (frames image, clip image, spa table (V, 64), tem table (seg, 256)), cached."""
        key = ops._cache_key(list(self.parameters()) + list(self.buffers()))
        f = self._infer_cache.get('images')
        if f is None or f[0] != key:
            with torch.no_grad():          # whatever the caller's grad mode: the cache holds leaves without a graph
                frames, clip = self._folded()
                secs = {n: (o, s) for n, o, s in ops.sgn15_image_sections(self.num_point, self.num_segment, self.num_class,
                                                                          *self._geometry())[0]}
                wf = torch.cat([t.reshape(-1) for t in frames])
                wc = torch.cat([t.reshape(-1) for t in clip])
                o, s = secs['spa']
                wf_t, wc_t = ops.sgn15_transpose_images(wf, wc, self.num_point, self.num_segment, self.num_class,
                                                        *self._geometry())
                f = self._infer_cache['images'] = (key, wf, wc, wf[o:o + math.prod(s)].view(s),
                                                   wc[:self.num_segment * 256].view(self.num_segment, 256), wf_t, wc_t)
        return f[1:5]

    def _images_t(self):
        """-> (transposed frames image, transposed clip image) of the input-gradient kernels, cached with ``_images``
        under the same key and rebuilt with them."""
        self._images()
        return self._infer_cache['images'][5:]

    def _fusable(self, x):
        """What the eval-mode kernels take, whatever the grad mode."""
        if self.training or not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 3 and x.is_contiguous()):
            return False
        if x.shape[1] != self.num_segment or x.shape[2] != 3 * self.num_point or x.shape[0] < 1:
            return False
        if not (ops.sgn_hip_enabled() and self._structure_fused()):
            return False
        sp, tp = self._geometry()
        return (ops.sgn15_weights_floats(self.num_point, self.num_segment, self.num_class, sp, tp) is not None)

    def _bwd_domain(self):
        return ops.sgn15_bwd_weights_floats(self.num_point, self.num_segment, self.num_class, *self._geometry()) is not None

    def _fused_finetune(self, x):
        """The flag, eval mode, grad mode, the forward's and the backward's domain, and something to train."""
        return (self.fused_finetune and torch.is_grad_enabled() and self._fusable(x) and self._bwd_domain()
                and any(p.requires_grad for p in self.parameters()))

    def _finetune_images(self):
        """The four images for ``ops.SGN15FineTuneFunction``: the forward ones in the CURRENT grad mode from a fresh fold
        (never from ``_infer_cache``: they carry the autograd graph of this call), the transposed ones without grad from
        the same numbers."""
        frames, clip = self._folded()
        wf = torch.cat([t.reshape(-1) for t in frames])
        wc = torch.cat([t.reshape(-1) for t in clip])
        with torch.no_grad():
            wf_t, wc_t = ops.sgn15_transpose_images(wf.detach(), wc.detach(), self.num_point, self.num_segment,
                                                    self.num_class, *self._geometry())
        return wf, wc, wf_t, wc_t

    def _finetune_aux(self, N):
        """The embeddings' tables, as the fused forward returns them; the taping route stores no attention maps."""
        with torch.no_grad():
            aux = self._fused_aux(N, None, None)
        aux['spatial_attn_list'] = aux['temporal_attn_list'] = None
        return aux

    def forward(self, x):
        if self._fused_finetune(x):
            logits = ops.SGN15FineTuneFunction.apply(x, *self._finetune_images(), self.num_point, self.num_class,
                                                     *self._geometry())
            return logits, self._finetune_aux(x.shape[0])
        if torch.is_grad_enabled() or not self._fusable(x):
            ops.SGN_STATS['forward_tensor'] += 1
            return self.forward_tensor(x)
        wf, wc, _, _ = self._images()
        logits, _, sa, ta = ops.sgn15_fused_forward(x, wf, wc, self.num_point, self.num_class, *self._geometry(),
                                                    want_attn=self.fused_attention)
        return logits, self._fused_aux(x.shape[0], sa, ta)

    def _fused_aux(self, N, sa, ta):
        _, _, spa, tem = self._images()
        seg, V = self.num_segment, self.num_point
        return dict(tem_emb=tem.t()[None, :, None, :].expand(N, 256, V, seg),
                    spa_emb=spa.t()[None, :, :, None].expand(N, 64, V, seg),
                    spatial_attn_list=[sa] if self.fused_attention else None,
                    temporal_attn_list=[ta] if self.fused_attention else None)

    def _fused_gradient(self, x):
        """Whether ``input_gradient`` takes the HIP route for x: opted in, the forward's conditions, and both transposed
        images inside the backward's domain."""
        return self.fused_input_gradient and self._fusable(x) and self._bwd_domain()

    def parameter_gradients(self, x, cot, rows_per_split=0, max_tape_bytes=None):
        """-> (logits, aux, dx, {name: grad}) with the gradients of sum(logits * cot) in eval mode (BatchNorm on its running
        statistics), for every parameter that requires grad.  Needs no prior autograd state and leaves every ``.grad``
        alone.  On what the fused forward and the HIP backward take, the batch dimension is all HIP: the two forward
        launches, the two taping backward launches and the reductions of ``ops.sgn15_image_gradients`` (counted in
        ``ops.SGN15_STATS`` and ``ops.SGN15_WGRAD_STATS``); torch autograd only takes the two image gradients through the
        fold.  Otherwise the composition with torch autograd (counted in ``ops.SGN_STATS['forward_tensor']``).
        ``rows_per_split`` / ``max_tape_bytes``: see ``ops.sgn15_image_gradients``."""
        if self.training:
            raise ValueError("agcn_amd: SGN.parameter_gradients is the eval-mode gradient; call eval() first")
        named = [(n, p) for n, p in self.named_parameters() if p.requires_grad]
        if not (self._fusable(x) and self._bwd_domain()):
            ops.SGN_STATS['forward_tensor'] += 1
            logits, aux, dx, grads = ops.sgn_composition_gradients(self.forward_tensor, x, cot, [p for _, p in named])
            return logits, aux, dx, ops.sgn_named_gradients(named, grads)
        with torch.enable_grad():
            wf, wc, wf_t, wc_t = self._finetune_images()
        cap = ops.SGN_MAX_TAPE_BYTES if max_tape_bytes is None else max_tape_bytes
        logits, dx, d_wf, d_wc = ops.sgn15_image_gradients(x, wf.detach(), wc.detach(), wf_t, wc_t, cot, self.num_point,
                                                           self.num_class, *self._geometry(), rows_per_split, cap)
        grads = ops.sgn_fold_gradients((wf, wc), (d_wf, d_wc), named)
        return logits, self._finetune_aux(x.shape[0]), dx, grads

    def input_gradient(self, x, cot):
        """-> (logits, aux, dx) with dx = d sum(logits * cot) / dx in eval mode.  Needs no autograd state and ignores the
        parameters' requires_grad.  Two routes:

        * ``fused_input_gradient = True`` (a plain attribute, off by default, not in the state_dict) on what the fused
          forward takes: the two forward launches, then ``ops.sgn15_clip_bwd`` and ``ops.sgn15_frames_bwd``
          (csrc/sgn_v15_bwd.hip), which store nothing of the forward, sum in fixed orders and give a clip the same bits
          alone and in any batch; counted in ``ops.SGN15_STATS`` and ``ops.SGN15_BWD_STATS``.
        * otherwise the composition and torch autograd, counted in ``ops.SGN_STATS['forward_tensor']``."""
        if self.training:
            raise ValueError("agcn_amd: SGN.input_gradient is the eval-mode gradient; call eval() first")
        if self._fused_gradient(x):
            # no_grad around the whole route, the folds included: the cached images must stay leaves without a graph
            with torch.no_grad():
                wf, wc, _, _ = self._images()
                logits, sa, ta, dx = ops.sgn15_input_gradient(x, wf, wc, *self._images_t(), cot, self.num_point,
                                                              self.num_class, *self._geometry(),
                                                              want_attn=self.fused_attention)
                return logits, self._fused_aux(x.shape[0], sa, ta), dx
        ops.SGN_STATS['forward_tensor'] += 1
        return ops.sgn_composition_gradients(self.forward_tensor, x, cot)[:3]

    # ---- batch statistics: the forward half of train-mode BatchNorm ----
    def _batch_images(self, known):
        """Fresh images (never ``_infer_cache``) with the BatchNorms of ``known`` {name: (mean, var)} on those statistics
        and every other one on its running statistics: the specification of ``_batch_folder``.  A pass never reads a
        section that depends on a BatchNorm outside ``known`` (csrc/sgn_v15_stats_plan.h)."""
        return self._flatten(*self._folded(dict(known)))

    def _batch_folder(self):
        """-> fold(known) for ``ops.sgn15_batch_statistics``: ``_batch_images`` built incrementally.  One fold on the
        running statistics gives the working images, and the unfolded [Wq d_head^-1/2 | Wk | Wv] and W1, b1 of each block
        are kept; when a BatchNorm enters ``known`` its sections are written as base * scale and shift @ base (+ b1), the
        operations ``_fold_block`` applies to the same numbers, so the images hold the bits of ``_batch_images(known)``."""
        V = self.num_point
        work = list(self._flatten(*self._folded()))
        secs = [{n: (o, s) for n, o, s in sec}
                for sec in ops.sgn15_image_sections(V, self.num_segment, self.num_class, *self._geometry())]
        where = {}
        for which, (m, p) in enumerate(((self.spatial_mha, 's_'), (self.temporal_mha, 't_'))):
            layer = m.transformer.layers['l1']
            wqkv, w1, b1 = self._block_base(layer)
            for name, sec, base, bias in zip(ops.SGN15_BN_NAMES[2 + 2 * which:4 + 2 * which], ('qkv', 'f1'), (wqkv, w1),
                                             (None, b1)):
                where[name] = (which, p + sec, base, bias)
        done = set()

        def view(which, name):
            o, shape = secs[which][name]
            return work[which][o:o + math.prod(shape)].view(shape)

        def fold(known):
            for name in known:
                if name in done:
                    continue
                done.add(name)
                bn = self.get_submodule(name)
                s, sh = ops._fold((bn.weight, bn.bias, known[name][0], known[name][1]))
                if name in where:
                    which, p, base, bias = where[name]
                    torch.mul(base, s[:, None], out=view(which, p + '_w'))
                    view(which, p + '_b').copy_(sh @ base if bias is None else sh @ base + bias)
                else:                                  # DataNorm: BatchNorm feature c*V + v -> aff rows [v*3 + c]
                    row = 0 if name == ops.SGN15_BN_NAMES[0] else 2
                    aff = view(0, 'aff')
                    aff[row].copy_(s.reshape(3, V).t())
                    aff[row + 1].copy_(sh.reshape(3, V).t())
            return work[0], work[1]

        return fold

    def _batch_statistics_tensor(self, x):
        """The composition with every BatchNorm in batch mode and EVERY dropout of the module off -> (logits, aux, stats in
        the order the BatchNorms run).  Only Python flags are flipped for the duration of the call (a BatchNorm that does
        not track statistics touches no buffer); hooks read the inputs."""
        bns = {n: m for n, m in self.named_modules() if isinstance(m, nn.modules.batchnorm._BatchNorm)}
        mods = list(bns.values()) + [m for m in self.modules() if isinstance(m, nn.modules.dropout._DropoutNd)]
        flags = [(m.training, getattr(m, 'track_running_stats', None)) for m in mods]
        seen, hooks = {}, []

        def reader(name):
            def hook(_m, args):
                a = args[0]
                dims = [d for d in range(a.dim()) if d != 1]
                var, mean = torch.var_mean(a, dim=dims, unbiased=False)
                seen[name] = (mean, var, a.numel() // a.shape[1])
            return hook

        try:
            for n, m in bns.items():
                m.training, m.track_running_stats = True, False
                hooks.append(m.register_forward_pre_hook(reader(n)))
            for m in mods[len(bns):]:
                m.training = False
            logits, aux = self.forward_tensor(x)
        finally:
            for h in hooks:
                h.remove()
            for m, (tr, track) in zip(mods, flags):
                m.training = tr
                if track is not None:
                    m.track_running_stats = track
        return logits, aux, dict(seen)

    def _stats_fusable(self, x):
        """What the batch-statistics kernels take, whatever the grad mode and the ``training`` state."""
        if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 3 and x.is_contiguous()):
            return False
        if x.shape[1] != self.num_segment or x.shape[2] != 3 * self.num_point or x.shape[0] < 1:
            return False
        if not (ops.sgn_hip_enabled() and self._structure_fused()):
            return False
        return ops.sgn15_weights_floats(self.num_point, self.num_segment, self.num_class, *self._geometry()) is not None

    def batch_statistics(self, x, max_part_bytes=None):
        """-> (logits, aux, stats): what ONE train-mode forward of x (N, seg, 3V) as one batch computes with every dropout
        off (the reference's sgn_v15.py in train() with every dropout probability 0).  ``stats`` = {BatchNorm module name:
        (mean, biased var, count)} in dependency order (``ops.SGN15_BN_NAMES`` in the fused structure), each in its
        module's feature order; BatchNorm k sees activations normalised by the batch statistics of the BatchNorms before
        it.  Mutates nothing, runs under ``no_grad`` and works in any ``training`` state.  On a contiguous fp32 GPU tensor
        in the fused structure (``_structure_fused``, sizes inside the kernels' domain, AGCN_SGN_HIP != 0):
        ``ops.sgn15_batch_statistics``, the input pass, four truncated passes of the fused forward
        (csrc/sgn_v15_stats.hip) chunked under ``max_part_bytes`` and the two full-depth launches, with ``aux`` as the
        fine-tuning route returns it (the embeddings' tables, no attention maps); otherwise the composition (counted in
        ``ops.SGN_STATS['forward_tensor']``)."""
        if x.dim() != 3:
            raise ValueError(f"agcn_amd: SGN.batch_statistics takes (N, seg, 3 V), got {tuple(x.shape)}")
        N, seg = x.shape[0], x.shape[1]
        if N * seg < 2:
            raise ValueError(f"agcn_amd: SGN.batch_statistics needs more than one value per channel, got {N} x {seg} frames")
        V = self.num_point
        with torch.no_grad():
            if not self._stats_fusable(x):
                ops.SGN_STATS['forward_tensor'] += 1
                return self._batch_statistics_tensor(x)
            cap = ops.SGN_MAX_STATS_BYTES if max_part_bytes is None else max_part_bytes
            fold = self._batch_folder()
            logits, raw = ops.sgn15_batch_statistics(x, fold, V, self.num_class, *self._geometry(), cap)
            counts = [N * seg] * 2 + [N * seg * V] * 2 + [N * seg] * 2
            stats = {}
            for i, (name, count) in enumerate(zip(ops.SGN15_BN_NAMES, counts)):
                mean, var = raw[name]
                if i < 2:                              # the kernels' [v*3 + c] -> the module's c*V + v
                    mean, var = (t.view(V, 3).t().reshape(-1) for t in (mean, var))
                stats[name] = (mean, var, count)
            wf, wc = fold({})                          # the final images: the embeddings' tables are sections of them
            o = ops.sgn15_image_sections(V, seg, self.num_class, *self._geometry())[0]
            spa = next(wf[off:off + math.prod(s)].view(s) for n, off, s in o if n == 'spa')
            tem = wc[:seg * 256].view(seg, 256)
            aux = dict(tem_emb=tem.t()[None, :, None, :].expand(N, 256, V, seg),
                       spa_emb=spa.t()[None, :, :, None].expand(N, 64, V, seg), spatial_attn_list=None,
                       temporal_attn_list=None)
            return logits, aux, stats

    def recalibrate_bn(self, x, momentum=None, reset=True, max_part_bytes=None):
        """Re-estimate the BatchNorms on x (AdaBN, or after frozen-BatchNorm fine-tuning moved the weights under them):
        ``batch_statistics(x)``, then ``running_mean``, ``running_var`` (unbiased, n / (n - 1)) and
        ``num_batches_tracked`` are updated in place exactly as one train-mode forward of x would (with every dropout off).
        ``momentum=None``: the cumulative average (after ``reset`` the running statistics ARE the batch's), a float: the
        exponential one.  ``reset=True`` calls ``reset_running_stats()`` first.  -> stats.  The in-place writes bump the
        buffers' versions: the next prediction rebuilds the cached weight images."""
        _, _, stats = self.batch_statistics(x, max_part_bytes)
        return ops.sgn_update_running_stats(self, stats, momentum, reset)
