"""Base SGN (reference model/architecture/sgn/archiv/sgn.py), the model the reference's online recogniser deploys
(infer/inference.py:129-150).  Module tree, parameter names, initialisation and state_dict are the reference's, so a
trained ``SGN-*.pt`` loads as it is; ``spa`` and ``tem`` are non-persistent buffers (the reference keeps them as plain
attributes), and the class constructs without a GPU.

Three routes:

* eval mode under ``no_grad`` on the GPU with ``step == seg``: three HIP launches (csrc/sgn.hip) on weight images with
  every BatchNorm folded -- ``ops.sgn_frames`` (joint-level module), ``ops.sgn_clip`` (frame-level module + fc).  The
  images are cached under ``ops._cache_key`` and rebuilt after any parameter or running statistic changes.
* the same launches in grad mode when x is the only tensor that asks for a gradient (every parameter frozen), behind
  ``ops.SGNInputGradFunction`` whose backward is ``ops.sgn_clip_bwd`` + ``ops.sgn_frames_bwd`` (csrc/sgn_bwd.hip);
  ``input_gradient(x, cot)`` is that without autograd state.
* with ``fused_finetune = True`` (a plain attribute, off by default, not in the state_dict), eval mode, grad mode and
  at least one trainable parameter: frozen-BatchNorm fine-tuning on the fused path.  ``ops.SGNFineTuneFunction`` runs the
  fused forward; its backward tapes the two backward kernels and reduces the tapes to the gradients of the two folded
  weight images (csrc/sgn_wgrad.hip), and torch autograd carries those through ``_folded()`` -- built in grad mode, fresh
  per call -- to the parameters.  ``parameter_gradients(x, cot)`` is that without autograd state.
* ``batch_statistics(x)`` / ``recalibrate_bn(x)`` in any ``training`` state: the batch statistics of the seven BatchNorms
  of x as one batch and the logits under them (the forward half of train-mode BatchNorm), as seven truncated passes of
  the fused forward (csrc/sgn_stats.hip) on freshly folded images plus the two full-depth launches.  The backward of
  batch-mode BatchNorm is not built in HIP.
* everything else (grad mode with trainable parameters and the flag off, ``train()``, a CPU tensor, ``step != seg``, ``AGCN_SGN_HIP=0``): the tensor-code
  composition below, channels last, ``F.linear`` / ``matmul`` on views and ``nn.BatchNorm`` modules.  It makes the class
  a complete ``nn.Module`` any torch optimiser can fine-tune and is the comparison of the fused path; it is NOT the hot
  path and is counted in ``ops.SGN_STATS['forward_tensor']``.

Activations of the composition are (bs, step, V, C); the reference's are (bs, C, V, step)."""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops

# the names of the sections of the two weight images, in their order (they do not depend on the sizes)
_FRAMES_SECTIONS, _CLIP_SECTIONS = ([n for n, _, _ in secs] for secs in ops.sgn_image_sections(2, 1, 1))


def _cl_to_cf(x):
    """(bs, step, V, C) -> (bs, C, V, step): the layout the reference's BatchNorm / pooling modules see."""
    return x.permute(0, 3, 2, 1)


class norm_data(nn.Module):
    """BatchNorm1d over the C*V features of a frame, feature c*V + v (reference sgn.py:107-117)."""

    def __init__(self, dim=64):
        super().__init__()
        self.bn = nn.BatchNorm1d(dim)

    def forward(self, x):
        bs, step, V, C = x.shape
        y = self.bn(_cl_to_cf(x).reshape(bs, C * V, step))
        return y.reshape(bs, C, V, step).permute(0, 3, 2, 1)


class cnn1x1(nn.Module):
    """The Conv2d holds the parameters under the reference's names; it is applied as a linear map of the last dim."""

    def __init__(self, dim1=3, dim2=3, bias=True):
        super().__init__()
        self.cnn = nn.Conv2d(dim1, dim2, kernel_size=1, bias=bias)

    def forward(self, x):
        return F.linear(x, self.cnn.weight.flatten(1), self.cnn.bias)


class embed(nn.Module):
    def __init__(self, dim=3, dim1=128, norm_dim=75, bias=False):
        super().__init__()
        layers = [cnn1x1(dim, 64, bias=bias), nn.ReLU(), cnn1x1(64, dim1, bias=bias), nn.ReLU()]
        self.cnn = nn.Sequential(*([norm_data(norm_dim)] if norm_dim > 0 else []), *layers)

    def forward(self, x):
        return self.cnn(x)


class local(nn.Module):
    """Frame-level module (reference sgn.py:155-177): maximum over the joints (adaptive in time when step != seg),
    3-tap temporal conv, 1x1 conv, each with BatchNorm + ReLU."""

    def __init__(self, dim1=3, dim2=3, bias=False, seg=20):
        super().__init__()
        self.maxpool = nn.AdaptiveMaxPool2d((1, seg))
        self.cnn1 = nn.Conv2d(dim1, dim1, kernel_size=(1, 3), padding=(0, 1), bias=bias)
        self.bn1 = nn.BatchNorm2d(dim1)
        self.relu = nn.ReLU()
        self.cnn2 = nn.Conv2d(dim1, dim2, kernel_size=1, bias=bias)
        self.bn2 = nn.BatchNorm2d(dim2)
        self.dropout = nn.Dropout2d(0.2)
        self.seg = seg

    @staticmethod
    def _bn(bn, x):
        """BatchNorm2d of x (bs, T, C) seen as (bs, C, 1, T)."""
        return bn(x.transpose(1, 2).unsqueeze(2)).squeeze(2).transpose(1, 2)

    def forward(self, x):
        if x.shape[1] == self.seg:
            h = x.amax(2)                                                  # (bs, T, C)
        else:
            h = self.maxpool(_cl_to_cf(x)).squeeze(2).transpose(1, 2)
        hp = F.pad(h, (0, 0, 1, 1))
        T = h.shape[1]
        taps = torch.cat([hp[:, dt:dt + T] for dt in range(3)], dim=2)     # feature dt * C + c
        w = self.cnn1.weight[:, :, 0, :].permute(0, 2, 1).flatten(1)
        y = self.relu(self._bn(self.bn1, F.linear(taps, w, self.cnn1.bias)))
        y = self.dropout(y.transpose(1, 2).unsqueeze(2)).squeeze(2).transpose(1, 2)
        y = F.linear(y, self.cnn2.weight.flatten(1), self.cnn2.bias)
        return self.relu(self._bn(self.bn2, y))


class gcn_spa(nn.Module):
    def __init__(self, in_feature, out_feature, bias=False):
        super().__init__()
        self.bn = nn.BatchNorm2d(out_feature)
        self.relu = nn.ReLU()
        self.w = cnn1x1(in_feature, out_feature, bias=False)
        self.w1 = cnn1x1(in_feature, out_feature, bias=bias)

    def forward(self, x1, g):
        y = self.w(g.matmul(x1)) + self.w1(x1)
        return self.relu(_cl_to_cf(self.bn(_cl_to_cf(y))))


class compute_g_spa(nn.Module):
    def __init__(self, dim1=64 * 3, dim2=64 * 3, bias=False):
        super().__init__()
        self.dim1, self.dim2 = dim1, dim2
        self.g1 = cnn1x1(dim1, dim2, bias=bias)
        self.g2 = cnn1x1(dim1, dim2, bias=bias)
        self.softmax = nn.Softmax(dim=-1)

    def forward(self, x1):
        return self.softmax(self.g1(x1).matmul(self.g2(x1).transpose(-1, -2)))


_t = ops._sgn_t


def _bias(conv, n, like):
    return conv.bias if conv.bias is not None else like.new_zeros(n)


class SGN(nn.Module):
    def __init__(self, num_class=60, num_point=25, in_channels=3, seg=20, bias=True):
        super().__init__()
        self.c1, self.c2, self.c3 = 64, 128, 256
        self.seg, self.num_point, self.in_channels, self.num_class = seg, num_point, in_channels, num_class

        self.joint_embed = embed(in_channels, self.c1, norm_dim=in_channels * num_point, bias=bias)
        self.dif_embed = embed(in_channels, self.c1, norm_dim=in_channels * num_point, bias=bias)
        # the reference's one-hot tensors, in its shapes: spa (1, V, V, seg) one-hot over the joint, tem (1, seg, V, seg)
        # one-hot over the frame
        self.register_buffer('spa', torch.eye(num_point)[None, :, :, None].repeat(1, 1, 1, seg), persistent=False)
        self.register_buffer('tem', torch.eye(seg)[None, :, None, :].repeat(1, 1, num_point, 1), persistent=False)
        self.tem_embed = embed(seg, self.c3, norm_dim=0, bias=bias)
        self.spa_embed = embed(num_point, self.c1, norm_dim=0, bias=bias)

        self.compute_g1 = compute_g_spa(self.c2, self.c3, bias=bias)
        self.gcn1 = gcn_spa(self.c2, self.c2, bias=bias)
        self.gcn2 = gcn_spa(self.c2, self.c3, bias=bias)
        self.gcn3 = gcn_spa(self.c3, self.c3, bias=bias)

        self.cnn = local(self.c3, self.c3 * 2, bias=bias, seg=seg)
        self.maxpool = nn.AdaptiveMaxPool2d((1, 1))
        self.fc = nn.Linear(self.c3 * 2, num_class)

        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                n = m.kernel_size[0] * m.kernel_size[1] * m.out_channels
                m.weight.data.normal_(0, math.sqrt(2. / n))
        for gcn in (self.gcn1, self.gcn2, self.gcn3):
            nn.init.constant_(gcn.w.cnn.weight, 0)
        self._infer_cache = {}
        self.fused_finetune = False        # opt in: eval-mode backward() to the parameters on the HIP kernels

    # ---- the input-independent embeddings (reference sgn.py:78-79) ----
    def _spa1(self):
        return self.spa_embed(self.spa[0, :, :, 0].t())                    # (V, 64)

    def _tem1(self):
        return self.tem_embed(self.tem[0, :, 0, :].t())                    # (seg, 256)

    # ---- tensor-code composition ----
    def forward_tensor(self, x):
        bs, step, dim = x.shape
        V = dim // self.in_channels
        if step != self.seg:           # the reference cannot add tem1 (seg frames) to step frames either (sgn.py:89)
            raise ValueError(f"agcn_amd: SGN was built for seg = {self.seg} frames (tem is one-hot over them), got {step}")
        x = x.reshape(bs, step, V, self.in_channels)
        dif = torch.cat([x.new_zeros(bs, 1, V, self.in_channels), x[:, 1:] - x[:, :-1]], dim=1)
        dy = self.joint_embed(x) + self.dif_embed(dif)
        h = torch.cat([dy, self._spa1().expand(bs, step, V, self.c1)], dim=3)
        g = self.compute_g1(h)
        h = self.gcn3(self.gcn2(self.gcn1(h, g), g), g)
        h = h + self._tem1()[None, :, None, :]
        y = self.cnn(h)                                                    # (bs, seg, 512)
        return self.fc(y.amax(1)), g

    # ---- folded weight images of the HIP path ----
    def _folded(self, override=None):
        """The folded tensors in the order of the weight images (csrc/sgn_plan.h): -> (frames list, clip list).
        ``override``: {BatchNorm module name: (mean, var)} folds that BatchNorm on the given statistics (in the module's
        own feature order) instead of its running ones, {name: None} folds it as the identity (scale 1, shift 0): the
        images of the batch-statistics passes.  Without it every BatchNorm is folded on its running statistics."""
        V, like = self.num_point, self.fc.weight
        names = {m: n for n, m in self.named_modules()} if override else {}

        def fold(bn):
            if override and names[bn] in override:
                stats = override[names[bn]]
                if stats is None:
                    return torch.ones_like(bn.weight), torch.zeros_like(bn.bias)
                return ops._fold((bn.weight, bn.bias, stats[0], stats[1]))
            return ops._fold((bn.weight, bn.bias, bn.running_mean, bn.running_var))

        def first(e, i):                       # the two 1x1 layers of an embedding: (w1, b1, w2, b2) images
            a, b = e.cnn[i].cnn, e.cnn[i + 2].cnn
            return [_t(a.weight), _bias(a, 64, like), _t(b.weight), _bias(b, b.out_channels, like)]

        def gcn(m):
            s, sh = fold(m.bn)
            wcat = torch.cat([_t(m.w.cnn.weight), _t(m.w1.cnn.weight)]) * s[None, :]
            return [wcat, _bias(m.w1.cnn, s.numel(), like) * s + sh]

        aff = []
        for e in (self.joint_embed, self.dif_embed):        # BatchNorm feature c*V + v -> [v*3 + c]
            aff += [c.reshape(3, V).t() for c in fold(e.cnn[0].bn)]
        g = self.compute_g1
        frames = (aff + first(self.joint_embed, 1) + first(self.dif_embed, 1) + [self._spa1()]
                  + [torch.cat([_t(g.g1.cnn.weight), _t(g.g2.cnn.weight)], dim=1),          # [g1 | g2]: (128, 512)
                     torch.cat([_bias(g.g1.cnn, 256, like), _bias(g.g2.cnn, 256, like)])]
                  + gcn(self.gcn1) + gcn(self.gcn2) + gcn(self.gcn3))
        c = self.cnn
        s1, sh1 = fold(c.bn1)
        s2, sh2 = fold(c.bn2)
        clip = [self._tem1(),
                (c.cnn1.weight[:, :, 0, :] * s1[:, None, None]).permute(2, 1, 0), _bias(c.cnn1, 256, like) * s1 + sh1,
                _t(c.cnn2.weight) * s2[None, :], _bias(c.cnn2, 512, like) * s2 + sh2,
                self.fc.weight.t(), self.fc.bias]
        return frames, clip

    @staticmethod
    def _flatten(frames, clip):
        """The two folded lists -> (frames image, clip image), each one flat tensor."""
        return torch.cat([t.reshape(-1) for t in frames]), torch.cat([t.reshape(-1) for t in clip])

    @staticmethod
    def _transposed(frames, clip):
        """The two folded lists -> the two images of the backward (csrc/sgn_bwd_plan.h: the same folded matrices stored
        (N, K)): W^T of je2, de2, [g1 | g2], gcn1..3 of the frames image; of the three taps of cnn1 and of cnn2."""
        f = dict(zip(_FRAMES_SECTIONS[1:], frames[4:]))      # 'aff' (4, V, 3) is the list's first four (V, 3) tensors
        c = dict(zip(_CLIP_SECTIONS, clip))
        wf_t = torch.cat([f[n].t().reshape(-1) for n in ('je2_w', 'de2_w', 'g_w', 'c1_w', 'c2_w', 'c3_w')])
        wc_t = torch.cat([c['t1_w'].transpose(1, 2).reshape(-1), c['t2_w'].t().reshape(-1)])
        return wf_t, wc_t

    def _images(self, transposed=False):
        """-> (frames image, clip image); with ``transposed`` also the two images of the backward.  Those are built on the
        first call that asks for them, under the same key: a model that only predicts never builds them."""
        srcs = list(self.parameters()) + list(self.buffers())
        key = ops._cache_key(srcs)
        f = self._infer_cache.get('images')
        if f is None or f[0] != key:
            f = self._infer_cache['images'] = (key,) + self._flatten(*self._folded())
        if not transposed:
            return f[1], f[2]
        t = self._infer_cache.get('images_t')
        if t is None or t[0] != key:
            t = self._infer_cache['images_t'] = (key,) + self._transposed(*self._folded())
        return f[1], f[2], t[1], t[2]

    def _in_domain(self, x):
        """What the kernels take, whatever the grad mode and the ``training`` state."""
        return (x.is_cuda and x.dtype == torch.float32
                and x.dim() == 3 and x.shape[1] == self.seg and self.in_channels == 3
                and x.shape[2] == 3 * self.num_point and ops.sgn_hip_enabled())

    def _fusable(self, x):
        """What the eval-mode kernels take, whatever the grad mode."""
        return not self.training and self._in_domain(x)

    def _fused(self, x):
        return not torch.is_grad_enabled() and self._fusable(x)

    def _fused_input_grad(self, x):
        """Grad mode with x the only thing that asks for a gradient: the fused forward with the HIP input backward."""
        return (torch.is_grad_enabled() and x.requires_grad and self._fusable(x)
                and not any(p.requires_grad for p in self.parameters()))

    def _fused_finetune(self, x):
        """The flag, eval mode, grad mode, the kernels' domain and something to train."""
        return (self.fused_finetune and torch.is_grad_enabled() and self._fusable(x)
                and any(p.requires_grad for p in self.parameters()))

    def _finetune_images(self):
        """The four images for ``ops.SGNFineTuneFunction``: the forward ones in the CURRENT grad mode from a fresh fold (not
        from ``_infer_cache``: they carry the autograd graph of this call), the transposed ones without grad from the
        same folded tensors."""
        frames, clip = self._folded()
        wf, wc = self._flatten(frames, clip)
        with torch.no_grad():
            wf_t, wc_t = self._transposed(frames, clip)
        return wf, wc, wf_t, wc_t

    def forward(self, x):
        if self._fused_finetune(x):
            return ops.SGNFineTuneFunction.apply(x, *self._finetune_images(), self.num_point, self.num_class)
        if self._fused_input_grad(x):
            with torch.no_grad():
                images = self._images(transposed=True)
            return ops.SGNInputGradFunction.apply(x, *images, self.num_point, self.num_class)
        if not self._fused(x):
            ops.SGN_STATS['forward_tensor'] += 1
            return self.forward_tensor(x)
        wf, wc = self._images()
        feat, g = ops.sgn_frames(x.contiguous(), wf, self.num_point)
        return ops.sgn_clip(feat, wc, self.num_class), g

    def parameter_gradients(self, x, cot, rows_per_split=0, max_tape_bytes=None):
        """-> (logits, g, dx, {name: grad}) with the gradients of sum(logits * cot) in eval mode (BatchNorm on its running
        statistics), for every parameter that requires grad.  Needs no prior autograd state and leaves every ``.grad``
        alone.  On the GPU (fp32, step == seg, in_channels == 3, AGCN_SGN_HIP != 0) the batch dimension is all HIP: the
        fused forward, the two taping backward kernels and the reductions of ``ops.sgn_image_gradients``; torch autograd
        only takes the two image gradients through the fold.  Otherwise the composition with torch autograd (counted in
        ``ops.SGN_STATS['forward_tensor']``).  ``rows_per_split`` / ``max_tape_bytes``: see ``ops.sgn_image_gradients``."""
        if self.training:
            raise ValueError("agcn_amd: SGN.parameter_gradients is the eval-mode gradient; call eval() first")
        named = [(n, p) for n, p in self.named_parameters() if p.requires_grad]
        if not self._fusable(x):
            ops.SGN_STATS['forward_tensor'] += 1
            logits, g, dx, grads = ops.sgn_composition_gradients(self.forward_tensor, x, cot, [p for _, p in named])
            return logits, g, dx, ops.sgn_named_gradients(named, grads)
        with torch.enable_grad():
            wf, wc, wf_t, wc_t = self._finetune_images()
        cap = ops.SGN_MAX_TAPE_BYTES if max_tape_bytes is None else max_tape_bytes
        logits, g, dx, d_wf, d_wc = ops.sgn_image_gradients(x, wf.detach(), wc.detach(), wf_t, wc_t, cot, self.num_point,
                                                            self.num_class, rows_per_split, cap)
        return logits, g, dx, ops.sgn_fold_gradients((wf, wc), (d_wf, d_wc), named)

    def input_gradient(self, x, cot):
        """-> (logits, g, dx) with dx = d sum(logits * cot) / dx, in eval mode.  Needs no autograd state and ignores the
        parameters' requires_grad.  On the GPU (fp32, step == seg, in_channels == 3, AGCN_SGN_HIP != 0) it is four
        launches: the two of the forward, ``ops.sgn_clip_bwd`` and ``ops.sgn_frames_bwd``; otherwise the composition with
        torch autograd (counted in ``ops.SGN_STATS['forward_tensor']``)."""
        if self.training:
            raise ValueError("agcn_amd: SGN.input_gradient is the eval-mode gradient; call eval() first")
        if not self._fusable(x):
            ops.SGN_STATS['forward_tensor'] += 1
            return ops.sgn_composition_gradients(self.forward_tensor, x, cot)[:3]
        with torch.no_grad():
            images = self._images(transposed=True)
        return ops.sgn_input_gradient(x, *images, cot, self.num_point, self.num_class)

    # ---- batch statistics: the forward half of train-mode BatchNorm ----
    def _batch_images(self, known, identity):
        """Fresh images (never cached) with the BatchNorms of ``known`` on those statistics and ``identity`` as it says:
        the specification of ``_batch_folder``."""
        override = dict(known)
        if identity is not None:
            override[identity] = None
        return self._flatten(*self._folded(override))

    def _batch_folder(self):
        """-> fold(known, identity) for ``ops.sgn_batch_statistics``: ``_batch_images`` built incrementally.  One fold with
        all seven BatchNorms as the identity gives the base images; a working copy takes the section of every BatchNorm
        that enters ``known`` as base * scale (+ shift), the operations ``_folded`` applies to the same numbers, so the
        sections a pass reads hold the bits of ``_batch_images(known, identity)``.  A pass never reads past the BatchNorm
        it measures, and that one is still the identity in the working copy."""
        V = self.num_point
        base = self._flatten(*self._folded(dict.fromkeys(ops.SGN_BN_NAMES)))
        work = [b.clone() for b in base]
        secs = [{n: (o, s) for n, o, s in sec} for sec in ops.sgn_image_sections(V, self.seg, self.num_class)]
        where = {'gcn1.bn': (0, 'c1'), 'gcn2.bn': (0, 'c2'), 'gcn3.bn': (0, 'c3'), 'cnn.bn1': (1, 't1'), 'cnn.bn2': (1, 't2')}
        done = set()

        def view(img, which, name):
            o, shape = secs[which][name]
            return img[which][o:o + math.prod(shape)].view(shape)

        def fold(known, identity):
            for name in known:
                if name in done:
                    continue
                done.add(name)
                bn = self.get_submodule(name)
                s, sh = ops._fold((bn.weight, bn.bias, known[name][0], known[name][1]))
                if name in where:
                    which, p = where[name]
                    torch.mul(view(base, which, p + '_w'), s[None, :], out=view(work, which, p + '_w'))
                    view(work, which, p + '_b').copy_(view(base, which, p + '_b') * s + sh)
                else:                                  # norm_data: BatchNorm feature c*V + v -> aff rows [v*3 + c]
                    row = 0 if name == ops.SGN_BN_NAMES[0] else 2
                    aff = view(work, 0, 'aff')
                    aff[row].copy_(s.reshape(3, V).t())
                    aff[row + 1].copy_(sh.reshape(3, V).t())
            assert identity is None or identity not in done
            return work[0], work[1]

        return fold

    def _batch_statistics_tensor(self, x):
        """The composition with every BatchNorm in batch mode and dropout off.  Only Python flags are flipped for the
        duration of the call (a BatchNorm that does not track statistics touches no buffer); hooks read the inputs."""
        bns = {n: self.get_submodule(n) for n in ops.SGN_BN_NAMES}
        mods = list(bns.values()) + [self.cnn.dropout]
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
            self.cnn.dropout.training = False
            logits, g = self.forward_tensor(x)
        finally:
            for h in hooks:
                h.remove()
            for m, (tr, track) in zip(mods, flags):
                m.training = tr
                if track is not None:
                    m.track_running_stats = track
        return logits, g, {n: seen[n] for n in ops.SGN_BN_NAMES}

    def batch_statistics(self, x, max_part_bytes=None):
        """-> (logits, g, stats): what ONE train-mode forward of x (N, seg, 3V) as one batch computes with dropout off (the
        reference's sgn.py in train() with cnn.dropout.p = 0).  ``stats`` = {BatchNorm module name: (mean, biased var,
        count)} for the seven BatchNorms in dependency order (``ops.SGN_BN_NAMES``), each in its module's feature order;
        BatchNorm k sees activations normalised by the batch statistics of the BatchNorms before it.  Mutates nothing and
        works in any ``training`` state.  On the GPU (fp32, step == seg, in_channels == 3, AGCN_SGN_HIP != 0):
        ``ops.sgn_batch_statistics``, seven truncated passes of the fused forward (csrc/sgn_stats.hip) chunked under
        ``max_part_bytes`` and the two full-depth launches; otherwise the composition under ``no_grad`` (counted in
        ``ops.SGN_STATS['forward_tensor']``)."""
        if x.dim() != 3:
            raise ValueError(f"agcn_amd: SGN.batch_statistics takes (N, seg, 3 V), got {tuple(x.shape)}")
        N, seg = x.shape[0], x.shape[1]
        if N * seg < 2:
            raise ValueError(f"agcn_amd: SGN.batch_statistics needs more than one value per channel, got {N} x {seg} frames")
        V = self.num_point
        with torch.no_grad():
            if not self._in_domain(x):
                ops.SGN_STATS['forward_tensor'] += 1
                return self._batch_statistics_tensor(x)
            cap = ops.SGN_MAX_STATS_BYTES if max_part_bytes is None else max_part_bytes
            logits, g, raw = ops.sgn_batch_statistics(x, self._batch_folder(), V, self.num_class, cap)
            counts = dict(zip(ops.SGN_BN_NAMES, [N * seg] * 2 + [N * seg * V] * 3 + [N * seg] * 2))
            stats = {}
            for i, name in enumerate(ops.SGN_BN_NAMES):
                mean, var = raw[name]
                if i < 2:                              # the kernels' [v*3 + c] -> the module's c*V + v
                    mean, var = (t.view(V, 3).t().reshape(-1) for t in (mean, var))
                stats[name] = (mean, var, counts[name])
            return logits, g, stats

    def recalibrate_bn(self, x, momentum=None, reset=True, max_part_bytes=None):
        """Re-estimate the seven BatchNorms on x (AdaBN): ``batch_statistics(x)``, then ``running_mean``, ``running_var``
        (unbiased, n / (n - 1)) and ``num_batches_tracked`` are updated in place exactly as one train-mode forward of x
        would.  ``momentum=None``: the cumulative average (after ``reset`` the running statistics ARE the batch's), a
        float: the exponential one.  ``reset=True`` calls ``reset_running_stats()`` first.  -> stats.  The in-place writes
        bump the buffers' versions: the next prediction rebuilds the cached weight images."""
        _, _, stats = self.batch_statistics(x, max_part_bytes)
        return ops.sgn_update_running_stats(self, stats, momentum, reset)
