"""Online action recognition (reference ``infer/inference.py::ActionRecognition`` with its
``infer/data_preprocess.py::DataPreprocessorV2``): skeletons arrive one frame at a time, the last ``max_frame`` frames of
up to ``max_num_skeleton`` tracked bodies are kept in a ring on the GPU, and a prediction selects the
``max_num_skeleton_true`` most active bodies, normalises the window and runs the model at batch 1.

Per frame: one host-to-device copy of the frame and one launch (``ops.skel_append``).  Per prediction: one launch for
selection + normalisation (``ops.prenorm``), the folded eval forward, softmax/argmax, and one device-to-host copy of the
scores and the label, which is the only synchronisation.

``RecordingRecognition`` labels a whole recording and ``MultiStreamRecognition`` serves several streams: both normalise
many windows in one launch (``ops.prenorm_windows``) and run them through the model as one batch.

With ``sgn_preprocess=True`` the recognisers run the reference's deployed SGN (``model.sgn.SGN``, or the attention SGN
``model.sgn_v15.SGN`` of its newer ``inference_221012.py``) as its
``inference.py:102-107, 148-150`` does: the normalised window goes through ``ops.sgn_sample`` (``NTUDataLoaders.to_fix_length``:
``multi_test`` random subsamples of ``model.seg`` rows), the model runs on the subsamples and their logits are averaged.

With ``streams=[(stream, model, model_args, weights), ...]`` (streams out of joint, bone, joint_motion, bone_motion) and
``alpha=[...]`` (one weight per stream, default ones) a recogniser serves the reference's multi-stream result
(``ensemble.py``: joint + alpha * bone) from the one joint window: the derived streams come out of one
``ops.skeleton_streams`` launch, each model runs on its stream, ``logits = sum_i alpha_i * logits_i`` (the per-stream logits
stay in ``stream_logits``), and ``explain`` folds the models' input gradients into one gradient with respect to the joint
window with one ``ops.streams_bwd`` launch.  Still one synchronising copy per prediction.  The parent table is
``stream_parents``, by default ``bone_parents`` of the first model's graph.

The frame handed to ``append_data`` always carries exactly ``max_num_skeleton`` bodies (absent ones as zeros), as the
reference's main loop does; its ``M < max_person`` case, which leaves stale rows in the window, is not reproduced."""
import numpy as np
import torch

from . import ops


def load_model(model, model_args=None, weights=None):
    """Instantiate ``model`` (a dotted class path such as ``model.aagcn.Model``) with ``model_args`` and load a weights
    file saved by the trainer (a state dict, optionally with DataParallel's ``module.`` prefix)."""
    from .processor import import_class
    net = import_class(model)(**(model_args or {}))
    if weights is not None:
        state = torch.load(weights, map_location='cpu', weights_only=True)
        state = {k.replace('module.', '', 1) if k.startswith('module.') else k: v for k, v in state.items()}
        net.load_state_dict(state)
    return net


def window_plan(L, T, ends):
    """The windows of a recording of ``L`` frames that a recogniser with a window of ``T`` frames holds after appending
    frame ``ends[i]``: -> (start, len) int32 arrays, start = max(0, end - T + 1), len = end - start + 1 (below T while
    the window fills).  Pure host arithmetic."""
    ends = np.asarray(ends, dtype=np.int64).reshape(-1)
    if L < 1 or T < 1:
        raise ValueError("agcn_amd: window_plan needs L >= 1 and T >= 1")
    if ends.size and (ends.min() < 0 or ends.max() >= L):
        raise ValueError(f"agcn_amd: window_plan takes frame indices in [0, {L}), got {ends.min()}..{ends.max()}")
    start = np.maximum(0, ends - T + 1)
    return start.astype(np.int32), (ends - start + 1).astype(np.int32)


def window_plan_device(L, T, device, interval=1, first=0):
    """``window_plan`` for ends = first, first + interval, ... < L, built on the device: nothing is uploaded.
    -> (start, len, ends) int32 tensors."""
    if L < 1 or T < 1 or interval < 1 or not 0 <= first < L:
        raise ValueError("agcn_amd: window_plan_device needs L >= 1, T >= 1, interval >= 1 and 0 <= first < L")
    ends = torch.arange(first, L, interval, dtype=torch.int32, device=device)
    start = torch.clamp(ends - (T - 1), min=0)
    return start, ends - start + 1, ends


class _Recogniser:
    """What the recognisers share: the model in eval mode on the device, the window geometry and the normalisation
    options."""

    def __init__(self, model=None, model_args=None, weights=None, max_frame=300, max_num_skeleton=4,
                 max_num_skeleton_true=2, num_joint=25, moving_avg=1, zaxis=(0, 1), xaxis=(8, 4), zaxis2=None,
                 device='cuda:0', sgn_preprocess=False, multi_test=5, streams=None, alpha=None, stream_parents=None):
        if not 1 <= max_num_skeleton_true <= max_num_skeleton:
            raise ValueError("agcn_amd: need 1 <= max_num_skeleton_true <= max_num_skeleton")
        if sgn_preprocess and (max_num_skeleton_true != 2 or multi_test < 1):
            raise ValueError("agcn_amd: sgn_preprocess interleaves exactly two selected bodies and needs multi_test >= 1")
        if not 1 <= moving_avg <= max_frame:
            raise ValueError("agcn_amd: need 1 <= moving_avg <= max_frame")
        self.device = torch.device(device)
        # several input streams served from one normalised window (the reference's two-stream result, ensemble.py:
        # joint + alpha * bone): one model per stream, the streams derived on the device, the logits fused
        self.stream_names = self.models = self.alpha = self.stream_parents = None
        self.stream_logits = None          # the per-stream logits of the last forward, in the order of `streams`
        if streams is not None:
            model = self._load_streams(model, sgn_preprocess, streams, alpha, stream_parents, num_joint)
        elif model is None:
            raise ValueError("agcn_amd: a recogniser needs `model` or `streams`")
        elif alpha is not None or stream_parents is not None:
            raise ValueError("agcn_amd: alpha and stream_parents belong to `streams`")
        if isinstance(model, str):
            model = load_model(model, model_args, weights)
            from .model.sgn_v15 import SGN as SGN15
            if isinstance(model, SGN15):
                model.fused_input_gradient = True      # explain() through the HIP backward (csrc/sgn_v15_bwd.hip)
        self.model = model.to(self.device).eval()
        self.max_frame, self.max_person, self.num_select = int(max_frame), int(max_num_skeleton), int(max_num_skeleton_true)
        self.num_joint, self.moving_avg = int(num_joint), int(moving_avg)
        self.zaxis, self.xaxis, self.zaxis2 = zaxis, xaxis, zaxis2
        # what the last prediction left on the device: the normalised windows (N, 3, T, V, K), the selected bodies
        # (N, K) int32, the energies (N, Mmax) and the logits (N, num_class)
        self.window = self.selected = self.energy = self.logits = None
        # reference inference.py:148-150 with an SGN: the normalised window goes through NTUDataLoaders.to_fix_length
        # (ops.sgn_sample: multi_test random subsamples of model.seg rows) and the logits of the draws are averaged.
        # aagcn_normalize=False (raw windows into the sampler) is not built.
        self.sgn_preprocess, self.multi_test = bool(sgn_preprocess), int(multi_test)
        self.seg = int(self.model.seg) if self.sgn_preprocess else None
        self.draws = self.rows = None          # the last draws (N, multi_test, seg) int32 bit patterns, and row counts

    def _load_streams(self, model, sgn_preprocess, streams, alpha, stream_parents, num_joint):
        """``streams`` = [(stream, model, model_args, weights), ...] (model a dotted class path or a module; the two
        trailing fields may be left out) -> the first model; fills stream_names, models, alpha, stream_parents."""
        if sgn_preprocess:
            raise ValueError("agcn_amd: sgn_preprocess with streams is not built: the SGN sampler reads joint windows")
        if model is not None:
            raise ValueError("agcn_amd: with `streams` the models are given per stream; leave `model` out")
        entries = [tuple(e) + (None,) * (4 - len(tuple(e))) for e in streams]
        names = [e[0] for e in entries]
        if not entries or any(len(e) != 4 for e in entries) or any(n not in ops.STREAMS for n in names) or \
                len(set(names)) != len(names):
            raise ValueError(f"agcn_amd: streams is a non-empty list of (stream, model[, model_args[, weights]]) with "
                             f"distinct streams out of {ops.STREAMS}, got {names}")
        alpha = [1.0] * len(entries) if alpha is None else [float(a) for a in alpha]
        if len(alpha) != len(entries):
            raise ValueError(f"agcn_amd: alpha has one weight per stream: {len(entries)}, got {len(alpha)}")
        nets = [load_model(m, a, w) if isinstance(m, str) else m for _, m, a, w in entries]
        nets = [net.to(self.device).eval() for net in nets]
        if any(n != 'joint' for n in names):
            if stream_parents is None:
                stream_parents = next((net.graph.bone_parents for net in nets
                                       if getattr(getattr(net, 'graph', None), 'bone_parents', None) is not None), None)
            if stream_parents is None:
                raise ValueError("agcn_amd: the streams need stream_parents: no model carries a graph with bone_parents")
            stream_parents = tuple(int(p) for p in stream_parents)
            if len(stream_parents) != int(num_joint) or any(not 0 <= p < int(num_joint) for p in stream_parents):
                raise ValueError(f"agcn_amd: stream_parents holds one joint index in [0, {num_joint}) per joint, got "
                                 f"{list(stream_parents)}")
        self.stream_names, self.models, self.alpha, self.stream_parents = names, nets, alpha, stream_parents
        return nets[0]

    def _stream_inputs(self, window):
        """The inputs of the stream models from the normalised window: every derived stream out of ONE launch."""
        want = tuple(n for n in self.stream_names if n != 'joint')
        inputs = ops.skeleton_streams(window, self.stream_parents, want) if want else {}
        inputs['joint'] = window
        return inputs

    def _draws(self, draws, N):
        """None -> fresh draws on the device; else (N, S, seg) (or (S, seg) for one window) uint32 / int32 patterns."""
        if draws is None:
            return ops.sgn_draws(N, self.multi_test, self.seg, self.device)
        if isinstance(draws, np.ndarray):
            draws = torch.from_numpy(np.ascontiguousarray(draws, dtype=np.uint32).view(np.int32))
        if draws.dtype == torch.uint32:
            draws = draws.view(torch.int32)
        return draws.to(self.device).reshape(N, self.multi_test, self.seg).contiguous()

    def forward(self, window, draws=None):
        """The model in eval mode under no_grad (the folded path) -> (logits, scores, label) on the device; no sync.
        With sgn_preprocess the window is sampled first and the logits are the mean over the draws (reference
        inference.py:103-106); ``draws`` injects the random numbers."""
        with torch.no_grad(), torch.cuda.device(self.device):
            if self.sgn_preprocess:
                N = window.shape[0]
                self.draws = self._draws(draws, N)
                rows, self.rows = ops.sgn_sample(window, self.draws, self.seg)
                out = self.model(rows.view(N * self.multi_test, self.seg, -1))
                self.logits = out[0].view(N, self.multi_test, -1).mean(1)
            elif self.models is not None:
                # logits = sum_i alpha_i * logits_i (reference ensemble.py:26-28: joint + alpha * bone)
                inputs = self._stream_inputs(window.contiguous())
                self.stream_logits, fused = [], None
                for name, net, a in zip(self.stream_names, self.models, self.alpha):
                    out = net(inputs[name])
                    out = out[0] if isinstance(out, tuple) else out
                    self.stream_logits.append(out)
                    fused = a * out if fused is None else fused + a * out
                self.logits = fused
            else:
                out = self.model(window)
                self.logits = out[0] if isinstance(out, tuple) else out
            scores = torch.softmax(self.logits, 1)
            return self.logits, scores, torch.argmax(scores, 1)

    def _explain_device(self, k=None):
        """The input gradient behind ``explain`` on the device, no sync: -> (dwin (N, 3, T, V, K), classes (N,))."""
        if self.window is None or self.logits is None:
            raise RuntimeError("agcn_amd: explain needs a prediction: call predict / forward first")
        window = self.window
        N = window.shape[0]
        if self.logits.shape[0] != N:
            raise RuntimeError("agcn_amd: explain covers the windows of the last forward; the kept logits are those of "
                               f"{self.logits.shape[0]} windows, the kept windows are {N}")
        num_class = self.logits.shape[1]
        if k is not None:
            # checked here, on the host: one_hot does not check a device tensor, and an index outside the classes would
            # only be caught by a device-side assertion that takes the whole process down
            if isinstance(k, bool) or int(k) != k or not 0 <= int(k) < num_class:
                raise ValueError(f"agcn_amd: explain takes a class index in [0, {num_class}) or None, got {k!r}")
            k = int(k)
        with torch.cuda.device(self.device):
            classes = torch.argmax(self.logits, 1) if k is None else torch.full((N,), k, device=self.device)
            onehot = torch.nn.functional.one_hot(classes, num_class).to(torch.float32)
            if self.sgn_preprocess:
                with torch.no_grad():
                    S = self.multi_test
                    rows, _ = ops.sgn_sample(window, self.draws, self.seg)
                    cot = (onehot / S).repeat_interleave(S, 0)               # the mean logit of the draws
                    _, _, dx = self.model.input_gradient(rows.view(N * S, self.seg, -1), cot)
                    dwin = ops.sgn_sample_bwd(window, self.draws, dx.view(N, S, self.seg, -1), self.seg)
            elif self.models is not None:
                # each model's gradient with respect to ITS input, then one launch that carries them back to the joint
                # window through the transposes of the streams, weighted by the alphas
                with torch.no_grad():
                    inputs = self._stream_inputs(window.contiguous())
                cot = {name: self._input_gradient(net, inputs[name], onehot).contiguous()
                       for name, net in zip(self.stream_names, self.models)}
                weights = dict(zip(self.stream_names, self.alpha))
                dwin = ops.streams_bwd(cot, self.stream_parents if self.stream_parents is not None else
                                       tuple(range(window.shape[3])), [weights.get(n, 0.0) for n in ops.STREAMS])
            else:
                dwin = self._input_gradient(self.model, window, onehot)
        return dwin, classes

    @staticmethod
    def _input_gradient(net, window, onehot):
        """AGCN / AAGCN: the eval-mode backward with respect to the window alone (tools/saliency.py::saliency).
        The parameters' requires_grad is switched off for the call on purpose: the units' autograd Functions
        decide at forward time, from it, whether their backward computes weight gradients and the BatchNorm
        parameter sums (agcn_bn_bwd_eval with want_sums = 1); autograd.grad(inputs=x) alone would still run
        all of that and throw it away.  It is put back in the finally clause."""
        params = [p for p in net.parameters() if p.requires_grad]
        for p in params:
            p.requires_grad_(False)
        try:
            with torch.enable_grad():
                x = window.detach().clone().requires_grad_(True)
                out = net(x)
                out = out[0] if isinstance(out, tuple) else out
                dwin, = torch.autograd.grad((out * onehot).sum(), x)
        finally:
            for p in params:
                p.requires_grad_(True)
        return dwin

    def explain(self, k=None):
        """Which joints and frames drove the last prediction: -> (saliency (N, T, K, V) float32 numpy, classes (N,) int64
        numpy) for the windows of the last ``forward`` / ``predict``; ``k`` None explains each window's predicted class,
        an int in [0, num_class) that class (ValueError otherwise, before any launch).  saliency[n, t, body, joint] is the L2 norm over xyz of the gradient of the (mean) logit with
        respect to the normalised window; with sgn_preprocess it goes through the kept draws (``ops.sgn_sample`` again,
        ``SGN.input_gradient``, ``ops.sgn_sample_bwd``), so frames no draw picked are zero.  The gradient is not taken
        through the pre-normalisation.  One synchronising copy."""
        dwin, classes = self._explain_device(k)
        N, _, T, V, K = dwin.shape
        sal = dwin.square().sum(1).sqrt().permute(0, 1, 3, 2).reshape(N, -1)
        both = torch.cat((sal, classes.to(sal.dtype).unsqueeze(1)), 1).cpu().numpy()     # the one synchronising copy
        return both[:, :-1].reshape(N, T, K, V).copy(), both[:, -1].astype(np.int64)

    def _frames(self, frames, lead, what):
        """``frames`` (lead, max_num_skeleton, [1,] V, 3), numpy array or tensor, ``lead`` None for any length ->
        contiguous fp32 (lead, max_num_skeleton, V, 3) on the device: the one upload."""
        body = (self.max_person, self.num_joint, 3)
        shape = tuple(frames.shape)
        n = shape[0] if shape else 0
        if n < 1 or (lead is not None and n != lead) or shape[1:] not in (body, body[:1] + (1,) + body[1:]):
            first = 'L' if lead is None else lead
            raise ValueError(f"agcn_amd: {what} takes frames of shape {(first, body[0], 1) + body[1:]} or "
                             f"{(first,) + body} (absent bodies as zeros), got {shape}")
        if isinstance(frames, np.ndarray):
            frames = torch.from_numpy(np.ascontiguousarray(frames, dtype=np.float32))
        return frames.to(device=self.device, dtype=torch.float32).reshape((n,) + body).contiguous()

    def _options(self):
        return dict(num_select=self.num_select, zaxis=self.zaxis, xaxis=self.xaxis, zaxis2=self.zaxis2)


class ActionRecognition(_Recogniser):
    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.ring = torch.zeros((self.max_person, self.max_frame, self.num_joint, 3), dtype=torch.float32,
                                device=self.device)
        self.reset()

    def reset(self):
        self.ring.zero_()
        self.counter = 0          # frames present, at most max_frame
        self.head = 0             # oldest slot once the ring is full = the slot the next frame goes to

    def append_data(self, frame):
        """frame (max_num_skeleton, 1, V, 3), numpy array or tensor."""
        want = (self.max_person, 1, self.num_joint, 3)
        if tuple(frame.shape) != want:
            raise ValueError(f"agcn_amd: append_data takes a frame of shape {want} (absent bodies as zeros), "
                             f"got {tuple(frame.shape)}")
        if isinstance(frame, np.ndarray):
            frame = torch.from_numpy(np.ascontiguousarray(frame, dtype=np.float32))
        frame = frame.to(device=self.device, dtype=torch.float32).reshape(self.max_person, self.num_joint, 3).contiguous()
        if self.counter < self.max_frame:
            slot = self.counter
            self.counter += 1
        else:
            slot = self.head
            self.head = (self.head + 1) % self.max_frame
        with torch.cuda.device(self.device):
            ops.skel_append(self.ring, frame, slot, self.counter, self.moving_avg)

    def normalize(self):
        """Selection + normalisation of the current window -> (1, 3, max_frame, V, K) on the device; no sync."""
        origin = self.head if self.counter == self.max_frame else 0
        with torch.cuda.device(self.device):
            self.window, self.selected, self.energy = ops.prenorm(
                self.ring.unsqueeze(0), num_select=self.num_select, origin=origin, zaxis=self.zaxis, xaxis=self.xaxis,
                zaxis2=self.zaxis2)
        return self.window

    def predict(self, draws=None):
        """-> (softmax scores of the current window as a list, label)."""
        _, scores, label = self.forward(self.normalize(), draws)
        both = torch.cat((scores[0], label.to(scores.dtype))).cpu()      # the one synchronising copy
        return both[:-1].tolist(), int(both[-1].item())


def _fetch(scores, labels):
    """(P, C) scores and (P,) labels on the device -> numpy (P, C) fp32 and (P,) int64 in one synchronising copy."""
    both = torch.cat((scores, labels.to(scores.dtype).unsqueeze(1)), 1).cpu().numpy()
    return both[:, :-1].copy(), both[:, -1].astype(np.int64)


class RecordingRecognition(_Recogniser):
    """Labels a whole recording: the window ``ActionRecognition`` holds after appending frame ``end``, for many ``end``
    at once.  One upload of the recording, one ``ops.skel_smooth``, then per batch of at most ``batch`` windows one
    ``ops.prenorm_windows`` and one eval forward; the scores of all batches come to the host in one copy."""

    def __init__(self, *args, batch=64, **kwargs):
        super().__init__(*args, **kwargs)
        if batch < 1:
            raise ValueError("agcn_amd: need batch >= 1")
        self.batch = int(batch)
        self.smoothed = None      # (max_num_skeleton, max(L, max_frame), V, 3): the recording as a ring would hold it

    def prepare(self, frames):
        """Upload + moving average -> the pool (1, Mmax, Lp, V, 3) the window kernel reads, Lp = max(L, max_frame): a
        recording shorter than the window is followed by zero frames, which no window reaches (len <= end + 1)."""
        raw = self._frames(frames, None, 'label')
        L = raw.shape[0]
        if self.moving_avg > L:
            raise ValueError(f"agcn_amd: a recording of {L} frames is shorter than moving_avg = {self.moving_avg}")
        if L < self.max_frame:
            raw = torch.cat((raw, raw.new_zeros((self.max_frame - L,) + tuple(raw.shape[1:]))))
        with torch.cuda.device(self.device):
            self.smoothed = ops.skel_smooth(raw, self.moving_avg)
        return self.smoothed.unsqueeze(0), L

    def normalize(self, pool, start, length):
        """Selection + normalisation of the windows (start, length) -> (N, 3, max_frame, V, K) on the device; no sync."""
        with torch.cuda.device(self.device):
            self.window, self.selected, self.energy = ops.prenorm_windows(pool, start, length, frames=self.max_frame,
                                                                          **self._options())
        return self.window

    def label(self, frames, interval=1, first=0, ends=None, draws=None):
        """frames (L, max_num_skeleton, [1,] V, 3), numpy array or tensor.  Predicts after frames first, first + interval,
        ... (or after the frames listed in ``ends``, in any order) -> (scores (P, num_class) fp32, labels (P,) int64,
        ends (P,) int64) as numpy arrays.  ``draws`` (P, multi_test, seg): the sampler's random numbers with sgn_preprocess
        (default: drawn on the device).  The logits of all P windows stay on the device in ``self.logits``; window,
        selected and energy are those of the last batch."""
        pool, L = self.prepare(frames)
        if ends is None:
            start, length, _ = window_plan_device(L, self.max_frame, self.device, interval, first)
            ends = np.arange(first, L, interval, dtype=np.int64)
        else:
            ends = np.asarray(ends, dtype=np.int64).reshape(-1)
            plan = np.stack(window_plan(L, self.max_frame, ends))
            start, length = torch.from_numpy(plan).to(self.device)         # one small upload for an explicit list
        if not len(ends):
            raise ValueError("agcn_amd: label needs at least one window")
        logits, scores, labels = [], [], []
        for b in range(0, len(ends), self.batch):
            win = self.normalize(pool, start[b:b + self.batch], length[b:b + self.batch])
            lg, sc, lb = self.forward(win, None if draws is None else draws[b:b + self.batch])
            logits.append(lg)
            scores.append(sc)
            labels.append(lb)
        self.logits = torch.cat(logits)
        scores, labels = _fetch(torch.cat(scores), torch.cat(labels))    # the one synchronising copy
        return scores, labels, ends


class MultiStreamRecognition(_Recogniser):
    """``num_streams`` independent streams on one device: one ring each, one launch per tick for all of them
    (``ops.skel_append_many``) and one batch per prediction (``ops.prenorm_windows`` over the rings, block = the stream,
    start = its oldest slot, len = its frame count).  The host keeps (count, head) per stream."""

    def __init__(self, model, num_streams, *args, **kwargs):
        super().__init__(model, *args, **kwargs)
        if num_streams < 1:
            raise ValueError("agcn_amd: need num_streams >= 1")
        self.num_streams = int(num_streams)
        self.rings = torch.zeros((self.num_streams, self.max_person, self.max_frame, self.num_joint, 3),
                                 dtype=torch.float32, device=self.device)
        self.streams = []         # the streams of the last predict(), in the order of its rows
        self.reset()

    def reset(self):
        self.rings.zero_()
        self.counter = np.zeros(self.num_streams, dtype=np.int32)      # frames present, at most max_frame
        self.head = np.zeros(self.num_streams, dtype=np.int32)         # oldest slot once a ring is full

    def append_data(self, frames, present=None):
        """frames (S, max_num_skeleton, [1,] V, 3), numpy array or tensor; ``present`` a host bool mask (S,), None =
        every stream has a frame this tick.  One frame upload, one index upload, one launch."""
        S = self.num_streams
        frames = self._frames(frames, S, 'append_data')
        present = np.ones(S, dtype=bool) if present is None else np.asarray(present, dtype=bool).reshape(-1)
        if present.shape != (S,):
            raise ValueError(f"agcn_amd: present is a mask of length {S}, got {present.shape}")
        filling = present & (self.counter < self.max_frame)
        full = present & ~filling
        slot = np.where(filling, self.counter, np.where(full, self.head, -1)).astype(np.int32)
        self.counter = self.counter + filling
        self.head = np.where(full, (self.head + 1) % self.max_frame, self.head).astype(np.int32)
        index = torch.from_numpy(np.stack((slot, self.counter.astype(np.int32)))).to(self.device)
        with torch.cuda.device(self.device):
            ops.skel_append_many(self.rings, frames, index[0], index[1], self.moving_avg)

    def plan(self, streams=None):
        """-> (streams that have frames, (3, N) int32 host plan: block, start, len)."""
        ids = range(self.num_streams) if streams is None else [int(s) for s in streams]
        if any(not 0 <= s < self.num_streams for s in ids):
            raise ValueError(f"agcn_amd: streams are numbered 0..{self.num_streams - 1}")
        ids = np.asarray([s for s in ids if self.counter[s] > 0], dtype=np.int32)
        count = self.counter[ids]
        start = np.where(count == self.max_frame, self.head[ids], 0)
        return ids, np.stack((ids, start, count)).astype(np.int32)

    def normalize(self, streams=None):
        """Selection + normalisation of the streams' current windows -> (S', 3, max_frame, V, K) on the device, None if
        no stream has a frame yet; no sync."""
        ids, plan = self.plan(streams)
        self.streams = ids.tolist()
        if not len(ids):
            self.window = self.selected = self.energy = None
            return None
        block, start, length = torch.from_numpy(plan).to(self.device)
        with torch.cuda.device(self.device):
            self.window, self.selected, self.energy = ops.prenorm_windows(self.rings, start, length, block=block,
                                                                          **self._options())
        return self.window

    def predict(self, streams=None, draws=None):
        """-> (scores (S', num_class) fp32, labels (S',) int64, streams (S',)) for the streams (default: all) that have
        received a frame, as numpy arrays."""
        win = self.normalize(streams)
        if win is None:
            self.logits = None
            return np.zeros((0, 0), dtype=np.float32), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
        _, scores, labels = self.forward(win, draws)
        scores, labels = _fetch(scores, labels)                          # the one synchronising copy
        return scores, labels, np.asarray(self.streams, dtype=np.int64)
