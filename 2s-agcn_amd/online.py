"""Online action recognition (reference ``infer/inference.py::ActionRecognition`` with its
``infer/data_preprocess.py::DataPreprocessorV2``): skeletons arrive one frame at a time, the last ``max_frame`` frames of
up to ``max_num_skeleton`` tracked bodies are kept in a ring on the GPU, and a prediction selects the
``max_num_skeleton_true`` most active bodies, normalises the window and runs the model at batch 1.

Per frame: one host-to-device copy of the frame and one launch (``ops.skel_append``).  Per prediction: one launch for
selection + normalisation (``ops.prenorm``), the folded eval forward, softmax/argmax, and one device-to-host copy of the
scores and the label, which is the only synchronisation.

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


class ActionRecognition:
    def __init__(self, model, model_args=None, weights=None, max_frame=300, max_num_skeleton=4,
                 max_num_skeleton_true=2, num_joint=25, moving_avg=1, zaxis=(0, 1), xaxis=(8, 4), zaxis2=None,
                 device='cuda:0'):
        if not 1 <= max_num_skeleton_true <= max_num_skeleton:
            raise ValueError("agcn_amd: need 1 <= max_num_skeleton_true <= max_num_skeleton")
        if not 1 <= moving_avg <= max_frame:
            raise ValueError("agcn_amd: need 1 <= moving_avg <= max_frame")
        self.device = torch.device(device)
        if isinstance(model, str):
            model = load_model(model, model_args, weights)
        self.model = model.to(self.device).eval()
        self.max_frame, self.max_person, self.num_select = int(max_frame), int(max_num_skeleton), int(max_num_skeleton_true)
        self.num_joint, self.moving_avg = int(num_joint), int(moving_avg)
        self.zaxis, self.xaxis, self.zaxis2 = zaxis, xaxis, zaxis2
        self.ring = torch.zeros((self.max_person, self.max_frame, self.num_joint, 3), dtype=torch.float32,
                                device=self.device)
        # what the last predict() left on the device: the normalised window (1, 3, T, V, K), the selected bodies (1, K)
        # int32, the energies (1, Mmax) and the logits (1, num_class)
        self.window = self.selected = self.energy = self.logits = None
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

    def forward(self, window):
        """The model in eval mode under no_grad (the folded path) -> (logits, scores, label) on the device; no sync."""
        with torch.no_grad(), torch.cuda.device(self.device):
            out = self.model(window)
            self.logits = out[0] if isinstance(out, tuple) else out
            scores = torch.softmax(self.logits, 1)
            return self.logits, scores, torch.argmax(scores, 1)

    def predict(self):
        """-> (softmax scores of the current window as a list, label)."""
        _, scores, label = self.forward(self.normalize())
        both = torch.cat((scores[0], label.to(scores.dtype))).cpu()      # the one synchronising copy
        return both[:-1].tolist(), int(both[-1].item())
