"""``SGNBatches``: the input side of SGN training and evaluation -- the reference's ``NTUDataLoaders`` with its three
collates (``feeders/loader.py:33-201``: ``collate_fn_fix_train`` / ``_val`` / ``_test``) on a dataset that lives on the
device, one ``ops.sgn_collate`` launch per batch instead of a Python loop over every frame in 16 DataLoader workers.

What differs from the reference, on purpose:

* Evaluation keeps the last partial batch (the reference's loaders all have ``drop_last=True``): every sample is scored,
  as ``ensemble.py`` needs one row per sample name.
* No sort.  The reference's training collate "sorts by valid length" a list of clips that all have ``seg`` rows: numpy's
  argsort of equal keys, reversed -- a permutation of the batch that keeps ``(x, y)`` paired and changes nothing a
  training step can see.  ``SGNBatches`` does not permute.
* The draws are 32-bit patterns reduced modulo the interval width (``ops.sgn_draws``), the angles come from the device
  generator (``ops.sgn_rotation_angles``); both are seeded per epoch and can be injected (``draws=``, ``angles=``).
"""
import numpy as np
import torch

from .. import ops
from .device import DeviceLoader

MAX_RESIDENT_BYTES = 64 << 30


def rotation_theta(dataset_name):
    """The rotation range of the training collate (reference feeders/loader.py:163-171)."""
    name = str(dataset_name)
    if 'NTU60' in name and 'CS' in name:
        return 0.3
    if 'NTU60' in name and 'CV' in name:
        return 0.5
    if 'NTU120' in name:
        return 0.3
    raise ValueError(f"agcn_amd.SGNBatches: unknown dataset name {dataset_name!r} (NTU60-CS, NTU60-CV, NTU120-*)")


class _Rows(torch.utils.data.Dataset):
    """(data, label, index) of ``dataset`` without its transforms: what the collate takes."""

    def __init__(self, dataset):
        self.data, self.label = dataset.data, dataset.label

    def __len__(self):
        return len(self.label)

    def __getitem__(self, i):
        return np.asarray(self.data[i], dtype=np.float32), int(self.label[i]), i


class _Order(torch.utils.data.Sampler):
    def __init__(self):
        self.indices = []

    def __iter__(self):
        return iter(list(self.indices))

    def __len__(self):
        return len(self.indices)


class SGNBatches:
    """Iterable over one epoch of collated SGN batches ``(x (B*S, seg, 3V), label (B,), index (B,))`` on ``device``.

    dataset: anything with ``data`` (P, 3, T, V, 2) and ``label`` (P,) (``feeders.Feeder`` with an SGN dataset,
    ``SyntheticFeeder``).  mode 'train': S = 1, the seeded permutation of ``set_epoch`` (seed + epoch), drop_last, and with
    ``aug=1`` the rotation of ``rotation_theta(dataset_name)``; 'val': S = 1, in order; 'test': S = multi_test, in order.
    Evaluation keeps the last partial batch.

    resident=True uploads ``dataset.data`` once (NTU60 is 7 GB of the MI355X's 288) and every batch is one collate launch
    by index.  Above ``max_resident_bytes``, or with resident=False, the raw clips of a batch arrive through
    ``feeders.DeviceLoader`` (pinned, copied ahead) and are collated with ``index=None``.

    ``last_draws`` (B, S, seg), ``last_angles`` (B, 3) or None and ``last_L`` (B,) hold the last batch's random numbers and
    row counts; ``draws=`` / ``angles=`` are callables ``(batch number, B) -> tensor`` that replace the generator."""

    def __init__(self, dataset, batch_size, seg, multi_test=1, mode='train', dataset_name='NTU60-CV', aug=1, seed=0,
                 device='cuda', resident=True, max_resident_bytes=MAX_RESIDENT_BYTES, draws=None, angles=None,
                 num_workers=0, prefetch_depth=2):
        if mode not in ('train', 'val', 'test'):
            raise ValueError(f"agcn_amd.SGNBatches: mode is 'train', 'val' or 'test', got {mode!r}")
        self.dataset, self.batch_size, self.seg, self.mode = dataset, int(batch_size), int(seg), mode
        self.S = int(multi_test) if mode == 'test' else 1
        if self.batch_size < 1 or self.seg < 1 or self.S < 1:
            raise ValueError("agcn_amd.SGNBatches: batch_size, seg and multi_test are at least 1")
        self.theta = rotation_theta(dataset_name) if (mode == 'train' and int(aug) == 1) else None
        self.seed, self.device = int(seed), torch.device(device)
        self.draws, self.angles = draws, angles
        self.label = torch.as_tensor(np.asarray(dataset.label), dtype=torch.int64).to(self.device)
        shape = tuple(dataset.data.shape)
        if len(shape) != 5 or shape[1] != 3 or shape[4] != 2:
            raise ValueError(f"agcn_amd.SGNBatches: the dataset holds (P, 3, T, V, 2), got {shape}")
        self.resident = bool(resident) and 4 * int(np.prod(shape)) <= int(max_resident_bytes)
        self.pool, self._loader = None, None
        if self.resident:
            self.pool = torch.as_tensor(np.ascontiguousarray(dataset.data, dtype=np.float32)).to(self.device)
        else:
            self._sampler = _Order()
            dl = torch.utils.data.DataLoader(_Rows(dataset), batch_size=self.batch_size, sampler=self._sampler,
                                             drop_last=mode == 'train', num_workers=int(num_workers),
                                             persistent_workers=int(num_workers) > 0)
            self._loader = DeviceLoader(dl, self.device, depth=prefetch_depth)
        self.gen = torch.Generator(device=self.device)
        self.last_draws = self.last_angles = self.last_L = None
        self.set_epoch(0)

    def set_epoch(self, epoch):
        """Fixes the epoch's order (train: the permutation of seed + epoch, as ``Processor._loader``) and reseeds the
        generator of the draws and angles."""
        self.epoch = int(epoch)
        n = len(self.dataset.label)
        if self.mode == 'train':
            g = torch.Generator().manual_seed(self.seed + self.epoch)
            self.order = torch.randperm(n, generator=g)
        else:
            self.order = torch.arange(n)
        return self

    def __len__(self):
        n, b = len(self.order), self.batch_size
        return n // b if self.mode == 'train' else (n + b - 1) // b

    def collate(self, k, pool, index, B):
        """Batch number k of the epoch: B clips of ``pool`` (by ``index``, or its first B) -> x (B*S, seg, 3V)."""
        if self.draws is not None:
            r = self.draws(k, B).to(self.device)
        else:
            r = ops.sgn_draws(B, self.S, self.seg, self.device, generator=self.gen)
        a = None
        if self.theta is not None:
            a = (self.angles(k, B).to(self.device) if self.angles is not None
                 else ops.sgn_rotation_angles(B, self.theta, self.device, generator=self.gen))
        x, L, _ = ops.sgn_collate(pool, r.contiguous(), self.seg, index=index, angles=a)
        self.last_draws, self.last_angles, self.last_L = r, a, L
        return x.view(B * self.S, self.seg, -1)

    def __iter__(self):
        self.gen.manual_seed(self.seed + self.epoch)
        if self.resident:
            order = self.order.to(self.device)
            for k in range(len(self)):
                index = order[k * self.batch_size:(k + 1) * self.batch_size].contiguous()
                yield self.collate(k, self.pool, index, index.numel()), self.label[index], index
        else:
            self._sampler.indices = self.order.tolist()
            for k, (data, label, index) in enumerate(self._loader):
                yield self.collate(k, data.float().contiguous(), None, data.shape[0]), label.long(), index.long()
