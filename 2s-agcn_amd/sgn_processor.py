"""``SGNProcessor``: training and evaluating ``model.sgn.SGN`` or ``model.sgn_v15.SGN`` through ``main.py``
(``use_sgn_dataloader: true``), the
counterpart of the reference's SGN route (utils/processor.py: load_data :479-520 with ``FeederDataLoader``, the Adam
branch of load_optimizer, ``LabelSmoothingLoss``, train :604-778 with clip_grad_norm_ 1.0 at :698, eval :784-914 with the
mean over ``multi_test`` draws).

The data side is ``feeders.sgn.SGNBatches``: the dataset lives on the device and every batch is one collate launch
(``ops.sgn_collate``: null-row removal, two-body interleave, padding, interval draws, the training rotation).  The
train-mode forward and backward are the tensor-code composition on vendor GEMMs (at training batch sizes it beats the
recompute kernels: DESIGN.md "SGN parameter gradients", "SGN batch statistics"); evaluation runs under ``no_grad`` in
eval mode, which is the fused HIP forward on ``B * multi_test`` clips.  Single process only; Adam and SGD are
``torch.optim``'s.  Checkpoints are ``<work_dir>/weight/SGN-<epoch>-<global_step>.pt``."""
import os
import time

import numpy as np
import torch

from .feeders.sgn import SGNBatches
from .model.sgn import SGN
from .model.sgn_v15 import SGN as SGN15
from .processor import Processor, import_class
from .trainer import learning_rate


def label_smoothing_loss(logits, target, smoothing):
    """The reference's ``LabelSmoothingLoss`` (utils/loss.py:25-39): cross-entropy against 1 - eps on the target and
    eps / (C - 1) on every other class, batch mean.  Not ``nn.CrossEntropyLoss(label_smoothing=eps)``, which puts
    eps / C on every class, the target included."""
    logp = torch.log_softmax(logits, dim=-1)
    C = logits.shape[-1]
    off = float(smoothing) / (C - 1)
    dist = torch.full_like(logp, off).scatter_(1, target.view(-1, 1), 1.0 - float(smoothing))
    return torch.mean(torch.sum(-dist * logp, dim=-1))


class SGNProcessor(Processor):
    def __init__(self, arg):
        self.arg = arg
        if int(getattr(arg, 'world_size', 1)) > 1 or int(os.environ.get('WORLD_SIZE', '1')) > 1:
            raise ValueError("agcn_amd.SGNProcessor: more than one process is not built for the SGN route (world_size > 1)")
        if (getattr(arg, 'stream', 'joint') or 'joint') != 'joint':
            raise ValueError(f"agcn_amd.SGNProcessor: --stream {arg.stream} is not built for the SGN route (its collate "
                             f"reads joint data)")
        self.rank, self.world = 0, 1
        dev = arg.device if isinstance(arg.device, int) else arg.device[0]
        torch.cuda.set_device(dev)
        self.device = torch.device('cuda', dev)
        torch.manual_seed(arg.seed)
        np.random.seed(arg.seed)
        os.makedirs(os.path.join(arg.work_dir, 'weight'), exist_ok=True)
        self.global_step = 0
        if import_class(arg.model) not in (SGN, SGN15):
            raise ValueError("agcn_amd.SGNProcessor: use_sgn_dataloader trains model.sgn.SGN or model.sgn_v15.SGN only, got "
                             f"{arg.model!r}")
        self.load_model()
        self.load_data()
        self.load_optimizer()
        self.smoothing = float(getattr(arg, 'label_smoothing', 0.0))
        self.best_acc = 0.0
        self.eval_draws = []

    def load_optimizer(self):
        name = str(self.arg.optimizer)
        if name.upper() == 'ADAM':
            self.optimizer = torch.optim.Adam(self.model.parameters(), lr=self.arg.base_lr,
                                              weight_decay=self.arg.weight_decay)
        elif name.upper() == 'SGD':                     # the reference's arguments (processor.py:395-401)
            self.optimizer = torch.optim.SGD(self.model.parameters(), lr=self.arg.base_lr, momentum=0.9,
                                             nesterov=self.arg.nesterov, weight_decay=self.arg.weight_decay)
        else:
            raise ValueError(f"agcn_amd.SGNProcessor: optimizer {name!r} is not built (Adam, SGD)")

    def load_data(self):
        Feeder = import_class(self.arg.feeder)
        self.datasets, self.batches = {}, {}

        def build(name, feeder_args, loader_args, batch_size, mode):
            la = dict(loader_args or {})
            ds = self.datasets[name] = Feeder(**dict(feeder_args))
            self.batches[name] = SGNBatches(ds, batch_size, seg=int(la.get('seg', self.model.seg)),
                                            multi_test=int(la.get('multi_test', 1)), mode=mode,
                                            dataset_name=la.get('dataset', 'NTU60-CV'), aug=int(la.get('aug', 1)),
                                            seed=int(self.arg.seed), device=self.device,
                                            resident=bool(la.get('resident', True)))
        if self.arg.phase == 'train':
            build('train', self.arg.train_feeder_args, self.arg.train_dataloader_args, self.arg.batch_size, 'train')
        build('test', self.arg.test_feeder_args or self.arg.train_feeder_args,
              self.arg.test_dataloader_args or self.arg.train_dataloader_args, self.arg.test_batch_size, 'test')
        for b in self.batches.values():
            if b.seg != self.model.seg:
                raise ValueError(f"agcn_amd.SGNProcessor: the collate's seg {b.seg} is not the model's {self.model.seg}")

    def loss(self, logits, label):
        if self.smoothing == 0.0:
            return torch.nn.functional.cross_entropy(logits, label)
        return label_smoothing_loss(logits, label, self.smoothing)

    def train_step(self, x, label):
        """One optimiser step: train-mode forward (tensor code), loss, backward, clip 1.0, step."""
        self.model.train()
        logits, _ = self.model(x)
        loss = self.loss(logits, label)
        self.optimizer.zero_grad(set_to_none=True)
        loss.backward()
        self.last_grad_norm = torch.nn.utils.clip_grad_norm_(self.model.parameters(), 1.0)
        self.optimizer.step()
        return loss

    def train(self, epoch):
        lr = learning_rate(epoch, self.arg.base_lr, self.arg.step, self.arg.warm_up_epoch)
        for group in self.optimizer.param_groups:
            group['lr'] = lr
        self.print_log(f'Training epoch: {epoch + 1}, lr {lr:.6f}')
        # the three buckets of Processor.train: waiting for data (here: enqueueing the collate) / the step /
        # statistics; nothing synchronises inside the loop, the device is drained once at the end, on `model`
        timer = dict(dataloader=0.0, model=0.0, statistics=0.0)
        losses = []
        batches = self.batches['train'].set_epoch(epoch)
        mark = time.perf_counter()

        def split():
            nonlocal mark
            now = time.perf_counter()
            dt, mark = now - mark, now
            return dt
        for step, (x, label, _) in enumerate(batches):
            timer['dataloader'] += split()
            loss = self.train_step(x, label)
            self.global_step += 1
            timer['model'] += split()
            if step % self.arg.log_interval == 0:
                losses.append(float(loss.detach()))
                self.print_log(f'\tBatch({step}/{len(batches)}) done. Loss: {losses[-1]:.4f}  lr:{lr:.6f}  '
                               f'grad-norm:{float(self.last_grad_norm):.3f}')
            timer['statistics'] += split()
            if self.arg.max_steps_per_epoch and step + 1 >= self.arg.max_steps_per_epoch:
                break
        torch.cuda.current_stream().synchronize()
        timer['model'] += split()
        tot = max(sum(timer.values()), 1e-9)
        self.last_timer = dict(timer)
        self.print_log(f'\tMean training loss: {np.mean(losses) if losses else float("nan"):.4f}.')
        self.print_log(f'\tTime consumption  : [Data] {100 * timer["dataloader"] / tot:02.0f}%, '
                       f'[Network] {100 * timer["model"] / tot:02.0f}%, [Statistics] {100 * timer["statistics"] / tot:02.0f}%')

    def eval(self, epoch, save_score=None, loader_name='test'):
        """Eval mode under no_grad: the fused HIP forward on B * multi_test clips, the logits of a sample's draws averaged
        (reference processor.py:841-843); then top-k, loss and the score pickle as ``Processor.eval``.  ``eval_draws``
        keeps the draws of every batch."""
        self.model.eval()
        batches = self.batches[loader_name].set_epoch(epoch)
        S = batches.S
        scores, loss_sum, seen = [], torch.zeros((), device=self.device), 0
        self.eval_draws = []
        with torch.no_grad():
            for x, label, _ in batches:
                out, _ = self.model(x)
                out = out.view(-1, S, out.shape[1]).mean(1)
                loss_sum += torch.nn.functional.cross_entropy(out, label, reduction='sum')
                seen += label.numel()
                scores.append(out)
                self.eval_draws.append(batches.last_draws)
        score = torch.cat(scores).float().cpu().numpy() if scores else np.zeros((0, 1), dtype=np.float32)
        return self._report(epoch, loader_name, score, float(loss_sum), seen, save_score)
