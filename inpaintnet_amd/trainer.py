"""Trainer base class: the reference's optimizer loop on the HIP kernels.

Mirrors utils/trainer.py:15-376 of the reference: Trainer(dataset, model, lr,
early_stopping), train_model, loss_and_acc_on_epoch, zero_grad, step, the
abstract loss_and_acc_for_batch / process_batch_data / update_scheduler, and
the static loss helpers.  Differences that are the point of the build:
  * zero_grad() / step() act on the model's flat arenas: one memset, one fused
    Adam kernel (torch.optim.Adam semantics, lr=1e-4, betas (0.9,0.999), eps 1e-8);
  * with torch.distributed initialised (one process per GPU, backend "nccl" =
    RCCL), step() first sums the flat gradient arena over ranks in ONE all-reduce
    and folds the 1/world_size into the Adam kernel;
  * losses are the fused cross-entropy / KL kernels (autograd Functions);
  * loss/accuracy are accumulated on the device, read back once per epoch
    (the reference syncs every batch: utils/trainer.py:154).
Plotting / tensorboard plumbing of the reference is out of scope.
"""
import contextlib
import gc
import math
import os
import struct
import sys
import time
from abc import ABC, abstractmethod
from collections import OrderedDict, deque

import torch

from . import dp, ops
from .feed import DeviceFeed


def _dist_ready():
    return torch.distributed.is_available() and torch.distributed.is_initialized()


def settle_python_heap():
    """gc.collect() + gc.freeze(): everything alive now (torch's, numpy's and this package's modules: ~170 k tracked objects)
    moves to the permanent generation, which later collections do not traverse.

    Why a trainer cares (round 5, profiles/r05_cold_start.txt): a training step queues ~80 launches in ~1 ms of host time and
    the GPU needs 3.6 ms for them, so the host runs ahead -- until CPython's cyclic collector decides on a FULL collection.
    In a fresh process the third generation's threshold trips within the first dozen steps (the step objects, autograd nodes
    and ctypes arguments are the young objects that count towards it), and one traversal of the import-time heap takes
    36-40 ms on the GPU box: the launch queue drains, the GPU idles for ten steps' worth of time, and a 20-step epoch (a
    validation pass, the driver's `bench.py --steps 20 --warmup 5`) measures 1.7x the steady state -- the whole of round 4's
    "cold-start transient" (6.31 vs 3.65 ms per step).  With the old heap frozen a full collection only looks at what was
    created since: < 1 ms.

    A process-global side effect (INTEGRATION.md section 1 states it): objects alive at the FIRST trainer's construction are never
    examined by the cyclic collector again (reference counting still frees them).  Once per process -- later trainers do not
    freeze what the application has built since; INET_GC_FREEZE=0 leaves the collector alone altogether."""
    global _heap_settled
    if _heap_settled or os.environ.get("INET_GC_FREEZE", "1") == "0":
        return False
    gc.collect()
    gc.freeze()
    _heap_settled = True
    return True


_heap_settled = False


class _CrossEntropyFn(torch.autograd.Function):
    """mean CE over rows + accuracy, one wavefront per row (utils/trainer.py:271-306)."""

    @staticmethod
    def forward(ctx, weights2d, targets1d):
        rows, V = weights2d.shape
        out = torch.zeros(2, dtype=torch.float32, device=weights2d.device)
        need = ctx.needs_input_grad[0]
        dW = torch.empty_like(weights2d) if need else None
        ops.cross_entropy(weights2d, targets1d, out, dW=dW, scale=1.0 / rows, out_scale=1.0 / rows)
        ctx.dW = dW
        loss, acc = out[0], out[1]                  # the kernel accumulated the means: no follow-up launch
        ctx.mark_non_differentiable(acc)
        ctx.set_materialize_grads(False)            # (no fill launch for the accuracy's gradient)
        return loss, acc

    @staticmethod
    def backward(ctx, gloss, _gacc):
        dW = ctx.dW
        ctx.dW = None
        if gloss is None or dW is None:
            return None, None
        return dW * gloss, None


class _ElboFn(torch.autograd.Function):
    """loss = mean CE + kscale * kl_sum, accuracy -- VAETrainer.loss_and_acc_for_batch (vae_trainer.py:29-40) in ONE launch
    forward (the CE kernel also adds the KL term) and ONE launch backward (the same kernel writes dW already multiplied
    by the upstream gradient, read on the device, and hands kscale * gradient on to the KL sum's producer): the dozen
    one-element torch kernels of the unfused expression (zeros, mul, add, select-backward, dW * g) are gone."""

    @staticmethod
    def forward(ctx, weights2d, targets1d, kl_sum, kscale, out2):
        rows, V = weights2d.shape
        ops.cross_entropy_ex(weights2d, targets1d, loss_sum=out2[0:1], correct=out2[1:2], out_scale=1.0 / rows,
                             add_term=kl_sum.reshape(1), add_scale=kscale)
        ctx.save_for_backward(weights2d, targets1d)
        ctx.kscale = kscale
        # (out2 is a slice of the gradient arena's tail, zeroed by the next zero_grad(): the caller gets its own two floats -- the
        #  reference returns independent tensors, and a training script may keep them across steps)
        res = out2.clone()
        loss, acc = res[0], res[1]
        ctx.mark_non_differentiable(acc)
        ctx.set_materialize_grads(False)            # (no fill launch for the accuracy's gradient)
        return loss, acc

    @staticmethod
    def backward(ctx, gloss, _gacc):
        if gloss is None:
            return None, None, None, None, None
        w, t = ctx.saved_tensors
        dW = torch.empty_like(w)
        gkl = torch.empty((), dtype=torch.float32, device=w.device)
        ops.cross_entropy_ex(w, t, dW=dW, scale=1.0 / w.shape[0], scale_dev=gloss.reshape(1).contiguous(),
                             fwd_out=gkl.reshape(1), fwd_scale=ctx.kscale)
        return dW, None, gkl, None, None


def _ce_w_forward(ctx, weights2d, targets1d, ce, sink, **glue):
    """The forward both weighted functions share: ONE counting launch (it also zeroes the statistics' words) and ONE loss launch.
    ce = (class weights on the device or None, label_smoothing, ignore_index); sink: a dict that receives the step's device
    tensors, or None."""
    rows, V = weights2d.shape
    counted = ops.class_counts(targets1d, V, ce[0], ce[2], extra=3 * V)
    out = torch.empty(2, dtype=torch.float32, device=weights2d.device)
    stats = counted.extra.view(V, 3)
    ops.cross_entropy_w(weights2d, targets1d, counted, *ce, loss=out[0:1], accuracy=out[1:2], class_stats=stats, **glue)
    ctx.save_for_backward(weights2d, targets1d)
    ctx.counted, ctx.ce = counted, ce            # the backward takes denom from the forward's count: it does not recount
    if sink is not None:
        sink.update(denom=counted.denom, n_valid=counted.n_valid, class_stats=stats)
    loss, acc = out[0], out[1]
    ctx.mark_non_differentiable(acc)
    ctx.set_materialize_grads(False)             # (no fill launch for the accuracy's gradient)
    return loss, acc


class _CrossEntropyWFn(torch.autograd.Function):
    """torch's F.cross_entropy(weights2d, targets1d, weight, label_smoothing=, ignore_index=) + the accuracy over the valid rows
    (DESIGN.md section 28): one counting launch plus one loss launch forward, one loss launch backward (dW already times the
    upstream gradient, read on the device)."""

    @staticmethod
    def forward(ctx, weights2d, targets1d, weight, label_smoothing, ignore_index, sink):
        return _ce_w_forward(ctx, weights2d, targets1d, (weight, label_smoothing, ignore_index), sink)

    @staticmethod
    def backward(ctx, gloss, _gacc):
        if gloss is None:
            return (None,) * 6
        w, t = ctx.saved_tensors
        dW = torch.empty_like(w)
        ops.cross_entropy_w(w, t, ctx.counted, *ctx.ce, dW=dW, scale_dev=gloss.reshape(1).contiguous())
        return (dW,) + (None,) * 5


class _ElboWFn(torch.autograd.Function):
    """_ElboFn on the weighted kernel: loss = weighted CE + kscale * kl_sum, accuracy; the same launches as _CrossEntropyWFn, the
    KL term folded into the loss launch and kscale * gradient handed on to the KL sum's producer by the backward launch."""

    @staticmethod
    def forward(ctx, weights2d, targets1d, kl_sum, kscale, weight, label_smoothing, ignore_index, sink):
        ctx.kscale = kscale
        return _ce_w_forward(ctx, weights2d, targets1d, (weight, label_smoothing, ignore_index), sink,
                             add_term=kl_sum.reshape(1), add_scale=kscale)

    @staticmethod
    def backward(ctx, gloss, _gacc):
        if gloss is None:
            return (None,) * 8
        w, t = ctx.saved_tensors
        dW = torch.empty_like(w)
        gkl = torch.empty((), dtype=torch.float32, device=w.device)
        ops.cross_entropy_w(w, t, ctx.counted, *ctx.ce, dW=dW, scale_dev=gloss.reshape(1).contiguous(), fwd_out=gkl.reshape(1),
                            fwd_scale=ctx.kscale)
        return (dW, None, gkl) + (None,) * 5


def _ce_weight_on(weight, V, device):
    """Class weights as the kernel takes them: None, or V float32 on `device`."""
    if weight is None:
        return None
    w = torch.as_tensor(weight, dtype=torch.float32).to(device).contiguous()
    if w.dim() != 1 or w.numel() != V:
        raise ValueError(f"weight must hold one value for each of the {V} classes, got shape {tuple(w.shape)}")
    return w


def class_stats_add(weights, targets, class_stats, confusion):
    """class_stats (V, 3) and confusion (V, V), int64 on the device, += the plain argmax statistics of one batch of logits (any
    leading shape) against its targets: the counting launch and one loss launch without a loss."""
    V = weights.size(-1)
    w2 = weights.detach().contiguous().view(-1, V)
    t1 = targets.contiguous().view(-1)
    if t1.dtype != torch.int64:
        t1 = t1.long()
    ops.cross_entropy_w(w2, t1, ops.class_counts(t1, V), class_stats=class_stats, confusion=confusion)


def class_report_from_counts(class_stats, confusion, names=None):
    """The per-class report of the testers from the integers the loss kernel accumulated: class_stats (V, 3) = {target count, hits,
    predicted}, confusion (V, V) indexed [target, argmax] (tensors or arrays; they are read on the host).  recall = hits / counts,
    precision = hits / predicted, f1 = 2 hits / (counts + predicted), each NaN where its denominator is 0; accuracy = sum hits /
    sum counts; balanced_accuracy = the mean recall over the classes present."""
    import numpy as np
    stats = np.asarray(class_stats.cpu() if isinstance(class_stats, torch.Tensor) else class_stats, dtype=np.int64)
    conf = np.asarray(confusion.cpu() if isinstance(confusion, torch.Tensor) else confusion, dtype=np.int64)
    counts, hits, predicted = stats[:, 0], stats[:, 1], stats[:, 2]

    def ratio(num, den):
        out = np.full(len(den), np.nan)
        np.divide(num, den, out=out, where=den > 0)
        return out
    recall = ratio(hits.astype(np.float64), counts)
    total = int(counts.sum())
    present = counts > 0
    return {"counts": counts, "predicted": predicted, "hits": hits, "recall": recall,
            "precision": ratio(hits.astype(np.float64), predicted), "f1": ratio(2.0 * hits, counts + predicted),
            "accuracy": float(hits.sum()) / total if total else float("nan"),
            "balanced_accuracy": float(recall[present].mean()) if present.any() else float("nan"),
            "confusion": conf, "names": names}


def index_to_note_names(dataset, V):
    """The dataset's index-to-note table as a list of V strings, or None where it has none."""
    dicts = getattr(dataset, "index2note_dicts", None)
    if not dicts:
        return None
    table = dicts[getattr(dataset, "NOTES", 0)] if len(dicts) > 1 else dicts[0]
    try:
        return [str(table[i]) for i in range(V)]
    except (KeyError, IndexError, TypeError):
        return None


def _ce_w_apply(weights, targets, weight, label_smoothing, ignore_index, sink):
    """_CrossEntropyWFn on logits of any leading shape; sink: a dict for the step's device tensors, or None."""
    V = weights.size(-1)
    w2 = weights.contiguous().view(-1, V)
    t1 = targets.contiguous().view(-1)
    if t1.dtype != torch.int64:
        t1 = t1.long()
    return _CrossEntropyWFn.apply(w2, t1, _ce_weight_on(weight, V, w2.device), float(label_smoothing), ignore_index, sink)


class _KLFn(torch.autograd.Function):
    """beta * mean_b sum_d KL(N(mu, sigma) || N(0,1))   (vae_trainer.py:128-139)."""

    @staticmethod
    def forward(ctx, mu, ls, beta):
        acc = torch.zeros(1, dtype=torch.float32, device=mu.device)
        ops.reparam_kl(mu, ls, None, kl_sum=acc)
        ctx.save_for_backward(mu, ls)
        ctx.k = beta / mu.shape[0]
        return acc[0] * ctx.k

    @staticmethod
    def backward(ctx, g):
        mu, ls = ctx.saved_tensors
        dmu, dls = ops.latent_bwd(None, mu, ls, None, ctx.k)
        return dmu * g, dls * g, None


class Trainer(ABC):
    """utils/trainer.py:15-39"""

    feed_fields = (0, 1)       # which members of a (score, metadata) batch the trainer needs on the device

    CE_SETTINGS = ("ce_weight", "label_smoothing", "ignore_index")

    def __init__(self, dataset, model, lr=1e-4, early_stopping=False, max_grad_norm=None, weight_decay=0.0, decay_all=False,
                 ema_decay=None, ema_warmup=False, ce_weight=None, label_smoothing=0.0, ignore_index=None):
        """max_grad_norm (None or 0 < value <= inf): clip the gradient arena by its global norm in front of every optimizer step, as
        torch.nn.utils.clip_grad_norm_(..., error_if_nonfinite=False) around optimizer.step() would, and DROP a step whose gradient
        holds an inf or a NaN instead of folding it into the weights -- both on the device (ops.grad_sqnorm in
        front of the optimizer launch, which takes its partial sums; inf = measure and drop only, never clip).  The step reports,
        read at the usual lag (check_steps), keep last_grad_norm, clipped_steps and nonfinite_steps up to date.  None: nothing changes.

        weight_decay (>= 0, finite): decoupled weight decay as torch.optim.AdamW applies it, p *= 1 - lr * weight_decay in front of
        every update, inside the optimizer launch (ops.adamw_step).  The weight matrices decay -- the entries
        of model._table with "weight" in the name and two dimensions, what Model.init_reference_style calls a weight matrix; biases,
        b_0 and x_0 do not.  decay_all=True decays every element, torch's default.
        ema_decay (None or in [0, 1)): keep `self.ema`, an exponential moving average of the weights, up to date inside the same
        launch: ema = ema_decay * ema + (1 - ema_decay) * p behind every applied step; a skipped or dropped step leaves it alone.
        ema_warmup: step t (t = adam_t of that launch) uses min(ema_decay, (1 + t) / (10 + t)), evaluated on the host per launch
        like lr.  ema_state_dict() and `with trainer.ema_weights():` read it; train_model validates under it.
        With weight_decay == 0 and ema_decay None the trainer launches what it launched before, under the same labels.

        ce_weight, label_smoothing, ignore_index: the reconstruction loss becomes torch's CrossEntropyLoss(weight=ce_weight,
        label_smoothing=label_smoothing, ignore_index=ignore_index).  ce_weight: None or one finite value
        >= 0 for each of the V tokens (a sequence or a tensor; 0 is legal: that class contributes nothing as a target and is still
        counted in the statistics); label_smoothing: finite, in [0, 1]; ignore_index: None (nothing is ignored) or an int outside
        [0, V).  The mean is over the weights of the valid targets the process sees: under data parallelism the denominator is the
        rank's own shard, with no collective -- the convention of free_nats_per='dim'.  The settings are part of the objective, so
        validation (train=False) uses them too; the accuracy stays the plain token accuracy over the valid rows.  After a step on
        this path `last_ce` holds the device tensors {'denom' () float64, 'n_valid' () int64, 'class_stats' (V, 3)
        int64: per class its count as a target, of those the hits, its count as the argmax} -- reading them is the caller's
        synchronisation.  With the defaults the trainer launches what it launched before and last_ce stays None."""
        self.ce_weight, self.label_smoothing, self.ignore_index = self._ce_settings(ce_weight, label_smoothing, ignore_index,
                                                                                    self._num_classes(dataset))
        self._ce_weight_dev = None                   # ce_weight on the logits' device, made at the first step that needs it
        self.last_ce = None
        weight_decay = float(weight_decay)
        if not (weight_decay >= 0.0 and math.isfinite(weight_decay)):          # (NaN fails the comparison)
            raise ValueError(f"weight_decay must be finite and >= 0, got {weight_decay}")
        if ema_decay is not None:
            ema_decay = float(ema_decay)
            if not 0.0 <= ema_decay < 1.0:
                raise ValueError(f"ema_decay must be None or in [0, 1), got {ema_decay}")
        elif ema_warmup:
            raise ValueError("ema_warmup needs ema_decay")
        if max_grad_norm is not None:
            max_grad_norm = float(max_grad_norm)
            if not max_grad_norm > 0.0:              # (NaN fails the comparison too)
                raise ValueError(f"max_grad_norm must be None or in (0, inf], got {max_grad_norm}")
        self.max_grad_norm = max_grad_norm
        self.last_grad_norm = None                   # the norm the newest report read so far holds (before clipping, gscale applied)
        self.clipped_steps = 0
        self.nonfinite_steps = 0                     # steps dropped for an inf / NaN gradient (not chain failures, not replayed)
        self._sqnorm = None                          # the norm kernel's float64 partial sums, allocated at the first clipped step
        self.dataset = dataset
        self.model = model
        self.lr = lr
        self.betas = (0.9, 0.999)
        self.eps = 1e-8
        self.adam_m = torch.zeros_like(model.flat)
        self.adam_v = torch.zeros_like(model.flat)
        self.adam_t = 0
        self.weight_decay, self.decay_all = weight_decay, bool(decay_all)
        self.ema_decay, self.ema_warmup = ema_decay, bool(ema_warmup)
        # built once: the mask only when something decays and not everything does, the EMA arena from the weights as they are now
        self._decay_mask = self._build_decay_mask() if weight_decay > 0.0 and not decay_all else None
        self.ema = model.flat.clone() if ema_decay is not None else None
        self._ema_swapped = None                     # model.flat's own values while ema_weights() holds the EMA in their place
        self.early_stopping = False
        if early_stopping:
            self.early_stopping = True
            self.early_stopper = EarlyStopping()
        self.last_epoch_seconds = None
        self.start_epoch = 0                         # load_training_state() moves it
        self.chain_fallback = True                   # on a chain-kernel timeout: per-step kernels + retry (else raise)
        self.chain_fallbacks = 0
        self.lost_steps = 0                          # optimizer steps the device skipped (their batches were run again)
        # deferred side-stream joins for zero_grad() -> forward -> backward -> step() sequences (see zero_grad)
        self.overlap_backward = False
        # Step reports (inet_adam_step_w): every optimizer launch leaves a record of what it decided; the host reads the
        # record of step k when it has queued step k + report_lag -- by then that kernel has normally run, so the read costs
        # nothing, and it happens at the SAME step on every rank of a data-parallel job (the decision itself is the ranks'
        # summed flag), so all ranks fall back and repeat the same batches together.
        # The lag is also how far the host may run ahead, and that must be FAR: with a lag of 2 the B = 256 step measured 3.87 ms
        # against 3.63 without any report (4: 3.78, 8: 3.66-3.73, 14: 3.62-3.64; one box, profiles/r04_b_report_lag.txt) whatever the
        # wait was made of (event synchronize, event query, a plain host spin on the pinned word): the host's launch loop has
        # pauses of several milliseconds now and then, and only a deep queue hides them from the GPU.
        self.report_lag = int(os.environ.get("INET_REPORT_LAG", "12"))
        self._tag = 0
        self._inflight = deque()                     # tags whose report has not been read yet, oldest first
        self._reports = None                         # ring of _NREP records in pinned host memory, written by the kernel
        self._report_events = None                   # one event per record, recorded behind its optimizer launch
        self._recent = deque(maxlen=self._NREP)      # (tag, batch) of the epoch loop's last steps: what a fallback runs again
        self._lost = []                              # tags found skipped since the last fallback
        # the host must stay ahead of the GPU from the first step on: no full garbage collection over the import-time heap
        # in the middle of the first steps (settle_python_heap)
        settle_python_heap()
        if model.grad.is_cuda:                       # the report ring and its events exist before the first step, not in it
            # ... and so does every kernel of the library: the HIP runtime loads code objects and builds function objects on the
            # launch path of a kernel's FIRST launch, and which kernels a step meets first depends on its branch (the first
            # free-running step of a process paid 1.3 ms of host time for it, 11-16 ms now and then: csrc/preload.hip)
            ops.preload()
            self._report_slot(0)
            for e in self._report_events:
                e.record()

    # ---- the weighted reconstruction loss --------------------
    @staticmethod
    def _num_classes(dataset):
        """V as the trainers' keyword checks see it: the size of every voice's vocabulary where they agree, else None."""
        dicts = getattr(dataset, "note2index_dicts", None)
        sizes = {len(d) for d in dicts} if dicts else set()
        return sizes.pop() if len(sizes) == 1 else None

    @staticmethod
    def _ce_settings(ce_weight, label_smoothing, ignore_index, V):
        """The three settings checked and in their stored form (ce_weight: a float32 host tensor or None)."""
        if ce_weight is not None:
            try:
                w = torch.as_tensor(ce_weight, dtype=torch.float32).detach().cpu().contiguous().clone()
            except (TypeError, ValueError, RuntimeError):
                raise ValueError(f"ce_weight must be None or a sequence of class weights, got {type(ce_weight).__name__}")
            if w.dim() != 1 or w.numel() == 0 or (V is not None and w.numel() != V):
                raise ValueError(f"ce_weight must hold one weight for each of the {V} tokens, got shape {tuple(w.shape)}")
            if not bool(torch.isfinite(w).all()) or bool((w < 0).any()):
                raise ValueError("ce_weight must be finite and >= 0")
            ce_weight = w
        if isinstance(label_smoothing, bool) or not isinstance(label_smoothing, (int, float)) or \
                not 0.0 <= label_smoothing <= 1.0:                              # (NaN fails both comparisons)
            raise ValueError(f"label_smoothing must be finite and in [0, 1], got {label_smoothing!r}")
        if ignore_index is not None:
            if isinstance(ignore_index, bool) or not isinstance(ignore_index, int) or not -2 ** 63 <= ignore_index < 2 ** 63 or \
                    (V is not None and 0 <= ignore_index < V):
                raise ValueError(f"ignore_index must be None or an int outside [0, {V}), got {ignore_index!r}")
        return ce_weight, float(label_smoothing), ignore_index

    def _ce_plain(self):
        return self.ce_weight is None and self.label_smoothing == 0.0 and self.ignore_index is None

    def _ce_args(self, device):
        """(class weights on `device` or None, label_smoothing, ignore_index): what the weighted functions take."""
        if self.ce_weight is not None and (self._ce_weight_dev is None or self._ce_weight_dev.device != device):
            self._ce_weight_dev = self.ce_weight.to(device)
        return (self._ce_weight_dev if self.ce_weight is not None else None), self.label_smoothing, self.ignore_index

    def _ce_loss(self, weights, targets):
        """mean_crossentropy_loss_and_accuracy under the trainer's settings; leaves last_ce."""
        if self._ce_plain():
            self.last_ce = None
            return self.mean_crossentropy_loss_and_accuracy(weights, targets)
        if type(self).mean_crossentropy_loss_and_accuracy is not Trainer.mean_crossentropy_loss_and_accuracy:
            self.last_ce = None                      # an override: it is handed the settings and keeps its own counsel
            w, e, i = self._ce_args(weights.device)
            return self.mean_crossentropy_loss_and_accuracy(weights, targets, weight=w, label_smoothing=e, ignore_index=i)
        self.last_ce = {}
        return _ce_w_apply(weights, targets, *self._ce_args(weights.device), self.last_ce)

    def class_counts(self, data_loader):
        """The int64 histogram (V,) of a loader's target tokens -- every token of every score a batch holds -- counted on the
        device (ops.class_counts), returned on the host: what class_weights() takes."""
        V = self._num_classes(self.dataset)
        if V is None:
            raise ValueError("class_counts: the dataset's voices do not share one vocabulary")
        total = None
        for batch in data_loader:
            score = batch[0] if isinstance(batch, (tuple, list)) else batch
            t = score.to(self.model.flat.device).reshape(-1)
            c = ops.class_counts((t if t.dtype == torch.int64 else t.long()).contiguous(), V).counts
            total = c.clone() if total is None else total + c
        if total is None:
            raise ValueError("class_counts: the loader is empty")
        ops.check_tokens("Trainer.class_counts")
        return total.cpu()

    @staticmethod
    def class_weights(counts, scheme='inverse', beta=0.999, normalize=True):
        """Class weights from a histogram, on the host, in float64 -> a float32 tensor (V,).  scheme 'inverse': 1 / n_c;
        'inverse_sqrt': 1 / sqrt(n_c); 'effective': (1 - beta) / (1 - beta^n_c), the effective number of samples of Cui et al. 2019
        (0 <= beta < 1).  A class with count 0 gets the weight of the rarest present class.  normalize: scaled so that sum_c w_c n_c
        = sum_c n_c -- the weighted loss then stays on the plain loss's scale on the counted data."""
        n = torch.as_tensor(counts).detach().cpu().to(torch.float64).reshape(-1)
        if n.numel() == 0 or bool((n < 0).any()) or not bool(torch.isfinite(n).all()) or not bool((n > 0).any()):
            raise ValueError("class_weights: counts must be non-negative with at least one class present")
        present = n > 0
        safe = torch.where(present, n, torch.ones_like(n))
        if scheme == 'inverse':
            w = 1.0 / safe
        elif scheme == 'inverse_sqrt':
            w = 1.0 / safe.sqrt()
        elif scheme == 'effective':
            beta = float(beta)
            if not 0.0 <= beta < 1.0:
                raise ValueError(f"class_weights: beta must lie in [0, 1), got {beta}")
            w = (1.0 - beta) / (1.0 - torch.pow(torch.full_like(safe, beta), safe))
        else:
            raise ValueError(f"class_weights: scheme must be 'inverse', 'inverse_sqrt' or 'effective', got {scheme!r}")
        w = torch.where(present, w, w[present].max())                           # (the rarest present class has the largest weight)
        if normalize:
            w = w * (n.sum() / (w * n).sum())
        return w.to(torch.float32)

    # ---- utils/trainer.py:41-124 (plot/log plumbing omitted) -----------------------
    def train_model(self, batch_size, num_epochs, plot=False, log=False, seed=0):
        """Epoch loop of the reference (train pass, validation pass, stats, save, optional early stopping).
        `batch_size` is the GLOBAL batch.  Under torch.distributed every rank iterates the same loader (same shuffle:
        the host generators are seeded identically), takes its contiguous shard of every batch, and sees the same
        epoch statistics (they are summed over ranks), so save / early-stopping decisions agree on all ranks."""
        if dp.world_size() > 1:
            dp.seed_shared(seed)
            dp.seed_rank(seed)
            dp.broadcast_params(self.model.flat)
        train_loader, val_loader, _ = self.dataset.data_loaders(batch_size=batch_size, split=(0.70, 0.20))
        print('Num Train Batches: ', len(train_loader))
        print('Num Valid Batches: ', len(val_loader))
        try:
            for epoch in range(self.start_epoch, num_epochs):
                self.update_scheduler(epoch)
                stats = []
                for loader, train in ((train_loader, True), (val_loader, False)):
                    self.model.train(train)
                    # with an EMA the validation pass -- and with it early stopping -- looks at the EMA weights
                    with (self.ema_weights() if self.ema is not None and not train else contextlib.nullcontext()):
                        stats += self.loss_and_acc_on_epoch(data_loader=loader, epoch_num=epoch, train=train)
                self.print_epoch_stats(epoch, num_epochs, *stats)
                if dp.rank() == 0:
                    self.model.save()
                    if self.ema is not None:
                        torch.save({k: v.cpu() for k, v in self.ema_state_dict().items()}, self.model.filepath + '_ema')
                    if epoch > 0 and epoch % 10 == 0:
                        self.model.save_checkpoint(epoch)
                        self.save_training_state(self.model.filepath + f'_{epoch}.trainer', epoch + 1)
                if self.early_stopping and self.early_stopper(stats[2], self.model):
                    print("Early Stopping")
                    return
        finally:
            if self._inflight:                       # (every exit path: nothing a late report holds may go unread)
                if sys.exc_info()[0] is None:
                    self.finish()
                else:                                # an exception is on its way out already: do not mask it (as __exit__)
                    try:
                        self.finish()
                    except Exception:
                        pass

    # ---- utils/trainer.py:126-163 ---------------------------------------------------
    def loss_and_acc_on_epoch(self, data_loader, epoch_num=None, train=True):
        dev = self.model.flat.device
        sums = torch.zeros(5, dtype=torch.float32, device=dev)        # loss sum, accuracy sum, batches, chain timeouts, bad tokens
        t0 = time.time()
        prev_overlap, self.overlap_backward = self.overlap_backward, bool(train)
        try:
            if not isinstance(data_loader, DeviceFeed):
                # this rank's shard of every batch, copied on a side stream two batches ahead (feed.py)
                data_loader = DeviceFeed(data_loader, fields=self.feed_fields, device=dev)
            for sample_id, batch in enumerate(data_loader):
                batch_data = self.process_batch_data(batch)
                self._run_batch(batch_data, epoch_num, train, sums)
            if train:                                # the reports of the last report_lag steps (replays what they lost)
                self._settle(epoch_num, sums)
        finally:
            self.overlap_backward = prev_overlap
            ops.side_defer(False)
            self._recent.clear()
        # Chain launches outside optimizer steps (validation passes) have no step report: their status travels with the sums, so
        # that every rank sees every rank's failures and all of them raise together instead of one leaving the others in a
        # collective.  (One synchronisation per epoch; the sums' read-back was one already.)
        if sums.is_cuda:
            torch.cuda.synchronize(dev)
            sums[3] = float(max(ops.chain_status(), 0))
            sums[4] = float(max(ops.token_status(), 0))     # (validation passes have no step report: the count travels here)
        dp.allreduce_sum_(sums)                      # every rank reports (and early-stops on) the global means
        out = sums.tolist()                          # the one device->host sync of the epoch
        if sums.is_cuda:
            ops.chain_status(reset=True)             # persistent kernels: bounded spins report here instead of hanging
            ops.token_status(reset=True)
        if out[4] > 0:                               # on every rank together (decoder.py:36-45 check_index)
            raise ops.TokenRangeError(f"Invalid Value of index: {int(out[4])} launch(es) (all ranks) met a token outside "
                                      "[0, num_notes) (Trainer.loss_and_acc_on_epoch); the results computed from it are not valid")
        if out[3] > 0:
            raise RuntimeError(f"{int(out[3])} chain-kernel workgroups (all ranks) gave up waiting for their group during "
                               "this epoch outside an optimizer step (inet_chain_status); its results are not valid")
        n = max(out[2], 1.0)
        self.last_epoch_seconds = time.time() - t0
        return out[0] / n, out[1] / n

    def _run_batch(self, batch_data, epoch_num, train, sums, replay=False):
        """One batch of the epoch loop.  A ChainTimeoutError out of step() means: an optimizer step issued report_lag steps ago
        (or later) skipped itself because a persistent kernel of some rank gave up waiting for its group.  Nothing is corrupted
        -- on EVERY rank the optimizer kernel has left the weights alone since (it reads the ranks' summed flag) and the masked
        epoch statistics left those batches out -- so all ranks switch to the per-step kernels and run the lost batches again,
        in order."""
        try:
            self.zero_grad()
            if train:
                loss, accuracy = self.loss_and_acc_for_batch(batch_data, epoch_num, train=True)
                loss.backward()
                self._recent.append((self._tag, batch_data))       # step() issues its optimizer launch under this tag
                self.step()
            else:
                with torch.no_grad():
                    loss, accuracy = self.loss_and_acc_for_batch(batch_data, epoch_num, train=False)
        except ops.ChainTimeoutError:
            if replay or not self.chain_fallback:
                raise
            self._replay(self._fall_back_from_chains(), epoch_num, sums)
            return
        self._accumulate_stats(sums, loss, accuracy, self._flag())

    def _replay(self, lost, epoch_num, sums):
        batches = dict(self._recent)
        for tag in lost:
            if tag not in batches:
                raise RuntimeError(f"optimizer step {tag} was skipped after a chain-kernel timeout and its batch is no longer "
                                   "held (report_lag too large for the replay window)")
            self._run_batch(batches[tag], epoch_num, True, sums, replay=True)
        self._settle(epoch_num, sums, replay=True)

    def _settle(self, epoch_num, sums, replay=False):
        """Read every outstanding step report (waits for those optimizer launches); lost steps are run again."""
        try:
            self.check_steps(wait_all=True)
        except ops.ChainTimeoutError:
            if replay or not self.chain_fallback:
                raise
            self._replay(self._fall_back_from_chains(), epoch_num, sums)

    def _flag(self):
        """The device word that decides whether this step counts: the ranks' summed chain status under data parallelism
        (None = the process's own status word)."""
        return self.model.step_flag if dp.world_size() > 1 and self._reports_on() else None

    @staticmethod
    def _accumulate_stats(sums, loss, accuracy, step_flag=None):
        """sums[:3] += (loss, accuracy, 1) on the device in one launch (inet_epoch_stats_add_ex); a batch whose chain kernels
        timed out on any rank -- its results are not valid and the optimizer kernel skipped it -- stays out of the means."""
        loss = loss.detach()
        if loss.dim() > 0:
            loss = loss.mean()
        loss = loss.reshape(1).to(sums.dtype).contiguous()
        acc = None if accuracy is None else accuracy.detach().reshape(1).to(sums.dtype).contiguous()
        if not sums.is_cuda:                         # (the world_size-2 gloo tests drive this loop with host tensors)
            if step_flag is not None and float(step_flag[0]) != 0.0:
                return
            sums[0] += loss[0]
            if acc is not None:
                sums[1] += acc[0]
            sums[2] += 1.0
            return
        ops.epoch_stats_add(sums, loss, acc, step_flag)

    def zero_grad(self):
        """utils/trainer.py:165-170.  With `overlap_backward` set (the epoch loop and bench.py set it) the step that
        starts here runs with deferred side-stream joins: the gradient arena is only complete after step() (or
        ops.side_join()), not right after loss.backward()."""
        dp.reset_buckets(self.model.grad)            # nothing may survive from a step that never reached step()
        self.model.__dict__.pop("_dp_open", None)    # (nor counts of forward passes that never saw their backward)
        ops.side_defer(bool(self.overlap_backward))
        self.model.zero_grad()

    def step(self):
        """utils/trainer.py:172-177 (+ the data-parallel gradient exchange).  May raise ops.ChainTimeoutError / ValueError
        for an EARLIER step (see check_steps)."""
        if self._ema_swapped is not None:
            raise RuntimeError("step() inside ema_weights(): model.flat holds the EMA weights, not the trained ones")
        self._join_side_work()
        m = self.model
        flag = self._flag()
        if flag is not None:
            self._export_flag(flag)                  # this rank's chain status -> the word in front of the arena ...
        gscale = dp.allreduce_grads(m.grad, store=m._grad_store, head=m._HEAD)     # ... summed with the gradients
        ops.release_held()                           # (after the exchange: the buckets' streams were ordered behind side work)
        self.adam_t += 1
        tag = self._tag
        self._tag += 1
        if self._reports_on():
            if len(self._inflight) >= self._NREP - 1:     # (only if check_steps() was overridden away: never reuse an unread record)
                self.check_steps(wait_all=True)
            self._launch_optimizer(tag, gscale, flag)
            self._inflight.append(tag)
            self.check_steps()
        else:                                        # (no reports: host arenas never get here, a device trainer always reports)
            ops.adamw_step(m.flat, m.grad, self.adam_m, self.adam_v, self.lr, self.adam_t, **self._adamw_args(gscale))

    # ---- decoupled weight decay and the EMA shadow weights ----
    def _build_decay_mask(self):
        """The elements that decay by default: the weight matrices, by the criterion Model.init_reference_style uses."""
        ranges = [(off, off + shape[0] * shape[1]) for name, off, shape in self.model._table if "weight" in name and len(shape) == 2]
        return ops.pack_decay_mask(self.model.flat.numel(), ranges, device=self.model.flat.device)

    def ema_decay_at(self, t):
        """The EMA decay of the launch whose bias-correction step number is t: ema_decay, behind min(., (1 + t) / (10 + t)) with
        ema_warmup.  t is adam_t as the host knows it at the launch: after a dropped step it runs one too high for up to report_lag
        launches, exactly as the bias correction does (check_steps)."""
        if self.ema_warmup:
            return min(self.ema_decay, (1.0 + t) / (10.0 + t))
        return self.ema_decay

    def _adamw_args(self, gscale, step_flag=None, report=None):
        """What ops.adamw_step takes beyond the arenas, lr and the step number: the one optimizer launch of the trainer, whatever is
        switched on.  The partials only with max_grad_norm and a report, which is where grad_sqnorm ran in front (_launch_optimizer;
        the report-less branch of step() does not measure)."""
        on = report is not None and self.max_grad_norm is not None
        return dict(weight_decay=self.weight_decay, decay_mask=self._decay_mask, ema=self.ema,
                    ema_decay=0.0 if self.ema is None else self.ema_decay_at(self.adam_t),
                    max_norm=self.max_grad_norm if on else None, partials=self._sqnorm if on else None,
                    b1=self.betas[0], b2=self.betas[1], eps=self.eps, gscale=gscale, step_flag=step_flag, report=report)

    def ema_state_dict(self):
        """The EMA weights under the keys and shapes of model.state_dict(): load them into a model to evaluate or sample from it."""
        if self.ema is None:
            raise RuntimeError("this trainer keeps no EMA (ema_decay=None)")
        out = OrderedDict()
        for name, off, shape in self.model._table:
            out[name] = self.ema[off:off + math.prod(shape)].view(shape).detach().clone()
        return out

    @contextlib.contextmanager
    def ema_weights(self):
        """Inside the context model.flat holds the EMA weights: the model's own are copied aside and the EMA copied over them on the
        current stream, behind everything queued; they come back on exit, also on an exception.  The parameter views alias
        model.flat and nothing in the library keeps values derived from the weights across calls, so every forward pass inside sees
        the EMA.  step() inside raises RuntimeError."""
        if self.ema is None:
            raise RuntimeError("this trainer keeps no EMA (ema_decay=None)")
        if self._ema_swapped is not None:
            raise RuntimeError("ema_weights() is not re-entrant")
        self._ema_swapped = self.model.flat.clone()
        self.model.flat.copy_(self.ema)
        try:
            yield self.model
        finally:
            self.model.flat.copy_(self._ema_swapped)
            self._ema_swapped = None

    # ---- the device-touching pieces of the protocol, one method each: tests/test_dp_gloo.py drives step(), check_steps() and the
    # ---- fallback / replay logic with host stand-ins for them (world 2, gloo)
    def _reports_on(self):
        return self.model.grad.is_cuda

    def _join_side_work(self):
        ops.side_defer(False, release=False)         # joins; deferred mode only lives between zero_grad() and step()

    def _export_flag(self, flag):
        ops.step_flag_export(flag)

    def _launch_optimizer(self, tag, gscale, flag):
        m = self.model
        rec = self._report_slot(tag)
        rec.zero_()                                  # host write: the launch that last wrote this record was waited for when it was read
        if self.max_grad_norm is not None:
            # m.grad is the arena alone (the 16-byte head of its store holds the ranks' flags, not gradients); both launches sit
            # behind the gradient exchange, so every rank measures the same all-reduced arena in the same fixed order and all
            # ranks clip and drop together: no collective of their own
            self._sqnorm = ops.grad_sqnorm(m.grad, self._sqnorm)
        # decay and EMA are element-wise functions of values that are bit-identical on every rank behind the exchange: the
        # replicas and their EMA arenas stay bit-identical with nothing to coordinate
        ops.adamw_step(m.flat, m.grad, self.adam_m, self.adam_v, self.lr, self.adam_t, **self._adamw_args(gscale, flag, rec))
        self._report_events[tag % self._NREP].record()

    def _device_sync(self):
        torch.cuda.synchronize()

    def _chains_off(self):
        """Clear the status words and switch this process to the per-step kernels; returns this rank's timed-out workgroups."""
        n = ops.chain_status(reset=True)
        ops.set_option(4, 0)                          # per-step kernels from here on (INET_CHAIN=0 semantics, in-process)
        return n

    _NREP = 16

    def _report_slot(self, tag):
        if self._reports is None:
            # eight words per record, whatever is switched on now or by a later load_training_state (inet_adam_step_w)
            self._reports = torch.zeros(self._NREP, 8, dtype=torch.int32).pin_memory()
            self._report_events = [torch.cuda.Event() for _ in range(self._NREP)]
        return self._reports[tag % self._NREP]

    def _read_report(self, tag):
        """(executed, skipped, nonfinite, bad token) of the optimizer launch issued under `tag`, after the event behind it; with
        max_grad_norm set also (clipped, dropped for a non-finite gradient, the gradient norm)."""
        self._report_events[tag % self._NREP].synchronize()
        r = self._reports[tag % self._NREP].tolist()
        if not r[0]:
            raise RuntimeError(f"optimizer launch {tag} left no report (the kernel did not run?)")
        rep = bool(r[0]), bool(r[1]), bool(r[2]), bool(r[3])
        if self.max_grad_norm is not None:           # (an eight-word record of inet_adam_step_w without partials carries no norm)
            rep += (bool(r[4]), bool(r[5]), struct.unpack("<f", struct.pack("<i", r[6]))[0])
        return rep

    def _note_clip(self, tag, rep):
        """The clipping part of a step report (absent without max_grad_norm).  A step dropped for a non-finite gradient changed
        nothing: its count comes back out of the bias-correction step number, as _fall_back_from_chains does for lost steps.  Nothing
        is raised and nothing is run again -- the batch is gone, as under torch's GradScaler."""
        if len(rep) <= 4 or rep[1]:                  # (a step the chain flag skipped reports no norm decision)
            return
        self.last_grad_norm = rep[6]
        self.clipped_steps += int(rep[4])
        if rep[5]:
            self.nonfinite_steps += 1
            self.adam_t = max(self.adam_t - 1, 0)
            print(f"[inpaintnet_amd] rank {dp.rank()}: optimizer step {tag} was dropped on every rank: its gradient held an inf "
                  f"or a NaN (norm {rep[6]}); weights and moments were left alone")

    def check_steps(self, wait_all=False):
        """Read the reports of the optimizer steps issued at least `report_lag` steps ago (all outstanding ones with
        wait_all).  Raises ops.ChainTimeoutError if one of them skipped itself -- a persistent kernel of SOME rank had timed out,
        see _run_batch --, ValueError if a parameter became NaN / inf in one of them (the reference's "... has become nan",
        MeasureVAE/encoder.py:111-116, decoder.py:424-429), ops.TokenRangeError for a token outside the vocabulary
        (decoder.py:36-45).  Identical on every rank of a data-parallel job: same reports, read at the same step.

        With max_grad_norm set a report also carries the gradient norm and what the kernel did about it: last_grad_norm,
        clipped_steps and nonfinite_steps follow the reports read here.  A step dropped for an inf / NaN gradient raises nothing: one
        line is printed and adam_t goes down by one.  The host learns of it `report_lag` steps late, so the up to `report_lag` steps
        queued in between ran with a bias-correction step number one too high; from the next launch on it is right again.  The
        warm-up of the EMA decay (ema_warmup, ema_decay_at) is evaluated at the same step number and lags in the same way."""
        newest = self._tag - 1
        skipped = nonfinite = badtok = False
        while self._inflight and (wait_all or self._inflight[0] <= newest - self.report_lag):
            tag = self._inflight.popleft()
            rep = self._read_report(tag)
            skip, bad, tok = rep[1], rep[2], (rep[3] if len(rep) > 3 else False)
            self._note_clip(tag, rep)
            if skip:
                self._lost.append(tag)
            skipped |= skip
            nonfinite |= bad
            badtok |= tok
        if skipped:
            raise ops.ChainTimeoutError(
                f"optimizer step(s) {self._lost} skipped: a chain kernel gave up waiting for its group (on this or another "
                "rank), the gradients of those steps are not valid and the weights were left alone.  All workgroups of such a "
                "launch must be resident at once -- is the GPU shared, partitioned or CU-masked?  INET_CHAIN=0 (or "
                f"ops.set_option(4, 0)) selects the per-step kernels.  Recorder: {ops.slow_waits_summary()}")
        if nonfinite:
            raise ValueError(f"{type(self.model).__name__} has become nan (a parameter left the finite range in an optimizer step)")
        if badtok:
            # data parallel: SOME rank's prologue kernels met a token outside the vocabulary (the token words travel with the
            # step flag and come back in the report): every rank raises here, at the same step -- nobody is left in a collective
            if self.model.flat.is_cuda:
                ops.token_status(reset=True)
            raise ops.TokenRangeError("Invalid Value of index: a token outside [0, num_notes) reached the model on this or another "
                                      "rank (Trainer.step); the results computed from it are not valid")
        if self.model.flat.is_cuda and self._flag() is None:
            ops.check_tokens("Trainer.step")         # single process: the host-mapped counter of this process

    def finish(self):
        """Read every outstanding step report NOW (waits for the optimizer launches still in flight) and raise what they hold.
        The errors of a step surface up to `report_lag` steps late by design (the host must run ahead of the GPU); a manual
        training loop -- zero_grad / loss / backward / step without loss_and_acc_on_epoch -- calls this after its last step,
        or runs inside `with trainer:`, so that a NaN weight, a bad token or a chain timeout in the LAST steps is not lost.
        The epoch loop and train_model do it themselves."""
        self.check_steps(wait_all=True)

    close = finish

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None:
            self.finish()
        else:                                        # do not mask the exception that is already on its way out
            try:
                self.finish()
            except Exception:
                pass
        return False

    def _fall_back_from_chains(self):
        """After a ChainTimeoutError out of step() / check_steps(): wait for the device, find every skipped step, take their
        count back out of the bias-correction step number, clear the status words, switch this process to the per-step
        kernels.  Returns the tags of the lost steps, oldest first (every rank computes the same list)."""
        self._device_sync()
        while self._inflight:
            tag = self._inflight.popleft()
            rep = self._read_report(tag)
            self._note_clip(tag, rep)
            if rep[1]:
                self._lost.append(tag)
        lost, self._lost = sorted(set(self._lost)), []
        n = self._chains_off()
        self.chain_fallbacks += 1
        self.lost_steps += len(lost)
        self.adam_t = max(self.adam_t - len(lost), 0)  # those launches did not update anything
        print(f"[inpaintnet_amd] rank {dp.rank()}: {max(n, 0)} chain-kernel workgroups of this rank timed out; optimizer steps "
              f"{lost} were skipped on every rank; chain kernels are now OFF for this process and those batches are run again "
              "(is the GPU shared, partitioned or CU-masked?)")
        return lost

    # ---- optimizer / epoch resume (SURVEY 8f1 add-on: the reference saves weights only, utils/model.py:16-53) ----
    def training_state(self, next_epoch=0):
        return {"adam_m": self.adam_m.cpu(), "adam_v": self.adam_v.cpu(), "adam_t": self.adam_t, "lr": self.lr,
                "betas": self.betas, "eps": self.eps, "next_epoch": int(next_epoch),
                "num_parameters": int(self.model.flat.numel()),
                "weight_decay": self.weight_decay, "decay_all": self.decay_all, "ema_decay": self.ema_decay,
                "ema_warmup": self.ema_warmup, "ema": None if self.ema is None else self.ema.cpu(),
                "ce_weight": None if self.ce_weight is None else self.ce_weight.clone(), "label_smoothing": self.label_smoothing,
                "ignore_index": self.ignore_index}

    def save_training_state(self, path, next_epoch=0):
        torch.save(self.training_state(next_epoch), path)

    def load_training_state(self, path_or_state):
        """Restore the Adam moments, step count and the epoch to resume from (train_model starts there)."""
        st = torch.load(path_or_state, map_location="cpu") if isinstance(path_or_state, (str, bytes, os.PathLike)) \
            else path_or_state
        if int(st["num_parameters"]) != self.model.flat.numel():
            raise RuntimeError("training state belongs to a model with a different parameter arena")
        if self._inflight:
            # before adam_t is overwritten: a report read afterwards would take ITS dropped step off the loaded step count
            # (waits for those launches and raises what they report)
            self.check_steps(wait_all=True)
        self.adam_m.copy_(st["adam_m"])
        self.adam_v.copy_(st["adam_v"])
        self.adam_t = int(st["adam_t"])
        self.lr, self.betas, self.eps = float(st["lr"]), tuple(st["betas"]), float(st["eps"])
        self.start_epoch = int(st["next_epoch"])
        if "weight_decay" in st:
            self.weight_decay, self.decay_all = float(st["weight_decay"]), bool(st["decay_all"])
            self.ema_decay, self.ema_warmup = st["ema_decay"], bool(st["ema_warmup"])
            masked = self.weight_decay > 0.0 and not self.decay_all
            self._decay_mask = (self._decay_mask if self._decay_mask is not None else self._build_decay_mask()) if masked else None
            if self.ema_decay is None:
                self.ema = None
            elif st["ema"] is not None:
                self.ema = self.model.flat.clone() if self.ema is None else self.ema
                self.ema.copy_(st["ema"])
        elif self.ema is not None:
            # a state written before weight decay and EMA existed: the settings stay this trainer's, the EMA starts at the weights
            self.ema.copy_(self.model.flat)
            print("[inpaintnet_amd] training state without an EMA: the EMA arena was seeded from the model's weights as loaded")
        if "label_smoothing" in st:                  # (a state written before the three settings existed leaves the trainer's own)
            self.ce_weight, self.label_smoothing, self.ignore_index = self._ce_settings(
                st["ce_weight"], st["label_smoothing"], st["ignore_index"], self._num_classes(self.dataset))
            self._ce_weight_dev = None
        return self.start_epoch

    @abstractmethod
    def loss_and_acc_for_batch(self, batch, epoch_num=None, train=True):
        pass

    @abstractmethod
    def process_batch_data(self, batch):
        pass

    @abstractmethod
    def update_scheduler(self, epoch_num):
        pass

    @staticmethod
    def print_epoch_stats(epoch_index, num_epochs, mean_loss_train, mean_accuracy_train, mean_loss_val,
                          mean_accuracy_val):
        print(f'Train Epoch: {epoch_index + 1}/{num_epochs}')
        print(f'\tTrain Loss: {mean_loss_train}\tTrain Accuracy: {mean_accuracy_train * 100} %')
        print(f'\tValid Loss: {mean_loss_val}\tValid Accuracy: {mean_accuracy_val * 100} %')

    # ---- static losses, utils/trainer.py:271-376 -------------------------------------
    @staticmethod
    def mean_crossentropy_loss_and_accuracy(weights, targets, weight=None, label_smoothing=0.0, ignore_index=None):
        """With two arguments the plain mean cross-entropy and token accuracy (utils/trainer.py:271-306).  weight (V class weights),
        label_smoothing (in [0, 1]) and ignore_index (None: nothing is ignored) are torch.nn.CrossEntropyLoss's; any non-default
        one takes the weighted kernel, whose accuracy is over the valid rows."""
        if weight is None and label_smoothing == 0.0 and ignore_index is None:
            V = weights.size(-1)
            w2 = weights.contiguous().view(-1, V)
            t1 = targets.contiguous().view(-1)
            if t1.dtype != torch.int64:
                t1 = t1.long()
            return _CrossEntropyFn.apply(w2, t1)
        return _ce_w_apply(weights, targets, weight, label_smoothing, ignore_index, None)

    @staticmethod
    def mean_crossentropy_loss(weights, targets):
        """weights (B,T,V), targets (B,T)   (utils/trainer.py:271-288)"""
        batch_size, seq_len, num_notes = weights.size()
        assert batch_size == targets.size(0)
        assert seq_len == targets.size(1)
        return Trainer.mean_crossentropy_loss_and_accuracy(weights, targets)[0]

    @staticmethod
    def mean_accuracy(weights, targets):
        """utils/trainer.py:290-306 (argmax = lowest index among maxima, as Tensor.max(1))"""
        with torch.no_grad():
            return Trainer.mean_crossentropy_loss_and_accuracy(weights.detach(), targets)[1]

    @staticmethod
    def mean_crossentropy_loss_alt(weights, targets):
        """weights (B,M,T,V), targets (B,M,T)   (utils/trainer.py:344-359)"""
        return Trainer.mean_crossentropy_loss_and_accuracy(weights, targets)[0]

    @staticmethod
    def mean_accuracy_alt(weights, targets):
        """utils/trainer.py:361-376"""
        with torch.no_grad():
            return Trainer.mean_crossentropy_loss_and_accuracy(weights.detach(), targets)[1]

    @staticmethod
    def mean_mse_loss_rnn(weights, targets):
        """utils/trainer.py:327-342 (diagnostic only: never part of a training loss in the reference)"""
        assert weights.size() == targets.size()
        return ((weights - targets) ** 2).mean()

    @staticmethod
    def mean_l1_loss_rnn(weights, targets):
        """utils/trainer.py:308-325"""
        assert weights.size() == targets.size()
        return (weights - targets).abs().mean()


class EarlyStopping:
    """Patience counter on the validation loss (behaviour of utils/trainer.py:379-413): an epoch counts as an
    improvement only if the loss drops by at least `min_delta` below the best seen; `patience` epochs in a row without
    one set `early_stop`.  Calling the object returns the flag."""

    def __init__(self, patience=5, verbose=False, min_delta=1e-5):
        self.patience = patience
        self.verbose = verbose
        self.min_delta = min_delta
        self.counter = 0
        self.best_score = None
        self.early_stop = False
        self.val_loss_min = float("inf")

    def __call__(self, val_loss, model=None):
        score = -float(val_loss)
        if self.best_score is None or score - self.best_score >= self.min_delta:
            if self.best_score is not None:
                self.counter = 0
                self.val_loss_min = float(val_loss)
            self.best_score = score
        else:
            self.counter += 1
            self.early_stop = self.early_stop or self.counter >= self.patience
        return self.early_stop
