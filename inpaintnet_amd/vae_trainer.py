"""VAETrainer: MeasureVAE/vae_trainer.py:10-139 of the reference on the HIP kernels."""
import math
import os

import torch

from . import ops
from .helpers import to_cuda_variable_long
from .attributes import ATTRIBUTES, AttributeSpec
from .measure_vae import _AttrRegFn, _MmdFn, _attr_columns
from .trainer import Trainer, _ElboFn, _ElboWFn, _KLFn


class VAETrainer(Trainer):
    feed_fields = (0,)                     # the metadata tensor is never read (vae_trainer.py:42-55)

    KL_SETTINGS = ("kl_beta", "kl_warmup_steps", "kl_cycle_steps", "kl_ramp", "free_nats", "free_nats_per")
    MMD_SETTINGS = ("mmd_coeff", "mmd_kernel", "mmd_bandwidth", "mmd_estimator")
    ATTR_SETTINGS = ("attr_reg", "attr_gamma", "attr_delta", "attr_spec")

    def __init__(self, dataset, model, lr=1e-4, max_grad_norm=None, weight_decay=0.0, decay_all=False, ema_decay=None,
                 ema_warmup=False, kl_beta=0.001, kl_warmup_steps=0, kl_cycle_steps=0, kl_ramp=0.5, free_nats=0.0,
                 free_nats_per='measure', mmd_coeff=0.0, mmd_kernel='gaussian', mmd_bandwidth=None, mmd_estimator='unbiased',
                 ce_weight=None, label_smoothing=0.0, ignore_index=None, attr_reg=None, attr_gamma=10.0, attr_delta=10.0,
                 attr_spec=None):
        """The loss of a training step is CE + beta_t / B * kl_sum [+ mmd_coeff * MMD(z_tilde, z_prior)]
        [+ attr_gamma * sum_a L_a(z_tilde, attributes of the step's tokens)].  ce_weight, label_smoothing, ignore_index: Trainer's
        (CE becomes the class-weighted, label-smoothed cross-entropy of DESIGN.md section 28, still one launch each way next to
        the counting launch).

        kl_beta (finite, >= 0): the KL weight; the reference's 0.001.  kl_warmup_steps (an int >= 0): beta rises linearly from 0 to
        kl_beta over that many optimizer steps, then holds.  kl_cycle_steps = M > 0: cyclical annealing (Fu et al. 2019) -- within
        every period of M steps beta rises linearly over the first kl_ramp * M steps (0 < kl_ramp <= 1), then holds at kl_beta.
        Warm-up and cycle exclude each other.  beta_at(t) is evaluated on the host, per step, at adam_t as the host knows it when the
        loss is built: the first step sees t = 0, and after a dropped step t runs one too high for up to report_lag steps -- the
        convention and the lag of ema_decay_at.  Validation (train=False) always uses kl_beta.

        free_nats (finite, >= 0) with free_nats_per 'measure' or 'dim': the KL floor ("free bits").  'measure': every measure's KL,
        summed over the latent dimensions, counts with max(KL_b, free_nats) -- MusicVAE's hinge plus the constant.  'dim' (Kingma
        et al. 2016): every latent dimension's KL, summed over the batch, counts with max(KL_d, B * free_nats), i.e. its batch mean
        is floored at free_nats.  The batch is the one this process sees: under data parallelism the rank's own shard, as batch
        statistics would be; there is no collective for it.  A floored part passes no KL gradient; a part equal to its floor is
        floored; a NaN part is kept, so that a NaN reaches loss and gradient as on the plain path.  free_nats > 0 sets
        model.free_bits, which MeasureVAE.forward applies to training passes only; after such a step `last_kl` holds the device
        tensors {'raw': (), 'floored': (), 'parts': (B,) or (Z,), 'keep': the same shape, 1.0 = kept} -- reading them is the
        caller's synchronisation.  With the defaults the trainer launches what it launched before and last_kl stays None.

        mmd_coeff (finite, >= 0) > 0 adds the InfoVAE / WAE-MMD term: mmd_coeff times the MMD between the
        step's z_tilde and its prior draws z_prior, with mmd_kernel 'gaussian' (exp(-d / bandwidth)) or 'imq' (bandwidth / (bandwidth
        + d)) on the squared distance d, mmd_bandwidth (finite, > 0; None: 2 * z_dim, the expected squared distance of two prior
        draws) and mmd_estimator 'unbiased' (the U-statistic: needs a batch of 2 or more), 'biased' (the V-statistic) or 'reference'
        (the reference's compute_mmd_loss as written, which is negative for two samples of one distribution).  The term matches the
        aggregate posterior to the prior; it is independent of the KL settings and combines with them.  It is part of the objective,
        so validation (train=False) adds its value too, without the gradient phase.  Under data parallelism it is the MMD of the
        rank's own shard, as for free_nats_per='dim': no collective.  After a step `last_mmd` holds the device tensors {'value' (the
        term as added), 'S_xx', 'S_yy', 'S_xy' (the kernel sums, diagonals included)}.  With mmd_coeff == 0 nothing is launched
        and last_mmd stays None.

        attr_reg, a mapping from attribute name (attributes.ATTRIBUTES) to latent dimension such as {'num_notes': 0, 'note_range': 1},
        adds the attribute regularisation of AR-VAE (Pati & Lerch 2020): for every entry attr_gamma (finite,
        >= 0) times mean_ij |tanh(attr_delta (z_i - z_j)) - sgn(a_i - a_j)| over the batch's pairs, z the named dimension of the
        step's z_tilde and a the attribute of the step's own tokens (ops.measure_attributes with attr_spec, an AttributeSpec; None:
        AttributeSpec.from_dataset(dataset)).  After training, moving along that dimension moves the attribute.  The dimensions must
        be distinct ints inside z_dim, at most 8; attr_delta finite and > 0.  The term is added after the MMD term and combines with
        it and with the KL settings; a training pass takes its gradient, validation the value alone; under data parallelism it is
        computed on the rank's own shard.  After a step `last_attr_reg` holds the device tensors {'value' (the term as added),
        'per_attr' (A,), 'counts' (A, 3) int64: concordant, discordant, attribute-tied ordered pairs, 'attrs' (B, A)}, in the order
        of attr_reg's entries.  With attr_reg=None nothing is launched and last_attr_reg stays None."""
        kl_beta, kl_ramp, free_nats = float(kl_beta), float(kl_ramp), float(free_nats)
        if not (kl_beta >= 0.0 and math.isfinite(kl_beta)):                     # (NaN fails the comparison)
            raise ValueError(f"kl_beta must be finite and >= 0, got {kl_beta}")
        for name, v in (("kl_warmup_steps", kl_warmup_steps), ("kl_cycle_steps", kl_cycle_steps)):
            if isinstance(v, bool) or not isinstance(v, int) or v < 0:
                raise ValueError(f"{name} must be an integer >= 0, got {v!r}")
        if kl_warmup_steps > 0 and kl_cycle_steps > 0:
            raise ValueError("kl_warmup_steps and kl_cycle_steps exclude each other")
        if not 0.0 < kl_ramp <= 1.0:
            raise ValueError(f"kl_ramp must lie in (0, 1], got {kl_ramp}")
        if not (free_nats >= 0.0 and math.isfinite(free_nats)):
            raise ValueError(f"free_nats must be finite and >= 0, got {free_nats}")
        if free_nats_per not in ('measure', 'dim'):
            raise ValueError(f"free_nats_per must be 'measure' or 'dim', got {free_nats_per!r}")
        mmd_coeff = float(mmd_coeff)
        if not (mmd_coeff >= 0.0 and math.isfinite(mmd_coeff)):
            raise ValueError(f"mmd_coeff must be finite and >= 0, got {mmd_coeff}")
        if not isinstance(mmd_kernel, str) or mmd_kernel not in ops.MMD_KERNEL:
            raise ValueError(f"mmd_kernel must be 'gaussian' or 'imq', got {mmd_kernel!r}")
        if mmd_bandwidth is not None:
            if isinstance(mmd_bandwidth, bool) or not isinstance(mmd_bandwidth, (int, float)) or \
                    not (mmd_bandwidth > 0.0 and math.isfinite(mmd_bandwidth)):
                raise ValueError(f"mmd_bandwidth must be None or finite and > 0, got {mmd_bandwidth!r}")
            mmd_bandwidth = float(mmd_bandwidth)
        if not isinstance(mmd_estimator, str) or mmd_estimator not in ops.MMD_ESTIMATORS:
            raise ValueError(f"mmd_estimator must be one of {ops.MMD_ESTIMATORS}, got {mmd_estimator!r}")
        attr_reg, attr_gamma, attr_delta, attr_spec = self._attr_settings(attr_reg, attr_gamma, attr_delta, attr_spec)
        super().__init__(dataset, model, lr, max_grad_norm=max_grad_norm, weight_decay=weight_decay, decay_all=decay_all,
                         ema_decay=ema_decay, ema_warmup=ema_warmup, ce_weight=ce_weight, label_smoothing=label_smoothing,
                         ignore_index=ignore_index)
        self.kl_beta, self.kl_warmup_steps, self.kl_cycle_steps, self.kl_ramp = kl_beta, kl_warmup_steps, kl_cycle_steps, kl_ramp
        self.free_nats, self.free_nats_per = free_nats, free_nats_per
        self.last_kl = None
        self.mmd_coeff, self.mmd_kernel, self.mmd_bandwidth, self.mmd_estimator = mmd_coeff, mmd_kernel, mmd_bandwidth, mmd_estimator
        self.last_mmd = None
        self.attr_reg, self.attr_gamma, self.attr_delta, self.attr_spec = attr_reg, attr_gamma, attr_delta, attr_spec
        self.last_attr_reg = None
        if attr_reg is not None:
            z_dim = model.latent_space_dim
            if max(attr_reg.values()) >= z_dim:
                raise ValueError(f"attr_reg: every latent dimension must lie inside z_dim = {z_dim}, got {attr_reg}")
            if attr_spec is None:
                self.attr_spec = AttributeSpec.from_dataset(dataset)
        if free_nats > 0.0:
            model.free_bits = (free_nats, free_nats_per)

    @staticmethod
    def _attr_settings(attr_reg, attr_gamma, attr_delta, attr_spec):
        """The four attribute settings checked and in their stored form (attr_reg: a dict in the caller's order, or None)."""
        if attr_reg is not None:
            if not hasattr(attr_reg, "items") or len(attr_reg) == 0:
                raise ValueError(f"attr_reg must be None or a non-empty mapping from attribute name to latent dimension, got {attr_reg!r}")
            attr_reg = dict(attr_reg.items())
            for name, d in attr_reg.items():
                if name not in ATTRIBUTES:
                    raise ValueError(f"attr_reg: attribute names must come from {ATTRIBUTES}, got {name!r}")
                if isinstance(d, bool) or not isinstance(d, int) or d < 0:
                    raise ValueError(f"attr_reg: the latent dimension of {name!r} must be an int >= 0, got {d!r}")
            if len(set(attr_reg.values())) != len(attr_reg):
                raise ValueError(f"attr_reg: the latent dimensions must be distinct, got {attr_reg}")
        for name, v, strict in (("attr_gamma", attr_gamma, False), ("attr_delta", attr_delta, True)):
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v < 0.0 or (strict and v == 0.0):
                raise ValueError(f"{name} must be finite and {'> 0' if strict else '>= 0'}, got {v!r}")
        if attr_spec is not None and not isinstance(attr_spec, AttributeSpec):
            raise ValueError(f"attr_spec must be None or an AttributeSpec, got {type(attr_spec).__name__}")
        return attr_reg, float(attr_gamma), float(attr_delta), attr_spec

    def beta_at(self, t):
        """The KL weight of the step whose loss is built while adam_t == t (a pure function of the settings)."""
        if self.kl_cycle_steps > 0:
            return self.kl_beta * min(1.0, (t % self.kl_cycle_steps) / (self.kl_ramp * self.kl_cycle_steps))
        if self.kl_warmup_steps > 0:
            return self.kl_beta * min(1.0, t / self.kl_warmup_steps)
        return self.kl_beta

    def loss_and_acc_for_batch(self, batch, epoch_num=None, train=True):
        """loss = CE_mean + beta * mean_b KL ; accuracy   (vae_trainer.py:16-40; beta = 1e-3 there)"""
        score = batch
        weights, samples, z_dist, prior_dist, z_tilde, z_prior = self.model(measure_score_tensor=score, train=train)
        beta = self.beta_at(self.adam_t) if train else self.kl_beta
        if train:
            parts = getattr(z_dist, "kl_parts", None)
            self.last_kl = None if parts is None else {"raw": z_dist.kl_raw.detach(), "floored": z_dist.kl_sum.detach(),
                                                       "parts": parts, "keep": z_dist.kl_keep}
        kl_sum = getattr(z_dist, "kl_sum", None)
        if kl_sum is not None and type(self).compute_kld_loss is VAETrainer.compute_kld_loss and \
                type(self).mean_crossentropy_loss_and_accuracy is Trainer.mean_crossentropy_loss_and_accuracy:
            # the same three lines (vae_trainer.py:29-40: recons + 1e-3 * mean KL, accuracy) as one kernel each way
            V = weights.size(-1)
            t1 = score.contiguous().view(-1)
            if t1.dtype != torch.int64:
                t1 = t1.long()
            if self._ce_plain():
                self.last_ce = None
                loss, accuracy = _ElboFn.apply(weights.contiguous().view(-1, V), t1, kl_sum, beta / z_dist.loc.shape[0],
                                               self.model.take_stats(2))
            else:
                self.last_ce = {}
                loss, accuracy = _ElboWFn.apply(weights.contiguous().view(-1, V), t1, kl_sum, beta / z_dist.loc.shape[0],
                                                *self._ce_args(weights.device), self.last_ce)
            return self._add_attr_reg(self._add_mmd(loss, z_tilde, z_prior, train), z_tilde, score, train), accuracy
        recons_loss, accuracy = self._ce_loss(weights, score)
        # (an override written against the reference's two-argument call keeps working while beta is the reference's)
        dist_loss = self.compute_kld_loss(z_dist, prior_dist, **({} if beta == 0.001 else {"beta": beta}))
        loss = recons_loss + dist_loss
        return self._add_attr_reg(self._add_mmd(loss, z_tilde, z_prior, train), z_tilde, score, train), accuracy

    def _add_mmd(self, loss, z_tilde, z_prior, train):
        """loss + mmd_coeff * MMD(z_tilde, z_prior); a training pass takes the gradient phase along, validation the value alone."""
        if not self.mmd_coeff > 0.0:
            return loss
        args = (self.mmd_kernel, self.mmd_bandwidth, self.mmd_estimator, self.mmd_coeff)
        if train and torch.is_grad_enabled() and z_tilde.requires_grad:
            value, sxx, syy, sxy = _MmdFn.apply(z_tilde, z_prior, *args)
        else:
            value, sxx, syy, sxy = ops.mmd(z_tilde.detach().contiguous(), z_prior.detach().contiguous(), *args)[0].unbind(0)
        self.last_mmd = {"value": value.detach(), "S_xx": sxx, "S_yy": syy, "S_xy": sxy}
        return loss + value

    def _add_attr_reg(self, loss, z_tilde, score, train):
        """loss + attr_gamma * sum_a L_a; a training pass takes the gradient phase along, validation the value alone."""
        if self.attr_reg is None:
            return loss
        tokens = score.contiguous()
        if tokens.dtype != torch.int64:
            tokens = tokens.long()
        cols = [ATTRIBUTES.index(name) for name in self.attr_reg]
        attrs = ops.measure_attributes(tokens, self.attr_spec)
        if cols != list(range(len(ATTRIBUTES))):
            attrs = attrs.index_select(1, _attr_columns(tuple(cols), attrs.device))
        dims = list(self.attr_reg.values())
        if train and torch.is_grad_enabled() and z_tilde.requires_grad:
            value, per_attr, counts = _AttrRegFn.apply(z_tilde, dims, attrs, self.attr_delta, self.attr_gamma)
        else:
            out, counts, _ = ops.attr_reg(z_tilde.detach().contiguous(), dims, attrs, self.attr_delta, self.attr_gamma)
            value, per_attr = out[0], out[1:]
        self.last_attr_reg = {"value": value.detach(), "per_attr": per_attr, "counts": counts, "attrs": attrs}
        return loss + value

    def process_batch_data(self, batch):
        """(B,1,384) int32 -> (B*16, 24) int64 on the device   (vae_trainer.py:42-55)"""
        score_tensor = batch[0]
        n_bars = getattr(self.dataset, "n_bars", None)
        if n_bars is not None and score_tensor.dim() == 3:
            batch_size = score_tensor.size(0)
            score_tensor = score_tensor.reshape(batch_size, n_bars, -1)
            score_tensor = score_tensor.reshape(batch_size * n_bars, -1)
        return to_cuda_variable_long(score_tensor)

    def update_scheduler(self, epoch_num):
        return

    def training_state(self, next_epoch=0):
        st = super().training_state(next_epoch)
        st.update({k: getattr(self, k) for k in self.KL_SETTINGS + self.MMD_SETTINGS})
        st.update(attr_reg=None if self.attr_reg is None else dict(self.attr_reg), attr_gamma=self.attr_gamma,
                  attr_delta=self.attr_delta, attr_spec=None if self.attr_spec is None else self.attr_spec.state())
        return st

    def load_training_state(self, path_or_state):
        """... and the six KL, four MMD and four attribute settings (the three of the reconstruction loss are the base class's); a
        state written before they existed leaves this trainer's own."""
        st = torch.load(path_or_state, map_location="cpu") if isinstance(path_or_state, (str, bytes, os.PathLike)) \
            else path_or_state
        out = super().load_training_state(st)
        if "kl_beta" in st:
            for k in self.KL_SETTINGS:
                setattr(self, k, st[k])
            self.model.free_bits = (self.free_nats, self.free_nats_per) if self.free_nats > 0.0 else None
        if "mmd_coeff" in st:
            for k in self.MMD_SETTINGS:
                setattr(self, k, st[k])
        if "attr_reg" in st:
            spec = st["attr_spec"]
            self.attr_reg, self.attr_gamma, self.attr_delta, self.attr_spec = self._attr_settings(
                st["attr_reg"], st["attr_gamma"], st["attr_delta"], None if spec is None else AttributeSpec(**spec))
        return out

    @staticmethod
    def compute_mmd_loss(z_tilde, z_prior, coeff=10, kernel='gaussian', bandwidth=16.0, estimator='reference'):
        """vae_trainer.py:93-126 on the MMD kernels: with the defaults the reference's rule as written -- the
        Gaussian kernel exp(-d / 16), 1 / (B (B - 1)) / 2 on both self terms with their diagonals in, 2 / B^2 on the cross term --
        which is negative for two samples of one distribution and whose bandwidth leaves no gradient at z_dim 256; kernel, bandwidth
        and estimator select the textbook forms (ops.mmd).  z_tilde takes a gradient where it requires one, z_prior is a constant.
        The reference's helper compute_kernel, which materialises the B x B x Z differences, is not offered."""
        args = (kernel, bandwidth, estimator, float(coeff))
        if torch.is_grad_enabled() and z_tilde.requires_grad:
            return _MmdFn.apply(z_tilde, z_prior, *args)[0]
        return ops.mmd(z_tilde.detach().contiguous(), z_prior.detach().contiguous(), *args)[0][0]

    @staticmethod
    def compute_kld_loss(z_dist, prior_dist, beta=0.001):
        """vae_trainer.py:128-139; prior must be N(0,1) as built at measure_vae.py:122-125."""
        log_scale = getattr(z_dist, "log_scale", None)
        if log_scale is None:
            raise ValueError("compute_kld_loss expects the encoder's distribution (it carries log_scale)")
        kl_sum = getattr(z_dist, "kl_sum", None)
        if kl_sum is not None:
            # rsample() already summed the KL terms in the reparameterisation kernel; its backward handles dz and the KL
            # gradient in one pass (no second kernel, no gradient accumulation between two paths into mu / log sigma)
            return kl_sum * (beta / z_dist.loc.shape[0])
        return _KLFn.apply(z_dist.loc, log_scale, beta)
