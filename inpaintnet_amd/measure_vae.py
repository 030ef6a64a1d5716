"""MeasureVAE with the reference's Python surface, computed by the HIP library.

Mirrors MeasureVAE/measure_vae.py:10-169, MeasureVAE/encoder.py:9-134 and
MeasureVAE/decoder.py:313-529 of the reference: same constructor arguments,
attributes, method names, return arities, shapes and dtypes.  Each module is one
torch.autograd.Function whose forward/backward are single calls into the C-ABI
(include/inpaintnet_hip.h); parameter gradients are accumulated straight into
the model's flat gradient arena (`model.grad`) by the backward kernels.
"""
import contextlib
import functools
import os
import random

import numpy as np

import torch
from torch import distributions

from . import dp, ops
from .draw import DECODER, Draw
from .model import Model, default_device

_mask_counter = [0]


def _next_mask_offset(n):
    off = _mask_counter[0]
    _mask_counter[0] += int(n)
    return off


def set_dropout_seed(seed, rank=0):
    """Seed of the counter-based dropout stream (rank-offset for data parallel)."""
    _DropState.seed = (int(seed) * 1000003 + int(rank) * 7919) & (2 ** 63 - 1)
    _mask_counter[0] = 0


class _DropState:
    seed = 0x5eed


class _EncoderFn(ops.TrackedFunction):
    @staticmethod
    def forward(ctx, flat, enc, tokens, mask):
        need = ops.outer_grad() and ctx.needs_input_grad[0]     # grad mode is off inside forward(): ask the ctx
        mu, ls, ws = ops.encoder_fwd(enc.cfg, tokens, flat, mask=mask, save=need)
        ctx.enc, ctx.tokens, ctx.mask, ctx.ws = enc, tokens, mask, ws
        return mu, ls

    @staticmethod
    def backward(ctx, dmu, dls):
        enc = ctx.enc
        owner = enc.owner
        dmu, dls = dmu.contiguous(), dls.contiguous()
        buckets = getattr(owner, "encoder_early_buckets", None) if dp.world_size() > 1 else None
        if buckets:
            # data parallel: the heads and GRU layer 1 first -- 38 of the encoder's 44 MB of gradients are final about a
            # millisecond before the step ends -- their all-reduce runs under the layer-0 BPTT chain
            ops.encoder_bwd(enc.cfg, ctx.tokens, owner.flat, owner.grad, ctx.mask, dmu, dls, ctx.ws, stage=1)
            for lo, hi in buckets:
                dp.start_bucket(owner.grad, lo, hi, join_side=True)
            ops.encoder_bwd(enc.cfg, ctx.tokens, owner.flat, owner.grad, ctx.mask, dmu, dls, ctx.ws, stage=2)
        else:
            ops.encoder_bwd(enc.cfg, ctx.tokens, owner.flat, owner.grad, ctx.mask, dmu, dls, ctx.ws)
        ctx.ws = None
        return None, None, None, None


class _DecoderFn(ops.TrackedFunction):
    @staticmethod
    def forward(ctx, z, flat, dec, target, teacher_forced, mask_beat, mask_tick, multinomial_seed=0, draw=None, logp=None):
        """draw: the sampled call's Draw (None: the argmax / teacher-forced / multinomial call); logp: its output, or None"""
        need = ops.outer_grad() and (ctx.needs_input_grad[0] or ctx.needs_input_grad[1])
        kw = {}
        if draw is not None:
            kw = draw.device(z.device)
            kw.update(temperature=float(draw.temperature), uniforms=draw.uniforms.to(z.device).contiguous())
        weights, samples, ws = ops.decoder_fwd(dec.cfg, z.contiguous(), target, teacher_forced, flat, mask_beat,
                                               mask_tick, save=need, multinomial_seed=multinomial_seed, logp=logp, **kw)
        ctx.dec, ctx.ws, ctx.mb, ctx.mt = dec, ws, mask_beat, mask_tick
        if getattr(dec, "keep_ws", False):         # test hook: lets a parity test read intermediates (ops.ws_field)
            dec.last_ws = ws
        ctx.save_for_backward(weights, samples)
        ctx.mark_non_differentiable(samples)
        # (no zero tensor for the gradient of `samples`: autograd would launch a fill kernel for it in every backward pass -- 6 us of
        #  stream time for a tensor nobody reads)
        ctx.set_materialize_grads(False)
        return weights, samples

    @staticmethod
    def backward(ctx, dweights, _dsamples):
        dec = ctx.dec
        if dweights is None:                            # nothing downstream depends on the weights
            ctx.ws = None
            return (None,) * 10
        weights, samples = ctx.saved_tensors
        grads = dec.owner.grad if dec.owner.trainable else None
        dz = ops.decoder_bwd(dec.cfg, dweights.contiguous(), weights, samples, dec.owner.flat, grads, ctx.mb, ctx.mt,
                             ctx.ws, need_dz=ctx.needs_input_grad[0])
        ctx.ws = None
        if grads is not None:
            # data parallel: the decoder half of the arena is final now -> start its all-reduce under the encoder's backward
            if dp.world_size() > 1:
                # behind the decoder's leaf GEMMs on the side streams, without holding up the encoder's backward
                dp.start_bucket(grads, dec.owner.decoder_arena_start, grads.numel(), join_side=True)
        return (dz,) + (None,) * 9


class _ReparamFn(torch.autograd.Function):
    """z = mu + eps * exp(logsigma) (measure_vae.py:119 rsample) and, from the same pass over (mu, logsigma), the sum of
    the KL terms against N(0, 1) that VAETrainer.compute_kld_loss needs (vae_trainer.py:128-139)."""

    @staticmethod
    def forward(ctx, mu, ls, eps, kl=None):
        if kl is None:
            kl = torch.zeros(1, dtype=torch.float32, device=mu.device)
        z, _ = ops.reparam_kl(mu, ls, eps, kl_sum=kl)
        ctx.save_for_backward(mu, ls, eps)
        ctx.set_materialize_grads(False)
        return z, kl[0]

    @staticmethod
    def backward(ctx, dz, dkl):
        mu, ls, eps = ctx.saved_tensors
        if dz is not None:
            dz = dz.contiguous()
        if dkl is not None:
            dkl = dkl.reshape(1).contiguous()
        dmu, dls = ops.latent_bwd(dz, mu, ls, eps, 1.0 if dkl is not None else 0.0, kscale_dev=dkl)
        return dmu, dls, None, None


class _MmdFn(torch.autograd.Function):
    """The MMD between z_tilde and z_prior (ops.mmd) as a loss term: where z_tilde takes a gradient the pair
    launch of the forward also leaves G = d value / d z_tilde, and the backward is the device product G * gloss -- autograd adds it
    to the decoder's dz in front of the reparameterisation's backward.  z_prior is a constant.  -> value, S_xx, S_yy, S_xy."""

    @staticmethod
    def forward(ctx, z_tilde, z_prior, kernel, bandwidth, estimator, coeff):
        out4, G = ops.mmd(z_tilde.contiguous(), z_prior.detach().contiguous(), kernel, bandwidth, estimator, coeff,
                          want_grad=ctx.needs_input_grad[0])
        ctx.save_for_backward(G)
        value, sxx, syy, sxy = out4[0], out4[1], out4[2], out4[3]
        ctx.mark_non_differentiable(sxx, syy, sxy)
        ctx.set_materialize_grads(False)
        return value, sxx, syy, sxy

    @staticmethod
    def backward(ctx, gloss, _gxx, _gyy, _gxy):
        G, = ctx.saved_tensors
        if gloss is None or G is None:
            return None, None, None, None, None, None
        return G * gloss, None, None, None, None, None


@functools.lru_cache(maxsize=None)
def _attr_columns(dims, device):
    """The regularised columns as a device index, made once per (dims, device): no host-to-device copy inside a step."""
    return torch.tensor(dims, dtype=torch.int64, device=device)


class _AttrRegFn(torch.autograd.Function):
    """The attribute regularisation of z_tilde's dimensions `dims` towards the columns of `attrs` (ops.attr_reg)
    as a loss term: where z_tilde takes a gradient the pair launch of the forward also leaves G = d value / d z_tilde[:, dims], and
    the backward scatters G * gloss into a [B, Z] gradient that is zero outside those columns.  attrs is a constant.
    -> value, per_attr [A], counts [A, 3]."""

    @staticmethod
    def forward(ctx, z_tilde, dims, attrs, delta, coeff):
        out, counts, G = ops.attr_reg(z_tilde.contiguous(), dims, attrs.detach().contiguous(), delta, coeff,
                                      want_grad=ctx.needs_input_grad[0])
        ctx.save_for_backward(G)
        ctx.dims, ctx.z_shape = list(dims), tuple(z_tilde.shape)
        value, per_attr = out[0], out[1:]
        ctx.mark_non_differentiable(per_attr, counts)
        ctx.set_materialize_grads(False)
        return value, per_attr, counts

    @staticmethod
    def backward(ctx, gloss, _gper, _gcounts):
        G, = ctx.saved_tensors
        if gloss is None or G is None:
            return None, None, None, None, None
        dz = torch.zeros(ctx.z_shape, dtype=G.dtype, device=G.device)
        dz.index_copy_(1, _attr_columns(tuple(ctx.dims), G.device), G * gloss)
        return dz, None, None, None, None


class _ReparamFbFn(torch.autograd.Function):
    """_ReparamFn with the KL term summed into parts and floored ("free bits"): the forward kernel leaves the
    floored sum, the plain sum, the parts and their keep vector; the backward hands the KL gradient to the elements of kept parts
    only (ops.latent_bwd_fb with the saved keep vector)."""

    @staticmethod
    def forward(ctx, mu, ls, eps, free_nats, per, stats=None):
        if stats is None:
            stats = torch.zeros(2, dtype=torch.float32, device=mu.device)
        z, parts, keep, _, _ = ops.reparam_kl_fb(mu, ls, eps, free_nats, per, kl_sum=stats[0:1], kl_raw=stats[1:2])
        ctx.save_for_backward(mu, ls, eps, keep)
        ctx.per = per
        kl, raw = stats[0], stats[1]
        ctx.mark_non_differentiable(raw, parts, keep)
        ctx.set_materialize_grads(False)
        return z, kl, raw, parts, keep

    @staticmethod
    def backward(ctx, dz, dkl, _draw, _dparts, _dkeep):
        mu, ls, eps, keep = ctx.saved_tensors
        if dz is not None:
            dz = dz.contiguous()
        if dkl is not None:
            dkl = dkl.reshape(1).contiguous()
        dmu, dls = ops.latent_bwd_fb(dz, mu, ls, eps, 1.0 if dkl is not None else 0.0, keep, ctx.per, kscale_dev=dkl)
        return dmu, dls, None, None, None, None


class NormalLogScale(distributions.Normal):
    """torch Normal whose log-scale (the encoder's actual output) is kept alongside, so the KL kernel needs no log()
    round trip.  `scale` (= exp(log_scale), encoder.py:133) is computed the first time something reads it: the training
    step never does.  rsample()/sample() draw eps with torch's device generator and combine on the GPU with the
    reparameterisation kernel, which also leaves the KL sum in `kl_sum`.

    rsample(free_bits=(free_nats, per)) floors the KL term: per 'measure' sums KL[b, d] over d and floors
    every measure's sum at free_nats; per 'dim' sums over the rows of THIS call -- under data parallelism the rank's own shard, as
    batch statistics would be, no collective -- and floors every latent dimension's sum at rows * free_nats.  It leaves `kl_sum` (the
    floored sum), `kl_raw` (the plain sum), `kl_parts` and `kl_keep` (1.0 = the part is above its floor and passes its gradient)."""

    def __init__(self, loc, log_scale, owner=None):
        self.loc = loc
        self.log_scale = log_scale
        self._scale = None
        self.kl_sum = None
        self.kl_raw = self.kl_parts = self.kl_keep = None      # only rsample(free_bits=...) fills these
        self._owner = owner                      # the model whose arena tail holds the per-step accumulators (or None)
        distributions.Distribution.__init__(self, loc.size(), validate_args=False)

    @property
    def scale(self):
        if self._scale is None:
            self._scale = _ExpFn.apply(self.log_scale)
        return self._scale

    @scale.setter
    def scale(self, value):
        self._scale = value

    def rsample(self, sample_shape=torch.Size(), eps=None, free_bits=None):
        if len(sample_shape) != 0:
            return super().rsample(sample_shape)
        if eps is None:
            eps = torch.randn_like(self.loc)
        if free_bits is not None:
            free_nats, per = free_bits
            stats = self._owner.take_stats(2) if self._owner is not None else None
            z, self.kl_sum, self.kl_raw, self.kl_parts, self.kl_keep = _ReparamFbFn.apply(self.loc, self.log_scale, eps,
                                                                                          float(free_nats), per, stats)
            self.last_eps = eps
            return z
        kl = self._owner.take_stats(1) if self._owner is not None else None
        z, self.kl_sum = _ReparamFn.apply(self.loc, self.log_scale, eps, kl)
        self.last_eps = eps
        return z


class Encoder(torch.nn.Module):
    """MeasureVAE/encoder.py:9-134."""

    def __init__(self, owner, prefix, note_embedding_dim, rnn_hidden_size, num_layers, num_notes, dropout,
                 bidirectional, z_dim, rnn_class):
        super().__init__()
        if num_layers != 2 or not bidirectional:
            raise NotImplementedError("the HIP encoder implements the reference configuration: 2 layers, bidirectional")
        object.__setattr__(self, "owner", owner)
        self.prefix = prefix
        self.bidirectional = bidirectional
        self.num_directions = 2
        self.note_embedding_dim = note_embedding_dim
        self.num_layers = num_layers
        self.rnn_hidden_size = rnn_hidden_size
        self.z_dim = z_dim
        self.dropout = dropout
        self.rnn_class = rnn_class
        self.num_notes = num_notes

    @property
    def cfg(self):
        return self.owner.cfg

    def __repr__(self):
        return f'Encoder(' \
               f'{self.note_embedding_dim},' \
               f'{self.rnn_class},' \
               f'{self.num_layers},' \
               f'{self.rnn_hidden_size},' \
               f'{self.dropout},' \
               f'{self.bidirectional},' \
               f'{self.z_dim},' \
               f')'

    def forward(self, score_tensor, mask=None):
        """score_tensor (B, 24) int64 -> Normal(loc, scale)   (encoder.py:104-134)"""
        batch_size, T = score_tensor.size()
        tokens = score_tensor.contiguous()
        if mask is None and self.training and self.dropout > 0:
            n = T * batch_size * 2 * self.rnn_hidden_size
            mask = ops.dropout_mask((T, batch_size, 2 * self.rnn_hidden_size), self.dropout, _DropState.seed,
                                    _next_mask_offset(n), tokens.device)
        mu, ls = _EncoderFn.call(self.owner.flat_for_autograd(), self, tokens, mask)
        return NormalLogScale(mu, ls, self.owner)


class _ExpFn(torch.autograd.Function):
    """sigma = exp(logsigma)  (encoder.py:133), by the reparameterisation kernel."""

    @staticmethod
    def forward(ctx, ls):
        _, sigma = ops.reparam_kl(ls, ls, None, kl_sum=None, want_sigma=True)
        ctx.save_for_backward(sigma)
        return sigma

    @staticmethod
    def backward(ctx, dsigma):
        (sigma,) = ctx.saved_tensors
        return dsigma * sigma


class HierarchicalDecoder(torch.nn.Module):
    """MeasureVAE/decoder.py:313-529."""

    def __init__(self, owner, prefix, note_embedding_dim, num_notes, z_dim, num_layers, rnn_hidden_size, dropout,
                 rnn_class):
        super().__init__()
        if num_layers != 2:
            raise NotImplementedError("the HIP decoder implements the reference configuration: 2 layers")
        object.__setattr__(self, "owner", owner)
        self.prefix = prefix
        self.name = 'HierarchicalDecoder'
        self.num_notes = num_notes
        self.note_embedding_dim = note_embedding_dim
        self.z_dim = z_dim
        self.rnn_class = rnn_class
        self.num_layers = num_layers
        self.rnn_hidden_size = rnn_hidden_size
        self.dropout = dropout
        self.use_teacher_forcing = True
        self.teacher_forcing_prob = 0.5
        self.sampling = 'argmax'

    @property
    def cfg(self):
        return self.owner.cfg

    def __repr__(self):
        return f'{self.name}' \
               f'{self.note_embedding_dim},' \
               f'{self.rnn_class},' \
               f'{self.num_layers},' \
               f'{self.rnn_hidden_size},' \
               f'{self.dropout},' \
               f')'

    def forward(self, z, score_tensor, train, masks=None, teacher_forced=None, temperature=None, uniforms=None, top_k=None,
                top_p=None, allowed=None, forced=None):
        """z (B,Z), score_tensor (B,24) -> weights (B,24,V), samples (B,1,24)   (decoder.py:412-453).
        One Bernoulli(0.5) teacher-forcing coin per call when train=True (decoder.py:431-434); it can be
        injected with `teacher_forced=`.
        temperature (a finite float): a FREE-RUNNING call draws every token from softmax(temperature * weights[b, t]) with the uniform
        uniforms[b, t] (csrc/sample.h: np.random.choice's order, as ConstraintModelGaussianReg.generate) and feeds it back; uniforms
        (B,24) float64, host or device, or None: one np.random.random_sample((B, 24)) call.  Inference only (ValueError with
        train=True); a call whose `teacher_forced=True` was injected ignores both.  `sampling = 'multinomial'` and the training path
        are as they were.  The arguments are checked before anything random is drawn: a rejected call leaves every stream alone.
        top_k (an int; None, <= 0 or >= V: off) / top_p (in (0, 1]; None or 1: off), with a temperature only (ValueError without):
        every draw is taken from the top_k highest-ranked tokens, and among those from the shortest prefix of the ranking that
        holds top_p of their mass (csrc/sample.h: ranked by temperature * weight descending, lowest index first among equals).  Such a
        call leaves self.last_logp (B,24): the drawn tokens' log-probabilities under the truncated distribution, NaN where a tick
        took the argmax; every other call leaves it None.
        allowed (bool (B,24,V), host or device; inference only, ignored by a call whose `teacher_forced=True` was injected): the tokens
        each (row, tick) may return -- a ban clears entries, a note to keep is a tick with one entry set.  The mask is applied inside
        the launch, in front of the truncation (csrc/sample.h): the token fed back into tick t + 1 is the
        constrained one, a fixed tick's logp is exactly 0.  ValueError for a tick with nothing allowed.  Without a temperature the call
        runs as temperature 1, top_k = 1 with zero uniforms -- the argmax over the allowed tokens -- and leaves last_logp None.
        forced (an int tensor (B,24), host or device, -1 = a free tick; inference with a temperature only, ignored by a call whose
        `teacher_forced=True` was injected): the token a tick returns and feeds back instead of drawing one -- whether or not it is
        allowed or kept -- with its log-probability under the masked and truncated distribution a draw would have used (csrc/sample.h,
        DESIGN.md section 15): -inf for a banned or truncated token, NaN where the rule does not apply.  A forced tick does not use its
        uniform.  Every tick forced scores a given measure, the first ticks forced continue a prefix.  ValueError for a wrong shape or
        dtype or a value outside [-1, V).  A forced call always leaves last_logp (B,24)."""
        T = self.cfg.beats * self.cfg.ticks_per_beat
        d = Draw(temperature, uniforms, top_k, top_p, allowed, forced).check((z.size(0), T), int(self.cfg.num_notes), train, DECODER)
        self.last_logp = None
        if teacher_forced is None:
            if self.use_teacher_forcing and train:
                teacher_forced = random.random() < self.teacher_forcing_prob
            else:
                teacher_forced = False
        if self.sampling not in ('argmax', 'multinomial'):
            raise ValueError(f"sampling must be 'argmax' or 'multinomial' (decoder.py:506-516), got {self.sampling!r}")
        batch_size_z, z_dim = z.size()
        assert z_dim == self.z_dim
        batch_size = score_tensor.size(0)
        assert batch_size == batch_size_z
        target = None
        if teacher_forced:
            target = score_tensor.detach()
            if target.dtype != torch.int64:
                target = target.long()
            target = target.contiguous()
        mb = mt = None
        if masks is not None:
            mb, mt = masks
        elif self.training and self.dropout > 0:
            H = self.rnn_hidden_size
            dev = z.device
            mb = ops.dropout_mask((self.cfg.beats, batch_size, H), self.dropout, _DropState.seed,
                                  _next_mask_offset(self.cfg.beats * batch_size * H), dev)
            mt = ops.dropout_mask((T, batch_size, H), self.dropout, _DropState.seed,
                                  _next_mask_offset(T * batch_size * H), dev)
        if d.allowed is not None and d.temperature is None and not teacher_forced:
            # constraints without a temperature: top_k = 1 keeps the top-ranked allowed token whatever the uniform (DESIGN.md section 11's
            # top_k = 1 equality, over the allowed tokens)
            u = torch.zeros(batch_size, T, dtype=torch.float64, device=z.device)
            return _DecoderFn.call(z, self.owner.flat_for_autograd(), self, None, False, mb, mt, 0,
                                   Draw(1.0, u, 1, None, d.allowed, None, d.words))
        if d.temperature is not None and not teacher_forced:
            if d.uniforms is None:
                d.uniforms = torch.from_numpy(np.random.random_sample((batch_size, T)))
            logp = torch.empty(batch_size, T, dtype=torch.float32, device=z.device) if d.scored() else None
            out = _DecoderFn.call(z, self.owner.flat_for_autograd(), self, None, False, mb, mt, 0, d, logp)
            self.last_logp = logp
            return out
        seed = 0
        if self.sampling == 'multinomial' and not teacher_forced:
            # one counter-based stream per call, derived from the dropout seed (set_dropout_seed) and the call counter
            seed = ((_DropState.seed * 0x9E3779B97F4A7C15 + _next_mask_offset(T * batch_size) + 1) & (2 ** 64 - 1)) or 1
        weights, samples = _DecoderFn.call(z, self.owner.flat_for_autograd(), self, target, teacher_forced, mb, mt, seed)
        return weights, samples


class MeasureVAE(Model):
    """MeasureVAE/measure_vae.py:10-169."""

    def __init__(self, dataset, note_embedding_dim=10, metadata_embedding_dim=2, num_encoder_layers=2,
                 encoder_hidden_size=512, encoder_dropout_prob=0.5, latent_space_dim=256, num_decoder_layers=2,
                 decoder_hidden_size=512, decoder_dropout_prob=0.5, has_metadata=False, device=None):
        super().__init__()
        self.num_beats_per_measure = 4
        self.num_ticks_per_measure = 24
        self.num_ticks_per_beat = int(self.num_ticks_per_measure / self.num_beats_per_measure)
        self.dataset = dataset.__repr__()
        self.note_embedding_dim = note_embedding_dim
        self.metadata_embedding_dim = metadata_embedding_dim
        self.num_encoder_layers = num_encoder_layers
        self.encoder_hidden_size = encoder_hidden_size
        self.encoder_dropout_prob = encoder_dropout_prob
        self.latent_space_dim = latent_space_dim
        self.num_decoder_layers = num_decoder_layers
        self.decoder_hidden_size = decoder_hidden_size
        self.decoder_dropout_prob = decoder_dropout_prob
        self.has_metadata = has_metadata
        self.num_notes = len(dataset.note2index_dicts[0])
        self.trainable = True
        self.free_bits = None                    # (free_nats, 'measure' | 'dim'): the KL floor of TRAINING passes (VAETrainer sets it)
        self.cfg = ops.vae_config(self.num_notes, note_embedding_dim, encoder_hidden_size, latent_space_dim,
                                  decoder_hidden_size, self.num_beats_per_measure, self.num_ticks_per_beat)
        table, total = ops.vae_param_table(self.cfg)
        self._alloc_arena(table, total, device or default_device())
        self.decoder_arena_start = min(off for name, off, _ in table if name.startswith("decoder."))
        # arena ranges whose gradients are final after stage 1 of the encoder's backward (layer 1; the Linear heads): the
        # note embedding sits between them and is final only at the very end
        offs = {name: off for name, off, _ in table}
        self.encoder_early_buckets = ((offs["encoder.lstm.weight_ih_l1"], offs["encoder.note_embedding_layer.weight"]),
                                      (offs["encoder.linear_mean.0.weight"], self.decoder_arena_start))
        self._flat_leaf = None
        self.encoder = Encoder(self, "encoder", note_embedding_dim, encoder_hidden_size, num_encoder_layers,
                               self.num_notes, encoder_dropout_prob, True, latent_space_dim, torch.nn.GRU)
        self.decoder = HierarchicalDecoder(self, "decoder", note_embedding_dim, self.num_notes, latent_space_dim,
                                           num_decoder_layers, decoder_hidden_size, decoder_dropout_prob,
                                           torch.nn.GRU)
        self.init_reference_style()
        cur_dir = os.path.dirname(os.path.realpath(__file__))
        self.filepath = os.path.join(cur_dir, 'models/', self.__repr__())

    def flat_for_autograd(self):
        """The arena as an autograd leaf, so that the module Functions are recorded whenever the model is
        trainable.  Its own .grad is never populated: the backward kernels write into self.grad."""
        if not self.trainable:
            return self.flat
        if self._flat_leaf is None:
            self._flat_leaf = self.flat.detach().requires_grad_(True)     # shares storage
        return self._flat_leaf

    def freeze(self):
        """for p in vae.parameters(): p.requires_grad = False   (latent_rnn.py:42-43)"""
        self.trainable = False

    def __repr__(self):
        return f'MeasureVAE(' \
               f'{self.dataset},' \
               f'{self.encoder.__repr__()},' \
               f'{self.decoder.__repr__()},' \
               f')'

    def forward(self, measure_score_tensor, train=True, eps=None, teacher_forced=None):
        """(B,24) int64 -> (weights, samples, z_dist, prior_dist, z_tilde, z_prior)   (measure_vae.py:97-134)"""
        seq_len = measure_score_tensor.size(1)
        assert seq_len == self.num_ticks_per_measure
        enc_mask = dec_masks = None
        pe, pd = self.encoder.dropout, self.decoder.dropout
        if self.training and pe > 0 and pe == pd:
            # the three dropout masks of a step (encoder layer 0 -> 1, decoder beat and tick layers) in ONE launch: the mask
            # stream is a pure function of (seed, offset + index), and the three would have taken consecutive offsets
            B, T, nb = measure_score_tensor.size(0), seq_len, self.num_beats_per_measure
            He, Hd = self.encoder_hidden_size, self.decoder_hidden_size
            sizes = (T * B * 2 * He, nb * B * Hd, T * B * Hd)
            buf = ops.dropout_mask((sum(sizes),), pe, _DropState.seed, _next_mask_offset(sum(sizes)),
                                   measure_score_tensor.device)
            m0, m1, m2 = torch.split(buf, sizes)
            enc_mask = m0.view(T, B, 2 * He)
            dec_masks = (m1.view(nb, B, Hd), m2.view(T, B, Hd))
        z_dist = self.encoder(measure_score_tensor, mask=enc_mask)
        # prior_dist.sample() (measure_vae.py:127) for N(0, 1) is a plain standard-normal draw (torch.normal(mean, std)
        # would also validate std >= 0 with a device->host read, i.e. stall the host once per forward pass): eps of the
        # reparameterisation and z_prior come out of one generator call
        if eps is None:
            draws = torch.randn((2,) + tuple(z_dist.loc.shape), dtype=z_dist.loc.dtype, device=z_dist.loc.device)
            eps, z_prior = draws[0], draws[1]
        else:
            z_prior = torch.randn_like(z_dist.loc)
        # the KL floor is a training device: validation, the testers and forward_test always take the plain KL, so that their
        # losses stay comparable across epochs and with the reference
        if train and self.free_bits is not None:
            z_tilde = z_dist.rsample(eps=eps, free_bits=self.free_bits)
        else:
            z_tilde = z_dist.rsample(eps=eps)
        prior_dist = self._standard_normal(z_dist.loc)
        weights, samples = self.decoder(z=z_tilde, score_tensor=measure_score_tensor, train=train,
                                        teacher_forced=teacher_forced, masks=dec_masks)
        return weights, samples, z_dist, prior_dist, z_tilde, z_prior

    def decode(self, z, temperature=None, uniforms=None, top_k=None, top_p=None, allowed=None, forced=None):
        """z (B,Z) -> (weights (B,24,V), samples (B,1,24)): the free-running decoder alone (what VAETester.decode_mid_point does with
        a latent), by the argmax or -- temperature set -- drawn from softmax(temperature * weights), behind top-k / nucleus truncation
        with top_k / top_p (HierarchicalDecoder.forward; the draws' log-probabilities: self.decoder.last_logp); allowed (bool
        (B,24,V)): the tokens each tick may return, with or without a temperature (HierarchicalDecoder.forward); forced (int (B,24), -1 = a
        free tick; with a temperature): the tokens to return, feed back and score instead of drawing (HierarchicalDecoder.forward)."""
        dummy = torch.zeros(z.shape[0], self.num_ticks_per_measure, device=z.device)
        return self.decoder(z, dummy, train=False, temperature=temperature, uniforms=uniforms, top_k=top_k, top_p=top_p, allowed=allowed,
                            **({} if forced is None else {"forced": forced}))

    def log_weights(self, score, num_samples, eps=None, generator=None, max_rows=4096, reproducible=True):
        """The log importance weights of the IWAE bound: score (B, 24) int64 -> (logw, nll), both float32
        (B, K) on the device, K = num_samples.  logw[b, k] = log p(z) - log q(z | x_b) - nll[b, k] for z = mu_b + eps[b, k] * sigma_b,
        nll[b, k] the negative log-likelihood of x_b's 24 tokens under the decoder run on z with x_b's own tokens fed back
        (teacher-forced, eval mode).  ops.iw_finish turns them into (iwae, elbo, ess, rec, kl).  Runs under torch.no_grad(); ValueError
        in training mode: a likelihood under dropout is not the model's.  The encoder runs once; the decoder sees blocks of Bc = min(B,
        max_rows) measures and chunks of Kc = max(1, max_rows // Bc) samples, Bc * Kc rows a call.  eps: float32 (B, K, Z), the
        draws to use; None: drawn per (block, chunk), in that order, from `generator` (the device's default one if None) -- another
        max_rows then means other draws for the same seed.  reproducible: the encoder's and the decoder's products run with one k range
        each (ops.one_k_range: no f32 atomics), so that the same draws give the same bits from call to call -- 7 % slower at 256
        measures x 16 samples; False leaves the planner's choice, and two calls then agree to about 1e-7 of a weight only.  The call
        ends with a synchronisation and the chain / token checks."""
        if self.training:
            raise ValueError("log_weights: the model is in training mode; a likelihood under dropout is not the model's -- call eval()")
        K, max_rows = int(num_samples), int(max_rows)
        if K < 1 or max_rows < 1:
            raise ValueError(f"log_weights: num_samples and max_rows must be >= 1, got {num_samples} and {max_rows}")
        if score.dim() != 2 or score.size(1) != self.num_ticks_per_measure or score.size(0) < 1:
            raise ValueError(f"log_weights: score must be (B, {self.num_ticks_per_measure}), got {tuple(score.shape)}")
        B, Z = score.size(0), self.latent_space_dim
        score = score.long().contiguous()
        if eps is not None and not (isinstance(eps, torch.Tensor) and eps.dtype == torch.float32 and tuple(eps.shape) == (B, K, Z)
                                    and eps.device == score.device and eps.is_contiguous()):
            raise ValueError(f"log_weights: eps must be a contiguous float32 ({B}, {K}, {Z}) tensor on the score's device")
        with torch.no_grad(), (ops.one_k_range() if reproducible else contextlib.nullcontext()):
            z_dist = self.encoder(score)
            mu, ls = z_dist.loc.contiguous(), z_dist.log_scale.contiguous()
            logw = torch.empty(B, K, dtype=torch.float32, device=mu.device)
            nll = torch.empty_like(logw)
            Bc = min(B, max_rows)
            Kc = max(1, max_rows // Bc)
            for b0 in range(0, B, Bc):
                b1 = min(B, b0 + Bc)
                block = score[b0:b1]
                for k0 in range(0, K, Kc):
                    k1 = min(K, k0 + Kc)
                    if eps is None:
                        e = torch.randn(b1 - b0, k1 - k0, Z, dtype=torch.float32, device=mu.device, generator=generator)
                    else:
                        e = eps[b0:b1, k0:k1]
                    z, logr = ops.iw_draw(mu[b0:b1], ls[b0:b1], e)
                    rows = block.repeat_interleave(k1 - k0, 0)       # row b * Kc + j: measure b, as iw_draw orders z
                    weights, _ = self.decoder(z, rows, train=False, teacher_forced=True)
                    ops.nll_rows(weights, rows, logr, group=k1 - k0, out_nll=nll[b0:b1, k0:k1], out_logw=logw[b0:b1, k0:k1], ld_out=K)
        torch.cuda.synchronize()
        ops.check_chains("MeasureVAE.log_weights")
        return logw, nll

    def _standard_normal(self, like):
        """N(0, 1) of the latent's shape (measure_vae.py:122-125): the constant loc / scale tensors are built once."""
        key = (tuple(like.shape), like.device, like.dtype)
        cache = self.__dict__.setdefault("_prior_cache", {})
        if key not in cache:
            cache[key] = (torch.zeros_like(like), torch.ones_like(like))
        loc, scale = cache[key]
        return distributions.Normal(loc=loc, scale=scale, validate_args=False)

    def forward_test(self, measure_score_tensor):
        """(B,M,24) -> weights (B,M,24,V), samples (B,1,24M)   (measure_vae.py:136-169).  The M measures are
        independent, so they run as one batch of B*M."""
        batch_size, num_measures, seq_len = measure_score_tensor.size()
        assert seq_len == self.num_ticks_per_measure
        flat_in = measure_score_tensor.reshape(batch_size * num_measures, seq_len).contiguous()
        z = self.encoder(flat_in).rsample()
        w, s = self.decoder(z=z, score_tensor=flat_in, train=False)
        weights = w.view(batch_size, num_measures, seq_len, -1)
        samples = s.view(batch_size, 1, num_measures * seq_len)
        return weights, samples
