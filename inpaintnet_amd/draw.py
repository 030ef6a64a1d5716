"""What a call asks of the sampling rule, as one value (csrc/sample.h's Request is its C++ counterpart).

HierarchicalDecoder.forward, LatentRNN.forward and ConstraintModel.generate take temperature / uniforms / top_k / top_p / allowed /
forced as keywords; each builds a Draw at its top, asks check() once, and hands the value on to its private helpers as one argument."""
import math

import numpy as np
import torch

from . import ops

DECODER, LATENT, GENERATE = "decoder", "latent", "generate"      # check()'s `who`: the surface whose texts and forms it speaks


class Draw:
    __slots__ = ("temperature", "uniforms", "top_k", "top_p", "allowed", "forced", "words")

    def __init__(self, temperature=None, uniforms=None, top_k=None, top_p=None, allowed=None, forced=None, words=None):
        self.temperature, self.uniforms, self.top_k, self.top_p = temperature, uniforms, top_k, top_p
        self.allowed, self.forced = allowed, forced
        self.words = words                                          # ops.pack_allowed(allowed) where check() has packed it

    def check(self, shape, V, train, who):
        """ValueError for what the surface `who` refuses, BEFORE any random stream is touched: nothing here draws.  shape: the ticks the
        call generates -- (B, 24) for the decoder, (B, measures, 24) for LatentRNN, (L,) or (B, L) for generate; V: the vocabulary;
        train: the surface's flag (generate: False).  One order for all three: top_k / top_p, forced, allowed, uniforms, temperature;
        top_k / top_p need neither shape nor V, so both may be functions, called behind them (generate refuses a bad top_p without a
        score or a model to read them from: tests/test_arnn_trunc_host.py).
        Afterwards forced and allowed are tensors, uniforms a float64 tensor (generate: a float64 array), and `words` the packed mask
        (not for LatentRNN, whose decoder calls pack their own slices).  The surfaces differ in this much:
          generate  prefixes its texts, words the forced range its own way, takes float64 uniforms (rows, L) as they are instead of
                    converting, and leaves a temperature that is not finite to the library (which refuses it);
          latent    does not know V's place in `allowed` (the decoder checks it per measure) and says "nothing allowed" itself."""
        pre = "generate: " if who == GENERATE else ""
        if self.temperature is None and (self.top_k is not None or self.top_p is not None):
            raise ValueError("top_k / top_p without a temperature")
        if self.top_p is not None and not (0.0 < float(self.top_p) <= 1.0):
            raise ValueError(f"{pre}top_p {self.top_p!r} outside (0, 1]")
        ops._top_k(self.top_k)                                      # (ValueError for a top_k that is no integer)
        shape, V = (x() if callable(x) else x for x in (shape, V))
        shape = tuple(shape)
        if self.forced is not None:
            if train:
                raise ValueError("forced tokens are an inference call (train=False)")
            if self.temperature is None:
                raise ValueError("forced tokens need a temperature")
            f = torch.as_tensor(self.forced)
            if f.is_floating_point() or f.is_complex() or f.dtype == torch.bool or tuple(f.shape) != shape:
                raise ValueError(f"{pre}forced must be an int tensor of shape {shape}, got {f.dtype} {tuple(f.shape)}")
            if bool(((f < -1) | (f >= V)).any()):
                raise ValueError(f"generate: forced holds a value outside [-1, {V})" if who == GENERATE else
                                 f"forced: token indices in [0, {V}), or -1 for a free tick")
            self.forced = f
        if self.allowed is not None:
            if train:
                raise ValueError("token constraints are an inference call (train=False)")
            a = torch.as_tensor(self.allowed)
            if who == LATENT:
                if a.dtype != torch.bool or a.dim() != len(shape) + 1 or tuple(a.shape[:-1]) != shape:
                    raise ValueError(f"allowed must be bool of shape {shape} + (V,), got {a.dtype} {tuple(a.shape)}")
                if not bool(a.any(-1).all()):
                    raise ValueError("allowed: a tick with nothing allowed")
            else:
                if a.dtype != torch.bool or tuple(a.shape) != shape + (V,):
                    raise ValueError(f"{pre}allowed must be bool of shape {shape + (V,)}, got {a.dtype} {tuple(a.shape)}")
                self.words = ops.pack_allowed(a)                    # (ValueError for a tick with nothing allowed)
            self.allowed = a
        if self.uniforms is not None and self.temperature is None:
            raise ValueError("uniforms without a temperature")
        if self.temperature is not None:
            if train:
                raise ValueError("temperature sampling is an inference call (train=False)")
            if who != GENERATE and not math.isfinite(float(self.temperature)):
                raise ValueError(f"temperature {self.temperature!r} is not finite")
            if self.uniforms is not None and who == GENERATE:
                u, want = np.asarray(self.uniforms), (shape if len(shape) == 2 else (1,) + shape)
                if u.dtype != np.float64 or u.shape != want:
                    raise ValueError(f"generate: uniforms must be float64 of shape {want}, got {u.dtype} {u.shape}")
                self.uniforms = u
            elif self.uniforms is not None:
                u = torch.as_tensor(self.uniforms, dtype=torch.float64)
                if tuple(u.shape) != shape:
                    raise ValueError(f"uniforms of shape {tuple(u.shape)}, expected {shape}")
                self.uniforms = u
        return self

    def scored(self):
        """Does the call leave log-probabilities?  (truncation given, a mask, or forced tokens: the truncating kernels and up)"""
        return self.top_k is not None or self.top_p is not None or self.allowed is not None or self.forced is not None

    def _each(self, fn):
        pick = lambda x: None if x is None else fn(x)
        return Draw(self.temperature, pick(self.uniforms), self.top_k, self.top_p, pick(self.allowed), pick(self.forced), pick(self.words))

    def measure(self, i):
        """The request of measure i of (B, measures, ...) arrays"""
        return self._each(lambda x: x[:, i])

    def flat(self):
        """(B, measures, ...) arrays as (B * measures, ...): rows ordered (b, measure)"""
        return self._each(lambda x: x.reshape((x.shape[0] * x.shape[1],) + tuple(x.shape[2:])))

    def device(self, dev):
        """The keywords ops.decoder_fwd / ops.arnn_sample take for this request behind (temperature, uniforms): top_k, top_p, packed
        `allowed`, int32 `forced`, the arrays contiguous on `dev`"""
        kw = {"top_k": self.top_k, "top_p": self.top_p}
        if self.allowed is not None:
            words = self.words if self.words is not None else ops.pack_allowed(self.allowed)
            kw["allowed"] = words.to(dev).contiguous()
        if self.forced is not None:
            kw["forced"] = self.forced.to(dev).to(torch.int32).contiguous()
        return kw
