"""Gradient clipping without a GPU: the float64 restatement of the rule (tests/clip_ref.py) against torch's own clip_grad_norm_ + Adam,
the Trainer keyword's validation, and the binding of the three entry points against the header."""
import math
import os
import re

import numpy as np
import pytest
import torch

from inpaintnet_amd import _lib
from tests import clip_ref as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (5, 1000, 37)                   # an arena split into three tensors of unequal size
LR, B1, B2, EPS = (float(np.float32(x)) for x in (1e-3, 0.9, 0.999, 1e-8))      # what the ABI's `float` arguments hold


def _grads(step):
    g = torch.Generator().manual_seed(100 + step)
    return (torch.randn(sum(SIZES), generator=g) * 3.0).float()                  # float32 values, as the arena holds them


@pytest.mark.parametrize("factor", [0.5, 10.0])
def test_restatement_agrees_with_torch_clip_grad_norm_and_adam(factor):
    """Three steps of clip_grad_norm_(error_if_nonfinite=False) + torch.optim.Adam on float64 CPU tensors against three steps of the
    restatement, max_norm = factor x the first step's norm (0.5: every step clips; 10: none does).  Parameters within 1e-12 relative:
    both sides are float64 and only the order of the norm's sum differs (torch: the norm of three per-tensor norms).

    torch multiplies by the float64 coefficient c; the rule rounds it to float32 first (scale = (float)c: the kernel's arithmetic is
    float32).  So torch is compared with the restatement's round_scale=False form, and the rounded form may differ from it by what
    one float32 rounding of each step's gradient scale can do.  With relative changes d <= 2^-24 of the scales, m moves by at most
    d * sum_j w_j |g_j| (w: Adam's weights of the past gradients) and sqrt(v) by d of itself; by Cauchy-Schwarz the first is at most
    2 d times the bias-corrected denominator in the first three steps, and the update itself is at most 2 lr there: below 4 d lr a
    step, 12 * 2^-24 * lr for the three."""
    g0 = torch.Generator().manual_seed(7)
    p0 = torch.randn(sum(SIZES), generator=g0).double()
    max_norm = float(np.float32(factor * CR.norm_ref(_grads(1))))
    params = [torch.nn.Parameter(t.clone()) for t in p0.split(SIZES)]
    opt = torch.optim.Adam(params, lr=LR, betas=(B1, B2), eps=EPS)
    exact = [p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)]
    rounded = [t.clone() for t in exact]
    for step in (1, 2, 3):
        g = _grads(step)
        for prm, part in zip(params, g.double().split(SIZES)):
            prm.grad = part.clone()
        total = torch.nn.utils.clip_grad_norm_(params, max_norm, error_if_nonfinite=False)
        opt.step()
        *exact, rep, norm = CR.adam_clip_ref(*exact[:1], g, *exact[1:], LR, step, max_norm, round_scale=False)
        *rounded, rep_r, _ = CR.adam_clip_ref(*rounded[:1], g, *rounded[1:], LR, step, max_norm)
        assert abs(float(total) - norm) <= 1e-14 * norm
        assert rep == rep_r == [1, 0, 0, 0, int(factor < 1.0), 0]
    got = torch.cat([prm.detach().reshape(-1) for prm in params])
    rel = float(((got - exact[0]).abs() / exact[0].abs()).max())
    drift = float((rounded[0] - exact[0]).abs().max())
    print(f"factor {factor}: torch vs restatement {rel:.2e} relative; float32 scale moves p by {drift:.2e} (bound {12 * 2.0 ** -24 * LR:.2e})")
    assert rel <= 1e-12
    assert drift <= 12 * 2.0 ** -24 * LR
    if factor > 1.0:
        assert torch.equal(rounded[0], exact[0])                                # scale = 1: nothing to round


def test_restatement_skips_and_drops():
    p, m, v = torch.randn(9).double(), torch.rand(9).double(), torch.rand(9).double()
    g = torch.randn(9)
    out = CR.adam_clip_ref(p, g, m, v, LR, 2, 1.0, skip=True)
    assert out[3] == [1, 1, 0, 0, 0, 0] and all(torch.equal(a, b) for a, b in zip(out[:3], (p, m, v)))
    for bad in (float("inf"), float("-inf"), float("nan")):
        gb = g.clone()
        gb[4] = bad
        out = CR.adam_clip_ref(p, gb, m, v, LR, 2, 1.0)
        assert out[3] == [1, 0, 0, 0, 0, 1] and not math.isfinite(out[4])
        assert all(torch.equal(a, b) for a, b in zip(out[:3], (p, m, v)))
    assert CR.clip_decision(g, math.inf)[2:] == (False, 1.0)                    # max_norm = inf never clips


class _Untouchable:
    """A model no attribute of which may be read."""

    def __getattr__(self, name):
        raise AssertionError(f"the model was touched ({name}) before max_grad_norm was checked")


class _HostModel:
    def __init__(self):
        self.flat = torch.zeros(8)
        self.grad = torch.zeros(8)


def _trainer_class():
    from inpaintnet_amd.trainer import Trainer

    class T(Trainer):
        def loss_and_acc_for_batch(self, batch, epoch_num=None, train=True):
            raise NotImplementedError

        def process_batch_data(self, batch):
            return batch

        def update_scheduler(self, epoch_num):
            return
    return T


@pytest.mark.parametrize("bad", [0, -1, float("nan"), 0.0, -math.inf])
def test_trainer_rejects_a_max_grad_norm_outside_the_rule_before_touching_the_model(bad, monkeypatch):
    monkeypatch.setenv("INET_GC_FREEZE", "0")
    with pytest.raises(ValueError, match="max_grad_norm"):
        _trainer_class()(None, _Untouchable(), max_grad_norm=bad)


@pytest.mark.parametrize("good", [None, math.inf, 1.0, 1e-3])
def test_trainer_accepts_none_inf_and_positive_values(good, monkeypatch):
    monkeypatch.setenv("INET_GC_FREEZE", "0")                                   # (leave this process's collector alone)
    tr = _trainer_class()(None, _HostModel(), max_grad_norm=good)
    assert tr.max_grad_norm == good
    assert tr.last_grad_norm is None and tr.clipped_steps == 0 and tr.nonfinite_steps == 0


def test_subclass_trainers_take_the_keyword():
    import inspect
    from inpaintnet_amd.arnn import AnticipationRNNBaselineTrainer, AnticipationRNNGaussianRegTrainer
    from inpaintnet_amd.latent_rnn_trainer import LatentRNNTrainer
    from inpaintnet_amd.vae_trainer import VAETrainer
    for cls in (VAETrainer, LatentRNNTrainer, AnticipationRNNGaussianRegTrainer, AnticipationRNNBaselineTrainer):
        prm = inspect.signature(cls.__init__).parameters["max_grad_norm"]
        assert prm.default is None, cls


def test_signatures_hold_the_three_entry_points_with_the_headers_arity():
    text = open(os.path.join(ROOT, "include", "inpaintnet_hip.h")).read()
    for name in ("inet_sqnorm_parts", "inet_grad_sqnorm", "inet_adam_step_clip"):
        proto = re.search(r"^(\w+)\s+%s\(([^)]*)\);" % name, text, re.M)
        assert proto, name
        args = proto.group(2).strip()
        arity = 0 if args == "void" else len(args.split(","))
        res, argtypes = _lib._SIGNATURES[name]
        assert len(argtypes) == arity, (name, arity, len(argtypes))
        assert res is _lib.C.c_int and proto.group(1) == "int"
        assert name in _lib.EXPORTS
    floats = [i for i, t in enumerate(_lib._SIGNATURES["inet_adam_step_clip"][1]) if t is _lib.C.c_float]
    assert floats == [5, 6, 7, 8, 10, 11]                                       # lr, beta1, beta2, eps, gscale, max_norm
