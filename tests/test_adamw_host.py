"""Decoupled weight decay and EMA shadow weights without a GPU: the float64 restatement of the rule (tests/adamw_ref.py) against
torch.optim.AdamW and against the EMA's closed form, the Trainer keywords' validation, the decay mask built from a parameter table,
and the binding of inet_adam_step_w against the header."""
import ast
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

from inpaintnet_amd import _lib
from tests import adamw_ref as AR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (5, 1000, 37)                   # an arena split into three tensors of unequal size
LR, B1, B2, EPS, WD = (float(np.float32(x)) for x in (1e-3, 0.9, 0.999, 1e-8, 0.01))     # what the ABI's `float` arguments hold


def _grads(step):
    g = torch.Generator().manual_seed(300 + step)
    return (torch.randn(sum(SIZES), generator=g) * 3.0).float()


@pytest.mark.parametrize("masked", [False, True])
def test_restatement_agrees_with_torch_adamw(masked):
    """Three steps of torch.optim.AdamW on float64 CPU tensors against three steps of the restatement; masked: two param groups,
    weight_decay for the first and the third tensor and 0 for the second, against the restatement's bool mask.

    torch multiplies by the float64 1 - lr * wd; the rule rounds that factor to float32 once on the host.  So torch is compared with
    the restatement's round_decay=False form, within 1e-12 relative (both float64), and the rounded form may differ from it by what
    one float32 rounding of the factor can do: the factor lies just below 1, its rounding moves it by at most 2^-24, so one step moves
    a decaying parameter by at most 2^-24 |p|; the update term does not read p and the next step multiplies the difference by
    decay < 1, so three steps stay below 3 * 2^-24 * max_t |p_t| per element.  Measured: torch vs restatement 1.8e-16 / 2.1e-16
    relative (all / masked); the float32 factor moves p by at most 4.1e-08 / 4.1e-08 of |p| (bound 1.8e-07)."""
    g0 = torch.Generator().manual_seed(11)
    p0 = torch.randn(sum(SIZES), generator=g0).double()
    params = [torch.nn.Parameter(t.clone()) for t in p0.split(SIZES)]
    if masked:
        groups = [{"params": [params[0], params[2]], "weight_decay": WD}, {"params": [params[1]], "weight_decay": 0.0}]
        mask = AR.mask_from_ranges(sum(SIZES), [(0, SIZES[0]), (SIZES[0] + SIZES[1], sum(SIZES))])
    else:
        groups, mask = [{"params": params, "weight_decay": WD}], None
    opt = torch.optim.AdamW(groups, lr=LR, betas=(B1, B2), eps=EPS)
    exact = [p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)]
    rounded = [t.clone() for t in exact]
    pmax = p0.abs()
    for step in (1, 2, 3):
        g = _grads(step)
        for prm, part in zip(params, g.double().split(SIZES)):
            prm.grad = part.clone()
        opt.step()
        out = AR.adamw_ref(exact[0], g, exact[1], exact[2], LR, step, WD, mask, b1=B1, b2=B2, eps=EPS, round_decay=False)
        exact = list(out[:3])
        out_r = AR.adamw_ref(rounded[0], g, rounded[1], rounded[2], LR, step, WD, mask, b1=B1, b2=B2, eps=EPS)
        rounded = list(out_r[:3])
        assert out[4] == out_r[4] == [1, 0, 0, 0, 0, 0, 0, 0]
        pmax = torch.maximum(pmax, torch.maximum(exact[0].abs(), rounded[0].abs()))
    got = torch.cat([prm.detach().reshape(-1) for prm in params])
    rel = float(((got - exact[0]).abs() / exact[0].abs()).max())
    drift = (rounded[0] - exact[0]).abs()
    print(f"masked {masked}: torch vs restatement {rel:.2e} relative; the float32 factor moves p by at most "
          f"{float((drift / pmax).max()):.2e} of |p| (bound {3 * 2.0 ** -24:.2e})")
    assert rel <= 1e-12
    assert bool((drift <= 3 * 2.0 ** -24 * pmax).all())
    assert float(drift.max()) > 0.0                                             # (lr * wd = 1e-5: the rounding is there to be seen)
    if masked:
        assert torch.equal(rounded[0][~mask], exact[0][~mask])                  # no decay: no factor to round
        plain = AR.adamw_ref(p0, _grads(1), torch.zeros_like(p0), torch.zeros_like(p0), LR, 1, 0.0, None, b1=B1, b2=B2, eps=EPS)
        first = AR.adamw_ref(p0, _grads(1), torch.zeros_like(p0), torch.zeros_like(p0), LR, 1, WD, mask, b1=B1, b2=B2, eps=EPS)
        assert torch.equal(first[0][~mask], plain[0][~mask]) and not torch.equal(first[0][mask], plain[0][mask])


def test_no_decay_is_adam():
    from tests import pointwise_ref as R
    p, m, v, g = torch.randn(9).double(), torch.rand(9).double(), torch.rand(9).double(), torch.randn(9)
    assert AR.decay_factor(LR, 0.0) == 1.0
    out = AR.adamw_ref(p, g, m, v, LR, 4, 0.0)
    for a, b in zip(out[:3], R.adam_ref(p, g, m, v, LR, 4)):
        assert torch.equal(a, b)
    assert out[3] is None


@pytest.mark.parametrize("d", [0.9, 0.999, 0.0])
def test_ema_follows_the_closed_form(d):
    """e_T = d^T e_0 + omd * sum_k d^(T-k) p_k over five steps in float64, d and omd = (float)(1 - d) the float32 values of the rule."""
    gen = torch.Generator().manual_seed(5)
    p, m, v = torch.randn(50, generator=gen).double(), torch.zeros(50).double(), torch.zeros(50).double()
    e0 = torch.randn(50, generator=gen).double()
    e, ps = e0.clone(), []
    for step in range(1, 6):
        p, m, v, e, rep, _ = AR.adamw_ref(p, _grads(step)[:50], m, v, LR, step, WD, ema=e, ema_decay=d)
        ps.append(p)
    df, omd = AR.f32(d), AR.one_minus(d)
    closed = df ** 5 * e0 + omd * sum(df ** (5 - k) * ps[k - 1] for k in range(1, 6))
    assert float((e - closed).abs().max()) <= 1e-12 * float(closed.abs().max())
    if d == 0.0:
        assert torch.equal(e, p)                                                # omd = 1: the EMA is the weights


def test_warmup_schedule():
    assert AR.warmup_decay(0.999, 1) == 2.0 / 11.0
    assert AR.warmup_decay(0.999, 2) == 3.0 / 12.0
    assert AR.warmup_decay(0.999, 100) == 101.0 / 110.0
    assert AR.warmup_decay(0.9, 100) == 0.9 and AR.warmup_decay(0.1, 1) == 0.1
    tr = _trainer_class()(None, _HostModel(), ema_decay=0.999, ema_warmup=True)
    for t in (1, 2, 100, 100000):
        assert tr.ema_decay_at(t) == AR.warmup_decay(0.999, t)
    assert _trainer_class()(None, _HostModel(), ema_decay=0.999).ema_decay_at(1) == 0.999


def test_restatement_skips_and_drops_leave_the_ema_alone():
    p, m, v, e = torch.randn(9).double(), torch.rand(9).double(), torch.rand(9).double(), torch.randn(9).double()
    g = torch.randn(9)
    for max_norm in (None, 1.0):
        out = AR.adamw_ref(p, g, m, v, LR, 2, WD, ema=e, ema_decay=0.9, max_norm=max_norm, skip=True)
        assert out[4] == [1, 1, 0, 0, 0, 0, 0, 0] and all(torch.equal(a, b) for a, b in zip(out[:4], (p, m, v, e)))
    for bad in (float("inf"), float("-inf"), float("nan")):
        gb = g.clone()
        gb[4] = bad
        out = AR.adamw_ref(p, gb, m, v, LR, 2, WD, ema=e, ema_decay=0.9, max_norm=1.0)
        assert out[4] == [1, 0, 0, 0, 0, 1, 0, 0] and not math.isfinite(out[5])
        assert all(torch.equal(a, b) for a, b in zip(out[:4], (p, m, v, e)))
    out = AR.adamw_ref(p, g, m, v, LR, 2, WD, ema=e, ema_decay=0.9)
    assert not torch.equal(out[3], e) and not torch.equal(out[0], p)


class _Untouchable:
    """A model no attribute of which may be read."""

    def __getattr__(self, name):
        raise AssertionError(f"the model was touched ({name}) before the keywords were checked")


class _HostModel:
    def __init__(self, table=None, n=8):
        self.flat = torch.arange(n, dtype=torch.float32)
        self.grad = torch.zeros(n)
        self._table = table


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


@pytest.mark.parametrize("kw", [{"weight_decay": -1.0}, {"weight_decay": -1e-9}, {"weight_decay": float("nan")},
                                {"weight_decay": math.inf}, {"weight_decay": -math.inf},
                                {"ema_decay": -0.1}, {"ema_decay": 1.0}, {"ema_decay": 1.5}, {"ema_decay": float("nan")},
                                {"ema_warmup": True}, {"ema_warmup": True, "ema_decay": None}])
def test_trainer_rejects_bad_keywords_before_touching_the_model(kw, monkeypatch):
    monkeypatch.setenv("INET_GC_FREEZE", "0")
    with pytest.raises(ValueError, match="weight_decay|ema_decay"):
        _trainer_class()(None, _Untouchable(), **kw)


@pytest.mark.parametrize("kw", [{}, {"weight_decay": 0}, {"weight_decay": 0.0, "ema_decay": None}, {"ema_decay": 0},
                                {"ema_decay": 0.999, "ema_warmup": True}, {"weight_decay": 0.01, "decay_all": True}])
def test_trainer_accepts_none_zero_and_the_defaults(kw, monkeypatch):
    monkeypatch.setenv("INET_GC_FREEZE", "0")
    model = _HostModel()
    tr = _trainer_class()(None, model, **kw)
    assert tr.weight_decay == float(kw.get("weight_decay", 0.0)) and tr.decay_all == kw.get("decay_all", False)
    assert tr.ema_decay == kw.get("ema_decay") and tr.ema_warmup == kw.get("ema_warmup", False)
    assert tr._decay_mask is None                                               # nothing decays, or everything does
    if kw.get("ema_decay") is None:
        assert tr.ema is None
    else:
        assert torch.equal(tr.ema, model.flat) and tr.ema.data_ptr() != model.flat.data_ptr()
    st = tr.training_state()
    assert {"weight_decay", "decay_all", "ema_decay", "ema_warmup", "ema"} <= set(st)


def test_subclass_trainers_take_the_keywords():
    from inpaintnet_amd.arnn import AnticipationRNNBaselineTrainer, AnticipationRNNGaussianRegTrainer
    from inpaintnet_amd.latent_rnn_trainer import LatentRNNTrainer
    from inpaintnet_amd.trainer import Trainer
    from inpaintnet_amd.vae_trainer import VAETrainer
    for cls in (Trainer, VAETrainer, LatentRNNTrainer, AnticipationRNNGaussianRegTrainer, AnticipationRNNBaselineTrainer):
        prm = inspect.signature(cls.__init__).parameters
        assert prm["weight_decay"].default == 0.0 and prm["decay_all"].default is False, cls
        assert prm["ema_decay"].default is None and prm["ema_warmup"].default is False, cls


# offsets and sizes that are no multiples of 4 or 32: ranges begin and end inside mask words
TABLE = [("emb.weight", 0, (3, 7)), ("enc.bias", 21, (5,)), ("enc.weight_ih_l0", 26, (9, 5)), ("enc.bias_ih_l0", 71, (9,)),
         ("b_0", 80, (1, 13)), ("x_0", 93, (2, 1, 3)), ("out.weight", 99, (11, 3)), ("weight_vec", 132, (6,)), ("out.bias", 138, (11,))]
TABLE_N = 149


def _rule_bits(table, n):
    """The name / shape rule applied element by element, independently of pack_decay_mask: -> the words as Python ints."""
    words = [0] * ((n + 31) // 32)
    for name, off, shape in table:
        if "weight" in name and len(shape) == 2:
            for i in range(off, off + shape[0] * shape[1]):
                words[i >> 5] |= 1 << (i & 31)
    return words


def test_pack_decay_mask_follows_the_bit_convention():
    from inpaintnet_amd import ops
    ranges = [(0, 21), (26, 71), (99, 132)]
    got = ops.pack_decay_mask(TABLE_N, ranges, device="cpu")
    assert got.dtype == torch.int32 and got.numel() == 5
    assert [int(w) & 0xffffffff for w in got.tolist()] == _rule_bits(TABLE, TABLE_N)
    assert ops.pack_decay_mask(33, [], device="cpu").tolist() == [0, 0]
    assert [w & 0xffffffff for w in ops.pack_decay_mask(33, [(0, 33)], device="cpu").tolist()] == [0xffffffff, 1]
    assert [w & 0xffffffff for w in ops.pack_decay_mask(64, [(31, 33)], device="cpu").tolist()] == [0x80000000, 1]
    with pytest.raises(ValueError):
        ops.pack_decay_mask(10, [(5, 11)], device="cpu")


def test_trainer_builds_the_mask_from_the_table_once(monkeypatch):
    monkeypatch.setenv("INET_GC_FREEZE", "0")
    model = _HostModel(TABLE, TABLE_N)
    tr = _trainer_class()(None, model, weight_decay=0.01)
    assert [int(w) & 0xffffffff for w in tr._decay_mask.tolist()] == _rule_bits(TABLE, TABLE_N)
    # b_0 (two dimensions, no "weight"), weight_vec ("weight", one dimension), biases and x_0 do not decay
    bits = _rule_bits(TABLE, TABLE_N)
    for i in list(range(21, 26)) + list(range(71, 99)) + list(range(132, 149)):
        assert not (bits[i >> 5] >> (i & 31)) & 1
    assert _trainer_class()(None, _HostModel(TABLE, TABLE_N), weight_decay=0.01, decay_all=True)._decay_mask is None
    assert _trainer_class()(None, _HostModel(TABLE, TABLE_N))._decay_mask is None


def test_training_state_round_trip_on_the_host(monkeypatch, capsys):
    monkeypatch.setenv("INET_GC_FREEZE", "0")
    T = _trainer_class()
    a = T(None, _HostModel(TABLE, TABLE_N), weight_decay=0.02, ema_decay=0.99, ema_warmup=True)
    a.ema.mul_(3.0)
    b = T(None, _HostModel(TABLE, TABLE_N))
    b.load_training_state(a.training_state(4))
    assert (b.weight_decay, b.decay_all, b.ema_decay, b.ema_warmup, b.start_epoch) == (0.02, False, 0.99, True, 4)
    assert torch.equal(b.ema, a.ema) and torch.equal(b._decay_mask, a._decay_mask)
    old = {k: v for k, v in a.training_state().items() if k not in ("weight_decay", "decay_all", "ema_decay", "ema_warmup", "ema")}
    c = T(None, _HostModel(TABLE, TABLE_N), ema_decay=0.9)
    c.ema.zero_()
    c.load_training_state(old)
    assert torch.equal(c.ema, c.model.flat) and c.ema_decay == 0.9
    assert "seeded" in capsys.readouterr().out


def test_binding_has_the_headers_arity():
    text = open(os.path.join(ROOT, "include", "inpaintnet_hip.h")).read()
    proto = re.search(r"^(\w+)\s+inet_adam_step_w\(([^)]*)\);", text, re.M)
    assert proto and proto.group(1) == "int"
    arity = len(proto.group(2).split(","))
    assert arity == 20
    res, argtypes = _lib._SIGNATURES["inet_adam_step_w"]
    assert res is _lib.C.c_int and len(argtypes) == arity and "inet_adam_step_w" in _lib.EXPORTS
    # lr, beta1, beta2, eps, gscale, max_norm, weight_decay, ema_decay are the floats; n the int64; step the int
    assert [i for i, t in enumerate(argtypes) if t is _lib.C.c_float] == [5, 6, 7, 8, 10, 11, 13, 16]
    assert argtypes[4] is _lib.C.c_int64 and argtypes[9] is _lib.C.c_int
    assert all(argtypes[i] is _lib.C.c_void_p for i in (0, 1, 2, 3, 12, 14, 15, 17, 18, 19))
    # the ops layer passes that many arguments ...
    from inpaintnet_amd import ops
    calls = [n for n in ast.walk(ast.parse(inspect.getsource(ops.adamw_step)))
             if isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute) and n.func.attr == "inet_adam_step_w"]
    assert len(calls) == 1 and len(calls[0].args) == arity
    # ... and INTEGRATION.md quotes the same list
    from tests.test_integration_doc import quoted_argtypes
    quoted = dict(quoted_argtypes())
    assert "inet_adam_step_w" in quoted and len(quoted["inet_adam_step_w"]) == arity
    assert [_lib.C.sizeof(t) for t in quoted["inet_adam_step_w"]] == [_lib.C.sizeof(t) for t in argtypes]
    assert [i for i, t in enumerate(quoted["inet_adam_step_w"]) if t is _lib.C.c_float] == [5, 6, 7, 8, 10, 11, 13, 16]
    assert _lib.lib is not None and "INET_ABI_VERSION 1" in re.sub(r"\s+", " ", text)
