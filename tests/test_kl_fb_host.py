"""KL warm-up and free bits without a GPU: the float64 restatement (tests/kl_fb_ref.py) against torch autograd,
the condition the GPU test's inputs must meet (no part within its error bound of the threshold), beta_at for the three schedules,
the VAETrainer keywords' validation, the training-state round trip, and the binding of the new entries against the header."""
import ast
import ctypes as C
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

from inpaintnet_amd import _lib
from tests import kl_fb_ref as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# =============================================================================== 1. the restatement
@pytest.mark.parametrize("per", K.PER)
@pytest.mark.parametrize("shape", [(3, 5), (37, 64), (65, 257)])
def test_restatement_agrees_with_torch_autograd(shape, per):
    """loss = sum(dz * z) + k * clamp(parts, min=thr).sum() in float64 torch; its gradients against backward(), its value of the
    clamp sum against forward()['floored'].  The inputs are the GPU test's: off the ties (case()['margin'] > 0), so the clamp's
    subgradient at a tie does not come into it.  Both sides are float64: 1e-12 of the largest magnitude."""
    rows, Z = shape
    c = K.case(rows, Z, per)
    assert c["margin"] > 0.0
    mu = torch.from_numpy(c["mu"]).double().requires_grad_(True)
    ls = torch.from_numpy(c["ls"]).double().requires_grad_(True)
    eps, dz = torch.from_numpy(c["eps"]).double(), torch.from_numpy(c["dz"]).double()
    kscale, kdev = 0.031, 0.75
    k = float(np.float32(kscale) * np.float32(kdev))
    s = ls.exp()
    z = mu + eps * s
    parts = (0.5 * (s * s + mu * mu - 1.0) - ls).sum(1 if per == "measure" else 0)
    thr = K.threshold(rows, c["free_nats"], per)
    floored = torch.clamp(parts, min=thr).sum()
    ((dz * z).sum() + k * floored).backward()
    floored, parts, z = floored.detach(), parts.detach(), z.detach()
    f = K.forward(c["mu"], c["ls"], c["eps"], c["free_nats"], per)
    assert 0 < int(f["keep"].sum()) < f["keep"].size                             # some kept, some floored
    assert abs(f["floored"] - float(floored)) <= 1e-12 * abs(float(floored))
    assert abs(f["raw"] - float(parts.sum())) <= 1e-12 * abs(float(parts.sum()))
    assert np.abs(f["z"] - z.numpy()).max() <= 1e-12
    dmu, dls = K.backward(c["dz"], c["mu"], c["ls"], c["eps"], kscale, kdev, f["keep"], per)
    assert np.abs(dmu - mu.grad.numpy()).max() <= 1e-12 * np.abs(dmu).max()
    assert np.abs(dls - ls.grad.numpy()).max() <= 1e-12 * np.abs(dls).max()


def test_restatement_tie_nan_and_null_rules():
    mu = np.zeros((2, 2), np.float32)
    ls = np.zeros((2, 2), np.float32)
    mu[0, 0] = 1.0                                                               # KL = 0.5 exactly; every other element 0
    for per in K.PER:
        lam = 0.5 if per == "measure" else 0.25                                  # thr = 0.5 in both modes: a tie
        f = K.forward(mu, ls, None, lam, per)
        assert f["thr"] == 0.5 and not f["keep"].any()                           # a tie is floored
        assert f["floored"] == 1.0 and f["raw"] == 0.5 and np.array_equal(f["z"], mu.astype(np.float64))
        dmu, dls = K.backward(None, mu, ls, None, 2.0, None, f["keep"], per)
        assert not dmu.any() and not dls.any()                                   # nothing kept, no dz: no gradient at all
        f = K.forward(mu, ls, None, 0.0, per)
        assert f["keep"].tolist() == [True, False] and f["floored"] == f["raw"] == 0.5
        bad = mu.copy()
        bad[1, 1] = np.nan
        f = K.forward(bad, ls, None, lam, per)
        assert f["keep"].tolist() == [False, True] and math.isnan(f["floored"]) and math.isnan(f["raw"])
        dmu, _ = K.backward(None, bad, ls, None, 2.0, None, f["keep"], per)
        assert math.isnan(dmu[1, 1]) and dmu[0, 0] == 0.0


@pytest.mark.parametrize("per", K.PER)
@pytest.mark.parametrize("shape", K.SHAPES)
def test_gpu_cases_keep_every_part_off_its_threshold(shape, per):
    """The condition tests/test_gpu_kl_fb.py asserts again on the device's side: no reference part lies within its float32 error bound
    of the threshold, so the kernel's keep vector must EQUAL the reference's.  Checked here for every shape of that test."""
    c = K.case(*shape, per)
    f = K.forward(c["mu"], c["ls"], c["eps"], c["free_nats"], per)
    print(f"{per} {shape}: free_nats {c['free_nats']:.6g} thr {f['thr']:.6g} kept {int(f['keep'].sum())}/{f['keep'].size} "
          f"margin {c['margin']:.3g}")
    assert c["margin"] > 0.0
    if f["keep"].size > 1:
        assert 0 < int(f["keep"].sum()) < f["keep"].size


def test_depth_restates_the_launch_constants():
    """kl_fb_ref.depth() and SHAPES' last row count are derived from the launchers' grid caps: the constants here and in
    csrc/latent.hip must be the same numbers."""
    src = open(os.path.join(ROOT, "inpaintnet_amd", "csrc", "latent.hip")).read()
    assert int(re.search(r"constexpr int kFbMeasureGrid = (\d+);", src).group(1)) == K.MEASURE_GRID
    assert int(re.search(r"constexpr int kFbDimGrid = (\d+);", src).group(1)) == K.DIM_GRID
    rows = K.SHAPES[-1][0]
    assert K.MEASURE_PASS < rows < 2 * K.MEASURE_PASS and rows % 4 != 0 and rows > 2 * K.DIM_PASS


# =============================================================================== 2. the trainer's keywords
class _Untouchable:
    def __getattr__(self, name):
        raise AssertionError(f"the model was touched ({name}) before the keywords were checked")


class _HostModel:
    def __init__(self, n=8):
        self.flat = torch.arange(n, dtype=torch.float32)
        self.grad = torch.zeros(n)
        self._table = None
        self.free_bits = None


def _trainer(model=None, **kw):
    from inpaintnet_amd.vae_trainer import VAETrainer
    return VAETrainer(None, model or _HostModel(), **kw)


@pytest.fixture(autouse=True)
def _no_gc_freeze(monkeypatch):
    monkeypatch.setenv("INET_GC_FREEZE", "0")


def test_beta_at_three_schedules():
    tr = _trainer()
    assert all(tr.beta_at(t) == 0.001 for t in (0, 1, 7, 10 ** 9))              # the default: the reference's constant, exactly
    assert _trainer(kl_beta=0.25).beta_at(12345) == 0.25 and _trainer(kl_beta=0).beta_at(3) == 0.0
    tr = _trainer(kl_beta=0.5, kl_warmup_steps=10)
    assert tr.beta_at(0) == 0.0 and tr.beta_at(1) == 0.05 and tr.beta_at(5) == 0.25
    assert tr.beta_at(10) == 0.5 and tr.beta_at(11) == 0.5 and tr.beta_at(10 ** 9) == 0.5      # the ramp's end, and beyond
    tr = _trainer(kl_beta=0.5, kl_cycle_steps=8, kl_ramp=0.5)                    # ramp over 4 steps, hold for 4
    assert [tr.beta_at(t) for t in range(9)] == [0.0, 0.125, 0.25, 0.375, 0.5, 0.5, 0.5, 0.5, 0.0]
    assert tr.beta_at(8 * 10 ** 8) == 0.0 and tr.beta_at(8 * 10 ** 8 + 2) == 0.25 and tr.beta_at(8 * 10 ** 8 + 7) == 0.5
    tr = _trainer(kl_beta=0.5, kl_cycle_steps=8, kl_ramp=1.0)                    # a saw tooth: never holds
    assert tr.beta_at(7) == 0.4375 and tr.beta_at(8) == 0.0 and tr.beta_at(16) == 0.0
    tr = _trainer(kl_beta=1.0, kl_cycle_steps=10, kl_ramp=0.25)                  # a ramp end between two steps: 2.5
    assert tr.beta_at(2) == 0.8 and tr.beta_at(3) == 1.0


@pytest.mark.parametrize("kw", [{"kl_beta": -1e-9}, {"kl_beta": float("nan")}, {"kl_beta": math.inf},
                                {"kl_warmup_steps": -1}, {"kl_warmup_steps": 2.5}, {"kl_warmup_steps": True},
                                {"kl_cycle_steps": -3}, {"kl_cycle_steps": 4.0},
                                {"kl_warmup_steps": 5, "kl_cycle_steps": 5},
                                {"kl_ramp": 0.0}, {"kl_ramp": -0.5}, {"kl_ramp": 1.5}, {"kl_ramp": float("nan")},
                                {"free_nats": -0.1}, {"free_nats": float("nan")}, {"free_nats": math.inf},
                                {"free_nats_per": "row"}, {"free_nats_per": None}, {"free_nats_per": 0}])
def test_trainer_rejects_bad_keywords_before_touching_the_model(kw):
    with pytest.raises(ValueError, match="kl_beta|kl_warmup_steps|kl_cycle_steps|kl_ramp|free_nats"):
        _trainer(_Untouchable(), **kw)


def test_defaults_and_zero_free_nats_leave_the_model_alone():
    from inpaintnet_amd.vae_trainer import VAETrainer
    prm = inspect.signature(VAETrainer.__init__).parameters
    assert [prm[k].default for k in VAETrainer.KL_SETTINGS] == [0.001, 0, 0, 0.5, 0.0, "measure"]
    assert inspect.signature(VAETrainer.compute_kld_loss).parameters["beta"].default == 0.001
    for kw in ({}, {"free_nats": 0}, {"free_nats": 0.0, "free_nats_per": "dim"}, {"kl_warmup_steps": 100}):
        tr = _trainer(**kw)
        assert tr.model.free_bits is None and tr.last_kl is None
    for per in K.PER:
        tr = _trainer(free_nats=2, free_nats_per=per)
        assert tr.model.free_bits == (2.0, per) and tr.last_kl is None


def test_training_state_round_trip_carries_the_six_settings():
    a = _trainer(kl_beta=0.02, kl_cycle_steps=50, kl_ramp=0.25, free_nats=3.0, free_nats_per="dim")
    st = a.training_state(4)
    assert {k: st[k] for k in a.KL_SETTINGS} == dict(kl_beta=0.02, kl_warmup_steps=0, kl_cycle_steps=50, kl_ramp=0.25,
                                                     free_nats=3.0, free_nats_per="dim")
    b = _trainer()
    assert b.load_training_state(st) == 4
    assert [getattr(b, k) for k in b.KL_SETTINGS] == [getattr(a, k) for k in a.KL_SETTINGS]
    assert b.model.free_bits == (3.0, "dim") and b.beta_at(5) == a.beta_at(5)
    c = _trainer(free_nats=1.0)                                                  # loading a run without a floor takes it off the model
    c.load_training_state(_trainer(kl_warmup_steps=7).training_state())
    assert c.model.free_bits is None and c.kl_warmup_steps == 7 and c.free_nats == 0.0
    # a state written before the settings existed still loads and leaves this trainer's own
    old = {k: v for k, v in a.training_state(2).items() if k not in a.KL_SETTINGS}
    d = _trainer(kl_beta=0.5, free_nats=1.5)
    assert d.load_training_state(old) == 2
    assert d.kl_beta == 0.5 and d.free_nats == 1.5 and d.model.free_bits == (1.5, "measure")


# =============================================================================== 3. the binding
def test_binding_has_the_headers_arity_and_types():
    text = open(os.path.join(ROOT, "include", "inpaintnet_hip.h")).read()
    want = {"inet_reparam_kl_fb_ws_bytes": ("int64_t", 3), "inet_reparam_kl_fb": ("int", 15), "inet_latent_bwd_fb": ("int", 13)}
    from tests.test_integration_doc import quoted_argtypes
    quoted = dict(quoted_argtypes())
    for name, (res, arity) in want.items():
        proto = re.search(r"^(\w+)\s+%s\(([^)]*)\);" % name, text, re.M)
        assert proto and proto.group(1) == res, name
        params = [p.strip() for p in proto.group(2).split(",")]
        assert len(params) == arity, name
        r, argtypes = _lib._SIGNATURES[name]
        assert r is (C.c_int64 if res == "int64_t" else C.c_int) and len(argtypes) == arity and name in _lib.EXPORTS
        for prm, t in zip(params, argtypes):                                     # type by type against the prototype
            if "*" in prm:
                assert t is C.c_void_p, (name, prm)
            elif prm.startswith("int64_t"):
                assert t is C.c_int64, (name, prm)
            elif prm.startswith("float"):
                assert t is C.c_float, (name, prm)
            else:
                assert prm.startswith("int ") and t is C.c_int, (name, prm)
        assert name in quoted and [C.sizeof(t) for t in quoted[name]] == [C.sizeof(t) for t in argtypes], name
    from inpaintnet_amd import ops
    for fn, name in ((ops.reparam_kl_fb, "inet_reparam_kl_fb"), (ops.latent_bwd_fb, "inet_latent_bwd_fb")):
        calls = [n for n in ast.walk(ast.parse(inspect.getsource(fn)))
                 if isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute) and n.func.attr == name]
        assert len(calls) == 1 and len(calls[0].args) == want[name][1]
    assert ops.FB_PER == {"measure": 0, "dim": 1}


@pytest.fixture(scope="module")
def L():
    _lib.build(verbose=False)
    return _lib.lib()


X = C.c_void_p(16)                     # a pointer that is never followed: every call below is refused in front of the launch
NULL = None


def test_entries_refuse_bad_arguments_before_any_launch(L):
    fwd = lambda mu=X, ls=X, rows=4, Z=4, lam=1.0, per=0, parts=X, keep=X, kl=X, raw=X, ws=X, nb=1 << 20: \
        L.inet_reparam_kl_fb(mu, ls, X, X, rows, Z, lam, per, parts, keep, kl, raw, ws, nb, NULL)
    bwd = lambda mu=X, ls=X, keep=X, per=0, dmu=X, dls=X, rows=4, Z=4: \
        L.inet_latent_bwd_fb(X, mu, ls, X, 1.0, NULL, keep, per, dmu, dls, rows, Z, NULL)
    calls = {
        "fwd mu": fwd(mu=NULL), "fwd logsigma": fwd(ls=NULL), "fwd parts": fwd(parts=NULL), "fwd keep": fwd(keep=NULL),
        "fwd kl_sum": fwd(kl=NULL), "fwd kl_raw": fwd(raw=NULL), "fwd rows": fwd(rows=0), "fwd rows<0": fwd(rows=-2),
        "fwd Z": fwd(Z=0), "fwd Z<0": fwd(Z=-1), "fwd free_nats<0": fwd(lam=-1e-6), "fwd free_nats nan": fwd(lam=float("nan")),
        "fwd free_nats inf": fwd(lam=math.inf), "fwd per 2": fwd(per=2), "fwd per -1": fwd(per=-1),
        "fwd dim without ws": fwd(per=1, ws=NULL), "fwd dim small ws": fwd(per=1, nb=15),
        "bwd mu": bwd(mu=NULL), "bwd logsigma": bwd(ls=NULL), "bwd keep": bwd(keep=NULL), "bwd dmu": bwd(dmu=NULL),
        "bwd dlogsigma": bwd(dls=NULL), "bwd rows": bwd(rows=0), "bwd Z": bwd(Z=0), "bwd per": bwd(per=2),
    }
    assert {k: v for k, v in calls.items() if v != -1} == {}
    assert L.inet_reparam_kl_fb_ws_bytes(0, 4, 1) == -1 and L.inet_reparam_kl_fb_ws_bytes(4, 0, 1) == -1
    assert L.inet_reparam_kl_fb_ws_bytes(4, 4, 2) == -1
    assert L.inet_reparam_kl_fb_ws_bytes(4096, 256, 0) == 0                      # 'measure' needs no workspace
    # 'dim': one row of Z floats per workgroup of the first launch, min(ceil(rows / 4), DIM_GRID) of them
    assert L.inet_reparam_kl_fb_ws_bytes(4096, 256, 1) == K.DIM_GRID * 256 * 4
    assert L.inet_reparam_kl_fb_ws_bytes(5, 3, 1) == 2 * 3 * 4 and L.inet_reparam_kl_fb_ws_bytes(1, 1, 1) == 4
