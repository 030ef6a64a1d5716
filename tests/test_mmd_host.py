"""The MMD latent loss without a GPU: the float64 restatement (tests/mmd_ref.py) against what the reference's
own compute_mmd_loss returned (tests/golden/mmd_reference.npz), the two quirks of the reference's rule, the conditions the GPU test's
inputs and bounds must meet, the binding of the new entries against the header, the entry's refusals, and the VAETrainer keywords."""
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
from tests import mmd_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# =============================================================================== 1. the restatement
def test_restatement_reproduces_the_references_own_numbers():
    g = np.load(os.path.join(ROOT, "tests", "golden", "mmd_reference.npz"))
    assert [tuple(c) for c in g["cases"]] == [(1, 5), (2, 5), (37, 16), (16, 256)] and int(g["coeff"]) == 10
    for B, Z in g["cases"]:
        key = f"{B}x{Z}"
        x, y = M.inputs(int(B), int(Z))
        assert np.array_equal(x, g[key + "/z_tilde"]) and np.array_equal(y, g[key + "/z_prior"])
        e = M.evaluate(x, y, "gaussian", 16.0, "reference", 10)
        want, wgrad = float(g[key + "/value"]), g[key + "/grad"]
        assert wgrad.dtype == np.float64 and wgrad.shape == (B, Z)
        assert abs(e["value"] - want) <= 1e-13 * max(abs(want), e["scale"])
        assert np.abs(e["grad"] - wgrad).max() <= 1e-13 * max(np.abs(wgrad).max(), 1e-300) + 1e-18


@pytest.mark.parametrize("estimator", M.ESTIMATORS)
@pytest.mark.parametrize("kind", M.KERNELS)
def test_blockwise_sums_agree_with_the_value_written_out_whole(kind, estimator):
    """evaluate() adds the sums 32 rows at a time and combines autograd's gradients of the sums; value_autograd() is ONE expression
    with one backward pass.  (37, 16): two ragged blocks."""
    x, y = M.inputs(37, 16)
    e = M.evaluate(x, y, kind, 24.0, estimator, 3.0)
    value, grad = M.value_autograd(x, y, kind, 24.0, estimator, 3.0)
    assert abs(e["value"] - value) <= 1e-13 * e["scale"]
    assert np.abs(e["grad"] - grad).max() <= 1e-13 * np.abs(grad).max()


def test_the_references_rule_is_negative_for_one_distribution_and_unbiased_is_not():
    """The quirk of the reference's coefficients (1/2 on each self term against 2 on the cross term): for two samples of ONE
    distribution its value is far below zero, while the unbiased estimator's is within sampling noise of zero.  B = 256, Z = 16,
    bandwidth 2 Z; the U-statistic's standard deviation under H0 is of the order sqrt(2) E[k^2]^(1/2) / B < 1 / B."""
    B, Z = 256, 16
    rng = np.random.RandomState(5)
    x, y = rng.randn(B, Z).astype(np.float32), rng.randn(B, Z).astype(np.float32)
    for kind in M.KERNELS:
        u = M.evaluate(x, y, kind, 2.0 * Z, "unbiased", 1.0, key=("h0", kind))
        r = M.evaluate(x, y, kind, 2.0 * Z, "reference", 1.0, key=("h0", kind))
        b = M.evaluate(x, y, kind, 2.0 * Z, "biased", 1.0, key=("h0", kind))
        print(f"{kind}: unbiased {u['value']:.3g} biased {b['value']:.3g} reference {r['value']:.3g}")
        assert abs(u["value"]) <= 4.0 / B
        assert 0.0 <= b["value"] <= 4.0 / B                                      # the V-statistic is a squared norm: never negative
        assert r["value"] < -0.1                                                 # about -(mean off-diagonal k): nowhere near zero


def test_the_references_bandwidth_leaves_no_off_diagonal_terms_at_z_256():
    """The other quirk: var = 16 at Z = 256, where two N(0, 1) draws lie about 512 apart in squared distance."""
    B, Z = 64, 256
    rng = np.random.RandomState(6)
    x, y = rng.randn(B, Z).astype(np.float32), rng.randn(B, Z).astype(np.float32)
    e = M.evaluate(x, y, "gaussian", 16.0, "reference", 10.0)
    assert e["offdiag_share"] < 1e-6
    assert abs(e["value"] - 10.0 / (B - 1)) <= 1e-6                              # 10 / (B - 1): the diagonals alone
    assert np.abs(e["grad"]).max() < 1e-6
    assert M.evaluate(x, y, "gaussian", 2.0 * Z, "unbiased", 10.0)["offdiag_share"] > 0.9


@pytest.mark.parametrize("kind", M.KERNELS)
@pytest.mark.parametrize("B,Z,var", M.CASES)
def test_gpu_cases_meet_their_conditions(B, Z, var, kind):
    """What tests/test_gpu_mmd.py asserts again next to the device's numbers: from B = 16 on the off-diagonal pairs carry at least 0.9
    of S_xx, and the value's bound stays below 1e-4 of the magnitude of its three terms (Z <= 260) -- a few hundred u."""
    assert Z <= 260
    for estimator in M.ESTIMATORS:
        if B == 1 and estimator == "unbiased":
            continue
        _, _, v, e = M.case(B, Z, var, kind, estimator, 10.0)
        print(f"{kind} {estimator} ({B}, {Z}) var {v}: share {e['offdiag_share']:.3f} bound / scale {e['value_bound'] / e['scale']:.3g} "
              f"= {e['value_bound'] / e['scale'] / M.U:.0f} u; grad bound / max |g| {e['grad_bound'].max() / np.abs(e['grad']).max():.3g}")
        if B >= 16:
            assert e["offdiag_share"] >= 0.9
        assert 0.0 < e["value_bound"] <= 1e-4 * e["scale"]
        assert e["value_bound"] <= 400 * M.U * e["scale"]
        assert bool((e["grad_bound"] >= 0.0).all())
        # the gradient's bound is a bound, not a licence: below 1e-3 of the largest element everywhere
        assert e["grad_bound"].max() <= 1e-3 * np.abs(e["grad"]).max()


def test_case_list_covers_the_kernels_paths():
    shapes = {(B, Z) for B, Z, _ in M.CASES}
    for must in ((1, 1), (1, 256), (2, 5), (3, 5), (37, 16), (37, 64), (64, 63), (65, 257), (256, 256), (300, 256)):
        assert must in shapes
    assert (37, 16, 16.0) in M.CASES and (256, 256, 16.0) not in M.CASES        # the reference's var only where it hides nothing
    assert any(B == 2 * M.ROWS + 1 for B, _, _ in M.CASES)                       # one row past two row blocks
    assert any(B > M.TILE for B, _, _ in M.CASES) and any(Z > 256 for _, Z, _ in M.CASES) and any(Z % 32 for _, Z, _ in M.CASES)


def test_depths_restate_the_launch_constants():
    src = open(os.path.join(ROOT, "inpaintnet_amd", "csrc", "mmd.hip")).read()
    for name, want in (("kMmdRows", M.ROWS), ("kMmdTile", M.TILE), ("kMmdFinishBlock", M.FINISH), ("kMmdZc", 32), ("kMmdSpan", 256)):
        assert int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1)) == want, name
    assert "atomic" not in src.lower().replace("no float atomic", "")           # no atomics of any kind in the MMD kernels
    assert re.search(r"[^_\w]expf\(-d / var\)", src) and src.count("__expf") == 1       # (the one mention: the comment that says so)
    assert M.depth_s(256) == 3 + 1 + 9 + 1 + 9 and M.depth_s(4096) == 3 + 16 + 9 + 2 + 9 and M.depth_g(300) == 72


# =============================================================================== 2. the binding and the entry
def test_binding_has_the_headers_arity_and_types():
    text = open(os.path.join(ROOT, "include", "inpaintnet_hip.h")).read()
    want = {"inet_mmd_ws_bytes": ("int64_t", 2), "inet_mmd": ("int", 15)}
    from tests.test_integration_doc import quoted_argtypes
    quoted = dict(quoted_argtypes())
    for name, (res, arity) in want.items():
        proto = re.search(r"^(\w+)\s+%s\(([^)]*)\);" % name, text, re.M)
        assert proto and proto.group(1) == res, name
        params = [p.strip() for p in proto.group(2).split(",")]
        assert len(params) == arity, name
        r, argtypes = _lib._SIGNATURES[name]
        assert r is (C.c_int64 if res == "int64_t" else C.c_int) and len(argtypes) == arity and name in _lib.EXPORTS
        for prm, t in zip(params, argtypes):
            if "*" in prm:
                assert t is C.c_void_p, (name, prm)
            elif prm.startswith("int64_t"):
                assert t is C.c_int64, (name, prm)
            elif prm.startswith("float"):
                assert t is C.c_float, (name, prm)
            elif prm.startswith("double"):
                assert t is C.c_double, (name, prm)
            else:
                assert prm.startswith("int ") and t is C.c_int, (name, prm)
        assert name in quoted and [C.sizeof(t) for t in quoted[name]] == [C.sizeof(t) for t in argtypes], name
    from inpaintnet_amd import ops
    calls = [n for n in ast.walk(ast.parse(inspect.getsource(ops.mmd)))
             if isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute) and n.func.attr == "inet_mmd"]
    assert len(calls) == 1 and len(calls[0].args) == 15
    assert ops.MMD_KERNEL == {"gaussian": 0, "imq": 1} and ops.MMD_ESTIMATORS == M.ESTIMATORS
    assert "mmd.hip" in _lib.SOURCES


def test_ops_weights_are_the_restatements():
    from inpaintnet_amd import ops
    for B in (1, 2, 3, 37, 256, 4096):
        for est in M.ESTIMATORS:
            if B == 1 and est == "unbiased":
                with pytest.raises(ValueError, match="unbiased"):
                    ops.mmd_weights(B, est)
            else:
                assert ops.mmd_weights(B, est) == M.weights(B, est)
    assert ops.mmd_weights(1, "reference") == (1.0, 2.0, 0.0)
    with pytest.raises(ValueError):
        ops.mmd_weights(4, "u-statistic")


@pytest.fixture(scope="module")
def L():
    _lib.build(verbose=False)
    return _lib.lib()


X = C.c_void_p(16)                     # a pointer that is never followed: every call below is refused in front of the launch
NULL = None


def test_entry_refuses_bad_arguments_before_any_launch(L):
    call = lambda x=X, y=X, B=4, Z=4, kind=0, var=8.0, a=0.25, c=0.125, diag=0.0, coeff=1.0, out=X, grad=X, ws=X, nb=1 << 20: \
        L.inet_mmd(x, y, B, Z, kind, var, a, c, diag, coeff, out, grad, ws, nb, NULL)
    calls = {
        "x": call(x=NULL), "y": call(y=NULL), "out": call(out=NULL), "B 0": call(B=0), "B < 0": call(B=-3), "B > 2^24": call(B=(1 << 24) + 1),
        "Z 0": call(Z=0), "Z < 0": call(Z=-1), "var 0": call(var=0.0), "var < 0": call(var=-1.0), "var nan": call(var=float("nan")),
        "var inf": call(var=math.inf), "kind 2": call(kind=2), "kind -1": call(kind=-1), "ws null": call(ws=NULL),
        "ws small": call(nb=15), "ws 0": call(nb=0), "a nan": call(a=float("nan")), "c inf": call(c=math.inf),
        "coeff nan": call(coeff=float("nan")), "diag inf": call(diag=math.inf),
    }
    assert {k: v for k, v in calls.items() if v != -1} == {}
    assert L.inet_mmd_ws_bytes(0, 4) == -1 and L.inet_mmd_ws_bytes(4, 0) == -1 and L.inet_mmd_ws_bytes((1 << 24) + 1, 4) == -1
    # two floats per workgroup of the pair launch: ceil(B / ROWS) row blocks of x, as many of y
    assert L.inet_mmd_ws_bytes(4, 4) == 16 and L.inet_mmd_ws_bytes(256, 256) == 2 * 32 * 8
    assert L.inet_mmd_ws_bytes(4096, 256) == 2 * 512 * 8 and L.inet_mmd_ws_bytes(17, 1) == 2 * 3 * 8


# =============================================================================== 3. the trainer's keywords
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


@pytest.mark.parametrize("kw", [{"mmd_coeff": -1e-9}, {"mmd_coeff": float("nan")}, {"mmd_coeff": math.inf},
                                {"mmd_kernel": "rbf"}, {"mmd_kernel": None}, {"mmd_kernel": 0}, {"mmd_kernel": ["gaussian"]},
                                {"mmd_bandwidth": 0.0}, {"mmd_bandwidth": -2.0}, {"mmd_bandwidth": float("nan")},
                                {"mmd_bandwidth": math.inf}, {"mmd_bandwidth": "16"}, {"mmd_bandwidth": True},
                                {"mmd_estimator": "u"}, {"mmd_estimator": None}, {"mmd_estimator": 1}])
def test_trainer_rejects_bad_keywords_before_touching_the_model(kw):
    with pytest.raises(ValueError, match="mmd_coeff|mmd_kernel|mmd_bandwidth|mmd_estimator"):
        _trainer(_Untouchable(), **kw)


def test_defaults_leave_the_trainer_as_it_was():
    from inpaintnet_amd.vae_trainer import VAETrainer
    prm = inspect.signature(VAETrainer.__init__).parameters
    assert [prm[k].default for k in VAETrainer.MMD_SETTINGS] == [0.0, "gaussian", None, "unbiased"]
    assert [prm[k].default for k in VAETrainer.KL_SETTINGS] == [0.001, 0, 0, 0.5, 0.0, "measure"]
    tr = _trainer()
    assert tr.last_mmd is None and tr.last_kl is None and tr.model.free_bits is None and tr.mmd_coeff == 0.0
    # beta_at and the KL floor do not know about the MMD settings
    a, b = _trainer(kl_beta=0.5, kl_warmup_steps=10, free_nats=2.0), \
        _trainer(kl_beta=0.5, kl_warmup_steps=10, free_nats=2.0, mmd_coeff=10.0, mmd_kernel="imq", mmd_bandwidth=32, mmd_estimator="biased")
    assert [a.beta_at(t) for t in range(13)] == [b.beta_at(t) for t in range(13)]
    assert b.model.free_bits == (2.0, "measure") and b.last_kl is None and b.last_mmd is None
    assert (b.mmd_coeff, b.mmd_kernel, b.mmd_bandwidth, b.mmd_estimator) == (10.0, "imq", 32.0, "biased")
    # the reference's signature and rule: a static method, (z_tilde, z_prior, coeff=10), the settings as extra keywords
    assert isinstance(inspect.getattr_static(VAETrainer, "compute_mmd_loss"), staticmethod)
    prm = inspect.signature(VAETrainer.compute_mmd_loss).parameters
    assert list(prm)[:3] == ["z_tilde", "z_prior", "coeff"] and prm["coeff"].default == 10
    assert (prm["kernel"].default, prm["bandwidth"].default, prm["estimator"].default) == ("gaussian", 16.0, "reference")
    assert "compute_kernel" in VAETrainer.compute_mmd_loss.__doc__ and not hasattr(VAETrainer, "compute_kernel")


def test_training_state_round_trip_carries_the_four_settings():
    a = _trainer(mmd_coeff=10.0, mmd_kernel="imq", mmd_bandwidth=48.0, mmd_estimator="biased", free_nats=1.0)
    st = a.training_state(3)
    assert {k: st[k] for k in a.MMD_SETTINGS} == dict(mmd_coeff=10.0, mmd_kernel="imq", mmd_bandwidth=48.0, mmd_estimator="biased")
    b = _trainer()
    assert b.load_training_state(st) == 3
    assert [getattr(b, k) for k in b.MMD_SETTINGS] == [10.0, "imq", 48.0, "biased"] and b.free_nats == 1.0
    # a state written before the settings existed leaves this trainer's own -- also one that knows the KL settings only
    for drop in (a.MMD_SETTINGS, a.MMD_SETTINGS + a.KL_SETTINGS):
        old = {k: v for k, v in a.training_state(2).items() if k not in drop}
        d = _trainer(mmd_coeff=2.5, mmd_bandwidth=None, mmd_estimator="reference")
        assert d.load_training_state(old) == 2
        assert [getattr(d, k) for k in d.MMD_SETTINGS] == [2.5, "gaussian", None, "reference"]
