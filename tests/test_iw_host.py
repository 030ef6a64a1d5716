"""The importance-weighted log-likelihood without a GPU: the binding of the three entries against the header,
every refusal of the entries and of ops, the properties of the float64 restatement (tests/iw_ref.py) and a closed-form case."""
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
from tests import iw_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"inet_iw_draw": 10, "inet_nll_rows": 12, "inet_iw_finish": 7}


# =============================================================================== 1. the binding and the entries
def test_binding_has_the_headers_arity_and_types():
    text = open(os.path.join(ROOT, "include", "inpaintnet_hip.h")).read()
    from tests.test_integration_doc import quoted_argtypes
    quoted = dict(quoted_argtypes())
    for name, arity in ENTRIES.items():
        proto = re.search(r"^(\w+)\s+%s\(([^)]*)\);" % name, text, re.M)
        assert proto and proto.group(1) == "int", name
        params = [" ".join(p.split()) for p in proto.group(2).split(",")]
        assert len(params) == arity, name
        r, argtypes = _lib._SIGNATURES[name]
        assert r is C.c_int and len(argtypes) == arity and name in _lib.EXPORTS
        for prm, t in zip(params, argtypes):
            if "*" in prm:
                assert t is C.c_void_p, (name, prm)
            elif prm.startswith("int64_t"):
                assert t is C.c_int64, (name, prm)
            else:
                assert prm.startswith("int ") and t is C.c_int, (name, prm)
        assert name in quoted and [C.sizeof(t) for t in quoted[name]] == [C.sizeof(t) for t in argtypes], name
    from inpaintnet_amd import ops
    for fn, entry in ((ops.iw_draw, "inet_iw_draw"), (ops.nll_rows, "inet_nll_rows"), (ops.iw_finish, "inet_iw_finish")):
        calls = [n for n in ast.walk(ast.parse(inspect.getsource(fn)))
                 if isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute) and n.func.attr == entry]
        assert len(calls) == 1 and len(calls[0].args) == ENTRIES[entry], entry
    assert "iw.hip" in _lib.SOURCES and ops.IW_COLUMNS == R.COLUMNS


def test_the_rule_stands_in_the_header_the_kernels_header_and_the_restatement():
    want = ["z[b,k,d] = mu[b,d] + eps[b,k,d] * exp(ls[b,d])", "logr[b,k] = log p(z) - log q(z|x) = sum_d ( 0.5 eps^2 - 0.5 z^2 + ls[b,d] )",
            "logw[b,k] = logr[b,k] - nll[b,k]", "iwae[b] = m + log(s1 / K)", "ess[b] = s1^2 / s2"]
    squeeze = lambda t: re.sub(r"[\s*/]", "", t)                                   # (comment leaders, line breaks and spacing aside)
    for path in (("include", "inpaintnet_hip.h"), ("inpaintnet_amd", "csrc", "iw.h"), ("tests", "iw_ref.py")):
        text = squeeze(open(os.path.join(ROOT, *path)).read())
        for line in want:
            assert squeeze(line) in text, (path, line)
    src = open(os.path.join(ROOT, "inpaintnet_amd", "csrc", "iw.hip")).read()
    assert "atomic" not in src.lower().replace("no float atomics", "")           # no atomics of any kind
    assert "__expf" not in src and "__logf" not in src and "expf(l)" in src and "m + e * s" in src


@pytest.fixture(scope="module")
def L():
    _lib.build(verbose=False)
    return _lib.lib()


X = C.c_void_p(16)                     # a pointer that is never followed: every call below is refused in front of the launch
NULL = None


def test_iw_draw_refuses_bad_arguments_before_any_launch(L):
    call = lambda mu=X, ls=X, eps=X, stride=12, z=X, logr=X, B=2, Kc=3, Z=4: L.inet_iw_draw(mu, ls, eps, stride, z, logr, B, Kc, Z, NULL)
    calls = {"mu": call(mu=NULL), "ls": call(ls=NULL), "eps": call(eps=NULL), "z": call(z=NULL), "logr": call(logr=NULL),
             "B 0": call(B=0), "B < 0": call(B=-1), "Kc 0": call(Kc=0), "Kc < 0": call(Kc=-2), "Z 0": call(Z=0), "Z < 0": call(Z=-4),
             "rows > 2^24": call(B=(1 << 24) // 3 + 1), "B > 2^24": call(B=(1 << 24) + 1, Kc=1, stride=4),
             "stride < Kc Z": call(stride=11), "stride 0": call(stride=0), "stride < 0": call(stride=-12)}
    assert {k: v for k, v in calls.items() if v != -1} == {}


def test_nll_rows_refuses_bad_arguments_before_any_launch(L):
    call = lambda w=X, ld_w=20, tg=X, logr=X, nll=X, logw=X, ld_out=5, Rr=10, group=5, T=24, V=20: \
        L.inet_nll_rows(w, ld_w, tg, logr, nll, logw, ld_out, Rr, group, T, V, NULL)
    calls = {"weights": call(w=NULL), "targets": call(tg=NULL), "both outputs": call(nll=NULL, logw=NULL), "R 0": call(Rr=0),
             "R < 0": call(Rr=-5), "R > 2^24": call(Rr=(1 << 24) + 5), "group 0": call(group=0), "group < 0": call(group=-5),
             "T 0": call(T=0), "T < 0": call(T=-1), "V 0": call(V=0), "V < 0": call(V=-1), "ld_w < V": call(ld_w=19), "ld_w 0": call(ld_w=0),
             "R % group": call(Rr=11), "group > R": call(group=20, ld_out=20), "ld_out < group": call(ld_out=4), "ld_out 0": call(ld_out=0)}
    assert {k: v for k, v in calls.items() if v != -1} == {}


def test_iw_finish_refuses_bad_arguments_before_any_launch(L):
    call = lambda lw=X, nl=X, ld=8, B=3, K=8, out=X: L.inet_iw_finish(lw, nl, ld, B, K, out, NULL)
    calls = {"logw": call(lw=NULL), "nll": call(nl=NULL), "out": call(out=NULL), "B 0": call(B=0), "B < 0": call(B=-1),
             "B > 2^24": call(B=(1 << 24) + 1), "K 0": call(K=0), "K < 0": call(K=-8), "ld < K": call(ld=7), "ld 0": call(ld=0)}
    assert {k: v for k, v in calls.items() if v != -1} == {}


def _fake_cuda(t):
    """A CPU tensor that says it lies on the device: ops checks shapes, dtypes and strides before it touches memory."""
    class T(torch.Tensor):
        @property
        def is_cuda(self):
            return True
    return t.as_subclass(T)


def test_ops_refuse_bad_tensors():
    from inpaintnet_amd import ops
    f = lambda *s: _fake_cuda(torch.zeros(*s))
    mu, ls, eps = f(2, 4), f(2, 4), f(2, 3, 4)
    bad = [
        lambda: ops.iw_draw(torch.zeros(2, 4), ls, eps),                                     # not on the device
        lambda: ops.iw_draw(_fake_cuda(torch.zeros(2, 4, dtype=torch.float64)), ls, eps),    # dtype
        lambda: ops.iw_draw(f(4, 2).t(), f(4, 2).t(), eps),                                  # not contiguous
        lambda: ops.iw_draw(mu, f(2, 5), eps),                                               # shapes
        lambda: ops.iw_draw(mu, ls, f(2, 4)),                                                # eps not 3-D
        lambda: ops.iw_draw(mu, ls, f(3, 3, 4)),                                             # eps of another B
        lambda: ops.iw_draw(mu, ls, f(2, 3, 5)),                                             # eps of another Z
        lambda: ops.iw_draw(mu, ls, f(2, 4, 3).transpose(1, 2)),                             # eps rows not contiguous
        lambda: ops.iw_draw(mu, ls, f(2, 6, 4)[:, ::2]),                                     # a measure's rows not adjacent
        lambda: ops.iw_draw(mu, ls, None),
    ]
    w, tg = f(10, 24, 20), _fake_cuda(torch.zeros(10, 24, dtype=torch.int64))
    bad += [
        lambda: ops.nll_rows(torch.zeros(10, 24, 20), tg),
        lambda: ops.nll_rows(f(240, 20), tg),                                                # not [R, T, V]
        lambda: ops.nll_rows(f(10, 20, 24).transpose(1, 2), tg),                             # last dimension not contiguous
        lambda: ops.nll_rows(w, _fake_cuda(torch.zeros(10, 24, dtype=torch.int32))),         # targets' dtype
        lambda: ops.nll_rows(w, _fake_cuda(torch.zeros(10, 23, dtype=torch.int64))),         # targets' shape
        lambda: ops.nll_rows(w, tg, logr=f(9)),
        lambda: ops.nll_rows(w, tg, logr=_fake_cuda(torch.zeros(10, dtype=torch.float64))),
        lambda: ops.nll_rows(w, tg, group=3),                                                # does not divide R
        lambda: ops.nll_rows(w, tg, group=0),
        lambda: ops.nll_rows(w, tg, group=5, ld_out=4),                                      # ld_out < group
        lambda: ops.nll_rows(w, tg, group=5, out_nll=f(2, 4)),                               # an output of another shape
        lambda: ops.nll_rows(w, tg, group=5, out_nll=f(2, 8)[:, :5], out_logw=f(2, 9)[:, :5]),     # two row strides
        lambda: ops.nll_rows(w, tg, group=5, out_nll=f(2, 8)[:, :5], ld_out=7),              # ld_out against the output's stride
        lambda: ops.nll_rows(w, tg, group=5, out_nll=torch.zeros(2, 5)),
    ]
    bad += [
        lambda: ops.iw_finish(torch.zeros(3, 8), f(3, 8)),
        lambda: ops.iw_finish(f(3, 8), f(3, 7)),
        lambda: ops.iw_finish(f(24), f(24)),
        lambda: ops.iw_finish(f(8, 3).t(), f(8, 3).t()),
        lambda: ops.iw_finish(f(3, 8), f(3, 16)[:, :8]),                                     # two row strides
        lambda: ops.iw_finish(_fake_cuda(torch.zeros(3, 8, dtype=torch.float64)), f(3, 8)),
    ]
    for i, fn in enumerate(bad):
        with pytest.raises(ValueError):
            fn()
            pytest.fail(f"case {i} was not refused")


def test_model_and_tester_surface():
    from inpaintnet_amd.measure_vae import MeasureVAE
    from inpaintnet_amd.vae_tester import VAETester
    prm = inspect.signature(MeasureVAE.log_weights).parameters
    assert list(prm) == ["self", "score", "num_samples", "eps", "generator", "max_rows", "reproducible"]
    assert (prm["eps"].default, prm["generator"].default, prm["max_rows"].default, prm["reproducible"].default) == (None, None, 4096, True)
    prm = inspect.signature(VAETester.measure_log_likelihood).parameters
    assert list(prm) == ["self", "score_tensor", "num_samples", "eps", "generator", "max_rows"] and prm["num_samples"].default == 64
    prm = inspect.signature(VAETester.log_likelihood).parameters
    assert list(prm) == ["self", "data_loader", "num_samples", "generator", "max_rows"] and prm["num_samples"].default == 64
    assert VAETester.LL_COLUMNS == ("iwae", "elbo", "ess", "rec", "kl")
    assert "max_rows" in MeasureVAE.log_weights.__doc__ and "draws" in MeasureVAE.log_weights.__doc__


# =============================================================================== 2. the restatement
def _weights(rng, B, K, spread=3.0):
    logw = (-30.0 + spread * rng.standard_normal((B, K))).astype(np.float32)
    nll = (40.0 + rng.standard_normal((B, K))).astype(np.float32)
    return logw, nll


@pytest.mark.parametrize("K", [1, 2, 7, 64, 1000])
def test_restatement_properties(K):
    rng = np.random.default_rng(K)
    logw, nll = _weights(rng, 6, K)
    out = R.finish(logw, nll)
    iwae, elbo, ess, rec, kl = out.T
    tol = 1e-12 * np.abs(logw.astype(np.float64)).max()
    assert (iwae >= elbo - tol).all()                                            # Jensen
    assert (iwae <= logw.astype(np.float64).max(1) + tol).all()
    assert (ess >= 1.0 - 1e-12).all() and (ess <= K + 1e-9).all()
    assert np.abs(rec + kl + elbo).max() <= 1e-12 * np.abs(elbo).max()
    if K == 1:
        assert np.array_equal(iwae, logw[:, 0].astype(np.float64)) and np.array_equal(elbo, iwae) and np.array_equal(ess, np.ones(6))
        assert np.array_equal(rec, nll[:, 0].astype(np.float64))
        assert np.abs(kl - (-(logw[:, 0].astype(np.float64) + nll[:, 0]))).max() <= 1e-12 * 70


def test_restatement_special_values():
    lw = np.full((4, 7), -3.25, np.float32)
    lw[1, 2] = np.nan
    lw[2, :] = -np.inf
    lw[3, 1:] = -np.inf
    out = R.finish(lw, np.ones((4, 7), np.float32))
    assert out[0, 0] == -3.25 and out[0, 1] == -3.25 and out[0, 2] == 7.0
    assert np.isnan(out[1, :3]).all()
    assert out[2, 0] == -np.inf and out[2, 1] == -np.inf and out[2, 2] == 0.0
    assert out[3, 0] == -3.25 + math.log(1.0 / 7.0) and out[3, 1] == -np.inf and out[3, 2] == 1.0
    wide = np.array([[0.0, -800.0]], np.float32)
    assert abs(R.finish(wide, wide)[0, 2] - 1.0) <= 1e-12


def test_restatement_of_draw_and_nll_rows_against_torch():
    rng = np.random.default_rng(3)
    B, K, Z, T, V = 3, 4, 7, 5, 11
    mu, ls, eps = rng.standard_normal((B, Z)), 0.3 * rng.standard_normal((B, Z)), rng.standard_normal((B, K, Z))
    d = R.draw(mu, ls, eps)
    q = torch.distributions.Normal(torch.from_numpy(mu)[:, None], torch.from_numpy(np.exp(ls))[:, None])
    z = torch.from_numpy(d["z"])
    want = torch.distributions.Normal(0.0, 1.0).log_prob(z).sum(-1) - q.log_prob(z).sum(-1)
    assert np.abs(d["logr"] - want.numpy()).max() <= 1e-12 * np.abs(want.numpy()).max()
    assert (d["logr_bound"] > 0).all() and (d["logr_bound"] <= 1e-4 * np.abs(d["logr"]).max()).all()
    w = (4.0 * rng.standard_normal((B * K, T, V))).astype(np.float32)
    tg = rng.integers(0, V, (B * K, T))
    n = R.nll_rows(w, tg, d["logr"].reshape(-1))
    want = -torch.log_softmax(torch.from_numpy(w).double(), -1).gather(-1, torch.from_numpy(tg)[..., None])[..., 0].sum(-1).numpy()
    assert np.abs(n["nll"] - want).max() <= 1e-12 * want.max()
    assert np.abs(n["logw"] - (d["logr"].reshape(-1) - want)).max() <= 1e-12 * 100
    assert (n["nll_bound"] > 0).all() and (n["nll_bound"] <= 1e-5 * n["nll"]).all()
    # all-equal rows: T log V
    eq = R.nll_rows(np.full((2, T, V), 1.5, np.float32), np.zeros((2, T), np.int64))
    assert np.abs(eq["nll"] - T * math.log(V)).max() <= 1e-13 * T * math.log(V)
    # the depths restate the launch constants of csrc/iw.hip
    src = open(os.path.join(ROOT, "inpaintnet_amd", "csrc", "iw.hip")).read()
    assert int(re.search(r"constexpr int kIwBlock = (\d+);", src).group(1)) == 256
    assert R.depth_draw(256) == 4 + 3 + 6 and R.depth_v(65) == 2 + 6 and R.depth_t(24) == 6 + 2 and R.depth_t(30) == 8 + 2


# =============================================================================== 3. a closed-form case
def test_iwae_of_a_linear_gaussian_model_lands_on_its_marginal_likelihood():
    """p(z) = N(0, I_Z), p(x | z) = N(W z + b, s^2 I_D): log p(x) = log N(x; b, W W' + s^2 I) in closed form, the posterior is Gaussian
    with covariance (I + W' W / s^2)^-1.  q(z | x) = N(the posterior's mean, 1.1^2 x the DIAGONAL of its covariance): close to the
    posterior, so that the weights have a small variance, but not equal to it.  The restatement's iwae at K = 4096 from a seeded
    generator must land within 4 standard errors of log p(x); the standard error of log(mean w) is std(w) / (sqrt(K) mean w) (the
    delta method), computed here from the same weights.  The estimator's bias, -se^2 / 2, is far inside that."""
    rng = np.random.default_rng(20161)
    Z, D, K, s = 4, 6, 4096, 0.7
    W, b = 0.5 * rng.standard_normal((D, Z)), rng.standard_normal(D)
    z_true = rng.standard_normal((2, Z))
    x = z_true @ W.T + b + s * rng.standard_normal((2, D))
    C_x = W @ W.T + s * s * np.eye(D)
    diff = x - b
    truth = -0.5 * (np.einsum("bi,ij,bj->b", diff, np.linalg.inv(C_x), diff) + np.linalg.slogdet(C_x)[1] + D * math.log(2 * math.pi))
    S = np.linalg.inv(np.eye(Z) + W.T @ W / (s * s))
    mu = diff @ W @ S.T / (s * s)
    ls = np.broadcast_to(np.log(1.1 * np.sqrt(np.diag(S))), mu.shape)
    eps = rng.standard_normal((2, K, Z))
    d = R.draw(mu, ls, eps)
    res = x[:, None, :] - (d["z"] @ W.T + b)
    nll = 0.5 * (res * res).sum(-1) / (s * s) + D * math.log(s) + 0.5 * D * math.log(2 * math.pi)      # -log p(x | z), a density
    logw = d["logr"] - nll
    out = R.finish(logw, nll)
    w = np.exp(logw - logw.max(1, keepdims=True))
    se = w.std(1, ddof=1) / (math.sqrt(K) * w.mean(1))
    print("log p(x)", truth, "iwae", out[:, 0], "elbo", out[:, 1], "ess", out[:, 2], "standard error", se)
    assert (se < 0.02).all() and (out[:, 2] > K / 2).all()
    assert (np.abs(out[:, 0] - truth) <= 4 * se).all()
    assert (out[:, 1] < truth).all() and (out[:, 0] >= out[:, 1]).all()                     # the ELBO lies below, the IWAE bound above it
