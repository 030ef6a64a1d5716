"""Host-side checks of the decoder's temperature sampling (no GPU).

tests/golden/decoder_sample.npz holds calls of the reference's HierarchicalDecoder (MeasureVAE/decoder.py:412-529) in its multinomial
branch with the draw replaced by the project's rule on stored uniforms (tools/gen_golden_decoder_sample.py).  The float64 oracle with
the fixture's tokens fed back plus the float64 restatement of the rule (tests/decoder_sample_ref.py) reproduces tokens and logits:
this pins the reading of the reference that the kernels implement -- the drawn token is the one fed back and the one reported.  The
planner's answer for a sampled call (inet_decode_b1_plan_sample) passes its self-check for every call size, and the argument errors
of the new entry points are raised in front of any launch."""
import ctypes as C

import numpy as np
import pytest
import torch

from inpaintnet_amd import _lib, ops
from tests import decoder_sample_ref as R
from tests import golden_util as G

X = C.c_void_p(16)              # a pointer that is never followed (tests/test_pointwise_host.py)
NULL = None


@pytest.fixture(scope="module")
def L():
    _lib.build(verbose=False)
    return _lib.lib()


@pytest.fixture(scope="module")
def small():
    fx = G.load("decoder_sample")
    P64 = {k: v.double() for k, v in G.vae_params("small").items()}
    return fx, P64, torch.from_numpy(fx["z"])


@pytest.mark.parametrize("ti", [0, 1])
def test_oracle_and_restatement_reproduce_the_reference(small, ti):
    fx, P64, z = small
    temp = float(fx["temperatures"][ti])
    u, ref_tok, ref_w = fx[f"t{ti}/uniforms"], fx[f"t{ti}/tokens"].astype(np.int64), fx[f"t{ti}/weights"]
    assert np.array_equal(u, np.random.RandomState(int(fx[f"t{ti}/seed"])).random_sample(u.shape))
    assert float(fx[f"t{ti}/margin"].min()) >= float(fx["min_margin"]) == R.MARGIN
    w = R.oracle_logits(P64, z, ref_tok)
    assert G.rel_err(w, ref_w) < 1e-6, G.rel_err(w, ref_w)
    tok, mg = R.sample_rows(w, temp, u)
    assert np.array_equal(tok, ref_tok), np.argwhere(tok != ref_tok)[:4]
    assert np.allclose(mg, fx[f"t{ti}/margin"], rtol=1e-3, atol=1e-6)
    # ... and without the fixture's tokens: the trajectory found by feeding the picks back is the reference's
    w2, tok2, _ = R.sampled_trajectory(P64, z, temp, u)
    assert np.array_equal(tok2, ref_tok) and G.rel_err(w2, ref_w) < 1e-6
    # the draws are draws: not the argmax trajectory, and the two temperatures differ
    assert (tok != w.argmax(-1)).mean() > 0.2
    assert not np.array_equal(fx["t0/tokens"], fx["t1/tokens"])


def test_the_restated_rule_at_its_edges():
    x = np.array([0.0, 1.0, 1.0, 0.5])
    assert R.pick(x, 1.0, 0.0)[0] == 0 and R.pick(x, 1.0, np.nextafter(1.0, 0.0))[0] == 3
    p = np.exp(x) / np.exp(x).sum()
    assert R.pick(x, 1.0, p[0] + 1e-9)[0] == 1 and R.pick(x, 1.0, p[0] - 1e-9)[0] == 0
    assert abs(R.pick(x, 1.0, p[0] + 1e-9)[1] - 1e-9) < 1e-12
    assert R.pick(x, -1.0, 0.0)[0] == 0 and R.pick(x, 0.0, 0.6)[0] == 2          # any finite temperature is taken as it is
    for u in (1.0, 2.0, -1e-9, np.nan):
        assert R.pick(x, 1.0, u)[0] == -1
    assert R.pick(np.array([0.0, np.inf]), 1.0, 0.5)[0] == -1 and R.pick(np.array([0.0, np.inf]), 0.0, 0.5)[0] == -1
    tok, _ = R.sample_rows(np.array([[0.0, 3.0, 3.0], [np.nan, 1.0, 0.0]]), 1.0, np.array([2.0, 0.5]))
    assert tok.tolist() == [1, 0]                                                # the argmax rule: lowest index, a NaN is the maximum


def plan(L, B, V, Z, sample=True):
    out = (C.c_int * 8)()
    rc = (L.inet_decode_b1_plan_sample if sample else L.inet_decode_b1_plan)(B, V, Z, out)
    return rc, dict(zip(("teams", "team_rows", "rgroups", "crit", "placed", "grid", "live", "ok"), list(out)))


@pytest.mark.parametrize("Z", [128, 256])
@pytest.mark.parametrize("V", [20, 32, 33, 48, 64, 65, 100, 128])
def test_the_sampled_plans_pass_the_planners_self_check(L, V, Z):
    for B in range(1, 17):
        rc, p = plan(L, B, V, Z)
        assert rc == 0 and p["ok"] == 1, (B, V, Z, rc, p)
        assert p["placed"] == 1 and p["grid"] <= 256 and p["live"] <= 256 and p["teams"] * p["team_rows"] >= B, (B, V, Z, p)
        # the argmax call's plan, except where the merged sampling build does not exist (two-row teams beside groups of six rows,
        # V <= 32): there workgroup C is placed, 17 critical workgroups per team instead of 16
        rc0, p0 = plan(L, B, V, Z, sample=False)
        assert rc0 == 0
        if V <= 32 and B >= 11:
            assert p0["crit"] == 16 and p["crit"] == 17 and p["live"] == p0["live"] + p["teams"], (B, V, Z, p, p0)
            assert {k: p[k] for k in ("teams", "team_rows", "rgroups")} == {k: p0[k] for k in ("teams", "team_rows", "rgroups")}
        else:
            assert p == p0, (B, V, Z, p, p0)


def test_calls_the_sampled_launch_does_not_take(L):
    assert plan(L, 17, 48, 256)[0] == -1 and plan(L, 0, 48, 256)[0] == -1 and plan(L, 4, 129, 256)[0] == -1
    try:                                       # the sampling build exists for the default mode's plans
        for m in (0, 1, 2, 3, 5):
            assert L.inet_set_option(15, m) == 0
            assert plan(L, 4, 48, 256)[0] == -1, m
            assert plan(L, 4, 48, 256, sample=False)[0] == (-1 if m == 0 else 0), m
    finally:
        L.inet_set_option(15, 4)
    assert plan(L, 4, 48, 256)[0] == 0


def test_argument_errors(L):
    cfg = ops.vae_config(48)
    inf, nan = float("inf"), float("nan")
    big = 1 << 40
    calls = {
        "st weights": L.inet_sample_temperature(NULL, 4, 1, 4, 1.0, X, 1, X, 1, NULL),
        "st uniforms": L.inet_sample_temperature(X, 4, 1, 4, 1.0, NULL, 1, X, 1, NULL),
        "st out": L.inet_sample_temperature(X, 4, 1, 4, 1.0, X, 1, NULL, 1, NULL),
        "st rows": L.inet_sample_temperature(X, 4, 0, 4, 1.0, X, 1, X, 1, NULL),
        "st V": L.inet_sample_temperature(X, 4, 1, 0, 1.0, X, 1, X, 1, NULL),
        "st V > 512": L.inet_sample_temperature(X, 513, 1, 513, 1.0, X, 1, X, 1, NULL),
        "st inf": L.inet_sample_temperature(X, 4, 1, 4, inf, X, 1, X, 1, NULL),
        "st nan": L.inet_sample_temperature(X, 4, 1, 4, nan, X, 1, X, 1, NULL),
        "dec z": L.inet_vae_decoder_sample(C.byref(cfg), 1, NULL, X, NULL, NULL, X, X, X, big, 0, 1.0, X, NULL),
        "dec params": L.inet_vae_decoder_sample(C.byref(cfg), 1, X, NULL, NULL, NULL, X, X, X, big, 0, 1.0, X, NULL),
        "dec weights": L.inet_vae_decoder_sample(C.byref(cfg), 1, X, X, NULL, NULL, NULL, X, X, big, 0, 1.0, X, NULL),
        "dec samples": L.inet_vae_decoder_sample(C.byref(cfg), 1, X, X, NULL, NULL, X, NULL, X, big, 0, 1.0, X, NULL),
        "dec ws": L.inet_vae_decoder_sample(C.byref(cfg), 1, X, X, NULL, NULL, X, X, NULL, big, 0, 1.0, X, NULL),
        "dec ws_bytes": L.inet_vae_decoder_sample(C.byref(cfg), 1, X, X, NULL, NULL, X, X, X, 16, 0, 1.0, X, NULL),
        "dec uniforms": L.inet_vae_decoder_sample(C.byref(cfg), 1, X, X, NULL, NULL, X, X, X, big, 0, 1.0, NULL, NULL),
        "dec batch": L.inet_vae_decoder_sample(C.byref(cfg), 0, X, X, NULL, NULL, X, X, X, big, 0, 1.0, X, NULL),
        "dec inf": L.inet_vae_decoder_sample(C.byref(cfg), 1, X, X, NULL, NULL, X, X, X, big, 0, inf, X, NULL),
        "dec -inf": L.inet_vae_decoder_sample(C.byref(cfg), 1, X, X, NULL, NULL, X, X, X, big, 0, -inf, X, NULL),
        "dec nan": L.inet_vae_decoder_sample(C.byref(cfg), 1, X, X, NULL, NULL, X, X, X, big, 0, nan, X, NULL),
        "plan out": L.inet_decode_b1_plan_sample(1, 48, 256, NULL),
    }
    assert {k: v for k, v in calls.items() if v != -1} == {}
    with pytest.raises(ValueError):
        ops.decoder_fwd(cfg, None, None, False, None, temperature=1.0)
    with pytest.raises(ValueError):
        ops.decoder_fwd(cfg, None, None, False, None, uniforms=torch.zeros(1, 24, dtype=torch.float64))
