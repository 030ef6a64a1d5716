"""Host-side checks of the decoder's top-k / nucleus truncated sampling (no GPU): the float64 restatement of the rule
(tests/decoder_trunc_ref.py) against itself and against the untruncated restatement, the argument errors of the two new entry points in
front of any launch, the planner's self-check for a truncated call, and the count of draws that lie within 2e-5 of a step -- of the
kept CDF or of the nucleus boundary -- for the very seeds the GPU tests run (tests/test_gpu_decoder_trunc.py), held to the caps: at most
1 % of a test function's draws and at most 3 % of any single (V, temperature, top_k, top_p) setting."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from inpaintnet_amd import _lib, layout, ops, synthetic
from tests import decoder_sample_ref as R
from tests import decoder_trunc_ref as TR
from tests import golden_util as G

X = C.c_void_p(16)              # a pointer that is never followed (tests/test_pointwise_host.py)
NULL = None


@pytest.fixture(scope="module")
def L():
    _lib.build(verbose=False)
    return _lib.lib()


def rows(tag, n, V, scale=0.6):
    x = np.maximum(synthetic.det_normal(f"decoder_trunc/host/{tag}", (n, V), scale), 0.0).astype(np.float32)
    u = synthetic.det_uniform(f"decoder_trunc/host/u/{tag}", (n,), 0.0, 1.0).astype(np.float64)
    return x, u


def kept_set(x, temp, k, p):
    """the kept tokens of a row: what u = 0 .. 1 can draw -- read off the restatement by its kept count and the order"""
    x = np.asarray(x, dtype=np.float32)
    n = TR.pick(x, temp, 0.5, k, p)[2]
    s = (np.float32(temp) * x).astype(np.float32)
    return set(np.lexsort((np.arange(x.size), -s.astype(np.float64)))[:n].tolist())


def test_truncation_off_is_the_sampling_rule():
    """top_k in {0, V, V + 5, -3} with top_p = 1: the token of decoder_sample_ref.pick (float64 throughout; here e is rounded to f32 as
    the kernels have it, so draws within the margin of a CDF step are left out: at most 1 % of them)"""
    near = draws = 0
    for V in (5, 48, 100):
        x, u = rows(f"off/{V}", 200, V)
        for temp in (1.0, 6.0, -2.0):
            for k in (0, V, V + 5, -3):
                for xi, ui in zip(x, u):
                    want, mg = R.pick(xi, temp, ui)
                    tok, lp, n, cm, bm = TR.pick(xi, temp, ui, k, 1.0)
                    assert n == V and bm == np.inf
                    draws += 1
                    if mg < R.MARGIN:
                        near += 1
                        continue
                    assert tok == want, (V, temp, k)
                    p = np.exp(np.float64(temp) * xi.astype(np.float64))
                    assert abs(float(lp) - math.log(p[tok] / p.sum())) < 1e-5 * max(1.0, abs(float(lp)))
    assert near <= 0.01 * draws, (near, draws)


def test_top_k_one_is_the_argmax():
    for V in (1, 2, 48, 100):
        x, u = rows(f"k1/{V}", 100, V)
        x[::3] = 0.0                                           # rows of zeros: the lowest index
        for temp in (1.0, 6.0, 1e-3):
            for xi, ui in zip(x, u):
                tok, lp, n, cm, bm = TR.pick(xi, temp, ui, 1, 1.0)
                assert tok == R.argmax_first(xi) and n == 1 and float(lp) == 0.0 and cm == 1.0


def test_kept_sets_are_nested():
    for V in (20, 100):
        x, _ = rows(f"nest/{V}", 20, V)
        for temp in (1.0, 6.0, -2.0):
            for xi in x:
                prev = set()
                for k in list(range(1, V + 1)):
                    cur = kept_set(xi, temp, k, 1.0)
                    assert len(cur) == k and prev <= cur
                    prev = cur
                prev = set()
                for p in (1e-9, 0.1, 0.3, 0.5, 0.7, 0.9, 0.999, 1.0):
                    cur = kept_set(xi, temp, 0, p)
                    assert len(cur) >= 1 and prev <= cur
                    assert cur <= kept_set(xi, temp, 0, 1.0)
                    prev = cur
                assert kept_set(xi, temp, 8, 0.7) <= kept_set(xi, temp, 8, 1.0) <= kept_set(xi, temp, 0, 1.0)


def test_all_equal_rows_keep_the_lowest_indices():
    """every e is 1 and every A_i = i exactly: with top_p V not an integer the kept count is ceil(top_p V), the lowest indices"""
    for V in (3, 20, 65, 100):
        for val in (0.0, 0.75):
            x = np.full(V, val, dtype=np.float32)
            for p in (0.313, 0.577, 0.871, 0.999):
                assert abs(p * V - round(p * V)) > 1e-9
                n = math.ceil(p * V)
                assert kept_set(x, 6.0, 0, p) == set(range(n)), (V, p)
                # ... and the draw is uniform over them: u picks index floor(u n)
                for u in (0.0, 0.26, 0.51, 0.98):
                    tok, lp, kept, _, _ = TR.pick(x, 6.0, u, 0, p)
                    assert tok == int(u * n) and kept == n and abs(float(lp) + math.log(n)) < 1e-6
            assert kept_set(x, 1.0, 4 if V > 4 else 2, 1.0) == set(range(4 if V > 4 else 2))
            k = min(7, V - 1)
            assert kept_set(x, 1.0, k, 0.51) == set(range(math.ceil(0.51 * k)))        # the nucleus of what top-k kept


def test_a_negative_temperature_orders_by_s():
    x = np.array([0.0, 2.0, 1.0, 0.0, 3.0], dtype=np.float32)
    assert kept_set(x, -1.0, 2, 1.0) == {0, 3}                 # the zeros have the largest s = -x, lowest index first
    assert kept_set(x, -1.0, 3, 1.0) == {0, 3, 2}
    assert kept_set(x, 1.0, 2, 1.0) == {4, 1}
    assert kept_set(x, 0.0, 2, 1.0) == {0, 1}                  # T = 0: all tie
    assert TR.pick(x, -1.0, 0.99, 1, 1.0)[0] == 0


def test_rows_outside_the_rule():
    x = np.array([0.0, 1.0, 1.0, 0.5], dtype=np.float32)
    for u in (1.0, 2.0, -1e-9, np.nan):
        tok, lp, n, _, _ = TR.pick(x, 1.0, u, 2, 0.9)
        assert tok == -1 and np.isnan(lp) and n == 0
    assert TR.pick(np.array([0.0, np.inf], dtype=np.float32), 1.0, 0.5, 1, 1.0)[0] == -1
    assert TR.pick(np.array([0.0, np.nan], dtype=np.float32), 1.0, 0.5, 1, 1.0)[0] == -1
    tok, lp, n, cm, bm, d = TR.pick_rows(np.array([[0.0, 3.0, 3.0], [np.nan, 1.0, 0.0]]), 1.0, np.array([2.0, 0.5]), 2, 0.5)
    assert tok.tolist() == [1, 0] and np.isnan(lp).all()
    for bad in (0.0, -0.1, 1.0000001, np.nan, np.inf):
        with pytest.raises(ValueError):
            TR.pick(x, 1.0, 0.5, 0, bad)


def test_the_one_pass_trajectory_is_the_oracles():
    """decoder_trunc_ref.trajectory restates the oracle's tick loop to choose the fed token tick by tick: with the argmax as the choice
    it must reproduce oracle.torch_ref.decoder_forward, and fed its own tokens the oracle returns its logits."""
    P64 = {k: v.double() for k, v in G.vae_params("small").items()}
    z = torch.from_numpy(G.load("decoder_sample")["z"])
    w, tok = TR.trajectory(P64, z, lambda t, wt: wt.argmax(-1))
    from oracle import torch_ref as O
    with torch.no_grad():
        w0, s0 = O.decoder_forward(P64, z.double(), None, False)
    assert np.array_equal(tok, s0[:, 0].numpy()) and np.array_equal(w, w0.numpy())
    u = synthetic.det_uniform("decoder_trunc/host/traj", (z.shape[0], 24), 0.0, 1.0).astype(np.float64)
    w, tok, n, cm, bm = TR.truncated_trajectory(P64, z, 6.0, u, 0, 0.9)
    assert np.array_equal(R.oracle_logits(P64, z, tok), w)
    assert (tok != w.argmax(-1)).any() and n.min() >= 1 and n.max() < w.shape[-1]


def plan_params(V, Z):
    c = G.CFGS["full"]
    P = {k: torch.from_numpy(synthetic.det_param(k, s)) for k, s in layout.vae_param_shapes(V, c["E"], c["H"], Z, c["H"]).items()}
    return {k: v.double() for k, v in P.items()}


@pytest.mark.parametrize("Z", TR.PLAN_Z)
@pytest.mark.parametrize("V", TR.PLAN_V)
def test_margin_counts_of_the_every_plan_test(V, Z):
    """Along the oracle's own truncated trajectory for the seeds of test_gpu_decoder_trunc.test_every_plan_of_a_truncated_call: draws with
    a margin below 2e-5, per setting (cap 3 %) and over the function's 2520 draws (cap 1 %).  The settings truncate: fewer than V kept."""
    P64 = plan_params(V, Z)
    near_all = draws_all = 0
    for si, (temp, k, p) in enumerate(TR.SETTINGS):
        zs, us = zip(*(TR.plan_inputs(V, Z, B, si) for B in TR.PLAN_B))
        w, tok, n, cm, bm = TR.truncated_trajectory(P64, torch.from_numpy(np.concatenate(zs)), temp, np.concatenate(us), k, p)
        near = int((~TR.firm(cm, bm)).sum())
        print(f"V {V} Z {Z} setting {(temp, k, p)}: {near} of {cm.size} draws within the margin, kept mean {n.mean():.1f} of {V}")
        assert near <= 0.03 * cm.size, (V, Z, temp, k, p, near, cm.size)
        assert n.max() <= (k if k else V) and n.mean() < V
        near_all, draws_all = near_all + near, draws_all + cm.size
    assert near_all <= 0.01 * draws_all, (V, Z, near_all, draws_all)


@pytest.mark.parametrize("V", TR.ALONE_V)
def test_margin_counts_of_the_kernel_alone_test(V):
    """The same for the rows of test_gpu_decoder_trunc.test_the_truncating_kernel_alone: per (V, temperature, top_k, top_p) setting the 76
    draws of its three row counts (cap 3 %: two draws), per vocabulary all settings (cap 1 %)."""
    cases = [TR.alone_case(V, r) for r in TR.ALONE_ROWS]
    near_all = draws_all = 0
    for temp in TR.ALONE_TEMPS:
        for k in TR.alone_top_k(V):
            for p in TR.ALONE_TOP_P:
                near = draws = 0
                for x, u in cases:
                    _, _, _, cm, bm, _ = TR.pick_rows(x[:, :V], temp, u[:, 0], k, p)
                    near, draws = near + int((~TR.firm(cm, bm)).sum()), draws + cm.size
                assert near <= 0.03 * draws, (V, temp, k, p, near, draws)
                near_all, draws_all = near_all + near, draws_all + draws
    print(f"V {V}: {near_all} of {draws_all} draws within the margin")
    assert near_all <= 0.01 * draws_all, (V, near_all, draws_all)
    # the tie rows are compared exactly, no draw left out: their sums of a few distinct f32 values are exact in f64 in any order, and
    # neither the token nor the kept count depends on the last bit of expf (an e of exactly 1 -- every tied maximum -- is exact anyway)
    for temp in TR.ALONE_TEMPS:
        for k in TR.alone_top_k(V):
            for p in TR.ALONE_TOP_P:
                for row in TR.tie_rows(V):
                    for u in (0.05, 0.37, 0.81):
                        base = TR.pick(row, temp, u, k, p)
                        for ulps in (-1, 1):
                            other = TR.pick(row, temp, u, k, p, e_ulps=ulps)
                            assert (other[0], other[2]) == (base[0], base[2]), (V, temp, k, p, u, ulps)


def plan(L, B, V, Z, kind):
    out = (C.c_int * 8)()
    rc = {0: L.inet_decode_b1_plan, 1: L.inet_decode_b1_plan_sample, 2: L.inet_decode_b1_plan_trunc}[kind](B, V, Z, out)
    return rc, dict(zip(("teams", "team_rows", "rgroups", "crit", "placed", "grid", "live", "ok"), list(out)))


@pytest.mark.parametrize("Z", [128, 256])
@pytest.mark.parametrize("V", [20, 32, 33, 48, 64, 65, 100, 128])
def test_the_truncated_plans_pass_the_planners_self_check(L, V, Z):
    """A truncated call has a plan wherever a sampled call has one, with the same teams; where the truncating build has no merged build
    (two rows with V <= 32, one row with 32 < V <= 64: it would spill registers) workgroup C is placed instead."""
    for B in range(1, 17):
        rc, p = plan(L, B, V, Z, 2)
        assert rc == 0 and p["ok"] == 1, (B, V, Z, rc, p)
        assert p["placed"] == 1 and p["grid"] <= 256 and p["live"] <= 256 and p["teams"] * p["team_rows"] >= B, (B, V, Z, p)
        rc1, p1 = plan(L, B, V, Z, 1)
        assert rc1 == 0
        if p != p1:
            assert V <= 64 and p1["crit"] in (16, 32) and p["crit"] == 17, (B, V, Z, p, p1)
    assert plan(L, 17, V, Z, 2)[0] == -1 and plan(L, 1, 48, Z, 2)[0] == 0 and L.inet_decode_b1_plan_trunc(1, 48, Z, NULL) == -1


def test_argument_errors(L):
    cfg = ops.vae_config(48)
    inf, nan = float("inf"), float("nan")
    big = 1 << 40
    st = lambda *a: L.inet_sample_truncated(*a)
    dec = lambda *a: L.inet_vae_decoder_sample_ex(C.byref(cfg), *a)
    calls = {
        "st weights": st(NULL, 4, 1, 4, 1.0, X, 1, 2, 0.9, X, 1, X, 1, NULL),
        "st uniforms": st(X, 4, 1, 4, 1.0, NULL, 1, 2, 0.9, X, 1, X, 1, NULL),
        "st out": st(X, 4, 1, 4, 1.0, X, 1, 2, 0.9, NULL, 1, X, 1, NULL),
        "st rows": st(X, 4, 0, 4, 1.0, X, 1, 2, 0.9, X, 1, X, 1, NULL),
        "st V": st(X, 4, 1, 0, 1.0, X, 1, 2, 0.9, X, 1, X, 1, NULL),
        "st V > 512": st(X, 513, 1, 513, 1.0, X, 1, 2, 0.9, X, 1, X, 1, NULL),
        "st inf": st(X, 4, 1, 4, inf, X, 1, 2, 0.9, X, 1, X, 1, NULL),
        "st nan": st(X, 4, 1, 4, nan, X, 1, 2, 0.9, X, 1, X, 1, NULL),
        "st top_p 0": st(X, 4, 1, 4, 1.0, X, 1, 2, 0.0, X, 1, X, 1, NULL),
        "st top_p < 0": st(X, 4, 1, 4, 1.0, X, 1, 2, -0.5, X, 1, X, 1, NULL),
        "st top_p > 1": st(X, 4, 1, 4, 1.0, X, 1, 2, 1.0000001, X, 1, X, 1, NULL),
        "st top_p nan": st(X, 4, 1, 4, 1.0, X, 1, 2, nan, X, 1, X, 1, NULL),
        "st top_p inf": st(X, 4, 1, 4, 1.0, X, 1, 2, inf, X, 1, X, 1, NULL),
        "dec z": dec(1, NULL, X, NULL, NULL, X, X, X, big, 0, 1.0, X, 2, 0.9, X, NULL),
        "dec params": dec(1, X, NULL, NULL, NULL, X, X, X, big, 0, 1.0, X, 2, 0.9, X, NULL),
        "dec weights": dec(1, X, X, NULL, NULL, NULL, X, X, big, 0, 1.0, X, 2, 0.9, X, NULL),
        "dec samples": dec(1, X, X, NULL, NULL, X, NULL, X, big, 0, 1.0, X, 2, 0.9, X, NULL),
        "dec ws": dec(1, X, X, NULL, NULL, X, X, NULL, big, 0, 1.0, X, 2, 0.9, X, NULL),
        "dec ws_bytes": dec(1, X, X, NULL, NULL, X, X, X, 16, 0, 1.0, X, 2, 0.9, X, NULL),
        "dec uniforms": dec(1, X, X, NULL, NULL, X, X, X, big, 0, 1.0, NULL, 2, 0.9, X, NULL),
        "dec batch": dec(0, X, X, NULL, NULL, X, X, X, big, 0, 1.0, X, 2, 0.9, X, NULL),
        "dec inf": dec(1, X, X, NULL, NULL, X, X, X, big, 0, inf, X, 2, 0.9, X, NULL),
        "dec nan": dec(1, X, X, NULL, NULL, X, X, X, big, 0, nan, X, 2, 0.9, X, NULL),
        "dec top_p 0": dec(1, X, X, NULL, NULL, X, X, X, big, 0, 1.0, X, 2, 0.0, X, NULL),
        "dec top_p < 0": dec(1, X, X, NULL, NULL, X, X, X, big, 0, 1.0, X, 2, -1.0, NULL, NULL),
        "dec top_p > 1": dec(1, X, X, NULL, NULL, X, X, X, big, 0, 1.0, X, 0, 1.5, NULL, NULL),
        "dec top_p nan": dec(1, X, X, NULL, NULL, X, X, X, big, 0, 1.0, X, 0, nan, X, NULL),
    }
    assert {k: v for k, v in calls.items() if v != -1} == {}
    for bad in (dict(top_k=2), dict(top_p=0.9), dict(logp=torch.zeros(1, 24))):
        with pytest.raises(ValueError):
            ops.decoder_fwd(cfg, None, None, False, None, **bad)
    for bad in (0.0, -0.5, 1.5, nan):
        with pytest.raises(ValueError):
            ops.decoder_fwd(cfg, None, None, False, None, temperature=1.0, uniforms=torch.zeros(1, 24, dtype=torch.float64), top_p=bad)
    for bad in (2.5, nan, inf, "3", True):                     # top_k is an integer or None
        with pytest.raises((ValueError, TypeError)):
            ops._top_k(bad)
    assert [ops._top_k(k) for k in (None, 0, -3, 5, 5.0, np.int64(7), 1 << 40)] == [0, 0, 0, 5, 5, 7, 2 ** 31 - 1]
