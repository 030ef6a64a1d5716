"""Host-side checks of the decoder's forced tokens (no GPU): the float64 restatement of the rule (tests/decoder_forced_ref.py) against
the constrained restatement and the rule's consequences (a) to (d), the replay (b) over decoder_trunc_ref.alone_case rows, the anchor
at the reference's own teacher-forced logits (tests/golden/vae_*.npz), the argument errors of the Python surfaces and of the two new
entry points in front of any launch, the entry points' declarations, and the count of ticks that lie within 2e-5 of a step for the very
masks, patterns and seeds the GPU test runs (tests/test_gpu_decoder_forced.py), held to the caps: at most 3 % of a setting's free draws,
3 % of its forced ticks and 1 % of a test function's draws."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

from inpaintnet_amd import _lib, ops, synthetic
from inpaintnet_amd.latent_rnn import LatentRNN
from inpaintnet_amd.latent_rnn_tester import LatentRNNTester
from inpaintnet_amd.measure_vae import HierarchicalDecoder, MeasureVAE
from oracle import torch_ref as O
from tests import decoder_constraint_ref as CR
from tests import decoder_forced_ref as FR
from tests import decoder_trunc_ref as TR
from tests import golden_util as G
from tests.test_decoder_constraint_host import plan_params, rows, same

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
X = C.c_void_p(16)              # a pointer that is never followed (tests/test_pointwise_host.py)
NULL = None
SETTINGS = ((1.0, 0, 1.0), (1.0, 5, 1.0), (6.0, 0, 0.9), (6.0, 8, 0.7), (-2.0, 3, 0.5), (0.0, 0, 1.0))


@pytest.fixture(scope="module")
def L():
    _lib.build(verbose=False)
    return _lib.lib()


def test_the_settings_and_the_pattern():
    assert FR.FORCED_SETTINGS == ((1.0, 0, 1.0), (6.0, 0, 0.9), (6.0, 8, 0.7))
    f = FR.plan_forced(20, 7)
    assert f.dtype == np.int32 and f.shape == (7, 24)
    for r in range(7):
        for t in range(24):
            assert f[r, t] == ((5 * r + 11 * t + 2) % 20 if (r + 2 * t) % 3 == 0 else -1)
    assert FR.alone_forced(5, 4).tolist() == [1, -1, 3, -1, 1]


@pytest.mark.parametrize("V", [5, 48, 100])
def test_no_forced_tick_is_the_constrained_restatement(V):
    """Consequence (a): forced None, -1, V, V + 7, -2 and the int32 minimum: every return of decoder_constraint_ref.pick, margins included"""
    x, u, allow = rows(f"forced/free/{V}", 40, V)
    for temp, k, p in SETTINGS:
        for xi, ui, ai in zip(x, u, allow):
            want = CR.pick(xi, temp, ui, k, p, ai)
            for f in (None, -1, V, V + 7, -2, -2 ** 31):
                assert same(FR.pick(xi, temp, ui, k, p, ai, f), want), (V, temp, k, p, f)
        got = FR.pick_rows(x, temp, u, k, p, allow, np.full(40, -1))
        want = CR.pick_rows(x, temp, u, k, p, allow)
        assert all(np.array_equal(g, w, equal_nan=True) for g, w in zip(got, want))


@pytest.mark.parametrize("V", [1, 5, 48, 100])
def test_a_forced_token_is_returned_whatever_holds(V):
    """Consequences (c) and (d) and steps 1 to 3: the token is f for every mask, truncation and uniform (NaN and 2.0 among them); a banned
    or truncated f has logp exactly -inf; a one-bit mask at f gives exactly 0.0f; an allowed and kept f gives (s_f - m) - log S, which
    is what a draw of f reports; a NaN among s, or no finite m, gives NaN and still f"""
    x, u, allow = rows(f"forced/any/{V}", 24, V)
    for temp, k, p in SETTINGS:
        for r, (xi, ai) in enumerate(zip(x, allow)):
            for f in sorted({0, (5 * r + 2) % V, V - 1}):
                kept = CR.kept_rows(xi, temp, k, p, ai)
                for uu in (0.0, 0.4, 2.0, np.nan):
                    t, lp, n, cm, bm = FR.pick(xi, temp, uu, k, p, ai, f)
                    assert t == f and lp.dtype == np.float32 and cm == np.inf
                    if not kept[f]:
                        assert lp == -np.inf, (V, temp, k, p, f)
                    else:
                        assert np.isfinite(lp) and lp <= 0.0
                        # the draw that returns f reports the same logp: search a uniform that draws it
                        for ud in np.linspace(0.0, 0.999, 200):
                            d = CR.pick(xi, temp, ud, k, p, ai)
                            if d[0] == f:
                                assert d[1] == lp and d[2] == n and d[4] == bm
                                break
                one = np.arange(V) == f
                t, lp, n, *_ = FR.pick(xi, temp, np.nan, k, p, one, f)
                assert t == f and float(lp) == 0.0 and not np.signbit(lp) and n >= 1, (V, temp, k, p, f, lp)
                if V > 1:
                    t, lp, *_ = FR.pick(xi, temp, 0.3, k, p, ~one, f)                  # banned: still returned
                    assert t == f and lp == -np.inf
            bad = xi.copy()
            bad[V // 2] = np.nan
            t, lp, n, *_ = FR.pick(bad, temp, 0.3, k, p, ai, r % V)
            assert t == r % V and np.isnan(lp) and n == 0
            t, lp, *_ = FR.pick(np.full(V, -np.inf, dtype=np.float32), 1.0, 0.3, k, p, None, r % V)
            assert t == r % V and np.isnan(lp)
        # pick_rows: a free row outside the rule takes the masked argmax, a forced row its token
        uu = u.copy()
        uu[::3] = 2.0
        f = np.where(np.arange(24) % 2 == 0, np.arange(24) % V, -1)
        tok, lp, *_ = FR.pick_rows(x, temp, uu, k, p, allow, f)
        assert np.array_equal(tok[::2], f[::2])
        base = CR.pick_rows(x, temp, uu, k, p, allow)
        assert np.array_equal(tok[1::2], base[0][1::2]) and np.array_equal(lp[1::2], base[1][1::2], equal_nan=True)
        assert not np.isnan(lp[::6]).any() or temp == 0.0 or not np.isfinite(x).all()      # a forced row ignores its uniform


@pytest.mark.parametrize("V", [2, 63, 65, 129])
def test_replay_on_the_restatement(V):
    """Consequence (b) over decoder_trunc_ref.alone_case rows: forcing the tokens a constrained draw returned gives its logp bit for bit
    (NaN where it was NaN) under any uniforms, with and without a mask"""
    for nrows in TR.ALONE_ROWS[:2]:
        x, u = TR.alone_case(V, nrows)
        x = x[:, :V]
        for allow in (None, CR.alone_mask(x)):
            for temp in TR.ALONE_TEMPS:
                for k in TR.alone_top_k(V):
                    for p in TR.ALONE_TOP_P:
                        tok, lp, n, cm, bm, d = CR.pick_rows(x, temp, u[:, 0], k, p, allow)
                        for other in (u[:, 1], np.full(nrows, np.nan), np.full(nrows, 7.0)):
                            rt, rlp, rn, _, rbm, rd = FR.pick_rows(x, temp, other, k, p, allow, tok)
                            assert np.array_equal(rt, tok) and np.array_equal(rn, n) and np.array_equal(rbm, bm)
                            assert np.array_equal(rlp.view(np.int32), lp.view(np.int32)), (V, nrows, temp, k, p)
                            assert np.array_equal(rd, d)


@pytest.mark.parametrize("name", ["small", "mid", "full"])
def test_forcing_the_fixture_tokens_is_the_reference_teacher_forced_pass(name):
    """forced = the fixture's tokens, T = 1, no truncation: the forced trajectory's logits are oracle.torch_ref.decoder_forward(...,
    teacher_forced=True) (the same float64 arithmetic: 1e-12) and the reference's own dec_tf_weights within the 5e-5 test_oracle_golden
    holds the oracle to; its -mean logp is the cross-entropy of dec_tf_weights against the tokens.  Bound on that: a logit error eps
    moves a log-softmax entry by at most 2 eps, eps = (5e-5 + 2^-23, the restatement's f32 rounding of the logits) max|dec_tf_weights|;
    plus logp's own f32 rounding, decoder_trunc_ref.logp_tol."""
    fx = G.load("vae_" + name)
    c = G.CFGS[name]
    P64 = {k: v.double() for k, v in G.vae_params(name, fx).items()}
    z, tok = torch.from_numpy(fx["dec_z"]), fx["tokens"]
    B, T = tok.shape
    w, got, lp, n, cm, bm, d = FR.forced_trajectory(P64, z, 1.0, np.full((B, T), np.nan), 0, 1.0, None, tok)
    assert np.array_equal(got, tok) and (n == c["V"]).all() and np.isfinite(lp).all()
    with torch.no_grad():
        wr, sr = O.decoder_forward(P64, z.double(), torch.from_numpy(tok), teacher_forced=True)
    assert G.rel_err(w, wr.numpy()) < 1e-12
    tf = fx["dec_tf_weights"].astype(np.float64)
    assert G.rel_err(w, tf) < 5e-5
    ls = tf - tf.max(-1, keepdims=True)
    ls = ls - np.log(np.exp(ls).sum(-1, keepdims=True))
    want = np.take_along_axis(ls, tok[..., None], -1)[..., 0]
    eps = (5e-5 + 2.0 ** -23) * np.abs(tf).max()
    err = np.abs(lp.astype(np.float64) - want)
    print(name, "logp error max %.3g, bound %.3g; cross-entropy %.9f against %.9f" % (err.max(), 2 * eps, -lp.astype(np.float64).mean(), -want.mean()))
    assert (err <= 2 * eps + TR.logp_tol(d)).all()
    assert abs(-lp.astype(np.float64).mean() + want.mean()) <= 2 * eps + float(TR.logp_tol(d).max())


@pytest.mark.parametrize("Z", TR.PLAN_Z)
@pytest.mark.parametrize("V", TR.PLAN_V)
def test_margin_counts_of_the_every_plan_test(V, Z):
    """Along the restatement's own trajectory for the seeds, the mask and the pattern of
    test_gpu_decoder_forced.test_every_plan_of_a_forced_call: per setting 420 free draws (ticks with more than one allowed token and no
    forced one) and 280 forced ticks; free draws with a margin below 2e-5 (cap 3 %), forced ticks with the nucleus margin below it (cap
    3 %), both over the function's 2100 draws (cap 1 %).  Every forced tick returns its token; its logp is -inf exactly where the token
    is banned or truncated away; the un-truncated setting leaves every non-banned forced tick finite."""
    P64 = plan_params(V, Z)
    near_all = draws_all = ninf_all = banned_all = 0
    for si, (temp, k, p) in enumerate(FR.FORCED_SETTINGS):
        zs, us = zip(*(TR.plan_inputs(V, Z, B, si) for B in TR.PLAN_B))
        allow = np.concatenate([CR.plan_mask(V, B) for B in TR.PLAN_B])
        forced = np.concatenate([FR.plan_forced(V, B) for B in TR.PLAN_B])
        w, tok, lp, n, cm, bm, d = FR.forced_trajectory(P64, torch.from_numpy(np.concatenate(zs)), temp, np.concatenate(us), k, p, allow, forced)
        isf = forced >= 0
        free = CR.free(allow) & ~isf
        near_free = int((~TR.firm(cm, bm) & free).sum())
        near_forced = int(((bm < TR.MARGIN) & isf).sum())
        is_banned = isf & ~np.take_along_axis(allow, np.maximum(forced, 0)[..., None], -1)[..., 0]
        ninf = int((np.isneginf(lp) & isf).sum())
        print(f"V {V} Z {Z} setting {(temp, k, p)}: {near_free} of {int(free.sum())} free draws within a margin, {near_forced} of "
              f"{int(isf.sum())} forced ticks within the nucleus margin; {ninf} forced ticks -inf, {int(is_banned.sum())} of them banned")
        assert int(free.sum()) == 420 and int(isf.sum()) == 280
        assert np.array_equal(tok[isf], forced[isf]) and not np.isnan(lp).any()
        assert np.isneginf(lp[is_banned]).all()
        kept = CR.kept_rows(w.astype(np.float32), temp, k, p, allow)
        assert np.array_equal(np.isneginf(lp[isf]), ~np.take_along_axis(kept, np.maximum(forced, 0)[..., None], -1)[..., 0][isf])
        if k == 0 and p == 1.0:
            assert np.array_equal(np.isneginf(lp) & isf, is_banned)
        assert np.take_along_axis(allow, tok[..., None], -1)[~isf].all()                  # free ticks: no banned token
        assert near_free <= 0.03 * 420 and near_forced <= 0.03 * 280, (V, Z, temp, k, p, near_free, near_forced)
        near_all, draws_all = near_all + near_free + near_forced, draws_all + 700
        ninf_all, banned_all = ninf_all + ninf, banned_all + int(is_banned.sum())
    print(f"V {V} Z {Z}: {near_all} of {draws_all} draws within a margin; {ninf_all} of 840 forced ticks -inf, {banned_all} banned")
    assert draws_all == 2100 and near_all <= 0.01 * draws_all, (V, Z, near_all, draws_all)
    assert 0.3 * 840 <= banned_all <= 0.5 * 840                                           # (about 40 %: consequence (c) throughout)


@pytest.mark.parametrize("V", TR.ALONE_V)
def test_margin_counts_of_the_kernel_alone_test(V):
    """The same for the rows, masks and pattern of test_gpu_decoder_forced.test_the_forced_kernel_alone: per (mask or none, temperature,
    top_k, top_p) setting the forced rows of its three row counts with the nucleus margin below 2e-5 (cap 3 %), per vocabulary all
    settings (cap 1 %).  The tie rows compare exactly: whether a forced token is kept does not depend on expf's last bit."""
    near_all = rows_all = 0
    cases = [TR.alone_case(V, r) for r in TR.ALONE_ROWS]
    for masked in (True, False):
        for temp in TR.ALONE_TEMPS:
            for k in TR.alone_top_k(V):
                for p in TR.ALONE_TOP_P:
                    near = n = 0
                    for x, u in cases:
                        f = FR.alone_forced(len(x), V)
                        isf = f >= 0
                        a = CR.alone_mask(x[:, :V])[isf] if masked else None
                        bm = FR.pick_rows(x[isf, :V], temp, u[isf, 0], k, p, a, f[isf])[4]
                        near, n = near + int((bm < TR.MARGIN).sum()), n + int(isf.sum())
                    assert near <= 0.03 * n, (V, masked, temp, k, p, near, n)
                    near_all, rows_all = near_all + near, rows_all + n
    print(f"V {V}: {near_all} of {rows_all} forced rows within the nucleus margin")
    assert near_all <= 0.01 * rows_all, (V, near_all, rows_all)
    t = TR.tie_rows(V)
    a = np.broadcast_to(np.arange(V) % 2 == 1, t.shape) if V > 1 else np.ones_like(t, dtype=bool)
    for temp in TR.ALONE_TEMPS:
        for k in TR.alone_top_k(V):
            for p in TR.ALONE_TOP_P:
                for r, (row, ai) in enumerate(zip(t, a)):
                    for shift in (0, 1, 63, 64):
                        f = (r + shift) % V
                        base = FR.pick(row, temp, np.nan, k, p, ai, f)
                        for ulps in (-1, 1):
                            other = FR.pick(row, temp, np.nan, k, p, ai, f, e_ulps=ulps)
                            assert (other[0], other[2], np.isneginf(other[1])) == (base[0], base[2], np.isneginf(base[1])), (V, temp, k, p, f)


def _tester_stub(V=11):
    stub = types.SimpleNamespace(measure_seq_len=24,
                                 model=types.SimpleNamespace(vae_model=types.SimpleNamespace(decoder=types.SimpleNamespace(
                                     cfg=types.SimpleNamespace(num_notes=V)))))
    stub._allowed = types.MethodType(LatentRNNTester._allowed, stub)
    return stub


def test_the_python_surfaces_refuse_bad_forced_tokens():
    """ValueError in front of any work and before anything random is drawn: score()'s fillings of another shape, type or range, a
    temperature that is none; generate(score_fixed=True) without a temperature; forced of a wrong shape or dtype, outside [-1, V), with
    train=True or without a temperature at HierarchicalDecoder.forward and LatentRNN.forward; ops.decoder_fwd without a temperature"""
    V = 11
    stub = _tester_stub(V)
    past = future = torch.zeros(1, 2, 24, dtype=torch.int64)
    good = torch.zeros(2, 3, 24, dtype=torch.int64)
    state = np.random.get_state()[1].copy()
    for bad in (dict(fillings=good.float()), dict(fillings=good[:, :, :23]), dict(fillings=good[0]), dict(fillings=good.bool()),
                dict(fillings=good + V), dict(fillings=good - 1), dict(fillings=good[:0]), dict(fillings=good, temperature=None),
                dict(fillings=good, temperature=float("inf")), dict(fillings=good, top_p=0.0), dict(fillings=good, top_p=1.5),
                dict(fillings=good, top_k=2.5), dict(fillings=good, banned_tokens=[V]), dict(fillings=good, banned_tokens=list(range(V)))):
        with pytest.raises(ValueError):
            LatentRNNTester.score(stub, past, future, **bad)
    with pytest.raises(ValueError):
        LatentRNNTester.score(stub, past.expand(2, -1, -1), future, good)
    fixed = torch.full((3, 24), -1, dtype=torch.int64)
    fixed[1, 4] = 3
    with pytest.raises(ValueError, match="score_fixed"):
        LatentRNNTester.generate(stub, past, future, None, 3, fixed_tokens=fixed, score_fixed=True)
    with pytest.raises(ValueError):
        LatentRNNTester.generate(stub, past, future, None, 3, temperature=6.0, fixed_tokens=fixed + V, score_fixed=True)
    dec = types.SimpleNamespace(cfg=types.SimpleNamespace(beats=4, ticks_per_beat=6, num_notes=V))
    z = torch.zeros(2, 8)
    f = torch.full((2, 24), -1, dtype=torch.int64)
    for kw in (dict(forced=f.float(), temperature=1.0), dict(forced=f.bool(), temperature=1.0), dict(forced=f[:, :23], temperature=1.0),
               dict(forced=f[:1], temperature=1.0), dict(forced=f + V + 1, temperature=1.0), dict(forced=f - 1, temperature=1.0),
               dict(forced=f), dict(forced=f, temperature=1.0, train=True)):
        with pytest.raises(ValueError):
            HierarchicalDecoder.forward(dec, z, None, **{"train": False, **kw})
    with pytest.raises(ValueError):
        MeasureVAE.decode(types.SimpleNamespace(num_ticks_per_measure=24, decoder=lambda *a, **k: HierarchicalDecoder.forward(dec, *a, **k)),
                          z, forced=f)
    rnn = types.SimpleNamespace(vae_model=types.SimpleNamespace(decoder=dec))
    f3 = torch.full((1, 3, 24), -1, dtype=torch.int64)
    for kw in (dict(forced=f3.float(), temperature=1.0), dict(forced=f3[:, :2], temperature=1.0), dict(forced=f3 + V + 1, temperature=1.0),
               dict(forced=f3 - 1, temperature=1.0), dict(forced=f3), dict(forced=f3, temperature=1.0, train=True),
               dict(forced=f3.view(3, 24), temperature=1.0)):
        with pytest.raises(ValueError):
            LatentRNN.forward(rnn, past, future, None, 3, **{"train": False, **kw})
    assert np.array_equal(np.random.get_state()[1], state)                      # nothing random was drawn
    with pytest.raises(ValueError):
        ops.decoder_fwd(ops.vae_config(48), None, None, False, None, forced=torch.zeros(1, 24, dtype=torch.int32))


def test_argument_errors_of_the_new_entry_points(L):
    """-1 in front of any launch: a null required pointer, rows / V out of range, a non-finite temperature, a top_p outside (0, 1] -- with
    and without a mask beside the forced tokens (X is never followed)"""
    cfg = ops.vae_config(48)
    inf, nan = float("inf"), float("nan")
    big = 1 << 40
    sf = lambda *a: L.inet_sample_forced(*a)
    dec = lambda *a: L.inet_vae_decoder_sample_fx(C.byref(cfg), *a)
    calls = {}
    for tag, al, fo in (("mask + forced", X, X), ("forced", NULL, X), ("mask", X, NULL), ("neither", NULL, NULL)):
        calls.update({
            f"sf weights {tag}": sf(NULL, 4, 1, 4, 1.0, X, 1, 2, 0.9, X, 1, X, 1, al, 1, fo, 1, NULL),
            f"sf uniforms {tag}": sf(X, 4, 1, 4, 1.0, NULL, 1, 2, 0.9, X, 1, X, 1, al, 1, fo, 1, NULL),
            f"sf out {tag}": sf(X, 4, 1, 4, 1.0, X, 1, 2, 0.9, NULL, 1, X, 1, al, 1, fo, 1, NULL),
            f"sf rows {tag}": sf(X, 4, 0, 4, 1.0, X, 1, 2, 0.9, X, 1, X, 1, al, 1, fo, 1, NULL),
            f"sf V {tag}": sf(X, 4, 1, 0, 1.0, X, 1, 2, 0.9, X, 1, X, 1, al, 1, fo, 1, NULL),
            f"sf V > 512 {tag}": sf(X, 513, 1, 513, 1.0, X, 1, 2, 0.9, X, 1, X, 1, al, 9, fo, 1, NULL),
            f"sf inf {tag}": sf(X, 4, 1, 4, inf, X, 1, 2, 0.9, X, 1, X, 1, al, 1, fo, 1, NULL),
            f"sf nan {tag}": sf(X, 4, 1, 4, nan, X, 1, 2, 0.9, X, 1, X, 1, al, 1, fo, 1, NULL),
            f"sf top_p 0 {tag}": sf(X, 4, 1, 4, 1.0, X, 1, 2, 0.0, X, 1, X, 1, al, 1, fo, 1, NULL),
            f"sf top_p > 1 {tag}": sf(X, 4, 1, 4, 1.0, X, 1, 2, 1.0000001, X, 1, X, 1, al, 1, fo, 1, NULL),
            f"sf top_p nan {tag}": sf(X, 4, 1, 4, 1.0, X, 1, 2, nan, X, 1, X, 1, al, 1, fo, 1, NULL),
            f"dec z {tag}": dec(1, NULL, X, NULL, NULL, X, X, X, big, 0, 1.0, X, 2, 0.9, X, al, fo, NULL),
            f"dec params {tag}": dec(1, X, NULL, NULL, NULL, X, X, X, big, 0, 1.0, X, 2, 0.9, X, al, fo, NULL),
            f"dec weights {tag}": dec(1, X, X, NULL, NULL, NULL, X, X, big, 0, 1.0, X, 2, 0.9, X, al, fo, NULL),
            f"dec samples {tag}": dec(1, X, X, NULL, NULL, X, NULL, X, big, 0, 1.0, X, 2, 0.9, X, al, fo, NULL),
            f"dec ws {tag}": dec(1, X, X, NULL, NULL, X, X, NULL, big, 0, 1.0, X, 2, 0.9, X, al, fo, NULL),
            f"dec ws_bytes {tag}": dec(1, X, X, NULL, NULL, X, X, X, 16, 0, 1.0, X, 2, 0.9, X, al, fo, NULL),
            f"dec uniforms {tag}": dec(1, X, X, NULL, NULL, X, X, X, big, 0, 1.0, NULL, 2, 0.9, X, al, fo, NULL),
            f"dec batch {tag}": dec(0, X, X, NULL, NULL, X, X, X, big, 0, 1.0, X, 2, 0.9, X, al, fo, NULL),
            f"dec inf {tag}": dec(1, X, X, NULL, NULL, X, X, X, big, 0, inf, X, 2, 0.9, X, al, fo, NULL),
            f"dec top_p 0 {tag}": dec(1, X, X, NULL, NULL, X, X, X, big, 0, 1.0, X, 2, 0.0, X, al, fo, NULL),
            f"dec top_p nan {tag}": dec(1, X, X, NULL, NULL, X, X, X, big, 0, 1.0, X, 0, nan, X, al, fo, NULL),
        })
    assert {k: v for k, v in calls.items() if v != -1} == {}
    # a forced call has the constrained call's plan: no plan entry of its own; the ABI version did not move
    assert not hasattr(L, "inet_decode_b1_plan_force") and L.inet_abi_version() == 1


def test_the_new_entry_points_are_declared_as_bound():
    """include/inpaintnet_hip.h declares inet_vae_decoder_sample_fx = inet_vae_decoder_sample_cx + `const int32_t* forced` in front of the
    stream and inet_sample_forced = inet_sample_constrained + `const int32_t* forced, int64_t forced_stride`; _lib's argtypes match the
    declarations type by type, and INTEGRATION.md quotes both"""
    hdr = open(os.path.join(REPO, "include", "inpaintnet_hip.h")).read()

    def decl(name):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, name
        return [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]

    def ctype(arg):
        if "*" in arg:
            return C.c_void_p
        return {"int": C.c_int, "int64_t": C.c_int64, "float": C.c_float, "double": C.c_double}[arg.rsplit(" ", 1)[0]]
    fx, cx = decl("inet_vae_decoder_sample_fx"), decl("inet_vae_decoder_sample_cx")
    assert fx == cx[:-1] + ["const int32_t* forced"] + cx[-1:]
    sf, sc = decl("inet_sample_forced"), decl("inet_sample_constrained")
    assert sf == sc[:-1] + ["const int32_t* forced", "int64_t forced_stride"] + sc[-1:]
    for name, args in (("inet_vae_decoder_sample_fx", fx), ("inet_sample_forced", sf)):
        assert name in _lib.EXPORTS
        res, argtypes = _lib._SIGNATURES[name]
        assert res is C.c_int and len(argtypes) == len(args), name
        for a, t in zip(args, argtypes):
            if "inet_vae_config" in a:
                assert t is not C.c_void_p and issubclass(t, C._Pointer), (name, a)
            else:
                assert t is ctype(a), (name, a, t)
    md = open(os.path.join(REPO, "INTEGRATION.md")).read()
    assert "_L.inet_vae_decoder_sample_fx.argtypes" in md and "_L.inet_sample_forced.argtypes" in md
    for text in (hdr, open(os.path.join(REPO, "inpaintnet_amd", "csrc", "sample.h")).read(), open(os.path.join(REPO, "DESIGN.md")).read(),
                 open(os.path.join(REPO, "tests", "decoder_forced_ref.py")).read()):
        flat = re.sub(r"[\s/*#`]+", " ", text)
        for phrase in ("A value f with 0 <= f < V forces that tick", "The tick's uniform is not used",
                       "It is exactly -inf when f is banned or truncated away", "One-bit mask. A forced tick whose mask has the single bit f set"):
            assert phrase in flat, phrase
