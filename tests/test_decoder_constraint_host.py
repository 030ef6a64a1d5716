"""Host-side checks of the decoder's per-tick token constraints (no GPU): the float64 restatement of the rule
(tests/decoder_constraint_ref.py) against the truncated restatement and against the rule's four consequences, ops.pack_allowed's bit
order, the argument errors of generate() and of the two new entry points in front of any launch, and the count of free draws that lie
within 2e-5 of a step -- of the kept CDF or of the nucleus boundary -- for the very masks and seeds the GPU tests run
(tests/test_gpu_decoder_constraint.py), held to the caps: at most 1 % of a test function's free draws and 3 % of a setting's."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from inpaintnet_amd import _lib, layout, ops, synthetic
from inpaintnet_amd.latent_rnn_tester import LatentRNNTester
from tests import decoder_constraint_ref as CR
from tests import decoder_trunc_ref as TR
from tests import golden_util as G

X = C.c_void_p(16)              # a pointer that is never followed (tests/test_pointwise_host.py)
NULL = None
SETTINGS = ((1.0, 0, 1.0), (1.0, 5, 1.0), (6.0, 0, 0.9), (6.0, 8, 0.7), (-2.0, 3, 0.5), (0.0, 0, 1.0))


@pytest.fixture(scope="module")
def L():
    _lib.build(verbose=False)
    return _lib.lib()


def rows(tag, n, V, scale=0.6):
    x = np.maximum(synthetic.det_normal(f"decoder_cons/host/{tag}", (n, V), scale), 0.0).astype(np.float32)
    u = synthetic.det_uniform(f"decoder_cons/host/u/{tag}", (n,), 0.0, 1.0).astype(np.float64)
    allow = synthetic.det_uniform(f"decoder_cons/host/allow/{tag}", (n, V), 0.0, 1.0) < 0.6
    allow[np.arange(n), np.arange(n) % V] = True                # (no empty row)
    return x, u, allow


def same(a, b):
    """two pick() returns, NaN == NaN"""
    return all((x == y) or (x != x and y != y) for x, y in zip(a, b))


@pytest.mark.parametrize("V", [5, 48, 100])
def test_a_full_mask_is_the_truncated_restatement(V):
    """allow None, all ones and all zeros (the empty mask counts as all ones): every return of decoder_trunc_ref.pick, margins included"""
    x, u, _ = rows(f"full/{V}", 60, V)
    for temp, k, p in SETTINGS:
        for xi, ui in zip(x, u):
            want = TR.pick(xi, temp, ui, k, p)
            for allow in (None, np.ones(V, dtype=bool), np.zeros(V, dtype=bool)):
                assert same(CR.pick(xi, temp, ui, k, p, allow), want), (V, temp, k, p)
        assert np.array_equal(CR.kept_rows(x, temp, k, p), TR.kept_rows(x, temp, k, p))
        got, want = CR.pick_rows(x, temp, u, k, p, np.ones((60, V), dtype=bool)), TR.pick_rows(x, temp, u, k, p)
        assert all(np.array_equal(g, w, equal_nan=True) for g, w in zip(got, want))


@pytest.mark.parametrize("V", [5, 48, 100])
def test_a_masked_draw_is_the_unmasked_draw_on_minus_infinity(V):
    """Consequence 4, T > 0: the masked draw on x = decoder_trunc_ref.pick on x with -inf written at the banned places, every return"""
    x, u, allow = rows(f"inf/{V}", 60, V)
    for temp, k, p in SETTINGS:
        if temp <= 0:
            continue
        for xi, ui, ai in zip(x, u, allow):
            filled = np.where(ai, xi, np.float32(-np.inf)).astype(np.float32)
            got, want = CR.pick(xi, temp, ui, k, p, ai), TR.pick(filled, temp, ui, k, p)
            assert same(got, want), (V, temp, k, p, got, want)
            assert got[0] >= 0 and ai[got[0]]


@pytest.mark.parametrize("V", [1, 5, 48, 100])
def test_a_one_bit_mask_returns_its_token_with_logp_zero(V):
    """Consequence 2: for every u in [0, 1) and every finite temperature the token is the mask's, logp is exactly 0.0f and one token is
    kept; on a fallback tick (u outside [0, 1) or NaN, a NaN among s) the token is still the mask's and logp is NaN"""
    x, _, _ = rows(f"one/{V}", 12, V)
    for r, xi in enumerate(x):
        tok = (5 * r + 2) % V
        one = np.arange(V) == tok
        for temp in (1.0, 6.0, -2.0, 0.0, 1e30, -1e-30):
            for k, p in ((0, 1.0), (1, 1.0), (3, 0.5), (V + 5, 1e-9)):
                for u in (0.0, 0.25, 0.999999, np.nextafter(1.0, 0.0)):
                    t, lp, n, cm, bm = CR.pick(xi, temp, u, k, p, one)
                    assert t == tok and lp.dtype == np.float32 and float(lp) == 0.0 and not np.signbit(lp), (V, temp, k, p, u, t, lp)
                assert CR.kept_rows(xi, temp, k, p, one).tolist() == one.tolist()
                for u in (1.0, 2.0, -0.5, np.nan):
                    assert CR.pick(xi, temp, u, k, p, one)[0] == -1
                    t, lp, *_ = CR.pick_rows(xi[None], temp, np.array([u]), k, p, one[None])
                    assert t[0] == tok and np.isnan(lp[0])
        bad = xi.copy()
        bad[(tok + 1) % V] = np.inf                             # (V > 1: a banned +inf; times T = 0 a NaN among s -- the tick falls back)
        t, lp, *_ = CR.pick_rows(bad[None], 0.0, np.array([0.3]), 0, 1.0, one[None])
        assert t[0] == tok and (np.isnan(lp[0]) or V == 1)


@pytest.mark.parametrize("V", [5, 48, 100])
def test_no_banned_token_is_ever_returned(V):
    """Consequence 3, fallback ticks included: uniforms outside [0, 1), NaN and infinite logits at banned and allowed places, allowed
    tokens that are all -inf"""
    x, u, allow = rows(f"ban/{V}", 60, V)
    x[3, np.flatnonzero(~allow[3])[:1]] = np.nan
    x[4, np.flatnonzero(~allow[4])[:1]] = np.inf
    x[5, np.flatnonzero(allow[5])[:1]] = np.nan
    x[6, np.flatnonzero(allow[6])[:1]] = np.inf
    x[7, allow[7]] = -np.inf
    uu = u.copy()
    uu[8::4] = 2.0
    uu[9::4] = np.nan
    for temp, k, p in SETTINGS:
        tok, lp, n, cm, bm, d = CR.pick_rows(x, temp, uu, k, p, allow)
        assert allow[np.arange(60), tok].all(), (V, temp, k, p)
        assert np.isnan(lp[8::4]).all() and np.isnan(lp[9::4]).all() and np.isnan(lp[3]) and np.isnan(lp[7])
        kept = CR.kept_rows(x, temp, k, p, allow)
        assert not (kept & ~allow).any()
    assert CR.masked_argmax(x[7], allow[7]) == np.flatnonzero(allow[7])[0]
    assert CR.masked_argmax(x[5], allow[5]) == np.flatnonzero(allow[5])[0]                 # a NaN is the maximum
    filled = np.where(allow[10], x[10], -np.inf)
    assert CR.masked_argmax(x[10], allow[10]) == int(np.argmax(filled))


def test_pack_allowed_packs_the_bit_order():
    """token v = bit v % 64 of word v // 64, bits at or above V zero: single bits at 0, 62, 63, 64, 65, V - 1 for V = 1, 63, 64, 65, 128,
    129, 512, random masks against the restatement's words(), leading dimensions kept; the ValueErrors"""
    for V in (1, 63, 64, 65, 128, 129, 512):
        nw = (V + 63) // 64
        for v in sorted({0, 62, 63, 64, 65, 127, 128, V - 1}):
            if v >= V:
                continue
            a = np.zeros((1, V), dtype=bool)
            a[0, v] = True
            w = ops.pack_allowed(torch.from_numpy(a))
            assert w.dtype == torch.int64 and tuple(w.shape) == (1, nw) and w.device.type == "cpu"
            got = w.numpy().view(np.uint64)[0]
            assert [int(g) for g in got] == [(1 << (v % 64)) if j == v // 64 else 0 for j in range(nw)], (V, v, got)
        a = synthetic.det_uniform(f"decoder_cons/host/pack/{V}", (3, 4, V), 0.0, 1.0) < 0.5
        a[..., 0] = True
        w = ops.pack_allowed(a)                                 # (an array: packed to a CPU tensor)
        assert tuple(w.shape) == (3, 4, nw) and w.is_contiguous()
        assert np.array_equal(w.numpy().view(np.uint64), CR.words(a))
        full = ops.pack_allowed(np.ones((2, V), dtype=bool)).numpy().view(np.uint64)
        last = V - 64 * (nw - 1)
        assert all(int(full[0, j]) == 2 ** 64 - 1 for j in range(nw - 1)) and int(full[0, nw - 1]) == 2 ** last - 1
    bit63 = np.zeros((1, 64), dtype=bool)
    bit63[0, 63] = True
    assert int(ops.pack_allowed(bit63)[0, 0]) == -2 ** 63       # (the int64 with that bit pattern)
    empty = np.ones((2, 3, 65), dtype=bool)
    empty[1, 2] = False
    with pytest.raises(ValueError, match=r"\[1, 2\]"):
        ops.pack_allowed(empty)
    for bad in (np.ones((2, 5)), np.ones((2, 5), dtype=np.int64), np.bool_(True), np.ones((2, 0), dtype=bool)):
        with pytest.raises(ValueError):
            ops.pack_allowed(bad)


def test_generate_refuses_bad_constraints():
    """banned_tokens / fixed_tokens outside [0, V), a ban of the whole vocabulary, a fixed_tokens of another shape or type: ValueError in
    front of any work; the mask they give: a fixed tick wins over a ban"""
    V = 11
    stub = types.SimpleNamespace(measure_seq_len=24,
                                 model=types.SimpleNamespace(vae_model=types.SimpleNamespace(decoder=types.SimpleNamespace(
                                     cfg=types.SimpleNamespace(num_notes=V)))))
    stub._allowed = types.MethodType(LatentRNNTester._allowed, stub)
    past = future = torch.zeros(1, 2, 24, dtype=torch.int64)
    free = torch.full((3, 24), -1, dtype=torch.int64)

    def fixed(t, v):
        f = free.clone()
        f[1, t] = v
        return f
    for bad in (dict(banned_tokens=[V]), dict(banned_tokens=[-1]), dict(banned_tokens=[2.5]), dict(banned_tokens=list(range(V))),
                dict(fixed_tokens=fixed(0, V)), dict(fixed_tokens=fixed(5, -2)), dict(fixed_tokens=free[:2]),
                dict(fixed_tokens=free.float()), dict(fixed_tokens=free[:, :23]), dict(banned_tokens=[0], fixed_tokens=fixed(3, 99))):
        for temp in (None, 6.0):
            with pytest.raises(ValueError):
                LatentRNNTester.generate(stub, past, future, None, 3, temperature=temp, **bad)
    assert stub._allowed(None, None, 3) is None
    a = stub._allowed([0, 4], fixed(7, 4), 3)
    assert tuple(a.shape) == (3, 24, V) and a.dtype == torch.bool
    assert a[1, 7].tolist() == [v == 4 for v in range(V)]                      # the fixed tick wins over the ban of token 4
    assert a[0, 0].tolist() == [v not in (0, 4) for v in range(V)] and int(a.sum()) == (3 * 24 - 1) * (V - 2) + 1
    assert stub._allowed(None, fixed(2, 0), 3)[1, 2].tolist() == [v == 0 for v in range(V)]
    with pytest.raises(ValueError):
        ops.decoder_fwd(ops.vae_config(48), None, None, False, None, allowed=torch.zeros(1, 24, 1, dtype=torch.int64))


def test_argument_errors_of_the_new_entry_points(L):
    """-1 in front of any launch: a null required pointer, rows / V out of range, a non-finite temperature, a top_p outside (0, 1] -- with
    and without a mask (X is never followed)"""
    cfg = ops.vae_config(48)
    inf, nan = float("inf"), float("nan")
    big = 1 << 40
    sc = lambda *a: L.inet_sample_constrained(*a)
    dec = lambda *a: L.inet_vae_decoder_sample_cx(C.byref(cfg), *a)
    calls = {}
    for tag, al in (("mask", X), ("null mask", NULL)):
        calls.update({
            f"sc weights {tag}": sc(NULL, 4, 1, 4, 1.0, X, 1, 2, 0.9, X, 1, X, 1, al, 1, NULL),
            f"sc uniforms {tag}": sc(X, 4, 1, 4, 1.0, NULL, 1, 2, 0.9, X, 1, X, 1, al, 1, NULL),
            f"sc out {tag}": sc(X, 4, 1, 4, 1.0, X, 1, 2, 0.9, NULL, 1, X, 1, al, 1, NULL),
            f"sc rows {tag}": sc(X, 4, 0, 4, 1.0, X, 1, 2, 0.9, X, 1, X, 1, al, 1, NULL),
            f"sc V {tag}": sc(X, 4, 1, 0, 1.0, X, 1, 2, 0.9, X, 1, X, 1, al, 1, NULL),
            f"sc V > 512 {tag}": sc(X, 513, 1, 513, 1.0, X, 1, 2, 0.9, X, 1, X, 1, al, 9, NULL),
            f"sc inf {tag}": sc(X, 4, 1, 4, inf, X, 1, 2, 0.9, X, 1, X, 1, al, 1, NULL),
            f"sc nan {tag}": sc(X, 4, 1, 4, nan, X, 1, 2, 0.9, X, 1, X, 1, al, 1, NULL),
            f"sc top_p 0 {tag}": sc(X, 4, 1, 4, 1.0, X, 1, 2, 0.0, X, 1, X, 1, al, 1, NULL),
            f"sc top_p > 1 {tag}": sc(X, 4, 1, 4, 1.0, X, 1, 2, 1.0000001, X, 1, X, 1, al, 1, NULL),
            f"sc top_p nan {tag}": sc(X, 4, 1, 4, 1.0, X, 1, 2, nan, X, 1, X, 1, al, 1, NULL),
            f"dec z {tag}": dec(1, NULL, X, NULL, NULL, X, X, X, big, 0, 1.0, X, 2, 0.9, X, al, NULL),
            f"dec params {tag}": dec(1, X, NULL, NULL, NULL, X, X, X, big, 0, 1.0, X, 2, 0.9, X, al, NULL),
            f"dec weights {tag}": dec(1, X, X, NULL, NULL, NULL, X, X, big, 0, 1.0, X, 2, 0.9, X, al, NULL),
            f"dec samples {tag}": dec(1, X, X, NULL, NULL, X, NULL, X, big, 0, 1.0, X, 2, 0.9, X, al, NULL),
            f"dec ws {tag}": dec(1, X, X, NULL, NULL, X, X, NULL, big, 0, 1.0, X, 2, 0.9, X, al, NULL),
            f"dec ws_bytes {tag}": dec(1, X, X, NULL, NULL, X, X, X, 16, 0, 1.0, X, 2, 0.9, X, al, NULL),
            f"dec uniforms {tag}": dec(1, X, X, NULL, NULL, X, X, X, big, 0, 1.0, NULL, 2, 0.9, X, al, NULL),
            f"dec batch {tag}": dec(0, X, X, NULL, NULL, X, X, X, big, 0, 1.0, X, 2, 0.9, X, al, NULL),
            f"dec inf {tag}": dec(1, X, X, NULL, NULL, X, X, X, big, 0, inf, X, 2, 0.9, X, al, NULL),
            f"dec top_p 0 {tag}": dec(1, X, X, NULL, NULL, X, X, X, big, 0, 1.0, X, 2, 0.0, X, al, NULL),
            f"dec top_p > 1 {tag}": dec(1, X, X, NULL, NULL, X, X, X, big, 0, 1.0, X, 0, 1.5, NULL, al, NULL),
            f"dec top_p nan {tag}": dec(1, X, X, NULL, NULL, X, X, X, big, 0, 1.0, X, 0, nan, X, al, NULL),
        })
    long_cfg = ops.vae_config(48, beats=11, ticks_per_beat=6)                      # 66 ticks: more than 64
    calls["dec 66 ticks"] = L.inet_vae_decoder_sample_cx(C.byref(long_cfg), 1, X, X, NULL, NULL, X, X, X, big, 0, 1.0, X, 2, 0.9, X, X, NULL)
    long_cfg = ops.vae_config(48, beats=4, ticks_per_beat=17)                      # 68 ticks in four beats
    calls["dec 68 ticks"] = L.inet_vae_decoder_sample_cx(C.byref(long_cfg), 1, X, X, NULL, NULL, X, X, X, big, 0, 1.0, X, 2, 0.9, X, X, NULL)
    assert {k: v for k, v in calls.items() if v != -1} == {}
    # a constrained call has the truncated call's plan: no plan entry of its own
    assert not hasattr(L, "inet_decode_b1_plan_cons")


def plan_params(V, Z):
    c = G.CFGS["full"]
    P = {k: torch.from_numpy(synthetic.det_param(k, s)) for k, s in layout.vae_param_shapes(V, c["E"], c["H"], Z, c["H"]).items()}
    return {k: v.double() for k, v in P.items()}


@pytest.mark.parametrize("Z", TR.PLAN_Z)
@pytest.mark.parametrize("V", TR.PLAN_V)
def test_margin_counts_of_the_every_plan_test(V, Z):
    """Along the restatement's own masked trajectory for the seeds and the mask of
    test_gpu_decoder_constraint.test_every_plan_of_a_constrained_call: free draws with a margin below 2e-5, per setting (cap 3 %) and over
    the function's free draws (cap 1 %).  Every fixed tick returns its token with logp exactly 0."""
    P64 = plan_params(V, Z)
    near_all = draws_all = 0
    for si, (temp, k, p) in enumerate(TR.SETTINGS):
        zs, us = zip(*(TR.plan_inputs(V, Z, B, si) for B in TR.PLAN_B))
        allow = np.concatenate([CR.plan_mask(V, B) for B in TR.PLAN_B])
        w, tok, n, cm, bm = CR.constrained_trajectory(P64, torch.from_numpy(np.concatenate(zs)), temp, np.concatenate(us), k, p, allow)
        free = CR.free(allow)
        near, draws = int((~TR.firm(cm, bm) & free).sum()), int(free.sum())
        print(f"V {V} Z {Z} setting {(temp, k, p)}: {near} of {draws} free draws within the margin, kept mean {n[free].mean():.1f} of {V}")
        assert np.take_along_axis(allow, tok[..., None], -1).all()
        assert np.array_equal(tok[~free], np.argmax(allow, -1)[~free])
        assert near <= 0.03 * draws, (V, Z, temp, k, p, near, draws)
        near_all, draws_all = near_all + near, draws_all + draws
    assert draws_all == 1890
    assert near_all <= 0.01 * draws_all, (V, Z, near_all, draws_all)


@pytest.mark.parametrize("V", TR.ALONE_V)
def test_margin_counts_of_the_kernel_alone_test(V):
    """The same for the rows and the mask of test_gpu_decoder_constraint.test_the_masked_kernel_alone: per (temperature, top_k, top_p)
    setting the free draws of its three row counts (cap 3 %), per vocabulary all settings (cap 1 %).  The row's single zero stays
    allowed.  The tie rows with every second token banned are compared exactly: neither token nor kept count depends on expf's last bit."""
    cases = [TR.alone_case(V, r) for r in TR.ALONE_ROWS]
    masks = [CR.alone_mask(x[:, :V]) for x, _ in cases]
    for (x, _), a in zip(cases, masks):
        assert a[x[:, :V] == 0].all()
    near_all = draws_all = 0
    for temp in TR.ALONE_TEMPS:
        for k in TR.alone_top_k(V):
            for p in TR.ALONE_TOP_P:
                near = draws = 0
                for (x, u), a in zip(cases, masks):
                    _, _, _, cm, bm, _ = CR.pick_rows(x[:, :V], temp, u[:, 0], k, p, a)
                    free = CR.free(a)
                    near, draws = near + int((~TR.firm(cm, bm) & free).sum()), draws + int(free.sum())
                assert near <= 0.03 * draws, (V, temp, k, p, near, draws)
                near_all, draws_all = near_all + near, draws_all + draws
    print(f"V {V}: {near_all} of {draws_all} free draws within the margin")
    assert near_all <= 0.01 * draws_all, (V, near_all, draws_all)
    t = TR.tie_rows(V)
    a = np.broadcast_to(np.arange(V) % 2 == 1, t.shape) if V > 1 else np.ones_like(t, dtype=bool)
    for temp in TR.ALONE_TEMPS:
        for k in TR.alone_top_k(V):
            for p in TR.ALONE_TOP_P:
                for row, ai in zip(t, a):
                    for u in (0.05, 0.37, 0.81):
                        base = CR.pick(row, temp, u, k, p, ai)
                        for ulps in (-1, 1):
                            other = CR.pick(row, temp, u, k, p, ai, e_ulps=ulps)
                            assert (other[0], other[2]) == (base[0], base[2]), (V, temp, k, p, u, ulps)
