"""Host-side checks of AnticipationRNN's forced tokens (no GPU): the consequences (a) to (e) of the rule (tests/decoder_forced_ref.py) along
the float64 oracle's trajectory (tests/arnn_forced_ref.py); the count of ticks within 2e-5 of a step for the very masks, patterns,
settings and seeds tests/test_gpu_arnn_forced.py runs, held to arnn_trunc_ref.NEAR_CAP and to the counts DESIGN.md section 17 records;
the new entry's signature in the header and in the package's binding; what the entry refuses; the argument errors of the Python
surfaces in front of any library call and before np.random moves."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

from inpaintnet_amd import _lib, ops
from tests import arnn_forced_ref as AF
from tests import arnn_trunc_ref as AR
from tests import decoder_constraint_ref as CR
from tests import decoder_forced_ref as FR
from tests import decoder_trunc_ref as TR

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.asarray(a, dtype=np.float32).view(np.int32)


def test_the_settings_and_the_pattern_are_the_decoders():
    assert FR.FORCED_SETTINGS == ((1.0, 0, 1.0), (6.0, 0, 0.9), (6.0, 8, 0.7)) and AR.L == 30
    f = FR.plan_forced(48, 11, AR.L)
    assert f.dtype == np.int32 and f.shape == (11, AR.L) and int((f >= 0).sum()) == 110
    assert (f[8:] != f[:3])[f[8:] >= 0].all()                  # rows of a second launch are forced to other tokens than the first's


@pytest.mark.parametrize("V,cfg", [(48, AR.FULL), (12, {k: v for k, v in AR.SMALL.items() if k != "V"})])
def test_the_consequences_on_the_oracle(V, cfg):
    """(a) no forced tick: the constrained trajectory; (b) the replay of a constrained trajectory under any uniforms: its logits, tokens
    and logp bit for bit; (c) a banned forced token is returned and FED BACK -- the logits are the network's function of the returned
    tokens --, logp -inf; (d) a forced tick under its own one-bit mask: exactly 0.0f; (e) the free ticks of a partly forced call are the
    constrained rule on the logits behind the forced tokens."""
    R = 5
    W = AR.net(V, **cfg)
    allow, forced = CR.plan_mask(V, R, AR.L), FR.plan_forced(V, R, AR.L)
    isf = forced >= 0
    for si, (temp, k, p) in enumerate(FR.FORCED_SETTINGS):
        oc, hc, u = AR.case(V, R, si, **cfg)
        # (a)
        w0, tok0, lp0, n0, cm0, bm0, d0 = AF.forced_trajectory(W, oc, hc, temp, u, k, p, allow, None)
        want, wlp, *_ = CR.pick_rows(w0.astype(np.float32), temp, u, k, p, allow)
        assert np.array_equal(tok0, want) and np.array_equal(bits(lp0), bits(wlp))
        for none in (np.full((R, AR.L), -1), np.full((R, AR.L), V), np.full((R, AR.L), -2 ** 31)):
            w1, tok1, lp1, *_ = AF.forced_trajectory(W, oc, hc, temp, u, k, p, allow, none)
            assert np.array_equal(w1, w0) and np.array_equal(tok1, tok0) and np.array_equal(bits(lp1), bits(lp0))
        # (b)
        for other in (np.full((R, AR.L), 1.0), np.full((R, AR.L), 2.0), np.full((R, AR.L), np.nan)):
            w1, tok1, lp1, *_ = AF.forced_trajectory(W, oc, hc, temp, other, k, p, allow, tok0)
            assert np.array_equal(w1, w0) and np.array_equal(tok1, tok0) and np.array_equal(bits(lp1), bits(lp0))
        # (c), (e)
        w, tok, lp, n, cm, bm, d = AF.forced_trajectory(W, oc, hc, temp, u, k, p, allow, forced)
        assert np.array_equal(tok[isf], forced[isf]) and not np.isnan(lp).any()
        banned = isf & ~np.take_along_axis(allow, np.maximum(forced, 0)[..., None], -1)[..., 0]
        assert banned.any() and np.isneginf(lp[banned]).all() and not np.isneginf(lp[~isf]).any()
        tf, _ = AR.trajectory(W, oc, hc, tokens=tok)
        assert np.array_equal(tf, w)
        want, wlp, *_ = CR.pick_rows(w.astype(np.float32), temp, u, k, p, allow)
        assert np.array_equal(tok[~isf], want[~isf]) and np.array_equal(bits(lp[~isf]), bits(wlp[~isf]))
        assert np.take_along_axis(allow, tok[..., None], -1)[~isf].all()
        # (d)
        one = allow.copy()
        one[isf] = False
        rr, tt = np.nonzero(isf)
        one[rr, tt, forced[rr, tt]] = True
        _, tok1, lp1, *_ = AF.forced_trajectory(W, oc, hc, temp, np.full((R, AR.L), np.nan), k, p, one, forced)
        assert np.array_equal(tok1[isf], forced[isf]) and (lp1[isf] == 0.0).all() and not np.signbit(lp1[isf]).any()


def margin_count(V, R, E, Hc, H, U):
    """-> (free draws within a margin, free draws, forced ticks within the nucleus margin, forced ticks) of the case (V, R) over the three
    settings, along the oracle's own forced trajectory"""
    W = AR.net(V, E, Hc, H, U)
    allow, forced = CR.plan_mask(V, R, AR.L), FR.plan_forced(V, R, AR.L)
    isf = forced >= 0
    free = CR.free(allow) & ~isf
    is_banned = isf & ~np.take_along_axis(allow, np.maximum(forced, 0)[..., None], -1)[..., 0]
    cnt = np.zeros(4, dtype=np.int64)
    for si, (temp, k, p) in enumerate(FR.FORCED_SETTINGS):
        oc, hc, u = AR.case(V, R, si, E, Hc, H, U)
        w, tok, lp, n, cm, bm, d = AF.forced_trajectory(W, oc, hc, temp, u, k, p, allow, forced)
        near_free = int((~TR.firm(cm, bm) & free).sum())
        near_forced = int(((bm < TR.MARGIN) & isf).sum())
        print(f"V {V} H {H} R {R} setting {(temp, k, p)}: {near_free} of {int(free.sum())} free draws within a margin, {near_forced} of "
              f"{int(isf.sum())} forced ticks within the nucleus margin; {int((np.isfinite(lp) & isf).sum())} forced ticks finite, "
              f"{int(is_banned.sum())} banned")
        assert np.array_equal(tok[isf], forced[isf]) and not np.isnan(lp).any()
        assert np.isneginf(lp[is_banned]).all() and np.take_along_axis(allow, tok[..., None], -1)[~isf].all()
        if k == 0 and p == 1.0:
            assert np.array_equal(np.isneginf(lp) & isf, is_banned)           # un-truncated: every non-banned forced tick is finite
        cnt += (near_free, int(free.sum()), near_forced, int(isf.sum()))
    return cnt, int(is_banned.sum()), int(isf.sum())


@pytest.mark.parametrize("R", AR.ROWS)
@pytest.mark.parametrize("V", AR.FULL_V)
def test_margin_counts_of_the_token_pass_cases(V, R):
    """Per case of test_gpu_arnn_forced.test_the_rule_on_the_calls_own_logits: the cap of 5 % of the free draws and of the forced ticks,
    and the counts DESIGN.md section 17 records -- at most 5 free draws at V = 48, R = 11 and 3 elsewhere, at most one forced tick;
    36 to 44 % of the forced tokens banned."""
    cnt, banned, nforced = margin_count(V, R, **AR.FULL)
    assert nforced == 10 * R and cnt[3] == 30 * R and 0 < cnt[1] < 3 * R * AR.L
    assert cnt[0] <= AR.NEAR_CAP * cnt[1] and cnt[2] <= AR.NEAR_CAP * cnt[3], (V, R, cnt)
    assert cnt[0] <= (5 if (V, R) == (48, 11) else 3) and cnt[2] <= 1, (V, R, cnt)
    assert 0.36 * nforced <= banned <= 0.44 * nforced or R == 1, (V, R, banned, nforced)


@pytest.mark.parametrize("R", (1, 5))
def test_margin_counts_of_the_per_tick_cases(R):
    c = dict(AR.SMALL)
    V = c.pop("V")
    cnt, banned, nforced = margin_count(V, R, **c)
    assert cnt[0] <= AR.NEAR_CAP * cnt[1] and cnt[2] <= AR.NEAR_CAP * cnt[3], (R, cnt)
    assert cnt[0] <= 3 and cnt[2] <= 1, (R, cnt)


def test_a_forced_token_moves_the_oracles_next_logits():
    """What the GPU feedback test relies on: with tick 9 forced to a token the free trajectory does not draw there, the oracle's logits are
    equal up to tick 9 and move at tick 10 by far more than 1e-3 of max |logit|."""
    W = AR.net(48, **AR.FULL)
    oc, hc, u = AR.case(48, 1, 1, **AR.FULL)
    w, tok, *_ = AF.forced_trajectory(W, oc, hc, 1.5, u, 0, 1.0, None, None)
    forced = np.full((1, AR.L), -1)
    forced[0, 9] = (tok[0, 9] + 17) % 48
    w2, tok2, *_ = AF.forced_trajectory(W, oc, hc, 1.5, u, 0, 1.0, None, forced)
    assert tok2[0, 9] == forced[0, 9] != tok[0, 9] and np.array_equal(w2[:, :10], w[:, :10])
    assert np.abs(w2[0, 10] - w[0, 10]).max() > 1e-3 * np.abs(w).max()


def test_header_and_binding_agree_on_the_new_entry():
    """inet_arnn_sample_fx = inet_arnn_sample_cx + `const int32_t* forced` in front of the stream, in the header and in _lib; the rule's
    text stands in the header and in DESIGN.md; INTEGRATION.md quotes the binding; the ABI version did not move"""
    hdr = open(os.path.join(REPO, "include", "inpaintnet_hip.h")).read()
    protos = {}
    for name in ("inet_arnn_sample_cx", "inet_arnn_sample_fx"):
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", hdr)
        assert m, name
        protos[name] = [" ".join(a.split()) for a in m.group(1).split(",")]
    old, new = protos["inet_arnn_sample_cx"], protos["inet_arnn_sample_fx"]
    assert new == old[:-1] + ["const int32_t* forced", "void* stream"] and old[-1] == "void* stream"
    res, args = _lib._SIGNATURES["inet_arnn_sample_fx"]
    res0, args0 = _lib._SIGNATURES["inet_arnn_sample_cx"]
    assert res is C.c_int and args == args0[:-1] + [C.c_void_p, C.c_void_p]
    assert "inet_arnn_sample_fx" in _lib.EXPORTS
    assert "_L.inet_arnn_sample_fx.argtypes" in open(os.path.join(REPO, "INTEGRATION.md")).read()
    design = open(os.path.join(REPO, "DESIGN.md")).read()
    assert re.search(r"^## 17\. ", design, flags=re.M)
    for text in (hdr[hdr.index("int inet_arnn_sample_cx("):], design[re.search(r"^## 17\. ", design, flags=re.M).start():]):
        flat = re.sub(r"[\s/*#`]+", " ", text)
        for phrase in ("A value f with 0 <= f < V forces that tick", "The tick's uniform is not used",
                       "It is exactly -inf when f is banned or truncated away", "The note head is not ReLU'd"):
            assert phrase in flat, phrase


def test_the_entry_refuses_what_inet_arnn_sample_cx_refuses():
    _lib.build(verbose=False)
    Lb = _lib.lib()
    X, NULL, big = C.c_void_p(16), None, 1 << 40      # X: a pointer that is never followed (tests/test_pointwise_host.py)
    net = [X] * 12
    calls = {}
    for tag, al, fo in (("mask + forced", X, X), ("forced", NULL, X), ("neither", NULL, NULL)):
        def fx(R=1, Ln=4, emb=X, oc=X, u=X, tokens=X, ws=X, nws=big, temp=1.0, k=0, p=1.0, H=256):
            return Lb.inet_arnn_sample_fx(R, Ln, 10, 256, H, 256, 48, emb, oc, 256, 256 * Ln, *net, temp, u, NULL, tokens, ws, nws, k, p,
                                          NULL, NULL, al, fo, NULL)
        nan, inf = float("nan"), float("inf")
        calls.update({f"{tag}: {k_}": v for k_, v in {
            "R": fx(R=0), "L": fx(Ln=0), "emb": fx(emb=NULL), "oc": fx(oc=NULL), "uniforms": fx(u=NULL), "tokens": fx(tokens=NULL),
            "ws": fx(ws=NULL), "ws_floats": fx(nws=16), "temperature inf": fx(temp=inf), "temperature nan": fx(temp=nan), "H": fx(H=250),
            "top_p 0": fx(p=0.0), "top_p > 1": fx(p=1.0000001), "top_p nan": fx(p=nan)}.items()})
    assert {k: v for k, v in calls.items() if v != -1} == {}
    assert Lb.inet_abi_version() == 1


def test_argument_errors_come_before_any_library_call_and_any_draw(monkeypatch):
    from inpaintnet_amd.arnn import ConstraintModelGaussianReg
    from inpaintnet_amd.arnn_tester import AnticipationRNNTester
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("a library call in front of the argument check"))
    state = np.random.get_state()[1].copy()
    V, L = 12, 96
    # ops.arnn_sample: the forced words' shape, dtype and place
    oc = torch.zeros(3, L, 16)
    net = [None] * 10 + [torch.zeros(V, 16), None]                       # (..., W2, b2)
    for bad in (torch.zeros(3, L, dtype=torch.int64), torch.zeros(3, L + 1, dtype=torch.int32), torch.zeros(2, L, dtype=torch.int32),
                torch.zeros(3, L, 1, dtype=torch.int32), torch.zeros(3, L, dtype=torch.float32),
                torch.zeros(3, L, dtype=torch.int32), np.zeros((3, L), dtype=np.int32)):          # (the last two: not on the device)
        with pytest.raises(ValueError):
            ops.arnn_sample(None, oc, *net, 1.0, None, forced=bad)
    # generate: an int tensor (L,) for the one row, (B, L) for a batch, values in [-1, V); uniforms float64 (B, L)
    me = types.SimpleNamespace(num_notes_per_voice=[V])
    one, batch = torch.zeros(1, L, dtype=torch.int64), torch.zeros(3, 1, L, dtype=torch.int64)
    f1, f3 = torch.full((L,), -1, dtype=torch.int64), torch.full((3, L), -1, dtype=torch.int64)
    for score, bad in ((one, f1.float()), (one, f1 == -1), (one, f1[:-1]), (one, f1[None]), (one, f1 + V + 1), (one, f1 - 1), (one, f3),
                       (batch, f1), (batch, f3[:2]), (batch, f3[:, None]), (batch, f3.double()), (batch, f3 + V + 1), (batch, f3 - 1)):
        with pytest.raises(ValueError):
            ConstraintModelGaussianReg.generate(me, score, None, None, forced=bad)
    for score, bad in ((one, np.zeros((1, L), dtype=np.float32)), (one, np.zeros(L)), (one, np.zeros((1, L + 1))), (batch, np.zeros((1, L))),
                       (batch, np.zeros((3, 1, L)))):
        with pytest.raises(ValueError):
            ConstraintModelGaussianReg.generate(me, score, None, None, uniforms=bad)
    # the tester: score()'s fillings, its context, its bans; generation(score_fixed=True)'s fixed tokens
    ds = types.SimpleNamespace(subdivision=6, num_beats_per_bar=4)
    te = types.SimpleNamespace(dataset=ds, measure_seq_len=24, model=types.SimpleNamespace(num_notes_per_voice=[V]), last_logp=None)
    te._allowed = types.MethodType(AnticipationRNNTester._allowed, te)
    te._to_score = lambda t: None
    score = torch.arange(L).remainder(V)[None]
    md = torch.zeros(1, L, 2, dtype=torch.int64)
    good = torch.zeros(2, 2, 24, dtype=torch.int64)
    for bad in (dict(fillings=good.float()), dict(fillings=good == 0), dict(fillings=good[:, :, :23]), dict(fillings=good[0]),
                dict(fillings=good[:, :1]), dict(fillings=good[:0]), dict(fillings=good + V), dict(fillings=good - 1),
                dict(fillings=good, banned_tokens=[V]), dict(fillings=good, banned_tokens=list(range(V))),
                dict(fillings=good, tensor_metadata=None)):
        with pytest.raises(ValueError):
            AnticipationRNNTester.score(te, score, 2, 2, **{"tensor_metadata": md, **bad})
    with pytest.raises(ValueError):
        AnticipationRNNTester.score(te, score, 4, 2, good, tensor_metadata=md)        # the window ends behind the score
    outside = score.clone()
    outside[0, 3] = V                                                              # the model's no-constraint symbol is no token of the head
    with pytest.raises(ValueError):
        AnticipationRNNTester.score(te, outside, 2, 2, good, tensor_metadata=md)
    below = score.clone()
    below[0, 90] = -1
    with pytest.raises(ValueError):
        AnticipationRNNTester.score(te, below, 2, 2, good, tensor_metadata=md)
    free = torch.full((2, 24), -1)
    for fixed in (free.clone().fill_(V), free.clone().fill_(-2), free.float(), free == -1, torch.full((24,), -1), torch.full((3, 24), -1)):
        with pytest.raises(ValueError):
            AnticipationRNNTester._generate_window(te, score, None, 2, 2, fixed_tokens=fixed, score_fixed=True)
    with pytest.raises(ValueError):
        AnticipationRNNTester._generate_window(te, score, None, 2, 2, fixed_tokens=free, banned_tokens=[V], score_fixed=True)
    with pytest.raises(ValueError):
        AnticipationRNNTester._generate_window(te, outside, None, 2, 2, fixed_tokens=free, clamp_context=True, score_fixed=True)
    assert np.array_equal(np.random.get_state()[1], state)                      # nothing random was drawn
