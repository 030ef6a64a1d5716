"""AnticipationRNN's forced tokens on the GPU (inet_arnn_sample_fx: the forced build of the persistent token pass and
head_b1_kernel<NI, 4> of the per-tick launches, csrc/arnn_gen.hip) and the public surface down from AnticipationRNNTester.score and
generation(score_fixed=True).

The reference for the rule is its float64 restatement (tests/decoder_forced_ref.py) APPLIED TO THE f32 LOGITS THE CALL RETURNED, as in
tests/test_gpu_arnn_constraint.py.  A free draw is left out of a comparison only when one of its two margins is below 2e-5, a forced
tick only when its nucleus margin is (whether f is kept may then go either way; it still returns f): at most 5 % of a case's free draws
and 5 % of its forced ticks (arnn_trunc_ref.NEAR_CAP) -- a case is a shape (V, R) under decoder_forced_ref.FORCED_SETTINGS; along the
oracle's own trajectory tests/test_arnn_forced_host.py counts the same masks, patterns and seeds.  The returned logits are the UNMASKED
ones, held to the float64 oracle run teacher-forced over the GPU's own tokens within DESIGN.md section 12's bound (TRAJ_TOL)."""
import numpy as np
import pytest
import torch

from tests import arnn_trunc_ref as AR
from tests import decoder_constraint_ref as CR
from tests import decoder_forced_ref as FR
from tests import decoder_trunc_ref as TR
from tests import golden_util as G

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from inpaintnet_amd import ops, synthetic
    from inpaintnet_amd.arnn import AnticipationRNNBaseline
    from inpaintnet_amd.arnn_tester import AnticipationRNNTester
    from tests.test_gpu_arnn_constraint import TRAJ_TOL, check_trajectory, dev_net, words_of
    from tests.test_gpu_arnn_generate import _inputs, _model
    from tests.test_gpu_decode_plans import labels_of

measured = {"logp": 0.0}        # the largest logp error in units of its tolerance, printed by the checks
LOWER = ("arnn_token_sample", "arnn_ticks", "sample_", "trunc_", "cons_")


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def call(Wd, oc, hc, u, temp, k, p, allow, forced):
    """One call (allow bool [R,L,V] or None, forced int [R,L] or None) -> (tokens [R,L], logp, logits, launch labels)"""
    ocd, hcd = torch.from_numpy(oc).cuda(), torch.from_numpy(hc).cuda() if hc is not None else None
    kw = {} if allow is None else {"allowed": words_of(allow)}
    if forced is not None:
        kw["forced"] = torch.from_numpy(np.ascontiguousarray(forced).astype(np.int32)).cuda()
    (tok, lp, lg), labels = labels_of(lambda: ops.arnn_sample(Wd[0], ocd, *Wd[1:], temp, u, hc_init=hcd, top_k=k, top_p=p, want_logp=True,
                                                              want_logits=True, **kw))
    status = ops.chain_status()
    assert status == 0, (tuple(oc.shape), temp, k, p, status, ops.slow_waits_summary())
    return tok.cpu().numpy(), lp.cpu().numpy(), lg.cpu().numpy(), labels


def check_labels(labels, R, L, V, persistent):
    want = f"force_arnn_token_sample R{R} L{L} V{V}" if persistent else f"force_arnn_ticks L{L} V{V}"
    assert sum(l.startswith(want) for l in labels) == ((R + 7) // 8 if persistent else R), (want, sorted(set(labels)))
    assert not any(l.startswith(LOWER) for l in labels), sorted(set(labels))


def check_rule(lg, tok, lp, temp, u, k, p, allow, forced, what):
    """Tokens and logp against the restatement on the returned logits -> (free draws within a margin, free draws, forced ticks within the
    nucleus margin, forced ticks)"""
    V = lg.shape[-1]
    if allow is None:
        allow = np.ones(lg.shape, dtype=bool)
    want, wlp, n, cm, bm, d = FR.pick_rows(lg, temp, u, k, p, allow, forced)
    isf = (forced >= 0) & (forced < V)
    assert tok.min() >= 0 and tok.max() < V, what
    assert np.array_equal(tok[isf], forced[isf]), (what, "a forced tick returns its token")
    free = CR.free(allow) & ~isf
    firm = np.where(isf, bm >= TR.MARGIN, TR.firm(cm, bm) | ~CR.free(allow))
    print(what, "within margin", int((~firm & ~isf).sum()), "of", int(free.sum()), "free draws,", int((~firm & isf).sum()), "of",
          int(isf.sum()), "forced ticks")
    eff = allow | ~allow.any(-1, keepdims=True)
    assert np.take_along_axis(eff, tok[..., None], -1)[~isf].all(), (what, "a banned token at a free tick")
    assert np.array_equal(tok[firm], want[firm]), (what, np.argwhere((tok != want) & firm)[:4])
    fixed = ~CR.free(allow) & ~isf
    assert np.array_equal(tok[fixed], np.argmax(allow, -1)[fixed]), what
    assert (lp[fixed & ~np.isnan(wlp)] == 0.0).all(), (what, "a one-bit free tick's logp is exactly 0")
    assert np.array_equal(np.isnan(lp), np.isnan(wlp)), what                  # NaN exactly where the rule does not apply
    assert np.array_equal(np.isneginf(lp)[firm], np.isneginf(wlp)[firm]), (what, "-inf exactly where the restatement has it")
    assert not np.isneginf(lp[~isf]).any() and not np.isposinf(lp).any(), what
    ok = firm & (tok == want) & np.isfinite(wlp) & np.isfinite(lp)
    if ok.any():
        err = np.abs(lp[ok].astype(np.float64) - wlp[ok].astype(np.float64)) / TR.logp_tol(d[ok])
        measured["logp"] = max(measured["logp"], float(err.max()))
        print(what, "logp error / tolerance: max %.3f (all checks so far %.3f)" % (float(err.max()), measured["logp"]))
        assert err.max() <= 1.0, (what, float(err.max()))
    return int((~firm & ~isf).sum()), int(free.sum()), int((~firm & isf).sum()), int(isf.sum())


def run_case(V, R, cfg, persistent):
    W, Wd = dev_net(V, **cfg)
    allow, forced = CR.plan_mask(V, R, AR.L), FR.plan_forced(V, R, AR.L)
    isf = forced >= 0
    banned = isf & ~np.take_along_axis(allow, np.maximum(forced, 0)[..., None], -1)[..., 0]
    cnt = np.zeros(4, dtype=np.int64)
    for si, (temp, k, p) in enumerate(FR.FORCED_SETTINGS):
        oc, hc, u = AR.case(V, R, si, **cfg)
        tok, lp, lg, labels = call(Wd, oc, hc, u, temp, k, p, allow, forced)
        what = (V, cfg["H"], R, temp, k, p)
        check_labels(labels, R, AR.L, V, persistent)
        check_trajectory(W, oc, hc, tok, lg, what)             # (the forced tokens were fed back, the banned ones among them)
        assert banned.any() and np.isneginf(lp[banned]).all(), what
        if k == 0 and p == 1.0:
            assert np.isfinite(lp[isf & ~banned]).all(), what
        cnt += check_rule(lg, tok, lp, temp, u, k, p, allow, forced, what)
    print((V, R), "left out", cnt[0], "of", cnt[1], "free draws,", cnt[2], "of", cnt[3], "forced ticks")
    assert cnt[0] <= AR.NEAR_CAP * cnt[1] and cnt[2] <= AR.NEAR_CAP * cnt[3], (V, R, cnt)
    assert ops.chain_status() == 0


@pytest.mark.parametrize("R", AR.ROWS)
@pytest.mark.parametrize("V", AR.FULL_V)
def test_the_rule_on_the_calls_own_logits(V, R):
    """H = U = 256 under plan_mask(V, R, 30) and plan_forced(V, R, 30): V <= 64 runs the forced build of the persistent token pass (R = 11:
    8 teams, then 3 -- the forced words' offset per launch), 64 < V <= 128 the per-tick launches with two mask words per tick.  Three
    settings per case."""
    run_case(V, R, AR.FULL, persistent=V <= 64)


@pytest.mark.parametrize("R", (1, 5))
def test_the_rule_on_the_per_tick_path(R):
    c = dict(AR.SMALL)
    V = c.pop("V")
    run_case(V, R, c, persistent=False)


def test_the_per_tick_path_of_the_token_pass_shape():
    """option key 14 = 0: H = 256, V = 48 through head_b1_kernel<NI, 4>"""
    try:
        ops.set_option(14, 0)
        run_case(48, 5, AR.FULL, persistent=False)
    finally:
        ops.set_option(14, 3)


@pytest.mark.parametrize("V", [48, 65])
def test_no_forced_tick_is_the_constrained_call(V):
    """Consequence (a) at R = 11: a null forced (the masked kernels) and one of all -1 (the forced kernels) return inet_arnn_sample_cx's
    tokens, logits and logp bit for bit, a fallback tick in every row included; at the C level a value >= V or < -1 is a free tick too."""
    W, Wd = dev_net(V, **AR.FULL)
    R = 11
    allow = CR.plan_mask(V, R, AR.L)
    for si, (temp, k, p) in ((1, (1.5, 0, 1.0)), (2, FR.FORCED_SETTINGS[2])):
        oc, hc, u = AR.case(V, R, si, **AR.FULL)
        u = u.copy()
        u[:, 5] = 2.0
        tok0, lp0, lg0, labels0 = call(Wd, oc, hc, u, temp, k, p, allow, None)
        assert any(l.startswith("cons_") for l in labels0) and not any(l.startswith("force_") for l in labels0), sorted(set(labels0))
        r, t = np.meshgrid(np.arange(R), np.arange(AR.L), indexing="ij")
        for forced in (np.full((R, AR.L), -1), np.where(t % 2 == 0, V + r, -2 - r)):
            tok, lp, lg, labels = call(Wd, oc, hc, u, temp, k, p, allow, forced)
            check_labels(labels, R, AR.L, V, V <= 64)
            assert np.array_equal(tok, tok0) and np.array_equal(bits(lg), bits(lg0)) and np.array_equal(bits(lp), bits(lp0)), (V, temp, k, p)
    assert ops.chain_status() == 0


@pytest.mark.parametrize("V", [48, 65, 12])
def test_replay_returns_the_call_bit_for_bit(V):
    """Consequence (b) at R = 11: force at every tick what a constrained call returned -- same temperature, top_k, top_p and mask, uniforms
    of 1.0, 2.0 and NaN: that call's tokens, logits and logp bit for bit (it has no NaN: its uniforms lie in [0, 1))."""
    cfg = {k_: v for k_, v in AR.SMALL.items() if k_ != "V"} if V == 12 else AR.FULL
    W, Wd = dev_net(V, **cfg)
    R = 11
    allow = CR.plan_mask(V, R, AR.L)
    for si, (temp, k, p) in ((1, (1.5, 0, 1.0)), (2, FR.FORCED_SETTINGS[2])):
        oc, hc, u = AR.case(V, R, si, **cfg)
        tok0, lp0, lg0, _ = call(Wd, oc, hc, u, temp, k, p, allow, None)
        assert not np.isnan(lp0).any()
        for other in (1.0, 2.0, np.nan):
            tok, lp, lg, labels = call(Wd, oc, hc, np.full((R, AR.L), other), temp, k, p, allow, tok0)
            check_labels(labels, R, AR.L, V, V != 12 and V <= 64)
            assert np.array_equal(tok, tok0) and np.array_equal(bits(lg), bits(lg0)) and np.array_equal(bits(lp), bits(lp0)), (V, temp, k, p, other)
    assert ops.chain_status() == 0


@pytest.mark.parametrize("V,small", [(48, False), (64, False), (65, False), (12, True)])
def test_every_row_gets_its_own_forced_words(V, small):
    """Consequences (c) and (d) at R = 11, every tick forced with another token per row and tick and NaN uniforms: under its own one-bit
    mask every tick returns f with logp exactly 0.0f; under the complement of that mask -- f banned -- it still returns f, with logp -inf,
    and the logits are the network's function of the banned tokens fed back; without a mask it returns f with a finite logp.  Rows 8 to 10
    (the second launch of the persistent pass) return THEIR OWN tokens, which differ from those of rows 0 to 2."""
    cfg = dict(AR.SMALL) if small else dict(AR.FULL, V=V)
    cfg.pop("V")
    W, Wd = dev_net(V, **cfg)
    R = 11
    r, t = np.meshgrid(np.arange(R), np.arange(AR.L), indexing="ij")
    fix = (7 * r + 3 * t + 1) % V
    assert (fix[8:] != fix[:3]).all()
    one = np.zeros((R, AR.L, V), dtype=bool)
    np.put_along_axis(one, fix[..., None], True, -1)
    nan = np.full((R, AR.L), np.nan)
    for si, (temp, k, p) in enumerate(FR.FORCED_SETTINGS):
        oc, hc, _ = AR.case(V, R, si, **cfg)
        for allow in (one, ~one, None):
            tok, lp, lg, labels = call(Wd, oc, hc, nan, temp, k, p, allow, fix)
            check_labels(labels, R, AR.L, V, not small and V <= 64)
            assert np.array_equal(tok, fix), (V, temp, k, p, np.argwhere(tok != fix)[:4])
            if allow is one:
                assert (lp == 0.0).all() and not np.signbit(lp).any(), (V, temp, k, p)
            elif allow is None:
                assert not np.isnan(lp).any() and not np.isposinf(lp).any() and (lp <= 0.0).all()
                if k == 0 and p == 1.0:
                    assert np.isfinite(lp).all()
            else:
                assert np.isneginf(lp).all(), (V, temp, k, p)
                check_trajectory(W, oc, hc, tok, lg, ("own words", V, temp, k, p))
    assert ops.chain_status() == 0


@pytest.mark.parametrize("V", [48, 65])
def test_the_forced_token_is_fed_back(V):
    """Tick 9 forced to a token the free call does not draw there: the call returns it, the logits up to tick 9 are the free call's bit for
    bit, and those of tick 10 are the float64 oracle's teacher-forced over the GPU's own tokens -- the network saw the forced token -- and
    differ from the free call's by more than 1e-3 of max |logit|."""
    W, Wd = dev_net(V, **AR.FULL)
    oc, hc, u = AR.case(V, 1, 1, **AR.FULL)
    tok0, lp0, lg0, _ = call(Wd, oc, hc, u, 1.5, 0, 1.0, None, None)
    t = 9
    forced = np.full((1, AR.L), -1)
    forced[0, t] = (int(tok0[0, t]) + 17) % V
    tok, lp, lg, labels = call(Wd, oc, hc, u, 1.5, 0, 1.0, None, forced)
    check_labels(labels, 1, AR.L, V, V <= 64)
    assert tok[0, t] == forced[0, t] != tok0[0, t] and np.isfinite(lp[0, t]) and lp[0, t] < 0.0
    assert np.array_equal(tok[0, :t], tok0[0, :t]) and np.array_equal(bits(lg[0, :t + 1]), bits(lg0[0, :t + 1]))
    assert np.array_equal(bits(lp[0, :t]), bits(lp0[0, :t]))
    ref = check_trajectory(W, oc, hc, tok, lg, ("fed back", V))
    scale = np.abs(ref).max()
    assert np.abs(lg[0, t + 1].astype(np.float64) - ref[0, t + 1]).max() <= TRAJ_TOL * scale
    moved = np.abs(lg[0, t + 1] - lg0[0, t + 1]).max()
    print("fed back", V, "tick t + 1 moved by %.3g of max |logit|" % (moved / scale))
    assert moved > 1e-3 * scale
    c = check_rule(lg, tok, lp, 1.5, u, 0, 1.0, None, forced, ("fed back", V))
    assert c[0] <= AR.NEAR_CAP * c[1]
    assert ops.chain_status() == 0


@pytest.mark.parametrize("V,small", [(48, False), (128, False), (12, True)])
def test_fallback_ticks_keep_the_forced_tokens(V, small):
    """Ticks outside the rule under plan_mask and plan_forced.  NaN head weights: every forced tick returns f, every logp is NaN, the free
    ticks take the lowest allowed token.  +inf in the head's bias at one token: m is not finite wherever that token is allowed -- logp NaN
    exactly there --, the forced ticks return f, the free ones stay inside the allowed set and follow the restatement.  Uniforms outside
    [0, 1): the forced ticks are untouched by them, the free ones fall back as in the constrained call."""
    cfg = dict(AR.SMALL) if small else dict(AR.FULL, V=V)
    cfg.pop("V")
    W, Wd = dev_net(V, **cfg)
    R = 5
    temp, k, p = FR.FORCED_SETTINGS[2]
    oc, hc, u = AR.case(V, R, 2, **cfg)
    allow, forced = CR.plan_mask(V, R, AR.L), FR.plan_forced(V, R, AR.L)
    isf = forced >= 0
    nanW = list(Wd)
    nanW[11] = torch.full_like(Wd[11], float("nan"))
    tok, lp, lg, labels = call(nanW, oc, hc, u, temp, k, p, allow, forced)
    check_labels(labels, R, AR.L, V, not small and V <= 64)
    assert np.array_equal(tok[isf], forced[isf]) and np.isnan(lp).all() and np.isnan(lg).all()
    assert np.array_equal(tok[~isf], np.argmax(allow, -1)[~isf])
    v0 = V // 2
    infb = list(Wd)
    infb[12] = Wd[12].clone()
    infb[12][v0] = float("inf")
    tok, lp, lg, _ = call(infb, oc, hc, u, temp, k, p, allow, forced)
    assert np.isposinf(lg[..., v0]).all() and np.array_equal(tok[isf], forced[isf])
    assert np.array_equal(np.isnan(lp), allow[..., v0]) and allow[..., v0][isf].any() and (~allow[..., v0])[isf].any()
    assert np.take_along_axis(allow, tok[..., None], -1)[~isf].all()
    check_rule(lg, tok, lp, temp, u, k, p, allow, forced, ("inf bias", V))
    tok, lp, lg, _ = call(infb, oc, hc, u, temp, k, p, None, forced)               # no mask: every tick is outside the rule
    assert np.array_equal(tok[isf], forced[isf]) and (tok[~isf] == v0).all() and np.isnan(lp).all()
    u = u.copy()
    u[:, 1::4], u[:, 3::4], u[:, 0::8] = 2.0, np.nan, -0.5
    out = ~((u >= 0.0) & (u < 1.0))
    tok, lp, lg, _ = call(Wd, oc, hc, u, temp, k, p, allow, forced)
    assert (out & isf).any() and not np.isnan(lp[isf]).any()
    assert np.isnan(lp[out & ~isf]).all() and not np.isnan(lp[~out]).any()
    assert np.array_equal(tok[out & ~isf], np.array([CR.masked_argmax(x, a) for x, a in zip(lg[out & ~isf], allow[out & ~isf])]))
    c = check_rule(lg, tok, lp, temp, u, k, p, allow, forced, ("outside", V))
    assert c[0] <= AR.NEAR_CAP * c[1] and c[2] <= AR.NEAR_CAP * c[3]
    check_trajectory(W, oc, hc, tok, lg, ("outside", V))
    assert ops.chain_status() == 0


@pytest.mark.parametrize("V,small", [(48, False), (128, False), (12, True)])
def test_scoring_given_tokens_is_the_log_softmax_of_the_teacher_forced_network(V, small):
    """The reference's metric: an all-forced, unmasked call at (1.0, 0, 1.0) over given tokens against float64 log_softmax of
    arnn_trunc_ref.trajectory(tokens=...) gathered at the tokens, within decoder_trunc_ref.logp_tol."""
    cfg = dict(AR.SMALL) if small else dict(AR.FULL, V=V)
    cfg.pop("V")
    W, Wd = dev_net(V, **cfg)
    R = 3
    oc, hc, _ = AR.case(V, R, 0, **cfg)
    given = synthetic.det_tokens(f"arnn_forced/given/{V}", (R, AR.L), V).astype(np.int64)
    tok, lp, lg, labels = call(Wd, oc, hc, np.zeros((R, AR.L)), 1.0, 0, 1.0, None, given)
    check_labels(labels, R, AR.L, V, not small and V <= 64)
    assert np.array_equal(tok, given) and np.isfinite(lp).all()
    ref, _ = AR.trajectory(W, oc, hc, tokens=given)
    ls = ref - ref.max(-1, keepdims=True)
    ls = ls - np.log(np.exp(ls).sum(-1, keepdims=True))
    want = np.take_along_axis(ls, given[..., None], -1)[..., 0]
    d = np.take_along_axis(ref - ref.max(-1, keepdims=True), given[..., None], -1)[..., 0]
    err = np.abs(lp.astype(np.float64) - want) / TR.logp_tol(d)
    print("given tokens", V, "logp error / tolerance: max %.3f; cross-entropy %.7f against the oracle's %.7f"
          % (float(err.max()), -lp.astype(np.float64).mean(), -want.mean()))
    assert err.max() <= 1.0, (V, float(err.max()))
    assert ops.chain_status() == 0


@pytest.mark.parametrize("name,key", [("full", "full/t1/0"), ("small", "small/t0/1")])
def test_generate_takes_forced_tokens_and_uniforms_and_without_them_is_todays_call(name, key, monkeypatch):
    """generate(forced=) with one row and with a batch of three agrees with ops.arnn_sample called on what generate handed it and always
    leaves last_logp; generate(uniforms=) leaves np.random's state unchanged and reproduces the seeded call; generate() without the two
    reproduces tests/golden/arnn_generate.npz with the kernels it always ran."""
    fx = G.load("arnn_generate")
    _, model = _model(name)
    s, m, c = _inputs(fx, name)
    ti, i = int(key.split("/")[1][1:]), int(key.split("/")[2])
    seed, temp = int(fx[key + "/seed"]), float(fx["temperatures"][ti])
    V = G.ARNN_CFGS[name]["V"]
    np.random.seed(seed)
    (_, gen, _), labels = labels_of(lambda: model.generate(s[i], m[i], c[i], temperature=temp))
    assert np.array_equal(gen[0].cpu().numpy(), fx[key + "/tokens"].astype(np.int64)) and model.last_logp is None
    assert not any(l.startswith(("force_", "cons_", "trunc_")) for l in labels), sorted(set(labels))
    Lg = gen.shape[1]
    np.random.seed(seed + 1)
    state = np.random.get_state()[1].copy()
    (_, gen_u, _), labels = labels_of(lambda: model.generate(s[i], m[i], c[i], temperature=temp,
                                                             uniforms=np.random.RandomState(seed).random_sample((1, Lg))))
    assert torch.equal(gen_u, gen) and np.array_equal(np.random.get_state()[1], state) and model.last_logp is None
    assert not any(l.startswith(("force_", "cons_", "trunc_")) for l in labels), sorted(set(labels))
    seen = {}
    real = ops.arnn_sample

    def recording(*a, **kw):
        seen["a"], seen["kw"] = a, dict(kw)
        return real(*a, **kw)
    monkeypatch.setattr(ops, "arnn_sample", recording)
    for B in (1, 3):
        allow, forced = CR.plan_mask(V, B, Lg), FR.plan_forced(V, B, Lg)
        sc, md, lc = (s[i], m[i], c[i]) if B == 1 else (s[:1].expand(B, -1, -1).reshape(B, 1, Lg).contiguous(),
                                                        m[:1].expand(B, -1, -1, -1).reshape(B, 1, Lg, -1).contiguous(),
                                                        c[:1].expand(B, -1, -1).reshape(B, 1, Lg).contiguous())
        mask = torch.from_numpy(allow[0] if B == 1 else allow)
        fo = torch.from_numpy(forced[0] if B == 1 else forced)
        np.random.seed(seed)
        (_, gen, _), labels = labels_of(lambda: model.generate(sc, md, lc, temperature=temp, top_k=8, top_p=0.9, keep_weights=True,
                                                               allowed=mask, forced=fo if B == 1 else fo.cuda().long()))
        want = f"force_arnn_token_sample R{B} " if name == "full" else "force_arnn_ticks "
        assert sum(l.startswith(want) for l in labels) == (1 if name == "full" else B), sorted(set(labels))
        a, kw = seen["a"], seen["kw"]
        assert kw["forced"].dtype == torch.int32 and np.array_equal(kw["forced"].cpu().numpy(), forced)
        u = np.random.RandomState(seed).random_sample((B, Lg))
        assert np.array_equal(np.asarray(a[15]), u)
        tok, lp, lg = real(*a[:15], u, hc_init=kw["hc_init"], top_k=8, top_p=0.9, want_logp=True, want_logits=True, allowed=words_of(allow),
                           forced=torch.from_numpy(forced).cuda())
        g = gen.view(B, Lg)
        assert torch.equal(g, tok) and torch.equal(model.last_logp.view(B, Lg).view(torch.int32), lp.view(torch.int32))
        assert torch.equal(model.last_weights, lg) and tuple(model.last_logp.shape) == ((B, 1, Lg) if B > 1 else (1, Lg))
        cnt = check_rule(lg.cpu().numpy(), tok.cpu().numpy(), lp.cpu().numpy(), temp, u, 8, 0.9, allow, forced, (name, "generate", B))
        assert cnt[0] <= AR.NEAR_CAP * cnt[1] and cnt[2] <= AR.NEAR_CAP * cnt[3]
        np.random.seed(seed)
        _, gen2, _ = model.generate(sc, md, lc, temperature=temp, forced=fo)                # forced alone: last_logp all the same
        isf = forced >= 0
        assert model.last_logp is not None and model.last_weights is None
        assert np.array_equal(gen2.view(B, Lg).cpu().numpy()[isf], forced[isf]) and not bool(torch.isnan(model.last_logp).any())
    assert ops.chain_status() == 0


@pytest.mark.parametrize("name", ["small", "full"])
def test_score_and_score_fixed(name):
    """AnticipationRNNTester.score of generation(clamp_context=True, num_variations=4, top_p=0.9, temperature=6.0)'s own fillings under
    the same arguments is that call's last_logp bit for bit and leaves np.random alone; a filling the ban excludes scores -inf in its
    measure; the original measures score finite at temperature 1; generation(score_fixed=True) keeps the same notes -- a fixed banned
    token too -- and changes last_logp on the measures with fixed ticks alone."""
    ds, model = _model(name, AnticipationRNNBaseline)
    tester = AnticipationRNNTester(ds, model)
    V = G.ARNN_CFGS[name]["V"]
    Lg, nv = 384, 4
    score = torch.from_numpy(synthetic.folk_score(1, V, seed=5)).long()[0].cuda()
    md = torch.from_numpy(synthetic.folk_metadata(1)).long()[0].cuda()
    a, b = 3 * 24, 6 * 24
    kw = dict(start_measure=4, num_measures_gen=3, tensor_metadata=md)
    np.random.seed(11)
    _, gen, _ = tester.generation(score, num_variations=nv, temperature=6.0, top_p=0.9, clamp_context=True, **kw)
    lp, tick = tester.last_logp.clone(), model.last_logp[:, 0, a:b].reshape(nv, 3, 24).clone()
    assert bool(torch.isfinite(lp).all())
    fill = gen[:, a:b].reshape(nv, 3, 24)
    state = np.random.get_state()[1].copy()
    got, labels = labels_of(lambda: tester.score(score, 4, 3, fill, tensor_metadata=md, temperature=6.0, top_p=0.9))
    assert np.array_equal(np.random.get_state()[1], state)
    want = f"force_arnn_token_sample R{nv} " if name == "full" else "force_arnn_ticks "
    assert sum(l.startswith(want) for l in labels) == (1 if name == "full" else nv), sorted(set(labels))
    assert tuple(got.shape) == (nv, 3) and got.dtype == torch.float32
    assert torch.equal(got.view(torch.int32), lp.view(torch.int32)), (got, lp)
    assert tuple(tester.last_tick_logp.shape) == (nv, 3, 24) and torch.equal(tester.last_tick_logp.view(torch.int32), tick.view(torch.int32))
    assert tuple(model.last_weights.shape) == (nv, Lg, V)
    # a banned note scores -inf in its measure alone; the original measures at temperature 1
    win = fill.cpu().numpy()
    banned = [int(np.bincount(win.reshape(-1), minlength=V).argmax())]
    worst = fill[:1].cpu().clone()
    worst[0, 1, 7] = banned[0]
    rest = worst[0] != banned[0]
    got = tester.score(score, 4, 3, worst, tensor_metadata=md, temperature=6.0, banned_tokens=banned)
    assert tuple(got.shape) == (1, 3) and bool(torch.isneginf(got[0, 1]))
    assert bool(torch.isneginf(tester.last_tick_logp[0][~rest]).all()) and bool(torch.isfinite(tester.last_tick_logp[0][rest]).all())
    got = tester.score(score, 4, 3, score[:, a:b].reshape(1, 3, 24), tensor_metadata=md)
    assert tuple(got.shape) == (1, 3) and bool(torch.isfinite(got).all()) and bool((got < 0).all())
    assert np.array_equal(np.random.get_state()[1], state)
    # kept notes: measures 0 and 2 have fixed ticks, measure 1 has none
    fixed = torch.full((3, 24), -1)
    fixed[0, 0], fixed[0, 5], fixed[2, 23] = banned[0], (banned[0] + 1) % V, V - 1
    keep = (fixed >= 0).reshape(-1)
    gkw = dict(num_variations=nv, temperature=6.0, top_p=1.0, banned_tokens=banned, fixed_tokens=fixed, clamp_context=True, **kw)
    np.random.seed(12)
    _, base, _ = tester.generation(score, **gkw)
    base_lp, base_tick = tester.last_logp.clone(), model.last_logp[:, 0, a:b].clone()
    np.random.seed(12)
    (_, full, _), labels = labels_of(lambda: tester.generation(score, score_fixed=True, **gkw))
    assert any(l.startswith("force_") for l in labels) and not any(l.startswith(LOWER) for l in labels), sorted(set(labels))
    tick = model.last_logp[:, 0, a:b]
    assert torch.equal(full, base)                              # the same notes: the kept ones are fed back either way
    w = full[:, a:b].cpu()
    assert torch.equal(w[:, keep], fixed.reshape(-1)[keep].expand(nv, -1))               # (the fixed banned token too)
    assert not bool(torch.isin(w[:, ~keep], torch.tensor(banned)).any())
    assert bool((base_tick[:, keep] == 0.0).all())
    assert bool(torch.isfinite(tick[:, keep]).all()) and bool((tick[:, keep] < 0.0).all())
    assert torch.equal(tick[:, ~keep].view(torch.int32), base_tick[:, ~keep].view(torch.int32))
    assert torch.equal(tester.last_logp, tick.reshape(nv, 3, 24).sum(-1))
    assert torch.equal(tester.last_logp[:, 1].view(torch.int32), base_lp[:, 1].view(torch.int32))
    assert bool((tester.last_logp[:, [0, 2]] < base_lp[:, [0, 2]]).all())
    assert ops.chain_status() == 0
