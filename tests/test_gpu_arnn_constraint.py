"""AnticipationRNN's per-tick token constraints on the GPU (inet_arnn_sample_cx: the masked build of the persistent token pass and
head_b1_kernel<NI, 3> of the per-tick launches, csrc/arnn_gen.hip) and the public surface down from
AnticipationRNNTester.generation(banned_tokens=, fixed_tokens=, clamp_context=).

The reference for the rule is its float64 restatement (tests/decoder_constraint_ref.py) APPLIED TO THE f32 LOGITS THE CALL RETURNED, as
in tests/test_gpu_arnn_trunc.py: ranks and ties compare exactly, and only expf's rounding and the order of the f64 sums are left to the
two margins (2e-5 around the kept CDF's steps and around the nucleus boundary).  A FREE draw (a tick with more than one allowed token)
is left out of the token comparison only when one of its margins is below 2e-5: at most 5 % of a case's free draws (DESIGN.md section
12's cap) -- a case is a shape (V, R) under the three settings; along the oracle's own masked trajectory
tests/test_arnn_constraint_host.py holds the same seeds and masks to half of that.  One-bit ticks are compared exactly and never left
out; no banned token is returned anywhere.  The returned logits are the UNMASKED ones, held to the float64 oracle run teacher-forced over
the GPU's own tokens.

TRAJ_TOL: DESIGN.md section 12's bound, 4 x 5.1e-7 of the case's max |logit|; the largest deviation measured over this file's cases is in
DESIGN.md section 14."""
import numpy as np
import pytest
import torch

from tests import arnn_trunc_ref as AR
from tests import decoder_constraint_ref as CR
from tests import decoder_trunc_ref as TR
from tests import golden_util as G

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from inpaintnet_amd import ops, synthetic
    from inpaintnet_amd.arnn import AnticipationRNNBaseline
    from inpaintnet_amd.arnn_tester import AnticipationRNNTester
    from tests.test_gpu_arnn_generate import _inputs, _model
    from tests.test_gpu_decode_plans import labels_of

TRAJ_TOL = 4 * 5.1e-7
measured = {"traj": 0.0, "logp": 0.0}        # the largest errors so far, printed by the checks
_nets = {}


def dev_net(V, E, Hc, H, U):
    key = (V, H)
    if key not in _nets:
        W = AR.net(V, E, Hc, H, U)
        _nets[key] = (W, [torch.from_numpy(w).cuda() for w in W])
    return _nets[key]


def words_of(allow):
    """bool [R,L,V] -> the kernel's words on the device, by the restatement's packing (not ops.pack_allowed)"""
    return torch.from_numpy(CR.words(allow).view(np.int64)).cuda().contiguous()


def call(Wd, oc, hc, u, temp, k, p, allow, want_logp=True, want_logits=True):
    """One call (allow bool [R,L,V], or None: the truncated call) -> (tokens [R,L], logp or None, logits or None, launch labels)"""
    ocd, hcd = torch.from_numpy(oc).cuda(), torch.from_numpy(hc).cuda() if hc is not None else None
    kw = {} if allow is None else {"allowed": words_of(allow)}
    (tok, lp, lg), labels = labels_of(lambda: ops.arnn_sample(Wd[0], ocd, *Wd[1:], temp, u, hc_init=hcd, top_k=k, top_p=p,
                                                              want_logp=want_logp, want_logits=want_logits, **kw))
    status = ops.chain_status()
    assert status == 0, (tuple(oc.shape), temp, k, p, status, ops.slow_waits_summary())
    return (tok.cpu().numpy(), lp.cpu().numpy() if lp is not None else None, lg.cpu().numpy() if lg is not None else None, labels)


def check_labels(labels, R, L, V, persistent):
    want = f"cons_arnn_token_sample R{R} L{L} V{V}" if persistent else f"cons_arnn_ticks L{L} V{V}"
    assert sum(l.startswith(want) for l in labels) == ((R + 7) // 8 if persistent else R), (want, sorted(set(labels)))
    assert not any(l.startswith(("arnn_token_sample", "trunc_", "sample_")) for l in labels), sorted(set(labels))


def check_rule(lg, tok, lp, temp, u, k, p, allow, what):
    """Tokens and logp against the restatement on the returned logits -> (free draws within a margin, free draws)"""
    V = lg.shape[-1]
    eff = allow | ~allow.any(-1, keepdims=True)
    assert tok.min() >= 0 and tok.max() < V, what
    assert np.take_along_axis(eff, tok[..., None], -1).all(), (what, "a banned token")
    want, wlp, n, cm, bm, d = CR.pick_rows(lg, temp, u, k, p, allow)
    free = CR.free(allow)
    firm = TR.firm(cm, bm) | ~free                              # one-bit ticks are never left out
    print(what, "within margin", int((~firm).sum()), "of", int(free.sum()), "free draws; differ", int((tok != want).sum()),
          "kept mean %.1f" % n.mean())
    assert np.array_equal(tok[firm], want[firm]), (what, np.argwhere((tok != want) & firm)[:4])
    fixed = ~free
    assert np.array_equal(tok[fixed], np.argmax(allow, -1)[fixed]), what
    # the kept set, at EVERY draw the rule applies to: it does not depend on u.  Where the nucleus margin alone is short the kernel may
    # have kept one token more: the first one outside the restatement's set, and nothing else
    kept = CR.kept_rows(lg, temp, k, p, allow)
    inside = np.take_along_axis(kept, tok[..., None], -1)[..., 0]
    for r, t in np.argwhere((n > 0) & ~inside):
        with np.errstate(invalid="ignore", over="ignore"):
            s = np.where(eff[r, t], (np.float32(temp) * lg[r, t]).astype(np.float32), np.float32(-np.inf))
        boundary = np.lexsort((np.arange(V), -s.astype(np.float64)))[n[r, t]] if n[r, t] < V else -1
        assert bm[r, t] < TR.MARGIN and tok[r, t] == boundary, (what, r, t, tok[r, t], boundary, bm[r, t])
    if lp is not None:
        rule = ~np.isnan(wlp)
        assert np.array_equal(np.isnan(lp), ~rule), what                      # NaN exactly where the tick took the argmax rule
        assert (lp[fixed & rule] == 0.0).all(), (what, "a fixed tick's logp is exactly 0")
        ok = firm & (tok == want) & rule
        assert ok.any(), what
        err = np.abs(lp[ok].astype(np.float64) - wlp[ok].astype(np.float64)) / TR.logp_tol(d[ok])
        measured["logp"] = max(measured["logp"], float(err.max()))
        print(what, "logp error / tolerance: max %.3f (all checks so far %.3f)" % (float(err.max()), measured["logp"]))
        assert err.max() <= 1.0, (what, float(err.max()))
    return int((~firm).sum()), int(free.sum())


def check_trajectory(W, oc, hc, tok, lg, what):
    """The returned logits of tick t are the network's function of the tokens < t: the float64 oracle teacher-forced over the GPU's tokens"""
    ref, _ = AR.trajectory(W, oc, hc, tokens=tok)
    err = float(np.abs(lg.astype(np.float64) - ref).max() / np.abs(ref).max())
    measured["traj"] = max(measured["traj"], err)
    print(what, "logits against the float64 oracle: %.3g of max |logit| (all checks so far %.3g)" % (err, measured["traj"]))
    assert err <= TRAJ_TOL, (what, err)
    return ref


def run_case(V, R, cfg, persistent):
    W, Wd = dev_net(V, **cfg)
    allow = CR.plan_mask(V, R, AR.L)
    near = draws = 0
    for si, (temp, k, p) in enumerate(AR.SETTINGS):
        oc, hc, u = AR.case(V, R, si, **cfg)
        tok, lp, lg, labels = call(Wd, oc, hc, u, temp, k, p, allow)
        what = (V, cfg["H"], R, temp, k, p)
        check_labels(labels, R, AR.L, V, persistent)
        check_trajectory(W, oc, hc, tok, lg, what)
        n, d = check_rule(lg, tok, lp, temp, u, k, p, allow, what)
        near, draws = near + n, draws + d
    print((V, R), "within margin", near, "of", draws, "free draws")
    assert near <= AR.NEAR_CAP * draws, (V, R, near, draws)
    assert ops.chain_status() == 0


@pytest.mark.parametrize("R", AR.ROWS)
@pytest.mark.parametrize("V", AR.FULL_V)
def test_the_rule_on_the_calls_own_logits(V, R):
    """H = U = 256 under plan_mask(V, R, 30) -- every fourth tick fixed, a fifth of the tokens banned elsewhere, another mask per row:
    V <= 64 runs the masked build of the persistent token pass (R = 11: 8 teams, then 3 -- the mask offset per launch), 64 < V <= 128 the
    per-tick launches with two words per tick.  Three settings per case."""
    run_case(V, R, AR.FULL, persistent=V <= 64)


@pytest.mark.parametrize("R", AR.ROWS)
def test_the_rule_on_the_per_tick_path(R):
    c = dict(AR.SMALL)
    V = c.pop("V")
    run_case(V, R, c, persistent=False)


def test_the_per_tick_path_of_the_token_pass_shape():
    """option key 14 = 0: H = 256, V = 48 through head_b1_kernel<NI, 3>"""
    try:
        ops.set_option(14, 0)
        run_case(48, 5, AR.FULL, persistent=False)
    finally:
        ops.set_option(14, 3)


@pytest.mark.parametrize("V", [48, 65])
def test_a_mask_of_all_ones_is_the_truncated_call(V):
    """Consequence 1 at R = 11: tokens, logits and logp of the truncated call bit for bit, with truncation off and on -- the persistent
    pass (V = 48: two launches) and the per-tick launches (V = 65: two words, the bits at and above V set or clear)."""
    W, Wd = dev_net(V, **AR.FULL)
    R = 11
    ones = np.ones((R, AR.L, V), dtype=bool)
    for si, (temp, k, p) in ((1, (1.5, 0, 1.0)), (2, AR.SETTINGS[2])):
        oc, hc, u = AR.case(V, R, si, **AR.FULL)
        tok0, lp0, lg0, labels0 = call(Wd, oc, hc, u, temp, k, p, None)
        assert any(l.startswith("trunc_") for l in labels0) and not any(l.startswith("cons_") for l in labels0), sorted(set(labels0))
        tok, lp, lg, labels = call(Wd, oc, hc, u, temp, k, p, ones)
        check_labels(labels, R, AR.L, V, V <= 64)
        assert np.array_equal(tok, tok0) and np.array_equal(lg.view(np.int32), lg0.view(np.int32)), (V, temp, k, p)
        assert np.array_equal(lp.view(np.int32), lp0.view(np.int32)), (V, temp, k, p)
        # the bits at and above V are ignored
        ocd, hcd = torch.from_numpy(oc).cuda(), torch.from_numpy(hc).cuda()
        full = torch.full((R, AR.L, (V + 63) // 64), -1, dtype=torch.int64, device="cuda")
        tok2, lp2, lg2 = ops.arnn_sample(Wd[0], ocd, *Wd[1:], temp, u, hc_init=hcd, top_k=k, top_p=p, want_logp=True, want_logits=True,
                                         allowed=full)
        assert np.array_equal(tok2.cpu().numpy(), tok0) and np.array_equal(lp2.cpu().numpy().view(np.int32), lp0.view(np.int32))
    assert ops.chain_status() == 0


@pytest.mark.parametrize("V,small", [(48, False), (64, False), (65, False), (12, True)])
def test_one_bit_ticks_return_their_token(V, small):
    """Consequence 2 at R = 11, every tick one-bit with another token per row and tick: that token for every u -- u = 1.0, 2.0 and NaN
    included, where the tick takes the masked argmax --, logp exactly 0.0f wherever the rule applies and NaN on exactly the other ticks.
    Rows 8 to 10 (the second launch of the persistent pass) return THEIR OWN tokens, which differ from those of rows 0 to 2."""
    cfg = dict(AR.SMALL) if small else dict(AR.FULL, V=V)
    cfg.pop("V")
    W, Wd = dev_net(V, **cfg)
    R = 11
    r, t = np.meshgrid(np.arange(R), np.arange(AR.L), indexing="ij")
    fix = (7 * r + 3 * t + 1) % V
    assert (fix[8:] != fix[:3]).all()
    allow = np.zeros((R, AR.L, V), dtype=bool)
    np.put_along_axis(allow, fix[..., None], True, -1)
    for si, (temp, k, p) in enumerate(AR.SETTINGS):
        oc, hc, u = AR.case(V, R, si, **cfg)
        u = u.copy()
        u[:, 5], u[3, 11], u[9, 12], u[10, AR.L - 1] = 1.0, 2.0, np.nan, 1.0
        out = ~((u >= 0.0) & (u < 1.0))
        tok, lp, lg, labels = call(Wd, oc, hc, u, temp, k, p, allow)
        check_labels(labels, R, AR.L, V, not small and V <= 64)
        assert np.array_equal(tok, fix), (V, temp, k, p, np.argwhere(tok != fix)[:4])
        assert np.array_equal(np.isnan(lp), out) and (lp[~out] == 0.0).all() and not np.signbit(lp[~out]).any(), (V, temp, k, p)
        check_trajectory(W, oc, hc, tok, lg, ("one-bit", V, temp, k, p))
    assert ops.chain_status() == 0


@pytest.mark.parametrize("V,small", [(48, False), (128, False), (12, True)])
def test_no_banned_token_outside_the_rule(V, small):
    """Ticks outside the rule under plan_mask: NaN head weights -- every token an allowed one, every logp NaN; a NaN logit at ONE place --
    every tick falls back, takes the NaN where it is allowed and the maximum of the ALLOWED logits where it is banned; uniforms of 1.0 --
    those ticks take the masked argmax of their returned logits with a NaN logp, every other tick follows the rule."""
    cfg = dict(AR.SMALL) if small else dict(AR.FULL, V=V)
    cfg.pop("V")
    W, Wd = dev_net(V, **cfg)
    R = 5
    temp, k, p = AR.SETTINGS[2]
    oc, hc, u = AR.case(V, R, 2, **cfg)
    allow = CR.plan_mask(V, R, AR.L)
    nanW = list(Wd)
    nanW[11] = torch.full_like(Wd[11], float("nan"))
    tok, lp, lg, _ = call(nanW, oc, hc, u, temp, k, p, allow)
    assert np.take_along_axis(allow, tok[..., None], -1).all() and np.isnan(lp).all() and np.isnan(lg).all()
    assert np.array_equal(tok, np.argmax(allow, -1))                       # (all NaN: the lowest allowed index)
    v0 = 3
    nanb = list(Wd)
    nanb[12] = Wd[12].clone()
    nanb[12][v0] = float("nan")
    tok, lp, lg, _ = call(nanb, oc, hc, u, temp, k, p, allow)
    assert np.isnan(lg[..., v0]).all() and not np.isnan(np.delete(lg, v0, -1)).any() and np.isnan(lp).all()
    want = np.array([[CR.masked_argmax(lg[r, t], allow[r, t]) for t in range(AR.L)] for r in range(R)])
    assert np.array_equal(tok, want) and np.take_along_axis(allow, tok[..., None], -1).all()
    assert (tok[allow[..., v0]] == v0).all() and (tok[~allow[..., v0]] != v0).all() and (~allow[..., v0]).any()
    u = u.copy()
    u[2, 7] = u[4, AR.L - 1] = u[0, 0] = u[1, 2] = 1.0                      # (free and fixed ticks)
    tok, lp, lg, _ = call(Wd, oc, hc, u, temp, k, p, allow)
    out = u >= 1.0
    assert np.array_equal(np.isnan(lp), out)
    assert np.array_equal(tok[out], np.array([CR.masked_argmax(x, a) for x, a in zip(lg[out], allow[out])]))
    n, d = check_rule(lg, tok, lp, temp, u, k, p, allow, ("outside", V))
    assert n <= AR.NEAR_CAP * d
    check_trajectory(W, oc, hc, tok, lg, ("outside", V))
    assert ops.chain_status() == 0


@pytest.mark.parametrize("V", [48, 65])
def test_the_fixed_token_is_fed_back(V):
    """Tick t fixed to a token the untruncated call does not draw there: the call returns it, the logits up to t are the unconstrained
    call's, and those of tick t + 1 are the float64 oracle's teacher-forced over the GPU's own tokens -- the network saw the fixed token --
    and differ from the unconstrained call's by more than 1e-3 of max |logit|."""
    W, Wd = dev_net(V, **AR.FULL)
    oc, hc, u = AR.case(V, 1, 1, **AR.FULL)
    tok0, _, lg0, _ = call(Wd, oc, hc, u, 1.5, 0, 1.0, None)
    t = 9
    f = (int(tok0[0, t]) + 17) % V
    allow = np.ones((1, AR.L, V), dtype=bool)
    allow[0, t] = False
    allow[0, t, f] = True
    tok, lp, lg, labels = call(Wd, oc, hc, u, 1.5, 0, 1.0, allow)
    check_labels(labels, 1, AR.L, V, V <= 64)
    assert tok[0, t] == f != tok0[0, t] and lp[0, t] == 0.0
    assert np.array_equal(tok[0, :t], tok0[0, :t]) and np.array_equal(lg[0, :t + 1], lg0[0, :t + 1])
    ref = check_trajectory(W, oc, hc, tok, lg, ("fed back", V))
    scale = np.abs(ref).max()
    assert np.abs(lg[0, t + 1].astype(np.float64) - ref[0, t + 1]).max() <= TRAJ_TOL * scale
    moved = np.abs(lg[0, t + 1] - lg0[0, t + 1]).max()
    print("fed back", V, "tick t + 1 moved by %.3g of max |logit|" % (moved / scale))
    assert moved > 1e-3 * scale
    n, d = check_rule(lg, tok, lp, 1.5, u, 0, 1.0, allow, ("fed back", V))
    assert n <= AR.NEAR_CAP * d
    assert ops.chain_status() == 0


@pytest.mark.parametrize("name,key", [("full", "full/t1/0"), ("small", "small/t0/1")])
def test_generate_takes_a_mask_and_without_one_is_todays_call(name, key, monkeypatch):
    """generate(allowed=) with one row and with a batch of three agrees with ops.arnn_sample called on what generate handed it -- the same
    constraint outputs, warm-up state and uniforms -- under the mask packed by the restatement; last_logp is left exactly when top_k /
    top_p is given.  generate(allowed=None) reproduces tests/golden/arnn_generate.npz with the kernels it always ran."""
    fx = G.load("arnn_generate")
    _, model = _model(name)
    s, m, c = _inputs(fx, name)
    ti, i = int(key.split("/")[1][1:]), int(key.split("/")[2])
    seed, temp = int(fx[key + "/seed"]), float(fx["temperatures"][ti])
    V = G.ARNN_CFGS[name]["V"]
    np.random.seed(seed)
    (_, gen, _), labels = labels_of(lambda: model.generate(s[i], m[i], c[i], temperature=temp))
    assert np.array_equal(gen[0].cpu().numpy(), fx[key + "/tokens"].astype(np.int64)) and model.last_logp is None
    assert not any(l.startswith(("cons_", "trunc_")) for l in labels), sorted(set(labels))
    np.random.seed(seed)
    _, gen_none, _ = model.generate(s[i], m[i], c[i], temperature=temp, allowed=None)
    assert torch.equal(gen_none, gen)
    Lg = gen.shape[1]
    seen = {}
    real = ops.arnn_sample

    def recording(*a, **kw):
        seen["a"], seen["kw"] = a, dict(kw)
        return real(*a, **kw)
    monkeypatch.setattr(ops, "arnn_sample", recording)
    for B in (1, 3):
        allow = CR.plan_mask(V, B, Lg)
        sc, md, lc = (s[i], m[i], c[i]) if B == 1 else (s[:1].expand(B, -1, -1).reshape(B, 1, Lg).contiguous(),
                                                        m[:1].expand(B, -1, -1, -1).reshape(B, 1, Lg, -1).contiguous(),
                                                        c[:1].expand(B, -1, -1).reshape(B, 1, Lg).contiguous())
        mask = torch.from_numpy(allow[0] if B == 1 else allow)
        np.random.seed(seed)
        (_, gen, _), labels = labels_of(lambda: model.generate(sc, md, lc, temperature=temp, top_k=8, top_p=0.9, keep_weights=True,
                                                               allowed=mask if B == 1 else mask.cuda()))
        want = f"cons_arnn_token_sample R{B} " if name == "full" else "cons_arnn_ticks "
        assert sum(l.startswith(want) for l in labels) == (1 if name == "full" else B), sorted(set(labels))
        a, kw = seen["a"], seen["kw"]
        assert np.array_equal(kw["allowed"].cpu().numpy().view(np.uint64), CR.words(allow))
        u = np.random.RandomState(seed).random_sample((B, Lg))
        assert np.array_equal(np.asarray(a[15]), u)
        tok, lp, lg = real(*a[:15], u, hc_init=kw["hc_init"], top_k=8, top_p=0.9, want_logp=True, want_logits=True, allowed=words_of(allow))
        g = gen.view(B, Lg)
        assert torch.equal(g, tok) and torch.equal(model.last_logp.view(B, Lg), lp) and torch.equal(model.last_weights, lg)
        assert tuple(model.last_logp.shape) == ((B, 1, Lg) if B > 1 else (1, Lg))
        n, d = check_rule(lg.cpu().numpy(), tok.cpu().numpy(), lp.cpu().numpy(), temp, u, 8, 0.9, allow, (name, "generate", B))
        assert n <= AR.NEAR_CAP * d
        np.random.seed(seed)
        _, gen2, _ = model.generate(sc, md, lc, temperature=temp, allowed=mask)              # no top_k / top_p: no last_logp
        assert model.last_logp is None and model.last_weights is None
        assert np.take_along_axis(allow, gen2.view(B, Lg).cpu().numpy()[..., None], -1).all()
    assert ops.chain_status() == 0


@pytest.mark.parametrize("name", ["small", "full"])
def test_the_tester_constrains_the_window_and_clamps_the_context(name, monkeypatch):
    """generation(clamp_context=True, num_variations=4, top_p=0.9): generate()'s OWN tokens equal the input outside the window in every
    row with model.last_logp exactly 0 there, the variations differ inside the window; with fixed_tokens and banned_tokens the fixed ticks
    are kept (also where the fixed token is a banned one), the banned tokens are absent from the free ticks; last_logp is the sum of the
    window's log-probabilities per measure; one variation with a constraint takes the batched call."""
    ds, model = _model(name, AnticipationRNNBaseline)
    tester = AnticipationRNNTester(ds, model)
    V = G.ARNN_CFGS[name]["V"]
    Lg, nv = 384, 4
    score = torch.from_numpy(synthetic.folk_score(1, V, seed=5)).long()[0].cuda()
    md = torch.from_numpy(synthetic.folk_metadata(1)).long()[0].cuda()
    a, b = 3 * 24, 6 * 24
    outside = torch.ones(Lg, dtype=torch.bool)
    outside[a:b] = False
    raw = {}
    real = model.generate

    def recording(**kw):
        out = real(**kw)
        raw["gen"] = out[1].clone()
        return out
    monkeypatch.setattr(model, "generate", recording)
    np.random.seed(11)
    (gen_score, gen_tensor, orig), labels = labels_of(lambda: tester.generation(score, start_measure=4, num_measures_gen=3,
                                                                                 tensor_metadata=md, num_variations=nv, temperature=6.0,
                                                                                 top_p=0.9, clamp_context=True))
    want = f"cons_arnn_token_sample R{nv} " if name == "full" else "cons_arnn_ticks "
    assert sum(l.startswith(want) for l in labels) == (1 if name == "full" else nv), sorted(set(labels))
    assert tuple(gen_tensor.shape) == (nv, Lg) and tuple(raw["gen"].shape) == (nv, 1, Lg)
    assert torch.equal(raw["gen"][:, 0][:, outside], score[:, outside].expand(nv, -1))         # what the network was fed: the true context
    assert torch.equal(gen_tensor[:, outside], score[:, outside].expand(nv, -1))
    assert bool((model.last_logp[:, 0][:, outside] == 0.0).all())
    win = gen_tensor[:, a:b].cpu().numpy()
    assert win.min() >= 0 and win.max() < V and len({tuple(r) for r in win.tolist()}) == nv
    lp = tester.last_logp
    assert tuple(lp.shape) == (nv, 3) and bool(torch.isfinite(lp).all()) and bool((lp < 0).all())
    assert torch.equal(lp, model.last_logp[:, 0, a:b].reshape(nv, 3, 24).sum(-1))
    # fixed and banned tokens (the most drawn token of the window banned, one fixed tick set to it), with the context clamped or not
    banned = [int(np.bincount(win.reshape(-1), minlength=V).argmax()), 0]
    fixed = torch.full((3, 24), -1)
    fixed[0, 0], fixed[1, 7], fixed[2, 23] = banned[0], (banned[0] + 1) % V, V - 1
    keep = (fixed >= 0).reshape(-1)
    for clamp in (True, False):
        np.random.seed(12)
        _, g, _ = tester.generation(score, start_measure=4, num_measures_gen=3, tensor_metadata=md, num_variations=nv, temperature=6.0,
                                    top_k=8, top_p=0.9, banned_tokens=banned, fixed_tokens=fixed if clamp else fixed.reshape(-1),
                                    clamp_context=clamp)
        w = g[:, a:b].cpu()
        assert torch.equal(w[:, keep], fixed.reshape(-1)[keep].expand(nv, -1))
        assert not bool(torch.isin(w[:, ~keep], torch.tensor(banned)).any())
        assert torch.equal(g[:, outside], score[:, outside].expand(nv, -1))
        assert torch.equal(raw["gen"][:, 0][:, outside], score[:, outside].expand(nv, -1)) == clamp
        mlp = model.last_logp[:, 0, a:b]
        assert bool((mlp[:, keep] == 0.0).all()) and bool(torch.isfinite(mlp).all())
        assert torch.equal(tester.last_logp, mlp.reshape(nv, 3, 24).sum(-1))
    # one variation with a constraint: the batched call, and no last_logp without top_k / top_p
    np.random.seed(13)
    (_, one, _), labels = labels_of(lambda: tester.generation(score, start_measure=4, num_measures_gen=3, tensor_metadata=md,
                                                              banned_tokens=banned))
    assert tuple(one.shape) == (1, Lg) and tester.last_logp is None and tuple(raw["gen"].shape) == (1, 1, Lg)
    assert any(l.startswith("cons_") for l in labels) and not bool(torch.isin(one[:, a:b].cpu(), torch.tensor(banned)).any())
    # today's call: the new arguments at their defaults
    np.random.seed(14)
    (_, today, _), labels = labels_of(lambda: tester.generation(score, start_measure=4, num_measures_gen=3, tensor_metadata=md))
    assert not any(l.startswith(("cons_", "trunc_")) for l in labels) and tuple(raw["gen"].shape) == (1, Lg)
    np.random.seed(14)
    _, again, _ = tester.generation(score, start_measure=4, num_measures_gen=3, tensor_metadata=md, banned_tokens=None, fixed_tokens=None,
                                    clamp_context=False)
    assert torch.equal(again, today)
    assert ops.chain_status() == 0
