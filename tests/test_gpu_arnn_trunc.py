"""AnticipationRNN's top-k / nucleus truncated sampling on the GPU (inet_arnn_sample_ex: the truncating build of the persistent token
pass and head_b1_kernel<NI, 2> of the per-tick launches, csrc/arnn_gen.hip), its log-probabilities and logits, and the public surface
down from AnticipationRNNTester.generation.

The reference for the rule is its float64 restatement (tests/decoder_trunc_ref.py) APPLIED TO THE f32 LOGITS THE CALL RETURNED: those
are bit for bit what the kernel ranked and drew from, so ranks and ties compare exactly and only expf's rounding and the order of the
f64 sums are left to the two margins (2e-5 around the kept CDF's steps and around the nucleus boundary).  A draw is left out only when
one of its margins is below 2e-5: at most 5 % of a case's draws -- a case is a shape (V, R) under the three settings, 90 R draws; along
the oracle's own trajectory tests/test_arnn_trunc_host.py holds the same seeds to half of that.  The returned logits themselves are
held to the float64 oracle run teacher-forced over the GPU's own tokens.

TRAJ_TOL: the largest deviation measured on an MI355X over all cases of this file is 5.1e-7 of the case's max |logit| (V = 65, R = 1
under (1, 5, 1.0), the per-tick launches; the persistent pass: 4.3e-7 -- DESIGN.md section 12); the bound is 4 x that, for box-to-box
and summation-order differences, and far below the project's fp32 parity bar of 1e-4."""
import numpy as np
import pytest
import torch

from tests import arnn_trunc_ref as AR
from tests import decoder_sample_ref as R_
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


def call(Wd, oc, hc, u, temp, k, p, want_logp=True, want_logits=True):
    """One truncated call -> (tokens [R,L], logp or None, logits or None, launch labels); a bounded-spin timeout fails here."""
    ocd, hcd = torch.from_numpy(oc).cuda(), torch.from_numpy(hc).cuda() if hc is not None else None
    (tok, lp, lg), labels = labels_of(lambda: ops.arnn_sample(Wd[0], ocd, *Wd[1:], temp, u, hc_init=hcd, top_k=k, top_p=p,
                                                              want_logp=want_logp, want_logits=want_logits))
    status = ops.chain_status()
    assert status == 0, (tuple(oc.shape), temp, k, p, status, ops.slow_waits_summary())
    return (tok.cpu().numpy(), lp.cpu().numpy() if lp is not None else None, lg.cpu().numpy() if lg is not None else None, labels)


def check_labels(labels, R, L, V, persistent):
    want = f"trunc_arnn_token_sample R{R} L{L} V{V}" if persistent else f"trunc_arnn_ticks L{L} V{V}"
    assert sum(l.startswith(want) for l in labels) == ((R + 7) // 8 if persistent else R), (want, sorted(set(labels)))
    assert not any(l.startswith(("arnn_token_sample", "sample_")) for l in labels), sorted(set(labels))


def check_rule(lg, tok, lp, temp, u, k, p, what):
    """Tokens and logp against the restatement on the returned logits -> (draws within a margin, draws)"""
    V = lg.shape[-1]
    assert tok.min() >= 0 and tok.max() < V, what
    want, wlp, n, cm, bm, d = TR.pick_rows(lg, temp, u, k, p)
    firm = TR.firm(cm, bm)
    print(what, "within margin", int((~firm).sum()), "of", firm.size, "differ", int((tok != want).sum()), "kept mean %.1f" % n.mean())
    assert np.array_equal(tok[firm], want[firm]), (what, np.argwhere((tok != want) & firm)[:4])
    # the kept set, at EVERY draw the rule applies to: it does not depend on u.  Where the nucleus margin alone is short the kernel may
    # have kept one token more: the first one outside the restatement's set, and nothing else
    kept = TR.kept_rows(lg, temp, k, p)
    inside = np.take_along_axis(kept, tok[..., None], -1)[..., 0]
    for r, t in np.argwhere((n > 0) & ~inside):
        s = (np.float32(temp) * lg[r, t]).astype(np.float32)
        boundary = np.lexsort((np.arange(V), -s.astype(np.float64)))[n[r, t]] if n[r, t] < V else -1
        assert bm[r, t] < TR.MARGIN and tok[r, t] == boundary, (what, r, t, tok[r, t], boundary, bm[r, t])
    if lp is not None:
        assert np.array_equal(np.isnan(lp), np.isnan(wlp)), what              # NaN exactly where the tick took the argmax rule
        ok = firm & (tok == want) & ~np.isnan(wlp)
        assert ok.any(), what
        err = np.abs(lp[ok].astype(np.float64) - wlp[ok].astype(np.float64)) / TR.logp_tol(d[ok])
        measured["logp"] = max(measured["logp"], float(err.max()))
        print(what, "logp error / tolerance: max %.3f (all checks so far %.3f)" % (float(err.max()), measured["logp"]))
        assert err.max() <= 1.0, (what, float(err.max()))
    return int((~firm).sum()), firm.size


def check_trajectory(W, oc, hc, tok, lg, what):
    """The returned logits of tick t are the network's function of the tokens < t: the float64 oracle teacher-forced over the GPU's tokens"""
    ref, _ = AR.trajectory(W, oc, hc, tokens=tok)
    err = float(np.abs(lg.astype(np.float64) - ref).max() / np.abs(ref).max())
    measured["traj"] = max(measured["traj"], err)
    print(what, "logits against the float64 oracle: %.3g of max |logit| (all checks so far %.3g)" % (err, measured["traj"]))
    assert err <= TRAJ_TOL, (what, err)


def run_case(V, R, cfg, persistent):
    W, Wd = dev_net(V, **cfg)
    near = draws = 0
    for si, (temp, k, p) in enumerate(AR.SETTINGS):
        oc, hc, u = AR.case(V, R, si, **cfg)
        tok, lp, lg, labels = call(Wd, oc, hc, u, temp, k, p)
        what = (V, cfg["H"], R, temp, k, p)
        check_labels(labels, R, AR.L, V, persistent)
        check_trajectory(W, oc, hc, tok, lg, what)
        n, d = check_rule(lg, tok, lp, temp, u, k, p, what)
        near, draws = near + n, draws + d
    assert near <= AR.NEAR_CAP * draws, (V, R, near, draws)
    assert ops.chain_status() == 0


@pytest.mark.parametrize("R", AR.ROWS)
@pytest.mark.parametrize("V", AR.FULL_V)
def test_the_rule_on_the_calls_own_logits(V, R):
    """H = U = 256: V <= 64 runs the truncating build of the persistent token pass (R = 11: 8 teams, then 3 -- logp and logits offset per
    launch), 64 < V <= 128 the per-tick launches (the two-chunk truncating build is not built: it spills).  Three settings per case."""
    run_case(V, R, AR.FULL, persistent=V <= 64)


@pytest.mark.parametrize("R", AR.ROWS)
def test_the_rule_on_the_per_tick_path(R):
    c = dict(AR.SMALL)
    V = c.pop("V")
    run_case(V, R, c, persistent=False)


def test_the_per_tick_path_of_the_token_pass_shape():
    """option key 14 = 0: H = 256, V = 48 through head_b1_kernel<NI, 2>"""
    try:
        ops.set_option(14, 0)
        run_case(48, 5, AR.FULL, persistent=False)
    finally:
        ops.set_option(14, 3)


@pytest.mark.parametrize("shape", ["full", "small"])
def test_exact_logits_leave_no_margin(shape):
    """W2 = 0: every tick's logits are exactly b2.  b2 has its maximum 3 at index 7, the value 2 at 3, 10 and 20 (11 for the small shape), 1 at 0
    and 30 (5) and 0.5 elsewhere: top_k = 3 puts its boundary between the equal 10 and 20 -- 20 is never drawn over R x L draws,
    3 and 10 are; top_k = 1 is the first argmax with logp exactly 0; under the three settings every token lies in the exactly known
    kept set."""
    cfg = dict(AR.FULL, V=48) if shape == "full" else dict(AR.SMALL)
    V = cfg.pop("V")
    R = 11
    W, _ = dev_net(V, **cfg)
    W = list(W)
    W[11] = np.zeros_like(W[11])
    b2 = np.full(V, 0.5, dtype=np.float32)
    last2 = 20 if V > 20 else 11
    b2[[0, 30 if V > 30 else 5]] = 1.0
    b2[[3, 10, last2]] = 2.0
    b2[7] = 3.0
    W[12] = b2
    Wd = [torch.from_numpy(w).cuda() for w in W]
    oc, hc, u = AR.case(V, R, 0, **cfg)
    tok, lp, lg, labels = call(Wd, oc, hc, u, 1.0, 3, 1.0)
    check_labels(labels, R, AR.L, V, shape == "full")
    assert np.array_equal(lg, np.broadcast_to(b2, lg.shape))
    assert set(np.unique(tok).tolist()) == {3, 7, 10} and last2 not in tok
    want = np.float32(np.float64(b2[tok] - np.float32(3.0)) - np.log(1.0 + 2.0 * np.exp(np.float32(-1.0)).astype(np.float64)))
    assert np.allclose(lp, want, rtol=0, atol=8 * 2.0 ** -23)
    tok, lp, lg, _ = call(Wd, oc, hc, u, 2.5, 1, 1.0)
    assert (tok == R_.argmax_first(b2)).all() and (tok == 7).all() and np.array_equal(lp, np.zeros_like(lp))
    for si, (temp, k, p) in enumerate(AR.SETTINGS):
        _, _, n, _, bm = TR.pick(b2, temp, 0.5, k, p)
        assert bm >= TR.MARGIN                                       # (precondition: the boundary of these logits is firm)
        kept = TR.kept_rows(b2, temp, k, p)
        assert kept.sum() == n < V
        tok, lp, lg, _ = call(Wd, oc, hc, AR.case(V, R, si, **cfg)[2], temp, k, p)
        assert kept[tok].all() and np.isfinite(lp).all() and (lp <= 0).all(), (temp, k, p, np.unique(tok))
    assert ops.chain_status() == 0


@pytest.mark.parametrize("V,small", [(48, False), (64, False), (12, True)])
def test_equalities_without_a_margin(V, small):
    """(top_k, top_p) = (0, 1.0) with logp and logits asked for: the tokens of the plain call on the same inputs, bit for bit, R = 11
    (the truncating build draws with the same instructions on the same values); with one or none of the two outputs the same tokens
    again.  top_k = 1: the first argmax of the returned logits at every tick."""
    cfg = dict(AR.SMALL) if small else dict(AR.FULL, V=V)
    cfg.pop("V")
    W, Wd = dev_net(V, **cfg)
    oc, hc, u = AR.case(V, 11, 1, **cfg)
    ocd, hcd = torch.from_numpy(oc).cuda(), torch.from_numpy(hc).cuda()
    plain, labels = labels_of(lambda: ops.arnn_sample(Wd[0], ocd, *Wd[1:], 1.5, u, hc_init=hcd))
    assert isinstance(plain, torch.Tensor) and not any(l.startswith("trunc_") for l in labels), sorted(set(labels))
    tok, lp, lg, labels = call(Wd, oc, hc, u, 1.5, 0, 1.0)
    check_labels(labels, 11, AR.L, V, not small)
    assert np.array_equal(tok, plain.cpu().numpy())
    assert np.isfinite(lp).all() and (lp < 0).all()
    for want_logp, want_logits in ((True, False), (False, True)):
        t2, lp2, lg2, labels = call(Wd, oc, hc, u, 1.5, 0, 1.0, want_logp=want_logp, want_logits=want_logits)
        check_labels(labels, 11, AR.L, V, not small)
        assert np.array_equal(t2, tok) and (lp2 is None) == (not want_logp) and (lg2 is None) == (not want_logits)
        assert lp2 is None or np.array_equal(lp2, lp)
        assert lg2 is None or np.array_equal(lg2, lg)
    # the new entry with (0, 1.0, null, null) is inet_arnn_sample: the kernels it always ran
    t3, lp3, lg3, labels = call(Wd, oc, hc, u, 1.5, None, 1.0, want_logp=False, want_logits=False)
    assert not any(l.startswith("trunc_") for l in labels), sorted(set(labels))
    assert np.array_equal(t3, tok) and lp3 is None and lg3 is None
    tok1, lp1, lg1, _ = call(Wd, oc, hc, u, 1.5, 1, 1.0)
    assert np.array_equal(tok1, np.array([[R_.argmax_first(x) for x in row] for row in lg1]))
    assert np.array_equal(lp1, np.zeros_like(lp1))
    assert ops.chain_status() == 0


@pytest.mark.parametrize("name,key", [("full", "full/t1/0"), ("small", "small/t0/1")])
def test_generate_reproduces_the_reference_tokens_through_the_new_build(name, key):
    """model.generate(..., top_p=1.0) under np.random.seed: the tokens of tests/golden/arnn_generate.npz, exactly L draws taken from the
    stream, a finite score everywhere."""
    fx = G.load("arnn_generate")
    _, model = _model(name)
    s, m, c = _inputs(fx, name)
    ti, i = int(key.split("/")[1][1:]), int(key.split("/")[2])
    seed = int(fx[key + "/seed"])
    np.random.seed(seed)
    (score, gen, md), labels = labels_of(lambda: model.generate(s[i], m[i], c[i], temperature=float(fx["temperatures"][ti]), top_p=1.0,
                                                                keep_weights=True))
    nxt = np.random.random_sample()
    Lg = gen.shape[1]
    assert any(l.startswith("trunc_arnn_token_sample" if name == "full" else "trunc_arnn_ticks") for l in labels), sorted(set(labels))
    assert np.array_equal(gen[0].cpu().numpy(), fx[key + "/tokens"].astype(np.int64))
    assert nxt == np.random.RandomState(seed).random_sample(Lg + 1)[Lg]
    lp = model.last_logp
    assert tuple(lp.shape) == tuple(gen.shape) and lp.dtype == torch.float32
    assert bool(torch.isfinite(lp).all()) and bool((lp <= 0).all())
    V = G.ARNN_CFGS[name]["V"]
    assert tuple(model.last_weights.shape) == (1, Lg, V)
    # ... and the score is the rule's on the weights the call kept
    n, d = check_rule(model.last_weights.cpu().numpy(), gen.cpu().numpy(), lp.cpu().numpy(), float(fx["temperatures"][ti]),
                      np.random.RandomState(seed).random_sample((1, Lg)), 0, 1.0, key)
    assert n <= AR.NEAR_CAP * d
    np.random.seed(seed)
    _, gen2, _ = model.generate(s[i], m[i], c[i], temperature=float(fx["temperatures"][ti]))
    assert torch.equal(gen2, gen) and model.last_logp is None and model.last_weights is None
    assert ops.chain_status() == 0


@pytest.mark.parametrize("V,small", [(48, False), (128, False), (12, True)])
def test_ticks_outside_the_rule(V, small):
    """NaN head weights: every token inside [0, V), every logp NaN.  One uniform set to 1.0: that tick takes the argmax of its logits
    with a NaN logp, every other tick follows the rule."""
    cfg = dict(AR.SMALL) if small else dict(AR.FULL, V=V)
    cfg.pop("V")
    W, Wd = dev_net(V, **cfg)
    temp, k, p = AR.SETTINGS[2]
    oc, hc, u = AR.case(V, 5, 2, **cfg)
    nanW = list(Wd)
    nanW[11] = torch.full_like(Wd[11], float("nan"))
    tok, lp, lg, _ = call(nanW, oc, hc, u, temp, k, p)
    assert tok.min() >= 0 and tok.max() < V and np.isnan(lp).all() and np.isnan(lg).all()
    u = u.copy()
    u[2, 7] = 1.0
    u[4, AR.L - 1] = 1.0
    tok, lp, lg, _ = call(Wd, oc, hc, u, temp, k, p)
    out = u >= 1.0
    assert np.isnan(lp[out]).all() and not np.isnan(lp[~out]).any()
    assert np.array_equal(tok[out], np.array([R_.argmax_first(x) for x in lg[out]]))
    n, d = check_rule(lg, tok, lp, temp, u, k, p, ("outside", V))
    assert n <= AR.NEAR_CAP * d
    check_trajectory(W, oc, hc, tok, lg, ("outside", V))
    assert ops.chain_status() == 0


@pytest.mark.parametrize("name", ["small", "full"])
def test_the_tester_generates_and_scores_variations(name):
    """generation(num_variations=4, temperature=6, top_k=8, top_p=0.9): (4, L) fillings of the one gap from one batched generate call,
    pairwise different inside the window, past and future the input's; last_logp (4, 3) = the window sums of model.last_logp.
    num_variations = 1 without truncation is today's call."""
    ds, model = _model(name, AnticipationRNNBaseline)
    tester = AnticipationRNNTester(ds, model)
    V = G.ARNN_CFGS[name]["V"]
    Lg = 384
    score = torch.from_numpy(synthetic.folk_score(1, V, seed=5)).long()[0].cuda()
    md = torch.from_numpy(synthetic.folk_metadata(1)).long()[0].cuda()
    a, b = 3 * 24, 6 * 24
    np.random.seed(11)
    (gen_score, gen_tensor, orig), labels = labels_of(lambda: tester.generation(score, start_measure=4, num_measures_gen=3,
                                                                                 tensor_metadata=md, num_variations=4, temperature=6.0,
                                                                                 top_k=8, top_p=0.9))
    assert np.random.random_sample() == np.random.RandomState(11).random_sample(4 * Lg + 1)[4 * Lg]      # ONE batched call's draws
    want = "trunc_arnn_token_sample R4 " if name == "full" else "trunc_arnn_ticks "
    assert sum(l.startswith(want) for l in labels) == (1 if name == "full" else 4), sorted(set(labels))
    assert gen_score is None and orig is None
    assert tuple(gen_tensor.shape) == (4, Lg) and gen_tensor.dtype == torch.int64
    assert torch.equal(gen_tensor[:, :a], score[:, :a].expand(4, -1)) and torch.equal(gen_tensor[:, b:], score[:, b:].expand(4, -1))
    win = gen_tensor[:, a:b].cpu().numpy()
    assert win.min() >= 0 and win.max() < V and len({tuple(r) for r in win.tolist()}) == 4
    lp = tester.last_logp
    assert tuple(lp.shape) == (4, 3) and lp.dtype == torch.float32 and bool(torch.isfinite(lp).all()) and bool((lp < 0).all())
    assert tuple(model.last_logp.shape) == (4, 1, Lg)
    assert torch.equal(lp, model.last_logp[:, 0, a:b].reshape(4, 3, 24).sum(-1))
    # the same seed again: the same fillings and scores
    np.random.seed(11)
    _, again, _ = tester.generation(score, start_measure=4, num_measures_gen=3, tensor_metadata=md, num_variations=4, temperature=6.0,
                                    top_k=8, top_p=0.9)
    assert torch.equal(again, gen_tensor) and torch.equal(tester.last_logp, lp)
    # today's call, and the new arguments at their defaults
    np.random.seed(12)
    _, today, _ = tester.generation(score, start_measure=4, num_measures_gen=3, tensor_metadata=md)
    assert tester.last_logp is None and tuple(today.shape) == (1, Lg)
    np.random.seed(12)
    _, one, _ = tester.generation(score, start_measure=4, num_measures_gen=3, tensor_metadata=md, temperature=1.5, num_variations=1)
    assert torch.equal(one, today) and tester.last_logp is None
    np.random.seed(12)
    _, scored, _ = tester.generation(score, start_measure=4, num_measures_gen=3, tensor_metadata=md, top_p=1.0)
    assert torch.equal(scored, today) and tuple(tester.last_logp.shape) == (1, 3)
    with pytest.raises(ValueError):
        tester.generation(score, start_measure=4, num_measures_gen=3, tensor_metadata=md, num_variations=0)
    assert ops.chain_status() == 0
