"""The decoder's per-tick token constraints on the GPU: inet_sample_constrained's kernel alone, the masked build of the register-resident
launch in every plan a constrained call can get (csrc/decode_b1.hip), the tick-by-tick path of every other shape, fallback ticks, and
the public surface down from LatentRNNTester.generate(banned_tokens=, fixed_tokens=).

The reference for the rule is its float64 restatement (tests/decoder_constraint_ref.py) APPLIED TO THE f32 LOGITS THE CALL RETURNED, as in
tests/test_gpu_decoder_trunc.py.  A draw is left out of a comparison only when one of its two margins is below 2e-5; at most 1 % of a
test function's FREE draws (ticks with more than one allowed token) and 3 % of a setting's may be -- the counts for these masks and seeds
are made on the CPU by tests/test_decoder_constraint_host.py, which holds them to the same caps.  One-bit ticks are compared exactly and
never left out; no banned token is returned anywhere."""
import numpy as np
import pytest
import torch

from tests import decoder_constraint_ref as CR
from tests import decoder_sample_ref as R
from tests import decoder_trunc_ref as TR
from tests import golden_util as G

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from inpaintnet_amd import ops, synthetic
    from inpaintnet_amd.latent_rnn_tester import LatentRNNTester
    from inpaintnet_amd.latent_rnn_trainer import LatentRNNTrainer
    from tests.test_gpu_decode_plans import decoder, labels_of
    from tests.test_gpu_decoder_sample import small_model

TOL = 2e-5
measured = {"logp": 0.0}        # the largest logp error in units of its tolerance, printed by the logp checks


def constrained(cfg, z, params, temp, u, top_k, top_p, allow, mask_tick=None):
    """One constrained call at the ops level (allow bool [B,T,V], or packed words) -> (weights, tokens [B,T], logp [B,T], launch labels)"""
    B = z.shape[0]
    ud = torch.from_numpy(np.ascontiguousarray(u)).cuda()
    words = allow if isinstance(allow, torch.Tensor) else ops.pack_allowed(torch.from_numpy(np.ascontiguousarray(allow)))
    lp = torch.full((B, 24), 7.0, dtype=torch.float32, device="cuda")
    (w, s_, _), labels = labels_of(lambda: ops.decoder_fwd(cfg, z, None, False, params, mask_tick=mask_tick, temperature=temp,
                                                           uniforms=ud, top_k=top_k, top_p=top_p, logp=lp,
                                                           allowed=words.cuda().contiguous()))
    status = ops.chain_status()
    assert status == 0, (tuple(z.shape), temp, top_k, top_p, status, ops.slow_waits_summary())
    return w.clone(), s_.cpu().numpy()[:, 0].copy(), lp.cpu().numpy(), labels


def check_rule(w, tok, lp, temp, u, top_k, top_p, allow, what):
    """Tokens and logp against the restatement on the returned weights -> (free draws within a margin, free draws)"""
    wn = w.cpu().numpy()
    want, wlp, n, cm, bm, d = CR.pick_rows(wn, temp, u, top_k, top_p, allow)
    free = CR.free(allow)
    firm = TR.firm(cm, bm) | ~free                              # one-bit ticks are never left out
    print(what, "within margin", int((~firm).sum()), "of", int(free.sum()), "free draws; differ", int((tok != want).sum()))
    assert np.take_along_axis(allow | ~allow.any(-1, keepdims=True), tok[..., None], -1).all(), (what, "a banned token")
    assert np.array_equal(tok[firm], want[firm]), (what, np.argwhere((tok != want) & firm)[:4])
    fixed = ~free
    assert np.array_equal(tok[fixed], np.argmax(allow, -1)[fixed]), what
    rule = ~np.isnan(wlp)
    assert (lp[fixed & rule] == 0.0).all(), (what, "a fixed tick's logp is exactly 0")
    assert np.array_equal(np.isnan(lp), np.isnan(wlp)), what                  # NaN exactly where the tick took the argmax rule
    ok = firm & (tok == want) & rule
    assert ok.any(), what
    err = np.abs(lp[ok].astype(np.float64) - wlp[ok].astype(np.float64)) / TR.logp_tol(d[ok])
    measured["logp"] = max(measured["logp"], float(err.max()))
    print(what, "logp error / tolerance: max %.3f (all checks so far %.3f)" % (float(err.max()), measured["logp"]))
    assert err.max() <= 1.0, (what, float(err.max()))
    return int((~firm).sum()), int(free.sum())


@pytest.mark.parametrize("V", TR.ALONE_V)
def test_the_masked_kernel_alone(V):
    """inet_sample_constrained: rows in {1, 5, 70}, a row stride larger than V with NaN in the padding, strided uniforms, outputs, logp and
    mask rows; top_k in {0, 1, 2, V - 1, V, V + 5} x top_p in {1, 0.999, 0.5, 1e-9} x temperatures {1, 6, -2}; the mask
    allow[r, v] = ((v + r) % 3 != 0) or x[r, v] == 0, an empty row left empty (the kernel's empty-mask rule).  Firm draws equal the
    restatement; for T > 0 EVERY draw is bit-equal to inet_sample_truncated on the -inf-filled input; a null mask and an all-ones mask are
    bit-equal to inet_sample_truncated; one-bit rows return their token with logp == 0.0; tie rows with every second token banned compare
    exactly; rows outside the rule take the masked argmax with logp NaN; no banned token anywhere."""
    L = ops._lib.lib()
    nw = (V + 63) // 64
    near = draws = 0
    per_setting = {}

    def run(xd, ud, temp, k, p, wd, out, lpo):
        ops.check(L.inet_sample_constrained(ops.ptr(xd), xd.stride(0), xd.shape[0], V, temp, ops.ptr(ud), ud.stride(0), k, p, ops.ptr(out),
                                            out.stride(0), ops.ptr(lpo), lpo.stride(0), ops.ptr(wd), wd.stride(0) if wd is not None else 0,
                                            ops.stream_ptr()), "sc")
        return out[:, 0].cpu().numpy(), lpo[:, 0].cpu().numpy()

    def trunc(xd, ud, temp, k, p, out, lpo):
        ops.check(L.inet_sample_truncated(ops.ptr(xd), xd.stride(0), xd.shape[0], V, temp, ops.ptr(ud), ud.stride(0), k, p, ops.ptr(out),
                                          out.stride(0), ops.ptr(lpo), lpo.stride(0), ops.stream_ptr()), "st")
        return out[:, 0].cpu().numpy(), lpo[:, 0].cpu().numpy()

    def same(a, b):
        return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.int32), b[1].view(np.int32))

    for rows in TR.ALONE_ROWS:
        x, u = TR.alone_case(V, rows)
        allow = CR.alone_mask(x[:, :V])
        eff = allow | ~allow.any(-1, keepdims=True)
        free = CR.free(allow)
        xd, ud = torch.from_numpy(x).cuda(), torch.from_numpy(u).cuda()
        filled = x.copy()
        filled[:, :V][~eff] = -np.inf
        fd = torch.from_numpy(filled).cuda()
        wd = torch.full((rows, nw + 2), -1, dtype=torch.int64, device="cuda")      # (strided mask rows; the padding words are all ones)
        wd[:, :nw] = torch.from_numpy(CR.words(allow).view(np.int64)).cuda()
        ones = torch.from_numpy(CR.words(np.ones((rows, V), dtype=bool)).view(np.int64)).cuda()
        out = torch.full((rows, 3), -7, dtype=torch.int64, device="cuda")
        lpo = torch.full((rows, 2), 7.0, dtype=torch.float32, device="cuda")
        out2, lpo2 = out.clone(), lpo.clone()
        for temp in TR.ALONE_TEMPS:
            for k in TR.alone_top_k(V):
                for p in TR.ALONE_TOP_P:
                    got, lp = run(xd, ud, temp, k, p, wd, out, lpo)
                    want, wlp, n, cm, bm, d = CR.pick_rows(x[:, :V], temp, u[:, 0], k, p, allow)
                    firm = TR.firm(cm, bm) | ~free
                    assert eff[np.arange(rows), got].all(), (V, rows, temp, k, p, "a banned token")
                    assert np.array_equal(got[firm], want[firm]), (V, rows, temp, k, p)
                    ok = firm & (got == want)
                    err = np.abs(lp[ok].astype(np.float64) - wlp[ok].astype(np.float64)) / TR.logp_tol(d[ok])
                    assert not np.isnan(lp[ok]).any() and (err <= 1.0).all(), (V, rows, temp, k, p, float(err.max()))
                    assert (lp[~free] == 0.0).all(), (V, rows, temp, k, p)
                    measured["logp"] = max(measured["logp"], float(err.max())) if ok.any() else measured["logp"]
                    if temp > 0:                                # consequence 4: every draw, bit for bit
                        assert same((got, lp), trunc(fd, ud, temp, k, p, out2, lpo2)), (V, rows, temp, k, p)
                    # consequence 1: a null mask and an all-ones mask
                    base = tuple(a.copy() for a in trunc(xd, ud, temp, k, p, out2, lpo2))
                    assert same(run(xd, ud, temp, k, p, None, out2, lpo2), base) and same(run(xd, ud, temp, k, p, ones, out2, lpo2), base)
                    nf = int((~firm).sum())
                    near, draws = near + nf, draws + int(free.sum())
                    key = (temp, k, p)
                    per_setting[key] = tuple(a + b for a, b in zip(per_setting.get(key, (0, 0)), (nf, int(free.sum()))))
        assert int(out[:, 1:].min()) == -7 and float(lpo[:, 1].min()) == 7.0           # the strides were respected
        # one-bit rows: the token for every u and temperature, logp exactly 0
        one = np.zeros((rows, V), dtype=bool)
        fix = (7 * np.arange(rows) + 1) % V
        one[np.arange(rows), fix] = True
        od = torch.from_numpy(CR.words(one).view(np.int64)).cuda()
        for temp in TR.ALONE_TEMPS + (0.0,):
            for k, p in ((0, 1.0), (1, 1.0), (2, 0.5), (V + 5, 1e-9)):
                got, lp = ops.sample_truncated(xd[:, :V], temp, ud[:, 0], top_k=k, top_p=p, allowed=od)
                assert np.array_equal(got.cpu().numpy(), fix) and (lp.cpu().numpy() == 0.0).all(), (V, rows, temp, k, p)
    print("V", V, "within margin", near, "of", draws, "free draws; logp error / tolerance so far %.3f" % measured["logp"])
    assert near <= 0.01 * draws, (V, near, draws)
    assert all(n_ <= 0.03 * d_ for n_, d_ in per_setting.values()), (V, {k_: v_ for k_, v_ in per_setting.items() if v_[0] > 0.03 * v_[1]})
    # tie rows with every second token banned: exact, nothing left out
    t = TR.tie_rows(V)
    ta = np.ascontiguousarray(np.broadcast_to(np.arange(V) % 2 == 1, t.shape)) if V > 1 else np.ones_like(t, dtype=bool)
    td, tw = torch.from_numpy(t).cuda(), torch.from_numpy(CR.words(ta).view(np.int64)).cuda()
    for temp in TR.ALONE_TEMPS:
        for k in TR.alone_top_k(V):
            for p in TR.ALONE_TOP_P:
                for uv in (0.05, 0.37, 0.81):
                    u = np.full(len(t), uv)
                    got, lp = ops.sample_truncated(td, temp, torch.from_numpy(u).cuda(), top_k=k, top_p=p, allowed=tw)
                    want, wlp, n, cm, bm, d = CR.pick_rows(t, temp, u, k, p, ta)
                    assert np.array_equal(got.cpu().numpy(), want), (V, temp, k, p, uv, got, want, n)
                    assert np.allclose(lp.cpu().numpy(), wlp, rtol=0, atol=float(TR.logp_tol(d).max())), (V, temp, k, p, uv)
    # rows outside the rule take the masked argmax, logp NaN: u outside [0, 1), a NaN logit, +inf -- at allowed and at banned places
    x = np.maximum(synthetic.det_normal(f"decoder_cons/alone/edge/{V}", (7, V), 2.0), 0.0).astype(np.float32)
    u = np.array([2.0, np.nan, -0.5, 0.3, 0.3, 1.0, 0.3])
    ea = np.ascontiguousarray(np.broadcast_to(np.arange(V) % 2 == (V - 1) % 2, x.shape)) if V > 1 else np.ones_like(x, dtype=bool)
    x[3, V // 2] = np.nan
    x[4, V - 1] = np.inf
    x[6, max(V - 2, 0)] = np.nan
    ew = torch.from_numpy(CR.words(ea).view(np.int64)).cuda()
    for k, p in ((0, 1.0), (2, 0.5), (1, 1.0)):
        got, lp = ops.sample_truncated(torch.from_numpy(x).cuda(), 1.0, torch.from_numpy(u).cuda(), top_k=k, top_p=p, allowed=ew)
        assert got.cpu().numpy().tolist() == [CR.masked_argmax(r, a) for r, a in zip(x, ea)], (got, k, p)
        assert ea[np.arange(7), got.cpu().numpy()].all() and np.isnan(lp.cpu().numpy()).all()
    for bad in (0.0, 1.5, float("nan")):
        with pytest.raises(ValueError):
            ops.sample_truncated(torch.zeros(2, 8, device="cuda"), 1.0, torch.zeros(2, dtype=torch.float64, device="cuda"), top_p=bad,
                                 allowed=torch.ones(2, 1, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError):
        ops.sample_truncated(torch.zeros(2, 65, device="cuda"), 1.0, torch.zeros(2, dtype=torch.float64, device="cuda"),
                             allowed=torch.ones(2, 1, dtype=torch.int64, device="cuda"))


@pytest.mark.parametrize("Z", TR.PLAN_Z)
@pytest.mark.parametrize("V", TR.PLAN_V)
def test_every_plan_of_a_constrained_call(V, Z):
    """B in {1, 2, 4, 5, 7, 16} x decoder_trunc_ref.SETTINGS per (V, Z) with plan_inputs' z and uniforms and the mask
    allow[r, t, v] = (v == (7 r + 3 t + 1) % V) where (r + t) % 4 == 0, else ((v + t + r) % 5 != 0): the merged build, workgroup C, the
    one-row and two-row teams, the shared recurrent groups and a last team with a repeated row.  Every launch label starts with
    cons_decode_b1; logits within 2e-5 of the float64 oracle fed the kernel's tokens; firm tokens and logp equal to the restatement; every
    fixed tick returns its token with logp exactly 0.0; no banned token; the caps (counted on the CPU by
    tests/test_decoder_constraint_host.py::test_margin_counts_of_the_every_plan_test)."""
    cfg, P, params = decoder(V, Z)
    P64 = {k: v.double() for k, v in P.items()}
    near = draws = 0
    for si, (temp, k, p) in enumerate(TR.SETTINGS):
        near_s = draws_s = 0
        for B in TR.PLAN_B:
            zn, u = TR.plan_inputs(V, Z, B, si)
            allow = CR.plan_mask(V, B)
            z = torch.from_numpy(zn).cuda()
            w, tok, lp, labels = constrained(cfg, z, params, temp, u, k, p, allow)
            folded = Z == 256 and B <= 6
            want = f"cons_decode_b1_beats T24 B{B} " if folded else f"cons_decode_b1 T24 B{B} "
            assert any(l.startswith(want) for l in labels), (V, Z, B, sorted(set(labels)))
            assert not any(l.startswith(("sample_", "trunc_", "decode_b1", "decode_chain")) for l in labels), sorted(set(labels))
            assert all(l.startswith("cons_decode_b1") for l in labels if "decode_b1" in l)
            assert tok.min() >= 0 and tok.max() < V
            wr = R.oracle_logits(P64, z.cpu(), tok)
            err = G.rel_err(w.cpu(), wr)
            assert err < TOL, (V, Z, B, temp, k, p, err)
            n, d = check_rule(w, tok, lp, temp, u, k, p, allow, (V, Z, B, temp, k, p))
            near_s, draws_s = near_s + n, draws_s + d
        assert near_s <= 0.03 * draws_s, (V, Z, temp, k, p, near_s, draws_s)
        near, draws = near + near_s, draws + draws_s
    assert near <= 0.01 * draws, (V, Z, near, draws)


@pytest.mark.parametrize("B", [1, 4, 16])
def test_two_equalities_without_a_margin(B):
    """V = 48.  The all-ones mask is the truncated call: tokens, logits and logp bit for bit.  The constrained argmax (no temperature, at
    the HierarchicalDecoder level) is the restatement with top_k = 1 on the returned weights, exactly, and leaves no logp."""
    from tests.test_gpu_decoder_trunc import truncated
    V, Z = 48, 256
    cfg, P, params = decoder(V, Z)
    z = torch.from_numpy(synthetic.det_normal(f"decoder_cons/z/equal/{B}", (B, Z))).cuda()
    u = synthetic.det_uniform(f"decoder_cons/u/equal/{B}", (B, 24), 0.0, 1.0).astype(np.float64)
    for temp, k, p in ((6.0, 8, 0.7), (1.5, 0, 1.0)):
        w0, tok0, lp0, labels0 = truncated(cfg, z, params, temp, u, k, p)
        assert any(l.startswith("trunc_decode_b1") for l in labels0)
        w1, tok1, lp1, labels = constrained(cfg, z, params, temp, u, k, p, np.ones((B, 24, V), dtype=bool))
        assert any(l.startswith("cons_decode_b1") for l in labels), sorted(set(labels))
        assert np.array_equal(tok1, tok0) and torch.equal(w1, w0) and np.array_equal(lp1.view(np.int32), lp0.view(np.int32))
    # the constrained argmax through the public decoder class
    from inpaintnet_amd.measure_vae import MeasureVAE
    c = G.CFGS["full"]
    ds = synthetic.SyntheticFolkDataset(num_notes=V)
    vae = MeasureVAE(ds, note_embedding_dim=c["E"], encoder_hidden_size=c["H"], latent_space_dim=Z, decoder_hidden_size=c["H"],
                     encoder_dropout_prob=0.0, decoder_dropout_prob=0.0)
    vae.load_state_dict({k: torch.from_numpy(synthetic.det_param(k, tuple(v.shape))) for k, v in vae.state_dict().items()})
    vae.eval()
    allow = CR.plan_mask(V, B)
    with torch.no_grad():
        (w, s), labels = labels_of(lambda: vae.decode(z, allowed=torch.from_numpy(allow)))
    assert ops.chain_status() == 0
    assert any(l.startswith("cons_decode_b1") for l in labels), sorted(set(labels))
    assert vae.decoder.last_logp is None
    tok = s.cpu().numpy()[:, 0]
    want = CR.pick_rows(w.cpu().numpy(), 1.0, np.zeros((B, 24)), 1, 1.0, allow)[0]
    assert np.array_equal(tok, want)
    wn = w.cpu().numpy()
    assert np.array_equal(tok, np.where(allow, wn, -np.inf).argmax(-1))            # the argmax over the allowed tokens
    with pytest.raises(ValueError):
        empty = allow.copy()
        empty[0, 3] = False
        vae.decode(z, allowed=torch.from_numpy(empty))
    with pytest.raises(ValueError):
        vae.decode(z, allowed=torch.from_numpy(allow[:, :23]))


def test_the_tick_by_tick_path_of_the_other_shapes():
    """Seventeen rows (V = 48, H = 512): 24 cons_sample launches behind the output projections, nothing register-resident; a tick mask on
    four rows takes the same path.  The same checks as the plans' test."""
    V, Z = 48, 256
    cfg, P, params = decoder(V, Z)
    P64 = {k: v.double() for k, v in P.items()}
    temp, k, p = 6.0, 8, 0.7
    near = draws = 0
    for B, masked in ((17, False), (4, True)):
        z = torch.from_numpy(synthetic.det_normal(f"decoder_trunc/z/fallback/{B}", (B, Z))).cuda()
        u = synthetic.det_uniform(f"decoder_trunc/u/fallback/{B}", (B, 24), 0.0, 1.0).astype(np.float64)
        allow = CR.plan_mask(V, B)
        mt = ops.dropout_mask((24, B, 512), 0.5, 78, 0, "cuda") if masked else None
        w, tok, lp, labels = constrained(cfg, z, params, temp, u, k, p, allow, mask_tick=mt)
        assert sum(l.startswith("cons_sample ") for l in labels) == 24, sorted(set(labels))
        assert not any("decode_b1" in l or l.startswith(("decode_chain", "sample_", "trunc_")) for l in labels), sorted(set(labels))
        wr = R.oracle_logits(P64, z.cpu(), tok, {"tick": mt.permute(1, 0, 2).double().cpu()} if masked else None)
        assert G.rel_err(w.cpu(), wr) < TOL
        n, d = check_rule(w, tok, lp, temp, u, k, p, allow, ("tick by tick", B, masked))
        near, draws = near + n, draws + d
    assert near <= 0.01 * draws, (near, draws)                # (one setting: the function's cap is the tighter one)


@pytest.mark.parametrize("V,Z,B", [(20, 256, 2), (48, 256, 1), (100, 128, 16)])
def test_fallback_ticks_keep_the_constraints(V, Z, B):
    """Uniforms outside [0, 1) on every other tick: logp is NaN exactly there, the tokens there are the masked argmax of the returned
    weights, the fixed ticks still hold -- inside the masked launch (the merged build, the one-row build, workgroup C with two chunks per
    lane)."""
    cfg, P, params = decoder(V, Z)
    z = torch.from_numpy(synthetic.det_normal(f"decoder_cons/z/edges/{V}/{Z}/{B}", (B, Z))).cuda()
    u = synthetic.det_uniform(f"decoder_cons/u/edges/{V}/{Z}/{B}", (B, 24), 0.0, 1.0).astype(np.float64)
    u[:, 1::4] = 2.0
    u[:, 3::4] = np.nan
    u[:, 0::8] = -0.5                                           # (ticks 0, 8, 16: fixed ticks of row 0 among them)
    allow = CR.plan_mask(V, B)
    w, tok, lp, labels = constrained(cfg, z, params, 6.0, u, 8, 0.7, allow)
    assert any(l.startswith("cons_decode_b1") for l in labels)
    out = ~((u >= 0.0) & (u < 1.0))
    assert np.isnan(lp[out]).all() and not np.isnan(lp[~out]).any()
    wn = w.cpu().numpy()
    assert np.array_equal(tok[out], np.where(allow, wn, -np.inf).argmax(-1)[out])
    fixed = ~CR.free(allow)
    assert (fixed & out).any() and np.array_equal(tok[fixed], np.argmax(allow, -1)[fixed])
    n, d = check_rule(w, tok, lp, 6.0, u, 8, 0.7, allow, ("edges", V, Z, B))
    assert n <= 0.01 * d, (V, Z, B, n, d)                     # (one setting: the function's cap is the tighter one)


@pytest.mark.parametrize("auto_reg", [False, True])
def test_generate_honours_bans_and_fixed_notes(auto_reg, monkeypatch):
    """LatentRNNTester.generate(temperature=6, top_p=0.9, num_variations=4, banned_tokens=, fixed_tokens=): the fixed ticks hold in every
    variation and measure, the banned tokens are absent, last_logp (4, 3) = the per-measure sums of the per-tick logp; without a
    temperature one filling that honours both and no last_logp; the argument errors."""
    fx = G.load("inference_small")
    tag = "gen_ar" if auto_reg else "gen_nar"
    c, ds, vae, model = small_model(auto_reg)
    V = c["V"]
    tester = LatentRNNTester(ds, model)
    score = torch.from_numpy(fx[f"{tag}_score"])
    past, future, target = LatentRNNTrainer.split_score(score, 5, 8, 3, 24)
    eps4 = torch.cat((torch.from_numpy(fx[f"{tag}_eps_past"]), torch.from_numpy(fx[f"{tag}_eps_future"])), 0).cuda()

    def run(nvar=4, **kw):
        queue = [eps4.view(1, 13, -1).expand(nvar, -1, -1).reshape(nvar * 13, -1)]
        if auto_reg:
            queue += [torch.from_numpy(fx[f"{tag}_eps_ar{i}"]).cuda().repeat(nvar, 1) for i in range(3)]
        monkeypatch.setattr(torch, "randn_like", lambda t: queue.pop(0))
        try:
            return tester.generate(past, future, None, 3, num_variations=nvar, **kw)[1]
        finally:
            monkeypatch.undo()

    # what the unconstrained call draws: ban its two most frequent tokens, fix ticks to tokens it did not draw there
    np.random.seed(21)
    plain = run(temperature=6.0, top_p=0.9)[:, 5:8].cpu().numpy()
    banned = [int(t) for t in np.argsort(-np.bincount(plain.reshape(-1), minlength=V))[:2]]
    fixed = torch.full((3, 24), -1, dtype=torch.int64)
    for m, t in ((0, 0), (0, 5), (1, 11), (2, 23), (2, 6)):
        fixed[m, t] = (int(plain[0, m, t]) + 1 + t) % V
    fixed[1, 2] = banned[0]                                     # a fixed tick wins over a ban
    keep = (fixed >= 0).numpy()
    np.random.seed(21)
    full = run(temperature=6.0, top_p=0.9, banned_tokens=banned, fixed_tokens=fixed)
    lp = tester.last_logp.clone()
    mlp = model.last_logp.clone()
    got = full[:, 5:8].cpu().numpy()
    assert full.shape == (4, 16, 24) and tuple(lp.shape) == (4, 3) and lp.dtype == torch.float32
    assert tuple(mlp.shape) == (4, 3, 24) and torch.equal(mlp.sum(-1), lp) and bool(torch.isfinite(lp).all())
    assert (got[:, keep] == fixed.numpy()[keep]).all()
    assert not np.isin(got[:, ~keep], banned).any()
    assert (mlp.cpu().numpy()[:, keep] == 0.0).all()
    assert torch.equal(full[:, :5], past.expand(4, -1, -1).to(full.device)) and not np.array_equal(got, plain)
    np.random.seed(21)
    assert torch.equal(run(temperature=6.0, top_p=0.9, banned_tokens=banned, fixed_tokens=fixed), full)
    # without a temperature: one filling, both constraints, no score
    one = run(nvar=1, banned_tokens=banned, fixed_tokens=fixed)
    g1 = one[:, 5:8].cpu().numpy()
    assert one.shape == (1, 16, 24) and tester.last_logp is None
    assert (g1[:, keep] == fixed.numpy()[keep]).all() and not np.isin(g1[:, ~keep], banned).any()
    w = tester.last_weights.cpu().numpy().reshape(1, 3, 24, V)
    allow = np.ones((3, 24, V), dtype=bool)
    allow[:, :, banned] = False
    allow[keep] = np.arange(V) == fixed.numpy()[keep][:, None]
    assert np.array_equal(g1[0], np.where(allow, w[0], -np.inf).argmax(-1))        # the argmax over the allowed tokens
    for bad in (dict(banned_tokens=[V]), dict(banned_tokens=[-1]), dict(banned_tokens=list(range(V))),
                dict(fixed_tokens=torch.full((3, 24), V)), dict(fixed_tokens=torch.full((3, 24), -2)),
                dict(fixed_tokens=torch.full((2, 24), -1)), dict(fixed_tokens=torch.zeros(3, 24))):
        for kw in (dict(temperature=6.0, top_p=0.9), dict(nvar=1)):
            with pytest.raises(ValueError):
                run(**kw, **bad)
    with pytest.raises(ValueError):
        model(past, future, None, 3, train=False, allowed=torch.zeros(1, 3, 24, V, dtype=torch.bool))
    with pytest.raises(ValueError):
        model(past, future, target, 3, train=True, allowed=torch.ones(1, 3, 24, V, dtype=torch.bool))
    assert ops.chain_status() == 0
