"""The decoder's forced tokens on the GPU: inet_sample_forced's kernel alone, the forced build of the register-resident launch in every
plan a forced call can get (csrc/decode_b1.hip), the replay and no-forced-tick equalities, the anchor at the reference's teacher-forced
logits, the tick-by-tick path of every other shape, fallback ticks, and the public surface down from LatentRNNTester.score and
generate(score_fixed=True).

The reference for the rule is its float64 restatement (tests/decoder_forced_ref.py) APPLIED TO THE f32 LOGITS THE CALL RETURNED, as in
tests/test_gpu_decoder_constraint.py.  A free draw is left out of a comparison only when one of its two margins is below 2e-5, a forced
tick only when its nucleus margin is; at most 3 % of a setting's free draws, 3 % of its forced ticks and 1 % of a test function's draws
may be -- the counts for these masks, patterns and seeds are made on the CPU by tests/test_decoder_forced_host.py, which holds them to
the same caps.  Every forced tick returns its token, nothing left out."""
import numpy as np
import pytest
import torch

from tests import decoder_constraint_ref as CR
from tests import decoder_forced_ref as FR
from tests import decoder_sample_ref as R
from tests import decoder_trunc_ref as TR
from tests import golden_util as G

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from inpaintnet_amd import ops, synthetic
    from inpaintnet_amd.latent_rnn_tester import LatentRNNTester
    from inpaintnet_amd.latent_rnn_trainer import LatentRNNTrainer
    from tests.test_gpu_decode_plans import decoder, labels_of
    from tests.test_gpu_decoder_constraint import constrained
    from tests.test_gpu_decoder_sample import small_model

TOL = 2e-5
measured = {"logp": 0.0, "logits": 0.0}    # the largest logp error in units of its tolerance and logits error, printed by the checks


def forced_call(cfg, z, params, temp, u, top_k, top_p, allow, forced, mask_tick=None):
    """One forced call at the ops level (allow bool [B,T,V] or None, forced int [B,T] or None) -> (weights, tokens, logp, labels)"""
    B = z.shape[0]
    ud = torch.from_numpy(np.ascontiguousarray(u)).cuda()
    words = None if allow is None else ops.pack_allowed(torch.from_numpy(np.ascontiguousarray(allow))).cuda().contiguous()
    fd = None if forced is None else torch.from_numpy(np.ascontiguousarray(forced).astype(np.int32)).cuda()
    lp = torch.full((B, 24), 7.0, dtype=torch.float32, device="cuda")
    (w, s_, _), labels = labels_of(lambda: ops.decoder_fwd(cfg, z, None, False, params, mask_tick=mask_tick, temperature=temp,
                                                           uniforms=ud, top_k=top_k, top_p=top_p, logp=lp, allowed=words, forced=fd))
    status = ops.chain_status()
    assert status == 0, (tuple(z.shape), temp, top_k, top_p, status, ops.slow_waits_summary())
    return w.clone(), s_.cpu().numpy()[:, 0].copy(), lp.cpu().numpy(), labels


def check_rule(w, tok, lp, temp, u, top_k, top_p, allow, forced, what):
    """Tokens and logp against the restatement on the returned weights -> (free draws within a margin, free draws, forced ticks within
    the nucleus margin, forced ticks).  Free ticks as test_gpu_decoder_constraint.check_rule."""
    wn = w.cpu().numpy()
    V = wn.shape[-1]
    if allow is None:
        allow = np.ones(wn.shape, dtype=bool)
    want, wlp, n, cm, bm, d = FR.pick_rows(wn, temp, u, top_k, top_p, allow, forced)
    isf = (forced >= 0) & (forced < V)
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
    assert (lp[fixed & ~np.isnan(wlp)] == 0.0).all(), (what, "a fixed free tick's logp is exactly 0")
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


@pytest.mark.parametrize("V", TR.ALONE_V)
def test_the_forced_kernel_alone(V):
    """inet_sample_forced: decoder_trunc_ref's rows, temperatures, top_k and top_p, strided rows, uniforms, outputs, logp, mask and
    forced words; forced = (3 r + 1) % V on every second row, with decoder_constraint_ref.alone_mask and without a mask.  A forced row
    returns its token, its logp against the restatement (-inf and NaN exactly); a free row is inet_sample_constrained's row bit for bit;
    a null forced and one of -1, V and -2 are inet_sample_constrained bit for bit; NaN uniforms change nothing on forced rows; tie rows
    compare exactly."""
    L = ops._lib.lib()
    nw = (V + 63) // 64
    near = ticks = 0
    per_setting = {}

    def run(xd, ud, temp, k, p, wd, fd, out, lpo):
        ops.check(L.inet_sample_forced(ops.ptr(xd), xd.stride(0), xd.shape[0], V, temp, ops.ptr(ud), ud.stride(0), k, p, ops.ptr(out),
                                       out.stride(0), ops.ptr(lpo), lpo.stride(0), ops.ptr(wd), wd.stride(0) if wd is not None else 0,
                                       ops.ptr(fd), fd.stride(0) if fd is not None else 0, ops.stream_ptr()), "sf")
        return out[:, 0].cpu().numpy(), lpo[:, 0].cpu().numpy()

    def cons(xd, ud, temp, k, p, wd, out, lpo):
        ops.check(L.inet_sample_constrained(ops.ptr(xd), xd.stride(0), xd.shape[0], V, temp, ops.ptr(ud), ud.stride(0), k, p, ops.ptr(out),
                                            out.stride(0), ops.ptr(lpo), lpo.stride(0), ops.ptr(wd), wd.stride(0) if wd is not None else 0,
                                            ops.stream_ptr()), "sc")
        return out[:, 0].cpu().numpy(), lpo[:, 0].cpu().numpy()

    def same(a, b, rows=slice(None)):
        return np.array_equal(a[0][rows], b[0][rows]) and np.array_equal(a[1][rows].view(np.int32), b[1][rows].view(np.int32))

    for rows in TR.ALONE_ROWS:
        x, u = TR.alone_case(V, rows)
        f = FR.alone_forced(rows, V)
        isf = f >= 0
        xd, ud = torch.from_numpy(x).cuda(), torch.from_numpy(u).cuda()
        und = torch.from_numpy(np.where(isf[:, None], np.nan, u)).cuda()          # NaN uniforms on the forced rows
        fd = torch.full((rows, 3), 5, dtype=torch.int32, device="cuda")            # (strided forced words)
        fd[:, 0] = torch.from_numpy(f).cuda()
        out = torch.full((rows, 3), -7, dtype=torch.int64, device="cuda")
        lpo = torch.full((rows, 2), 7.0, dtype=torch.float32, device="cuda")
        out2, lpo2 = out.clone(), lpo.clone()
        for allow in (CR.alone_mask(x[:, :V]), None):
            wd = None
            if allow is not None:
                wd = torch.full((rows, nw + 2), -1, dtype=torch.int64, device="cuda")
                wd[:, :nw] = torch.from_numpy(CR.words(allow).view(np.int64)).cuda()
            for temp in TR.ALONE_TEMPS:
                for k in TR.alone_top_k(V):
                    for p in TR.ALONE_TOP_P:
                        got, lp = (a.copy() for a in run(xd, ud, temp, k, p, wd, fd, out, lpo))
                        base = tuple(a.copy() for a in cons(xd, ud, temp, k, p, wd, out2, lpo2))
                        assert same((got, lp), base, ~isf), (V, rows, temp, k, p, "a free row")
                        assert np.array_equal(got[isf], f[isf]), (V, rows, temp, k, p)
                        want, wlp, n, cm, bm, d = FR.pick_rows(x[isf, :V], temp, u[isf, 0], k, p, None if allow is None else allow[isf], f[isf])
                        firm = bm >= TR.MARGIN
                        flp = lp[isf]
                        assert np.array_equal(np.isnan(flp), np.isnan(wlp)), (V, rows, temp, k, p)
                        assert np.array_equal(np.isneginf(flp)[firm], np.isneginf(wlp)[firm]) and not np.isposinf(flp).any(), (V, rows, temp, k, p)
                        ok = firm & np.isfinite(wlp) & np.isfinite(flp)
                        if ok.any():
                            err = np.abs(flp[ok].astype(np.float64) - wlp[ok].astype(np.float64)) / TR.logp_tol(d[ok])
                            assert (err <= 1.0).all(), (V, rows, temp, k, p, float(err.max()))
                            measured["logp"] = max(measured["logp"], float(err.max()))
                        assert same(run(xd, und, temp, k, p, wd, fd, out2, lpo2), (got, lp), isf), (V, rows, temp, k, p, "NaN uniforms")
                        nf = int((~firm).sum())
                        near, ticks = near + nf, ticks + int(isf.sum())
                        key = (allow is None, temp, k, p)
                        per_setting[key] = tuple(a + b for a, b in zip(per_setting.get(key, (0, 0)), (nf, int(isf.sum()))))
            # no forced row: inet_sample_constrained bit for bit
            for fv in (None, -1, V, -2):
                fn = None if fv is None else torch.full((rows,), fv, dtype=torch.int32, device="cuda")
                for temp, k, p in ((1.0, 0, 1.0), (6.0, 2, 0.5)):
                    base = tuple(a.copy() for a in cons(xd, ud, temp, k, p, wd, out2, lpo2))
                    assert same(run(xd, ud, temp, k, p, wd, fn, out2, lpo2), base), (V, rows, fv)
        assert int(out[:, 1:].min()) == -7 and float(lpo[:, 1].min()) == 7.0           # the strides were respected
    print("V", V, "within the nucleus margin", near, "of", ticks, "forced rows; logp error / tolerance so far %.3f" % measured["logp"])
    assert near <= 0.01 * ticks, (V, near, ticks)
    assert all(n_ <= 0.03 * d_ for n_, d_ in per_setting.values()), (V, {k_: v_ for k_, v_ in per_setting.items() if v_[0] > 0.03 * v_[1]})
    # tie rows, every second token banned, every row forced (row r to token r, r + 1, ... in turn): exact, nothing left out
    t = TR.tie_rows(V)
    ta = np.ascontiguousarray(np.broadcast_to(np.arange(V) % 2 == 1, t.shape)) if V > 1 else np.ones_like(t, dtype=bool)
    td, tw = torch.from_numpy(t).cuda(), torch.from_numpy(CR.words(ta).view(np.int64)).cuda()
    for temp in TR.ALONE_TEMPS:
        for k in TR.alone_top_k(V):
            for p in TR.ALONE_TOP_P:
                for shift in (0, 1, 63, 64):
                    f = ((np.arange(len(t)) + shift) % V).astype(np.int32)
                    u = np.full(len(t), np.nan)
                    got, lp = ops.sample_truncated(td, temp, torch.from_numpy(u).cuda(), top_k=k, top_p=p, allowed=tw,
                                                   forced=torch.from_numpy(f).cuda())
                    want, wlp, n, cm, bm, d = FR.pick_rows(t, temp, u, k, p, ta, f)
                    lp = lp.cpu().numpy()
                    assert np.array_equal(got.cpu().numpy(), f), (V, temp, k, p, shift)
                    assert np.array_equal(np.isneginf(lp), np.isneginf(wlp)) and not np.isnan(lp).any(), (V, temp, k, p, shift, lp, wlp)
                    fin = np.isfinite(wlp)
                    assert np.allclose(lp[fin], wlp[fin], rtol=0, atol=float(TR.logp_tol(d).max())), (V, temp, k, p, shift)
    with pytest.raises(ValueError):
        ops.sample_truncated(torch.zeros(2, 8, device="cuda"), 1.0, torch.zeros(2, dtype=torch.float64, device="cuda"),
                             forced=torch.zeros(2, dtype=torch.int64, device="cuda"))
    assert ops.chain_status() == 0


@pytest.mark.parametrize("Z", (256, 128))
@pytest.mark.parametrize("V", (20, 48, 100))
def test_every_plan_of_a_forced_call(V, Z):
    """B in {1, 2, 4, 5, 7, 16} x decoder_forced_ref.FORCED_SETTINGS per (V, Z) with plan_inputs' z and uniforms, plan_mask and
    plan_forced.  Every launch label starts with force_decode_b1; logits within 2e-5 of the float64 oracle fed the returned tokens; every
    forced tick returns f; free ticks as in the constrained test; a forced tick's logp is -inf and NaN exactly where the restatement's
    is, else within decoder_trunc_ref.logp_tol; the caps (counted on the CPU by
    tests/test_decoder_forced_host.py::test_margin_counts_of_the_every_plan_test)."""
    cfg, P, params = decoder(V, Z)
    P64 = {k: v.double() for k, v in P.items()}
    near = draws = 0
    for si, (temp, k, p) in enumerate(FR.FORCED_SETTINGS):
        cnt = np.zeros(4, dtype=np.int64)
        for B in TR.PLAN_B:
            zn, u = TR.plan_inputs(V, Z, B, si)
            allow, forced = CR.plan_mask(V, B), FR.plan_forced(V, B)
            z = torch.from_numpy(zn).cuda()
            w, tok, lp, labels = forced_call(cfg, z, params, temp, u, k, p, allow, forced)
            folded = Z == 256 and B <= 6
            want = f"force_decode_b1_beats T24 B{B} " if folded else f"force_decode_b1 T24 B{B} "
            assert any(l.startswith(want) for l in labels), (V, Z, B, sorted(set(labels)))
            assert not any(l.startswith(("sample_", "trunc_", "cons_", "decode_b1", "decode_chain")) for l in labels), sorted(set(labels))
            assert all(l.startswith("force_decode_b1") for l in labels if "decode_b1" in l)
            assert tok.min() >= 0 and tok.max() < V
            wr = R.oracle_logits(P64, z.cpu(), tok)
            err = G.rel_err(w.cpu(), wr)
            measured["logits"] = max(measured["logits"], err)
            assert err < TOL, (V, Z, B, temp, k, p, err)
            cnt += check_rule(w, tok, lp, temp, u, k, p, allow, forced, (V, Z, B, temp, k, p))
        print(f"V {V} Z {Z} setting {(temp, k, p)}: left out {cnt[0]} of {cnt[1]} free draws, {cnt[2]} of {cnt[3]} forced ticks; "
              f"logits error so far {measured['logits']:.3g}")
        assert cnt[0] <= 0.03 * cnt[1] and cnt[2] <= 0.03 * cnt[3], (V, Z, temp, k, p, cnt)
        near, draws = near + cnt[0] + cnt[2], draws + cnt[1] + cnt[3]
    assert draws == 2100 and near <= 0.01 * draws, (V, Z, near, draws)


@pytest.mark.parametrize("B", TR.PLAN_B)
def test_replay_returns_the_call_bit_for_bit(B):
    """Consequence (b), V = 48: force at every tick what a truncated call (no mask) and a constrained call (plan_mask) returned -- same
    temperature, top_k, top_p and mask, other uniforms and NaN uniforms: torch.equal on the weights, the tokens, bitwise equality on logp.
    B = 7 is a call behind the beat path's own launches whose four-beat products have 28 rows: a sampled call keeps one k range per tile
    in them (GemmArgs.one_range), or two identical calls would differ in the last bits of their logits.  DESIGN.md section 15."""
    from tests.test_gpu_decoder_trunc import truncated
    V, Z = 48, 256
    cfg, P, params = decoder(V, Z)
    z = torch.from_numpy(synthetic.det_normal(f"decoder_forced/z/replay/{B}", (B, Z))).cuda()
    u = synthetic.det_uniform(f"decoder_forced/u/replay/{B}", (B, 24), 0.0, 1.0).astype(np.float64)
    u2 = synthetic.det_uniform(f"decoder_forced/u/replay/other/{B}", (B, 24), 0.0, 1.0).astype(np.float64)
    for temp, k, p in ((6.0, 8, 0.7), (1.5, 0, 1.0)):
        for allow in (None, CR.plan_mask(V, B)):
            if allow is None:
                w0, tok0, lp0, _ = truncated(cfg, z, params, temp, u, k, p)
            else:
                w0, tok0, lp0, _ = constrained(cfg, z, params, temp, u, k, p, allow)
            assert not np.isnan(lp0).any()
            for other in (u2, np.full((B, 24), np.nan)):
                w1, tok1, lp1, labels = forced_call(cfg, z, params, temp, other, k, p, allow, tok0)
                assert any(l.startswith("force_decode_b1") for l in labels), sorted(set(labels))
                assert np.array_equal(tok1, tok0) and torch.equal(w1, w0), (B, temp, k, p, allow is None)
                assert np.array_equal(lp1.view(np.int32), lp0.view(np.int32)), (B, temp, k, p, allow is None)


@pytest.mark.parametrize("Z", (256, 128))
def test_a_sampled_call_reproduces_itself(Z):
    """What the replay rests on, V = 48, B = 3, 5, 7, 9, 12, 15 (and 8, 16): two identical truncated calls return the same logits bit for
    bit, also where the beat path runs as launches of its own in front of the decode launch and its products have 4 B rows -- 9 to 63 rows
    other than 32, which the f32 GEMM planner splits over K with f32 atomics unless the call asks for one k range per tile, as a sampled
    call does.  The argmax call of such a size keeps the planner's choice and its latency."""
    from tests.test_gpu_decoder_trunc import truncated
    V = 48
    cfg, P, params = decoder(V, Z)
    for B in (3, 5, 7, 8, 9, 12, 15, 16):
        z = torch.from_numpy(synthetic.det_normal(f"decoder_forced/z/twice/{B}", (B, Z))).cuda()
        u = synthetic.det_uniform(f"decoder_forced/u/twice/{B}", (B, 24), 0.0, 1.0).astype(np.float64)
        w0, tok0, lp0, labels = truncated(cfg, z, params, 6.0, u, 8, 0.7)
        assert any(l.startswith("trunc_decode_b1") for l in labels), sorted(set(labels))
        assert not any(" s2 " in l or " s3 " in l or " s4 " in l or " s6 " in l or " s8 " in l for l in labels), sorted(set(labels))
        for _ in range(2):
            w1, tok1, lp1, _ = truncated(cfg, z, params, 6.0, u, 8, 0.7)
            assert np.array_equal(tok1, tok0) and torch.equal(w1, w0) and np.array_equal(lp1.view(np.int32), lp0.view(np.int32)), (Z, B)


@pytest.mark.parametrize("B", [1, 4, 16])
def test_no_forced_tick_is_the_constrained_call(B):
    """Consequence (a), V = 48: a null forced and one of all -1 against inet_vae_decoder_sample_cx -- tokens, logits and logp bit for bit;
    the all -1 call runs the forced build, the null one the masked build."""
    V, Z = 48, 256
    cfg, P, params = decoder(V, Z)
    z = torch.from_numpy(synthetic.det_normal(f"decoder_forced/z/none/{B}", (B, Z))).cuda()
    u = synthetic.det_uniform(f"decoder_forced/u/none/{B}", (B, 24), 0.0, 1.0).astype(np.float64)
    u[:, 5] = 2.0                                                  # (a fallback tick in every row)
    allow = CR.plan_mask(V, B)
    for temp, k, p in ((6.0, 8, 0.7), (1.5, 0, 1.0)):
        w0, tok0, lp0, _ = constrained(cfg, z, params, temp, u, k, p, allow)
        for forced, prefix in ((None, "cons_decode_b1"), (np.full((B, 24), -1), "force_decode_b1")):
            w1, tok1, lp1, labels = forced_call(cfg, z, params, temp, u, k, p, allow, forced)
            assert any(l.startswith(prefix) for l in labels), sorted(set(labels))
            assert np.array_equal(tok1, tok0) and torch.equal(w1, w0) and np.array_equal(lp1.view(np.int32), lp0.view(np.int32))
        # C level: a forced value >= V or < -1 is a free tick
        odd = np.where(np.arange(24)[None, :] % 2 == 0, V + np.arange(B)[:, None], -2 - np.arange(B)[:, None])
        w1, tok1, lp1, _ = forced_call(cfg, z, params, temp, u, k, p, allow, odd)
        assert np.array_equal(tok1, tok0) and torch.equal(w1, w0) and np.array_equal(lp1.view(np.int32), lp0.view(np.int32))


def test_forcing_the_fixture_tokens_is_the_reference_teacher_forced_pass():
    """vae_full.npz (B = 5, V = 48, register-resident), forced = tokens, T = 1, no truncation, no mask: the weights within the 1e-4
    relative tolerance tests/test_gpu_kernels.py holds dec_tf_weights to; logp against float64 log_softmax(dec_tf_weights)[tokens] within
    twice that weight tolerance times max|dec_tf_weights| (a logit error eps moves a log-softmax entry by at most 2 eps).
    Measured on the MI355X: see DESIGN.md section 15."""
    from tests.test_gpu_kernels import pack
    fx = G.load("vae_full")
    c = G.CFGS["full"]
    cfg = ops.vae_config(c["V"], c["E"], c["H"], c["Z"], c["H"])
    table, total = ops.vae_param_table(cfg)
    params = pack(table, total, G.vae_params("full", fx))
    tok = fx["tokens"]
    z = torch.from_numpy(fx["dec_z"]).cuda()
    w, got, lp, labels = forced_call(cfg, z, params, 1.0, np.full(tok.shape, np.nan), None, None, None, tok)
    assert any(l.startswith("force_decode_b1") for l in labels), sorted(set(labels))
    assert np.array_equal(got, tok)
    tf = fx["dec_tf_weights"].astype(np.float64)
    werr = G.rel_err(w.cpu(), tf)
    ls = tf - tf.max(-1, keepdims=True)
    ls = ls - np.log(np.exp(ls).sum(-1, keepdims=True))
    want = np.take_along_axis(ls, tok[..., None], -1)[..., 0]
    bound = 2.0 * 1e-4 * np.abs(tf).max()
    err = float(np.abs(lp.astype(np.float64) - want).max())
    print("weights error %.3g (tolerance 1e-4), logp error %.3g (bound %.3g), cross-entropy %.7f against the reference's %.7f"
          % (werr, err, bound, -lp.astype(np.float64).mean(), -want.mean()))
    assert werr < 1e-4
    assert np.isfinite(lp).all() and err <= bound, (err, bound)


def test_the_tick_by_tick_path_of_the_other_shapes():
    """Seventeen rows, a tick mask on four rows (V = 48), and V = 129: 24 force_sample launches behind the output projections, nothing
    register-resident and no cons_ or trunc_ label.  The same checks as the plans' test, with and without a mask."""
    temp, k, p = 6.0, 8, 0.7
    cnt = np.zeros(4, dtype=np.int64)
    for V, B, masked, with_mask in ((48, 17, False, True), (48, 4, True, True), (129, 3, False, True), (48, 17, False, False)):
        cfg, P, params = decoder(V, 256)
        P64 = {k_: v.double() for k_, v in P.items()}
        z = torch.from_numpy(synthetic.det_normal(f"decoder_trunc/z/fallback/{B}", (B, 256))).cuda()
        u = synthetic.det_uniform(f"decoder_trunc/u/fallback/{B}", (B, 24), 0.0, 1.0).astype(np.float64)
        allow = CR.plan_mask(V, B) if with_mask else None
        forced = FR.plan_forced(V, B)
        mt = ops.dropout_mask((24, B, 512), 0.5, 78, 0, "cuda") if masked else None
        w, tok, lp, labels = forced_call(cfg, z, params, temp, u, k, p, allow, forced, mask_tick=mt)
        assert sum(l.startswith("force_sample ") for l in labels) == 24, sorted(set(labels))
        assert not any("decode_b1" in l or l.startswith(("decode_chain", "sample_", "trunc_", "cons_")) for l in labels), sorted(set(labels))
        wr = R.oracle_logits(P64, z.cpu(), tok, {"tick": mt.permute(1, 0, 2).double().cpu()} if masked else None)
        assert G.rel_err(w.cpu(), wr) < TOL
        cnt += check_rule(w, tok, lp, temp, u, k, p, allow, forced, ("tick by tick", V, B, masked, with_mask))
    assert cnt[0] + cnt[2] <= 0.01 * (cnt[1] + cnt[3]), cnt     # (one setting: the function's cap is the tighter one)


@pytest.mark.parametrize("V,Z,B", [(20, 256, 2), (48, 256, 1), (100, 128, 16)])
def test_fallback_ticks_keep_the_forced_tokens(V, Z, B):
    """Inside the forced launch (the merged build, the one-row build, workgroup C with two chunks per lane).  NaN in the head's weights
    (the kernel's ReLU turns a NaN logit into 0, so the rule still applies): the forced ticks return f, the tokens stay inside [0, V),
    logp is the restatement's on the returned weights.  +inf in the head's bias, no mask (m is not finite: every tick is outside the
    rule): the forced ticks still return f, logp is NaN everywhere, the free ticks take the argmax, the tokens stay inside [0, V); with the
    mask the ticks that ban the +inf token are inside the rule again, as the restatement says.  Finite weights with uniforms outside [0, 1): the
    forced ticks are untouched by them, the free ones fall back as in the constrained call."""
    from tests.test_gpu_kernels import pack
    cfg, P, params = decoder(V, Z)
    table, total = ops.vae_param_table(cfg)
    z = torch.from_numpy(synthetic.det_normal(f"decoder_forced/z/edges/{V}/{Z}/{B}", (B, Z))).cuda()
    u = synthetic.det_uniform(f"decoder_forced/u/edges/{V}/{Z}/{B}", (B, 24), 0.0, 1.0).astype(np.float64)
    allow, forced = CR.plan_mask(V, B), FR.plan_forced(V, B)
    isf = forced >= 0
    Pn = {k: v.clone() for k, v in P.items()}
    Pn["decoder.tick_emb_to_note_emb.0.weight"].view(-1)[3::7] = float("nan")
    w, tok, lp, labels = forced_call(cfg, z, pack(table, total, Pn), 6.0, u, 8, 0.7, allow, forced)
    assert any(l.startswith("force_decode_b1") for l in labels)
    assert np.array_equal(tok[isf], forced[isf]) and tok.min() >= 0 and tok.max() < V
    check_rule(w, tok, lp, 6.0, u, 8, 0.7, allow, forced, ("nan weights", V, Z, B))
    Pn = {k: v.clone() for k, v in P.items()}
    Pn["decoder.tick_emb_to_note_emb.0.bias"][V // 2] = float("inf")
    w, tok, lp, labels = forced_call(cfg, z, pack(table, total, Pn), 6.0, u, 8, 0.7, None, forced)
    assert any(l.startswith("force_decode_b1") for l in labels)
    assert np.isposinf(w.cpu().numpy()[..., V // 2]).all() and np.isnan(lp).all()
    assert np.array_equal(tok[isf], forced[isf]) and (tok[~isf] == V // 2).all()
    w, tok, lp, labels = forced_call(cfg, z, pack(table, total, Pn), 6.0, u, 8, 0.7, allow, forced)
    assert np.array_equal(tok[isf], forced[isf]) and tok.min() >= 0 and tok.max() < V
    assert np.array_equal(np.isnan(lp), allow[..., V // 2])                     # (m is not finite wherever the +inf token is allowed)
    check_rule(w, tok, lp, 6.0, u, 8, 0.7, allow, forced, ("inf bias", V, Z, B))
    u[:, 1::4] = 2.0
    u[:, 3::4] = np.nan
    u[:, 0::8] = -0.5
    w, tok, lp, labels = forced_call(cfg, z, params, 6.0, u, 8, 0.7, allow, forced)
    out = ~((u >= 0.0) & (u < 1.0))
    assert (out & isf).any() and not np.isnan(lp[isf]).any()
    assert np.isnan(lp[out & ~isf]).all() and not np.isnan(lp[~out]).any()
    wn = w.cpu().numpy()
    assert np.array_equal(tok[out & ~isf], np.where(allow, wn, -np.inf).argmax(-1)[out & ~isf])
    c = check_rule(w, tok, lp, 6.0, u, 8, 0.7, allow, forced, ("edges", V, Z, B))
    assert c[0] + c[2] <= 0.01 * (c[1] + c[3]), (V, Z, B, c)


@pytest.mark.parametrize("auto_reg", [False, True])
def test_score_and_score_fixed(auto_reg, monkeypatch):
    """LatentRNNTester.score of generate()'s own fillings under the same temperature, top_k, top_p and bans is that call's last_logp bit
    for bit and does not touch np.random; generate(fixed_tokens=, score_fixed=True) keeps the notes and reports finite, non-zero logp for
    them (the default reports exactly 0); score of the original target measures is finite at temperature 1."""
    fx = G.load("inference_small")
    tag = "gen_ar" if auto_reg else "gen_nar"
    c, ds, vae, model = small_model(auto_reg)
    V = c["V"]
    tester = LatentRNNTester(ds, model)
    score = torch.from_numpy(fx[f"{tag}_score"])
    past, future, target = LatentRNNTrainer.split_score(score, 5, 8, 3, 24)
    eps4 = torch.cat((torch.from_numpy(fx[f"{tag}_eps_past"]), torch.from_numpy(fx[f"{tag}_eps_future"])), 0).cuda()

    def run(fn, nvar):
        queue = [eps4.view(1, 13, -1).expand(nvar, -1, -1).reshape(nvar * 13, -1)]
        if auto_reg:
            queue += [torch.from_numpy(fx[f"{tag}_eps_ar{i}"]).cuda().repeat(nvar, 1) for i in range(3)]
        monkeypatch.setattr(torch, "randn_like", lambda t: queue.pop(0))
        try:
            return fn()
        finally:
            monkeypatch.undo()

    np.random.seed(21)
    plain = run(lambda: tester.generate(past, future, None, 3, num_variations=4, temperature=6.0, top_p=0.9)[1], 4)[:, 5:8].cpu().numpy()
    banned = [int(t) for t in np.argsort(-np.bincount(plain.reshape(-1), minlength=V))[:2]]
    fills = []
    for kw in (dict(temperature=6.0, top_p=0.9, banned_tokens=banned), dict(temperature=6.0, top_k=5, top_p=0.7), dict(temperature=1.5)):
        gkw = dict(kw) if len(kw) > 1 else dict(kw, top_p=1.0)     # (top_p = 1: a scored call without truncation)
        np.random.seed(21)
        full = run(lambda: tester.generate(past, future, None, 3, num_variations=4, **gkw)[1], 4)
        lp, tick = tester.last_logp.clone(), model.last_logp.clone()
        fills.append(full)
        assert bool(torch.isfinite(lp).all())
        state = np.random.get_state()[1].copy()
        got = run(lambda: tester.score(past, future, full[:, 5:8], **kw), 4)
        assert np.array_equal(np.random.get_state()[1], state)
        assert tuple(got.shape) == (4, 3) and got.dtype == torch.float32
        assert torch.equal(got.view(torch.int32), lp.view(torch.int32)), (kw, got, lp)
        assert tuple(tester.last_tick_logp.shape) == (4, 3, 24) and torch.equal(tester.last_tick_logp.view(torch.int32), tick.view(torch.int32))
        assert tuple(tester.last_weights.shape) == (4, 3, 24, V)
        assert ops.chain_status() == 0
    # a filling the ban excludes scores -inf in its measure
    worst = fills[0][:1, 5:8].clone()                           # (drawn under the ban)
    worst[0, 1, 7] = banned[0]
    got = run(lambda: tester.score(past, future, worst, temperature=6.0, banned_tokens=banned), 1)
    assert bool(torch.isneginf(got[0, 1])) and bool(torch.isfinite(got[0, 0]))
    # the original measures at temperature 1
    got = run(lambda: tester.score(past, future, target), 1)
    assert tuple(got.shape) == (1, 3) and bool(torch.isfinite(got).all()) and bool((got < 0).all())
    # kept notes
    fixed = torch.full((3, 24), -1, dtype=torch.int64)
    for m, t in ((0, 0), (0, 5), (1, 11), (2, 23), (2, 6)):
        fixed[m, t] = (int(plain[0, m, t]) + 1 + t) % V
    fixed[1, 2] = banned[0]                                     # a fixed tick wins over a ban
    keep = (fixed >= 0).numpy()
    gkw = dict(num_variations=4, temperature=6.0, banned_tokens=banned, fixed_tokens=fixed)
    np.random.seed(21)
    base = run(lambda: tester.generate(past, future, None, 3, **gkw)[1], 4)
    base_tick = model.last_logp.clone().cpu().numpy()
    np.random.seed(21)
    full = run(lambda: tester.generate(past, future, None, 3, score_fixed=True, **gkw)[1], 4)
    tick = model.last_logp.clone().cpu().numpy()
    g = full[:, 5:8].cpu().numpy()
    assert (g[:, keep] == fixed.numpy()[keep]).all() and not np.isin(g[:, ~keep], banned).any()
    assert torch.equal(full, base)                              # the same notes: the kept ones are fed back either way
    assert (base_tick[:, keep] == 0.0).all()
    assert np.isfinite(tick[:, keep]).all() and (tick[:, keep] != 0.0).all()
    assert np.array_equal(tick[:, ~keep].view(np.int32), base_tick[:, ~keep].view(np.int32))
    assert torch.equal(tester.last_logp, model.last_logp.sum(-1))
    with pytest.raises(ValueError):
        tester.generate(past, future, None, 3, fixed_tokens=fixed, score_fixed=True)
    assert ops.chain_status() == 0
