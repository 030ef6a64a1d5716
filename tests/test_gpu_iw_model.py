"""The importance-weighted log-likelihood at the model's level: MeasureVAE.log_weights, VAETester.
measure_log_likelihood / log_likelihood on the small synthetic MeasureVAE of tests/test_gpu_kl_schedule.py (V = 20, E = 6, H = 256,
Z = 24, det_param weights, eval mode).

Tolerances are the project's existing ones: a loss-like number within 1e-4 of its magnitude (LOSS_TOL of tests/test_gpu_kl_schedule.py);
the decoder's logits of two routes within 1e-4 of their largest element (tests/test_gpu_decoder_forced.py, tests/test_gpu_kernels.py: the
tolerance dec_tf_weights is held to), and a logit error of d moves a log-softmax entry by at most 2 d (the same file's argument), a
measure's 24 entries by 24 x 2 x d."""
import numpy as np
import pytest
import torch

from tests import iw_ref as R

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from inpaintnet_amd import ops, synthetic
    from inpaintnet_amd.vae_tester import VAETester
    from tests import decoder_trunc_ref as TR
    from tests.golden_util import rel_err
    from tests.test_gpu_kl_schedule import CFG, LOSS_TOL, _step, _tokens, _vae

WEIGHT_TOL = 1e-4                        # tests/test_gpu_decoder_forced.py: "assert werr < 1e-4" on the teacher-forced weights
NEW_LABELS = {"iw_draw", "nll_rows", "iw_finish"}
B0, K0 = 3, 5


@pytest.fixture(scope="module")
def vae():
    ds, model, _ = _vae()
    model.eval()
    P = {k: torch.from_numpy(synthetic.det_param(k, tuple(v.shape))) for k, v in model.state_dict().items()}
    return ds, model, VAETester(ds, model), P


def _eps(B, K, tag="iw/model/eps"):
    return synthetic.det_normal(f"{tag}/{B}x{K}", (B, K, CFG["Z"]))


@pytest.fixture(scope="module")
def oracle(vae):
    """The float64 log weights of the first B0 measures at K0 samples through oracle.torch_ref: computed once, never written to."""
    ds, model, tester, P = vae
    tok = _tokens()[:B0].cpu()
    eps = _eps(B0, K0)
    logw, nll, w = R.oracle_log_weights(P, tok, eps)
    return tok, eps, logw, nll, w


def _logged(model, tok, K, eps, max_rows):
    """log_weights with every decoder call's logits collected into their places of a (B, K, 24, V) tensor: the loop of the method, read
    back from a forward hook.  -> (logw, nll, logits)"""
    B = tok.shape[0]
    seen = []
    h = model.decoder.register_forward_hook(lambda mod, args, out: seen.append(out[0].detach().clone()))
    try:
        logw, nll = model.log_weights(tok, K, eps=eps, max_rows=max_rows)
    finally:
        h.remove()
    W = torch.full((B, K, 24, CFG["V"]), float("nan"), device="cuda")
    Bc = min(B, max_rows)
    Kc = max(1, max_rows // Bc)
    calls = iter(seen)
    for b0 in range(0, B, Bc):
        b1 = min(B, b0 + Bc)
        for k0 in range(0, K, Kc):
            k1 = min(K, k0 + Kc)
            W[b0:b1, k0:k1] = next(calls).view(b1 - b0, k1 - k0, 24, CFG["V"])
    assert next(calls, None) is None and not bool(torch.isnan(W).any())
    return logw, nll, W


def _own_bound(W, tok, K):
    """nll_rows' own bound for the logits W (B, K, 24, V) it was given (tests/iw_ref.py), as (B, K)."""
    B = W.shape[0]
    r = R.nll_rows(W.cpu().numpy().reshape(B * K, 24, -1), np.repeat(tok.cpu().numpy(), K, 0))
    return r["nll_bound"].reshape(B, K), r["nll"].reshape(B, K)


def test_log_weights_against_the_float64_oracle(vae, oracle):
    ds, model, tester, P = vae
    tok, eps, want_logw, want_nll, want_w = oracle
    eps_d = torch.from_numpy(eps).cuda()
    logw, nll, W = _logged(model, tok.cuda(), K0, eps_d, 4096)
    assert logw.shape == (B0, K0) and nll.shape == (B0, K0) and logw.dtype == torch.float32 and logw.is_cuda and nll.is_cuda
    lw, nl = logw.cpu().double().numpy(), nll.cpu().double().numpy()
    print("logits error %.3g of their largest; logw error / magnitude %.3g, nll error / magnitude %.3g (tolerance %g)"
          % (rel_err(W.cpu(), want_w), (np.abs(lw - want_logw) / np.abs(want_logw)).max(), (np.abs(nl - want_nll) / np.abs(want_nll)).max(),
             LOSS_TOL))
    print("logw", want_logw[0], "nll", want_nll[0])
    assert (np.abs(lw - want_logw) <= LOSS_TOL * np.abs(want_logw)).all()
    assert (np.abs(nl - want_nll) <= LOSS_TOL * np.abs(want_nll)).all()
    got = tester.measure_log_likelihood(tok, K0, eps=eps_d)
    assert got.shape == (B0, 5) and got.dtype == torch.float64 and got.is_cuda and tester.LL_COLUMNS == R.COLUMNS
    want = R.finish(want_logw, want_nll)
    g = got.cpu().numpy()
    for c, name in enumerate(R.COLUMNS):
        print(name, "got", g[:, c], "want", want[:, c], "error / magnitude %.3g" % (np.abs(g[:, c] - want[:, c]) / np.abs(want[:, c])).max())
    for c, name in enumerate(R.COLUMNS):
        assert (np.abs(g[:, c] - want[:, c]) <= LOSS_TOL * np.abs(want[:, c])).all(), name
    # iw_finish on the device's own weights: its own tolerance
    mine = R.finish(lw.astype(np.float32), nl.astype(np.float32))
    tol = R.FINISH_RTOL * np.abs(mine)
    tol[:, 2] = R.FINISH_RTOL
    assert (np.abs(ops.iw_finish(logw, nll).cpu().numpy() - mine) <= tol).all()


def test_chunking_moves_the_weights_by_no_more_than_the_logits_allow(vae, oracle):
    """max_rows in {1, 4, 4096} with the same eps: (1 measure x 1 sample), (3 measures x 1 sample), everything in one decoder call.
    iw_draw's rows do not depend on the chunking (tests/test_gpu_iw_kernels.py), so logr has the same bits; the decoder takes another
    route per batch size, and the logits of two routes differ by d, within the tolerance the decoder's tests hold between routes."""
    ds, model, tester, P = vae
    tok, eps = oracle[0].cuda(), torch.from_numpy(oracle[1]).cuda()
    runs = {mr: _logged(model, tok, K0, eps, mr) for mr in (1, 4, 4096)}
    for a, b in ((1, 4096), (4, 4096), (1, 4)):
        (lwa, nla, Wa), (lwb, nlb, Wb) = runs[a], runs[b]
        d = float((Wa - Wb).abs().max())
        scale = float(Wb.abs().max())
        ba, _ = _own_bound(Wa, tok, K0)
        bb, _ = _own_bound(Wb, tok, K0)
        lw = lwa.cpu().double().numpy()
        allowed = 24 * 2 * d + ba + bb + 2 * R.SLACK * R.U * np.abs(lw)
        diff = np.abs(lw - lwb.cpu().double().numpy())
        print(f"max_rows {a} against {b}: logits differ by {d:.3g} ({d / scale:.3g} of their largest, tolerance {WEIGHT_TOL}); "
              f"logw differs by {diff.max():.3g}, allowed {allowed.min():.3g}")
        assert d <= WEIGHT_TOL * scale
        assert (diff <= allowed).all()
        assert (np.abs(nla.cpu().double().numpy() - nlb.cpu().double().numpy()) <= 24 * 2 * d + ba + bb).all()


def test_the_teacher_forced_and_the_forced_sample_routes_score_alike(vae):
    """-nll of log_weights (teacher-forced logits, nll_rows) against the forced-token route of the sampled decoder: model.decode(z,
    temperature=1.0, forced=x) leaves the same tokens' log-probabilities in decoder.last_logp."""
    ds, model, tester, P = vae
    B = 4
    tok = _tokens()[B0:B0 + B]
    eps = torch.from_numpy(_eps(B, 1)).cuda()
    logw, nll, W = _logged(model, tok, 1, eps, 4096)
    with torch.no_grad():
        dist = model.encoder(tok)
        z, logr = ops.iw_draw(dist.loc.contiguous(), dist.log_scale.contiguous(), eps)
        wf, samples = model.decode(z, temperature=1.0, forced=tok)
        logp = model.decoder.last_logp.clone()
    torch.cuda.synchronize()
    ops.check_chains("forced route")
    assert torch.equal(samples.reshape(B, 24), tok)
    d = float((W[:, 0] - wf).abs().max())
    scale = float(wf.abs().max())
    own, _ = _own_bound(W, tok, 1)
    x = wf.cpu().double().numpy()
    margin = np.take_along_axis(x, tok.cpu().numpy()[..., None], -1)[..., 0] - x.max(-1)
    forced_own = TR.logp_tol(margin).sum(1)                                      # the sampled route's own tolerance, per tick
    got, want = -nll[:, 0].cpu().double().numpy(), logp.cpu().double().numpy().sum(1)
    print(f"logits differ by {d:.3g} ({d / scale:.3g} of their largest); -nll {got}, sum logp {want}, allowed {24 * 2 * d + own[:, 0] + forced_own}")
    assert d <= WEIGHT_TOL * scale
    assert (np.abs(got - want) <= 24 * 2 * d + own[:, 0] + forced_own).all()
    # and logw = logr - nll, on the device's own numbers
    lr = logr.cpu().double().numpy()
    assert (np.abs(logw[:, 0].cpu().double().numpy() - (lr + got)) <= R.U * np.abs(lr + got)).all()


def test_training_mode_is_refused(vae):
    ds, model, tester, P = vae
    model.train()
    try:
        with pytest.raises(ValueError, match="training mode"):
            model.log_weights(_tokens()[:2], 2)
    finally:
        model.eval()
    for bad in (dict(num_samples=0), dict(num_samples=2, max_rows=0), dict(num_samples=2, eps=torch.zeros(2, 3, CFG["Z"], device="cuda"))):
        with pytest.raises(ValueError):
            model.log_weights(_tokens()[:2], **bad)


def test_a_token_outside_the_vocabulary_raises_through_the_token_check(vae):
    ds, model, tester, P = vae
    ops.token_status(reset=True)
    bad = _tokens()[:2].clone()
    bad[1, 7] = CFG["V"]
    with pytest.raises(ops.TokenRangeError, match="Invalid Value of index"):
        model.log_weights(bad, 2, eps=torch.from_numpy(_eps(2, 2)).cuda())
    torch.cuda.synchronize()
    assert ops.token_status() == 0                                               # raising consumed the count


def test_log_likelihood_over_a_loader(vae):
    """Two batches, the first in (B, n_bars, 24) form: the measure-weighted means of measure_log_likelihood on the same draws (one
    seeded generator, consumed batch by batch in the same order)."""
    ds, model, tester, P = vae
    tok = _tokens().cpu()
    nb = ds.n_bars
    loader = [(tok[:nb].reshape(1, nb, 24), None), (tok[nb:nb + 5], None)]
    K = 3
    g = torch.Generator(device="cuda")
    g.manual_seed(77)
    got = tester.log_likelihood(loader, num_samples=K, generator=g)
    g.manual_seed(77)
    parts = [tester.measure_log_likelihood(t.reshape(-1, 24), K, generator=g) for t, _ in loader]
    cols = torch.cat(parts).cpu().numpy()
    assert cols.shape == (nb + 5, 5) and got["measures"] == nb + 5
    assert set(got) == set(R.COLUMNS) | {"measures", "nats_per_tick"}
    for c, name in enumerate(R.COLUMNS):
        assert abs(got[name] - cols[:, c].mean()) <= 1e-12 * np.abs(cols[:, c]).mean(), name
    assert got["nats_per_tick"] == -got["iwae"] / 24
    assert got["iwae"] >= got["elbo"] and 1.0 <= got["ess"] <= K and abs(got["rec"] + got["kl"] + got["elbo"]) <= 1e-9 * abs(got["elbo"])
    with pytest.raises(ValueError, match="empty"):
        tester.log_likelihood([], num_samples=K)
    # determinism: a seeded generator gives equal results
    g.manual_seed(77)
    again = tester.log_likelihood(loader, num_samples=K, generator=g)
    assert again == got
    g.manual_seed(78)
    assert tester.log_likelihood(loader, num_samples=K, generator=g)["iwae"] != got["iwae"]


def test_the_only_new_launch_labels_are_the_three_kernels(vae):
    from tests.test_gpu_decode_plans import labels_of
    ds, model, tester, P = vae
    tok = _tokens()[:B0]
    eps = torch.from_numpy(_eps(B0, K0)).cuda()

    def parts():
        with torch.no_grad(), ops.one_k_range():                                   # (the GEMM settings log_weights runs under)
            dist = model.encoder(tok)
            z = dist.loc.repeat_interleave(K0, 0).contiguous()
            model.decoder(z, tok.repeat_interleave(K0, 0), train=False, teacher_forced=True)
    _, before = labels_of(parts)
    _, mine = labels_of(lambda: tester.measure_log_likelihood(tok, K0, eps=eps))
    assert set(mine) - set(before) == NEW_LABELS, sorted(set(mine) - set(before))
    assert [l for l in mine if l not in NEW_LABELS] == before
    assert [l for l in mine if l in NEW_LABELS] == ["iw_draw", "nll_rows", "iw_finish"]


def test_a_default_training_step_launches_none_of_them():
    from tests.test_gpu_decode_plans import labels_of
    ds, model, trainer = _vae()
    tok = _tokens()
    _, labels = labels_of(lambda: _step(trainer, model, tok, 0))
    trainer.step()
    trainer.finish()
    assert labels and not [l for l in labels if l in NEW_LABELS or l.startswith(("iw_", "nll_"))]
