"""The decoder's temperature-sampled free-running decode on the GPU: the sampling build of the register-resident launch
(csrc/decode_b1.hip, every plan a sampled call can get), the tick-by-tick path of every other shape (csrc/vae.hip with
inet_sample_temperature's kernel), that kernel alone, and the public surface down from LatentRNNTester.generate.

The reference for every call is the float64 oracle with the KERNEL's tokens fed back (a draw next to a step of the CDF cannot
de-synchronise the two trajectories) plus the float64 restatement of the rule (tests/decoder_sample_ref.py): logits within 2e-5
relative, every token equal to the restatement's pick except on draws whose uniform lies within 2e-5 of a CDF step of the oracle,
and those may be at most 1 % of a test's draws."""
import numpy as np
import pytest
import torch

from tests import decoder_sample_ref as R
from tests import golden_util as G

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from inpaintnet_amd import _lib, ops, synthetic
    from inpaintnet_amd.latent_rnn import LatentRNN
    from inpaintnet_amd.latent_rnn_tester import LatentRNNTester
    from inpaintnet_amd.latent_rnn_trainer import LatentRNNTrainer
    from inpaintnet_amd.measure_vae import MeasureVAE
    from tests.test_gpu_decode_plans import decoder, labels_of
    from tests.test_gpu_kernels import pack

TOL = 2e-5
SIZES = (1, 2, 4, 5, 7, 16)
TEMPERATURES = (0.5, 1.0, 1.5)


def uniforms(tag, B):
    return synthetic.det_uniform(f"decoder_sample/u/{tag}", (B, 24), 0.0, 1.0).astype(np.float64)


def sample(cfg, z, params, temp, u, mask_beat=None, mask_tick=None):
    """One sampled call -> (weights, samples, launch labels); a bounded-spin timeout fails here."""
    ud = torch.from_numpy(np.ascontiguousarray(u)).cuda()
    (w, s_, _), labels = labels_of(lambda: ops.decoder_fwd(cfg, z, None, False, params, mask_beat=mask_beat, mask_tick=mask_tick,
                                                           temperature=temp, uniforms=ud))
    status = ops.chain_status()
    assert status == 0, (tuple(z.shape), temp, status, ops.slow_waits_summary())
    return w.clone(), s_.clone(), labels


def check_against_oracle(P64, z, w, s_, temp, u, V, what, masks=None):
    """Logits within TOL of the oracle fed the kernel's tokens, tokens equal to the restatement's outside the margin.
    -> (draws within the margin, draws, the oracle's logits): the caller holds the count to 1 % of its draws."""
    tok = s_.cpu().numpy()[:, 0]
    assert tok.min() >= 0 and tok.max() < V, what
    wr = R.oracle_logits(P64, z.cpu(), tok, masks)
    err = G.rel_err(w.cpu(), wr)
    want, mg = R.sample_rows(wr, temp, u)
    firm = mg >= R.MARGIN
    print(what, "rel err %.3g" % err, "within margin", int((~firm).sum()), "differ", int((tok != want).sum()))
    assert err < TOL, (what, err)
    assert np.array_equal(tok[firm], want[firm]), (what, np.argwhere((tok != want) & firm)[:4])
    return int((~firm).sum()), firm.size, wr


@pytest.mark.parametrize("Z", [256, 128])
@pytest.mark.parametrize("V", [20, 48, 100])
def test_every_plan_of_a_sampled_call(V, Z):
    """B in {1, 2, 4, 5, 7, 16} x three temperatures per (V, Z): with V = 20 / 48 / 100 the two-row merged build, the one-row
    merged build and workgroup C with two logit chunks per lane, with the beat path in the launch (Z = 256, up to six measures) and
    behind its own launches.  Draws within 2e-5 of a CDF step, counted on the CPU along the oracle's own sampled trajectory
    (decoder_sample_ref.sampled_trajectory) for these very seeds: 33 of the 15120 draws of the six cases (0.22 %), at most 8 of 2520 in one
    case (0.32 %; V = 100, Z = 256) -- the bound below is 1 %.  There the shifted tokens move the logits by 2.6 % to 8.1 % of their scale.
    Preconditions, on the sixteen-row calls: the oracle with every fed token shifted by one moves the logits by more than 100 x the
    tolerance (a kernel that feeds back another token than it reports cannot pass), and the sixteen rows are all different."""
    cfg, P, params = decoder(V, Z)
    P64 = {k: v.double() for k, v in P.items()}
    near = draws = 0
    for B in SIZES:
        z = torch.from_numpy(synthetic.det_normal(f"decoder_sample/z/{V}/{Z}/{B}", (B, Z))).cuda()
        for temp in TEMPERATURES:
            u = uniforms(f"{V}/{Z}/{B}/{temp}", B)
            w, s_, labels = sample(cfg, z, params, temp, u)
            folded = Z == 256 and B <= 6
            want = f"sample_decode_b1_beats T24 B{B} " if folded else f"sample_decode_b1 T24 B{B} "
            assert any(l.startswith(want) for l in labels), (V, Z, B, sorted(set(labels)))
            assert not any(l.startswith(("decode_b1", "decode_chain", "sample_temperature")) for l in labels), sorted(set(labels))
            n, d, wr = check_against_oracle(P64, z, w, s_, temp, u, V, (V, Z, B, temp))
            near, draws = near + n, draws + d
            if B == 16:
                tok = s_.cpu().numpy()[:, 0]
                shifted = R.oracle_logits(P64, z.cpu(), (tok + 1) % V)
                moved = float(np.abs(shifted - wr).max() / np.abs(wr).max())
                assert moved > 100 * TOL, (V, Z, temp, moved)
                assert len({tuple(r) for r in tok.tolist()}) == B, (V, Z, temp)
    assert near <= 0.01 * draws, (V, Z, near, draws)


def test_the_fixture_captured_from_the_reference():
    """tests/golden/decoder_sample.npz (the reference's decoder with the rule on stored uniforms, `small` configuration: the
    tick-by-tick path): tokens exact -- every draw of the fixture is at least 2e-5 from a CDF step --, logits to the tolerance of the
    decoder's golden tests."""
    fx = G.load("decoder_sample")
    c = G.CFGS["small"]
    P = G.vae_params("small")
    cfg = ops.vae_config(c["V"], c["E"], c["H"], c["Z"], c["H"])
    table, total = ops.vae_param_table(cfg)
    params = pack(table, total, P)
    z = torch.from_numpy(fx["z"]).cuda()
    for ti, temp in enumerate(fx["temperatures"]):
        w, s_, labels = sample(cfg, z, params, float(temp), fx[f"t{ti}/uniforms"])
        assert np.array_equal(s_.cpu().numpy()[:, 0], fx[f"t{ti}/tokens"]), ti
        assert G.rel_err(w.cpu(), fx[f"t{ti}/weights"]) < 1e-4, ti
        assert sum(l.startswith("sample_temperature ") for l in labels) == 24, sorted(set(labels))


@pytest.mark.parametrize("B", [17, 40])
def test_the_tick_by_tick_path_of_the_other_shapes(B):
    """More than sixteen rows (V = 48, H = 512): one sampling launch per tick behind the output projection, no register-resident
    decode launch and no exchange kernel; the same oracle check.  Within the margin on the CPU for these seeds: none of the 1368 draws."""
    V, Z = 48, 256
    cfg, P, params = decoder(V, Z)
    P64 = {k: v.double() for k, v in P.items()}
    z = torch.from_numpy(synthetic.det_normal(f"decoder_sample/z/fallback/{B}", (B, Z))).cuda()
    u = uniforms(f"fallback/{B}", B)
    w, s_, labels = sample(cfg, z, params, 1.0, u)
    assert sum(l.startswith("sample_temperature ") for l in labels) == 24, sorted(set(labels))
    assert not any("decode_b1" in l or l.startswith("decode_chain") for l in labels), sorted(set(labels))
    n, d, _ = check_against_oracle(P64, z, w, s_, 1.0, u, V, ("fallback", B))
    assert n <= 0.01 * d, (n, d)


def test_a_tick_mask_takes_the_tick_by_tick_path():
    """Within the margin on the CPU for this seed and this mask (tests/pointwise_ref.dropout_mask_ref mirrors the mask stream): none
    of the 96 draws, the nearest at 5.2e-5."""
    V, Z, B = 48, 256, 4
    cfg, P, params = decoder(V, Z)
    P64 = {k: v.double() for k, v in P.items()}
    z = torch.from_numpy(synthetic.det_normal("decoder_sample/z/tick_mask", (B, Z))).cuda()
    u = uniforms("tick_mask", B)
    mt = ops.dropout_mask((24, B, 512), 0.5, 77, 0, "cuda")
    w, s_, labels = sample(cfg, z, params, 1.5, u, mask_tick=mt)
    assert sum(l.startswith("sample_temperature ") for l in labels) == 24 and not any("decode_b1" in l for l in labels), sorted(set(labels))
    n, d, _ = check_against_oracle(P64, z, w, s_, 1.5, u, V, "tick mask", masks={"tick": mt.permute(1, 0, 2).double().cpu()})
    assert n <= 0.01 * d, (n, d)


@pytest.mark.parametrize("V,Z,B", [(20, 256, 2), (48, 256, 1), (48, 256, 4), (20, 128, 7), (20, 128, 16), (100, 256, 5), (100, 128, 16)])
def test_uniforms_outside_the_unit_interval_take_the_argmax_rule(V, Z, B):
    """u = 2.0 everywhere: the call is the argmax call -- tokens on every row whose oracle top-2 margin exceeds 1e-4, logits within
    2e-5 -- through the SAMPLING launch; u = 0 and u = the largest double below 1 (the first and the last token with mass), NaN and a
    negative u stay inside the vocabulary and match the restatement wherever u is 2e-5 or more from a CDF step.  (Every uniform of
    such a call is the same value on purpose: how many of them lie next to a step is not a sample of anything and is not counted.)"""
    cfg, P, params = decoder(V, Z)
    P64 = {k: v.double() for k, v in P.items()}
    z = torch.from_numpy(synthetic.det_normal(f"decoder_sample/z/edges/{V}/{Z}/{B}", (B, Z))).cuda()
    w2, s2, labels = sample(cfg, z, params, 1.0, np.full((B, 24), 2.0))
    assert any(l.startswith("sample_decode_b1") for l in labels), sorted(set(labels))
    w0, s0, _ = ops.decoder_fwd(cfg, z, None, False, params)
    assert ops.chain_status() == 0
    wr = R.oracle_logits(P64, z.cpu(), s2.cpu().numpy()[:, 0])
    assert G.rel_err(w2.cpu(), wr) < TOL
    top2 = np.sort(wr, -1)[..., -2:]
    rows = ((top2[..., 1] - top2[..., 0]) > 1e-4).all(-1)
    assert rows.any()
    assert np.array_equal(s2.cpu().numpy()[rows], s0.cpu().numpy()[rows])
    assert np.array_equal(s2.cpu().numpy()[:, 0][rows], wr.argmax(-1)[rows])
    assert float((w2[rows] - w0[rows]).abs().max()) < TOL * float(w0.abs().max())
    for name, val in (("zero", 0.0), ("below one", float(np.nextafter(1.0, 0.0))), ("nan", float("nan")), ("negative", -0.25)):
        u = np.full((B, 24), val)
        w, s_, _ = sample(cfg, z, params, 1.5, u)
        check_against_oracle(P64, z, w, s_, 1.5, u, V, (name, V, Z, B))


@pytest.mark.parametrize("B", [1, 16, 17])
def test_nan_weights_stay_inside_the_vocabulary(B):
    """NaN in the head's weights: every logit is ReLU(NaN) = 0, the draw is uniform over the vocabulary and stays inside it; NaN in a
    recurrent weight from the second tick on likewise.  chain_status() stays clean (a NaN is a value, not a timeout)."""
    V, Z = 48, 256
    cfg, P, params = decoder(V, Z)
    z = torch.from_numpy(synthetic.det_normal(f"decoder_sample/z/nan/{B}", (B, Z))).cuda()
    u = uniforms(f"nan/{B}", B)
    table, total = ops.vae_param_table(cfg)
    for key in ("decoder.tick_emb_to_note_emb.0.weight", "decoder.rnn_tick.weight_hh_l1", "decoder.note_embedding_layer.weight"):
        Pn = {k: v.clone() for k, v in P.items()}
        Pn[key].view(-1)[3::7] = float("nan")
        w, s_, labels = sample(cfg, z, pack(table, total, Pn), 1.5, u)
        assert any(l.startswith("sample_") for l in labels)
        assert int(s_.min()) >= 0 and int(s_.max()) < V, key
        assert ops.chain_status() == 0


@pytest.mark.parametrize("V", [1, 2, 20, 64, 65, 128, 512])
def test_the_sampling_kernel_alone(V):
    """inet_sample_temperature: rows in {1, 5, 70} (more rows than a workgroup's waves), a row stride larger than V with NaN in the
    padding, strided uniforms; against the restatement under the margin rule: tokens equal outside 2e-5 around the CDF steps, and at
    most 1 % of a vocabulary's 228 draws inside.  Counted on the CPU for these seeds: V = 65 one draw, V = 128 and V = 512 two each
    (0.88 %), the other vocabularies none.  Plus rows where the rule does not apply."""
    near = draws = 0
    for rows in (1, 5, 70):
        ld = V + 3
        x = synthetic.det_normal(f"decoder_sample/alone/{V}/{rows}", (rows, ld), 2.0)
        x[:, V:] = np.nan
        x[:, :V] = np.maximum(x[:, :V], 0.0)                  # post-ReLU logits: zeros (ties) among them
        u = synthetic.det_uniform(f"decoder_sample/alone/u/{V}/{rows}", (rows, 2), 0.0, 1.0).astype(np.float64)
        for temp in (0.5, 1.0, -1.5):
            got = ops.sample_temperature(torch.from_numpy(x).cuda()[:, :V], temp, torch.from_numpy(u).cuda()[:, 0]).cpu().numpy()
            want, mg = R.sample_rows(x[:, :V], temp, u[:, 0])
            firm = mg >= R.MARGIN
            assert got.min() >= 0 and got.max() < V
            assert np.array_equal(got[firm], want[firm]), (V, rows, temp)
            near, draws = near + int((~firm).sum()), draws + firm.size
    assert near <= 0.01 * draws, (V, near, draws)
    # rows outside the rule take argmax_first: u outside [0, 1), NaN logits (the lowest NaN wins), +inf
    x = np.maximum(synthetic.det_normal(f"decoder_sample/alone/edge/{V}", (6, V), 2.0), 0.0)
    u = np.array([2.0, np.nan, -0.5, 0.3, 0.3, 1.0])
    x[3, V // 2] = np.nan
    x[4, V - 1] = np.inf
    got = ops.sample_temperature(torch.from_numpy(x).cuda(), 1.0, torch.from_numpy(u).cuda()).cpu().numpy()
    assert got.tolist() == [int(np.argmax(r)) for r in x], (got, x.argmax(-1))
    assert got[3] == V // 2 and got[4] == V - 1


def test_the_kernel_refuses_what_it_is_not_built_for():
    w = torch.zeros(2, 513, device="cuda")
    u = torch.zeros(2, dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError):
        ops.sample_temperature(w, 1.0, u)
    with pytest.raises(ValueError):
        ops.sample_temperature(w[:, :8], float("inf"), u)
    cfg, P, params = decoder(20, 256)
    z = torch.zeros(2, 256, device="cuda")
    u2 = torch.zeros(2, 24, dtype=torch.float64, device="cuda")
    for bad in (dict(temperature=float("nan"), uniforms=u2), dict(temperature=1.0, uniforms=u2[:1]),
                dict(temperature=1.0, uniforms=u2.float()), dict(temperature=1.0), dict(uniforms=u2)):
        with pytest.raises(ValueError):
            ops.decoder_fwd(cfg, z, None, False, params, **bad)


def small_vae():
    c = G.CFGS["small"]
    ds = synthetic.SyntheticFolkDataset(num_notes=c["V"])
    vae = MeasureVAE(ds, note_embedding_dim=c["E"], encoder_hidden_size=c["H"], latent_space_dim=c["Z"],
                     decoder_hidden_size=c["H"], encoder_dropout_prob=0.0, decoder_dropout_prob=0.0)
    vae.load_state_dict(G.vae_params("small"))
    return c, ds, vae


def small_model(auto_reg):
    """(the LatentRNN's state dict carries its own frozen VAE weights, other than G.vae_params' -- as in the latent_* fixtures)"""
    c, ds, vae = small_vae()
    model = LatentRNN(ds, vae, num_rnn_layers=2, rnn_hidden_size=c["H"], dropout=0.0, rnn_class=torch.nn.GRU,
                      auto_reg=auto_reg, teacher_forcing=True)
    model.load_state_dict(G.latent_params("small", auto_reg))
    return c, ds, vae, model


@pytest.mark.parametrize("auto_reg", [False, True])
def test_generate_draws_variations_of_one_gap(auto_reg, monkeypatch):
    """LatentRNNTester.generate(temperature=1.5, num_variations=4) on the model of inference_small.npz: four rows, past and future
    untouched, reproducible under np.random.seed; temperature=None returns what it returned before."""
    fx = G.load("inference_small")
    tag = "gen_ar" if auto_reg else "gen_nar"
    c, ds, vae, model = small_model(auto_reg)
    tester = LatentRNNTester(ds, model)
    score = torch.from_numpy(fx[f"{tag}_score"])
    past, future, target = LatentRNNTrainer.split_score(score, 5, 8, 3, 24)
    eps4 = torch.cat((torch.from_numpy(fx[f"{tag}_eps_past"]), torch.from_numpy(fx[f"{tag}_eps_future"])), 0).cuda()

    def run(temperature, nvar):
        # generate() encodes past | future of every row (rows ordered (row, measure)); the auto-regressive path re-encodes each measure
        queue = [eps4.view(1, 13, -1).expand(nvar, -1, -1).reshape(nvar * 13, -1)]
        if auto_reg:
            queue += [torch.from_numpy(fx[f"{tag}_eps_ar{i}"]).cuda().repeat(nvar, 1) for i in range(3)]
        monkeypatch.setattr(torch, "randn_like", lambda t: queue.pop(0))
        try:
            return tester.generate(past, future, None, 3, temperature=temperature, num_variations=nvar)[1]
        finally:
            monkeypatch.undo()

    np.random.seed(11)
    full = run(1.5, 4)
    assert full.shape == (4, 5 + 3 + 8, 24) and full.dtype == torch.int64
    got = full.cpu().numpy()
    assert np.array_equal(got[:, :5], np.broadcast_to(past.cpu().numpy(), (4, 5, 24)))
    assert np.array_equal(got[:, 8:], np.broadcast_to(future.cpu().numpy(), (4, 8, 24)))
    assert got[:, 5:8].min() >= 0 and got[:, 5:8].max() < c["V"]
    assert len({r.tobytes() for r in got[:, 5:8]}) == 4                          # four fillings of the same gap
    np.random.seed(11)
    assert torch.equal(run(1.5, 4), full)
    np.random.seed(12)
    assert not torch.equal(run(1.5, 4), full)
    # temperature None: what a call without the new keywords returns, bit for bit (the argmax call of
    # test_gpu_inference.test_generate_inpaints_like_the_reference) -- and np.random is not read
    state = np.random.get_state()[1].copy()
    plain = run(None, 1)
    assert np.array_equal(np.random.get_state()[1], state)
    queue = [eps4] + ([torch.from_numpy(fx[f"{tag}_eps_ar{i}"]).cuda() for i in range(3)] if auto_reg else [])
    monkeypatch.setattr(torch, "randn_like", lambda t: queue.pop(0))
    before = tester.generate(past, future, None, 3)[1]
    monkeypatch.undo()
    assert plain.shape == (1, 16, 24) and torch.equal(plain, before)
    plain = plain.cpu().numpy()
    okg = G.unique_rows(fx[f"{tag}_margin"], 1e-4).reshape(1, 3, 24)
    if not auto_reg or np.array_equal(plain, fx[f"{tag}_full"]):
        assert np.array_equal(plain[:, 5:8][okg], fx[f"{tag}_full"][:, 5:8][okg])
    else:                                      # (a near-tie flipped a token of the first measure: what follows it is not comparable)
        assert np.array_equal(plain[:, 5][okg[:, 0] & (np.cumsum(~okg[:, 0], -1) == 0)],
                              fx[f"{tag}_full"][:, 5][okg[:, 0] & (np.cumsum(~okg[:, 0], -1) == 0)])
    with pytest.raises(ValueError):
        tester.generate(past, future, None, 3, num_variations=2)
    assert ops.chain_status() == 0


def test_the_public_classes_take_and_check_the_arguments():
    """HierarchicalDecoder.forward / MeasureVAE.decode / LatentRNN.forward: explicit uniforms reproduce ops.decoder_fwd, host-drawn
    uniforms follow np.random.seed, a call with an injected teacher_forced=True ignores the temperature, and the argument errors are
    ValueErrors raised before anything random is drawn (the teacher-forcing coin, the dropout-mask offsets, numpy's stream)."""
    vae = small_vae()[2]                        # the fixture's decoder
    vae.eval()
    fx = G.load("decoder_sample")
    z = torch.from_numpy(fx["z"]).cuda()
    with torch.no_grad():
        w, s_ = vae.decode(z, temperature=1.5, uniforms=fx["t1/uniforms"])
        assert np.array_equal(s_.cpu().numpy()[:, 0], fx["t1/tokens"]) and G.rel_err(w.cpu(), fx["t1/weights"]) < 1e-4
        np.random.seed(int(fx["t1/seed"]))
        _, s2 = vae.decode(z, temperature=1.5)                                  # one np.random.random_sample((B, 24)) call
        assert torch.equal(s2, s_)
        w0, s0 = vae.decode(z)
        wa, sa = vae.decoder(z, torch.zeros(4, 24, device="cuda"), train=False)
        assert torch.equal(s0, sa) and torch.equal(w0, wa)
        tgt = torch.from_numpy(fx["t0/tokens"].astype(np.int64)).cuda()
        wt, st = vae.decoder(z, tgt, train=False, teacher_forced=True, temperature=1.5)
        wt0, st0 = vae.decoder(z, tgt, train=False, teacher_forced=True)
        assert torch.equal(st, st0) and torch.equal(wt, wt0)
        # a rejected call leaves the random streams alone -- also in train() with dropout on, where an accepted call draws masks
        import random
        from inpaintnet_amd import measure_vae
        vae.train()
        vae.decoder.dropout = 0.5
        streams = lambda: (random.getstate(), measure_vae._mask_counter[0], np.random.get_state()[1].tolist())
        was = streams()
        for bad in (dict(train=False, temperature=float("inf")), dict(train=False, uniforms=fx["t1/uniforms"]),
                    dict(train=False, temperature=1.0, uniforms=fx["t1/uniforms"][:2]), dict(train=True, temperature=1.0),
                    dict(train=True, temperature=1.0, uniforms=fx["t1/uniforms"]), dict(train=True, uniforms=fx["t1/uniforms"])):
            with pytest.raises(ValueError):
                vae.decoder(z, tgt, **bad)
            assert streams() == was, bad
        vae.decoder.dropout = 0.0
        vae.eval()
        c, ds, vae, model = small_model(False)
        model.eval()
        score = torch.from_numpy(G.load("inference_small")["gen_nar_score"])
        past, future, target = LatentRNNTrainer.split_score(score, 5, 8, 3, 24)
        with pytest.raises(ValueError):
            model(past, future, target, 3, train=True, temperature=1.0)
        with pytest.raises(ValueError):
            model(past, future, None, 3, train=False, temperature=1.0, uniforms=np.zeros((1, 2, 24)))
        with pytest.raises(ValueError):
            model(past, future, None, 3, train=False, uniforms=np.zeros((1, 3, 24)))
        u = synthetic.det_uniform("decoder_sample/u/latent", (1, 3, 24), 0.0, 1.0).astype(np.float64)
        torch.manual_seed(5)
        wl, sl, gz = model(past, future, None, 3, train=False, temperature=1.5, uniforms=u)
        wd, sd = vae.decode(gz.reshape(3, -1).contiguous(), temperature=1.5, uniforms=u.reshape(3, 24))
        assert torch.equal(sl.view(3, 24), sd.view(3, 24)) and torch.equal(wl.view(3, 24, -1), wd)
    assert ops.chain_status() == 0
