"""The HIP path with dropout ON against what the REFERENCE computed with the same masks (tests/golden/*_drop.npz: the upstream models
in train(), every mask they drew recorded in their own call order; oracle/gen_golden.py).  Everything the project reports as its
headline runs with dropout on, and until these fixtures the only witness of where a mask acts was the oracle the kernels were
written against (tests/test_oracle_dropout_golden.py pins that oracle to the same fixtures on the CPU).

Two levels, both reading tests/golden/ only:
  kernel level   the C-ABI entry points with the reference's masks uploaded time-major as drawn;
  model level    the public classes driven as the reference's loop drives them, with ops.dropout_mask replaced by a server that
                 hands out the reference's masks in the PRODUCT's request order and layout (MaskServer) and fails on any request it
                 did not expect and on any mask left over.

Tolerances are those of the dropout-0 fixture tests for the same quantity (tests/test_gpu_kernels.py, test_gpu_model.py,
test_gpu_latent.py, test_gpu_arnn.py).  Every compared figure is printed before it is asserted."""
import types

import numpy as np
import pytest
import torch

from tests import golden_util as G

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from inpaintnet_amd import arnn as ARNN
    from inpaintnet_amd import latent_rnn as LR
    from inpaintnet_amd import ops, synthetic
    from inpaintnet_amd import measure_vae as MV
    from inpaintnet_amd._lib import LatentConfig
    from inpaintnet_amd.latent_rnn_trainer import LatentRNNTrainer
    from inpaintnet_amd.vae_trainer import VAETrainer
    from tests.test_gpu_kernels import DEV, _vae_step_hip, pack, relmax, unpack


def _grad_err(g, fx, prefix, k):
    """Error of one gradient tensor against the fixture: whole tensor where the fixture keeps it, else norm / head / tail."""
    if f"{prefix}grad/{k}" in fx.files:
        r = fx[f"{prefix}grad/{k}"]
        return float(np.abs(g - r).max() / (np.abs(r).max() + 1e-7))
    rn = float(fx[f"{prefix}gradnorm/{k}"])
    err = abs(float(np.sqrt((g.astype(np.float64) ** 2).sum())) - rn) / (rn + 1e-12)
    for part, sl in (("gradhead", slice(None, 64)), ("gradtail", slice(-64, None))):
        err = max(err, float(np.abs(g.reshape(-1)[sl] - fx[f"{prefix}{part}/{k}"]).max() / (np.abs(g).max() + 1e-12)))
    return err


class MaskServer:
    """Stands in for ops.dropout_mask: serves a prepared queue of (shape, p, mask) in order; a request of another shape or p, a request
    with the queue empty, and (done()) masks nobody asked for all fail the test."""

    def __init__(self, queue):
        self.queue = [(tuple(int(d) for d in s), float(p), m) for s, p, m in queue]
        self.served = 0

    def __call__(self, shape, p, seed, offset, device):
        shape = tuple(int(d) for d in shape)
        assert self.queue, f"mask request {shape} p={p} behind the {self.served} the reference drew"
        want, want_p, m = self.queue.pop(0)
        assert shape == want and float(p) == want_p, f"request {self.served}: product asks {shape} p={p}, expected {want} p={want_p}"
        assert m.numel() == int(np.prod(shape))
        self.served += 1
        return m.to(dtype=torch.float32).contiguous().view(shape).to(device).clone()

    def done(self):
        assert not self.queue, f"{len(self.queue)} recorded masks were never requested (next: {self.queue[0][0]})"
        print(f"mask server: all {self.served} requests served, nothing left over")


# ----------------------------------------------------------------------------------------------------------------------
# MeasureVAE
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small", "mid", "full"])
@pytest.mark.parametrize("mode", ["tf", "fr"])
def test_vae_kernels_with_reference_masks(name, mode):
    """encoder_fwd / decoder_fwd / decoder_bwd / encoder_bwd (tests/test_gpu_kernels.py: _vae_step_hip) under the reference's
    step-0 masks, time-major as drawn; then Adam, as test_vae_train_steps_golden does at dropout 0."""
    fx = G.load(f"vae_{name}_drop")
    c = G.CFGS[name]
    cfg = ops.vae_config(c["V"], c["E"], c["H"], c["Z"], c["H"])
    table, total = ops.vae_param_table(cfg)
    params = pack(table, total, G.vae_params(name))
    grads = torch.zeros_like(params)
    tok = torch.from_numpy(fx["tokens"]).to(DEV)
    eps = torch.from_numpy(fx[f"step_{mode}_eps0"]).to(DEV)
    sm = G.vae_step_masks(fx, mode, 0)
    masks = {k: sm[k].contiguous().to(DEV) for k in ("enc", "beat", "tick")}
    B, H = tok.shape[0], c["H"]
    assert masks["enc"].shape == (24, B, 2 * H) and masks["beat"].shape == (4, B, H) and masks["tick"].shape == (24, B, H)
    loss, ce, kl, acc, w, s, z = _vae_step_hip(cfg, table, params, grads, tok, eps, mode == "tf", masks)
    ref = fx[f"step_{mode}_losses"][0]
    ew, ez = relmax(w, fx[f"step_{mode}_weights"]), relmax(z, fx[f"step_{mode}_z"])
    errs = {p: _grad_err(unpack(table, grads, p).cpu().numpy(), fx, f"step_{mode}_", p) for p, _, _ in table}
    worst = max(errs, key=errs.get)
    print(f"HIP kernels vae_{name}_drop {mode}: weights {ew:.2e} z {ez:.2e} loss {abs(loss - ref[0]) / abs(ref[0]):.2e} "
          f"worst gradient {worst} {errs[worst]:.2e}")
    assert abs(loss - ref[0]) <= 1e-4 * abs(ref[0]) and abs(ce - ref[1]) <= 1e-4 * abs(ref[1]) and abs(kl - ref[2]) <= 1e-4 * abs(ref[2])
    assert ew < 1e-4
    assert ez < 1e-4
    ok = G.unique_rows(fx[f"step_{mode}_margin"])
    assert ok.mean() > 0.5
    assert np.array_equal(s.cpu().numpy()[:, 0][ok], fx[f"step_{mode}_samples"][:, 0][ok])
    wh = w.cpu().reshape(-1, w.shape[-1])
    own = float((wh.argmax(1) == tok.cpu().reshape(-1)).double().mean())
    assert abs(acc - own) < 1e-6, (acc, own)                        # the kernel's count = the first-argmax count of its own logits
    mg = fx[f"step_{mode}_margin"]
    near = float(((mg > 0) & (mg <= 1e-4)).mean())
    assert abs(acc - ref[3]) <= near + 1e-6, (acc, ref[3], near)
    assert errs[worst] < 5e-4, sorted(errs.items(), key=lambda kv: -kv[1])[:5]
    m, v = torch.zeros_like(params), torch.zeros_like(params)
    ops.adam_step(params, grads, m, v, 1e-4, 1)
    for p, _, _ in table:
        pv = unpack(table, params, p).cpu().numpy()
        if name == "small":
            assert np.abs(pv - fx[f"step_{mode}_after1/{p}"]).max() < 1e-5, p
        else:
            assert np.abs(pv.reshape(-1)[:64] - fx[f"step_{mode}_after1/head/{p}"]).max() < 1e-5, p
    assert ops.chain_status() == 0


@pytest.mark.parametrize("name", ["small", "mid", "full"])
@pytest.mark.parametrize("mode", ["tf", "fr"])
def test_vae_kernels_see_every_mask_placement(name, mode):
    """The control for the test above: one mask wrong at a time (omitted, read batch-major, unscaled, ticks shifted by one, beat and
    tick swapped; the table the CPU oracle is put through) must move the kernels' logits away from the fixture by at least 100 times
    the passing tolerance -- so the agreement above is not one that a misplaced mask would also reach."""
    fx = G.load(f"vae_{name}_drop")
    c = G.CFGS[name]
    cfg = ops.vae_config(c["V"], c["E"], c["H"], c["Z"], c["H"])
    table, total = ops.vae_param_table(cfg)
    params = pack(table, total, G.vae_params(name))
    tok = torch.from_numpy(fx["tokens"]).to(DEV)
    eps = torch.from_numpy(fx[f"step_{mode}_eps0"]).to(DEV)
    sm = G.vae_step_masks(fx, mode, 0)
    for what, mutate in G.VAE_MASK_MUTATIONS.items():
        mm = mutate(sm)
        assert all(mm[k].shape == sm[k].shape for k in ("enc", "beat", "tick"))
        masks = {k: mm[k].contiguous().to(DEV) for k in ("enc", "beat", "tick")}
        mu, ls, _ = ops.encoder_fwd(cfg, tok, params, mask=masks["enc"])
        z, _ = ops.reparam_kl(mu, ls, eps)
        w, _, _ = ops.decoder_fwd(cfg, z, tok, mode == "tf", params, masks["beat"], masks["tick"])
        moved = relmax(w, fx[f"step_{mode}_weights"])
        print(f"HIP kernels vae_{name}_drop {mode}: {what}: weights move by {moved:.3f}")
        assert moved >= 100 * 1e-4, f"vae_{name}_drop {mode}: the kernels do not see: {what} ({moved:.2e})"
    assert ops.chain_status() == 0


def _build_vae(name, dropout):
    c = G.CFGS[name]
    ds = synthetic.SyntheticFolkDataset(num_notes=c["V"])
    model = MV.MeasureVAE(ds, note_embedding_dim=c["E"], encoder_hidden_size=c["H"], latent_space_dim=c["Z"],
                          decoder_hidden_size=c["H"], encoder_dropout_prob=dropout, decoder_dropout_prob=dropout)
    model.load_state_dict(G.vae_params(name))
    return ds, model


@pytest.mark.parametrize("name", ["small", "mid", "full"])
@pytest.mark.parametrize("mode", ["tf", "fr"])
@pytest.mark.parametrize("overlap", [False, True])
def test_vae_trainer_five_steps_with_reference_masks(name, mode, overlap, monkeypatch):
    """The reference's loop body on MeasureVAE + VAETrainer (as test_trainer_trajectory_matches_reference drives it), five steps,
    fresh reference masks every step.  MeasureVAE.forward draws the three masks of a step as ONE flat buffer: encoder (24, B, 2H) |
    beat (4, B, H) | tick (24, B, H), each time-major."""
    fx = G.load(f"vae_{name}_drop")
    ds, model = _build_vae(name, 0.5)
    trainer = VAETrainer(ds, model, lr=1e-4)
    trainer.overlap_backward = overlap
    model.train()
    tok = torch.from_numpy(fx["tokens"]).cuda()
    monkeypatch.setattr(MV.random, "random", lambda: 0.0 if mode == "tf" else 0.9)
    queue = []
    for step in range(5):
        sm = G.vae_step_masks(fx, mode, step)
        flat = torch.cat([sm[k].reshape(-1) for k in ("enc", "beat", "tick")])
        queue.append(((flat.numel(),), sm["p"], flat))
    server = MaskServer(queue)
    monkeypatch.setattr(ops, "dropout_mask", server)
    seen = []
    model.register_forward_hook(lambda mod, args, out: seen.append(out))
    ref = fx[f"step_{mode}_losses"]
    for step in range(5):
        eps = torch.from_numpy(fx[f"step_{mode}_eps{step}"]).cuda()
        monkeypatch.setattr(torch, "randn", lambda *a, e=eps, **k: torch.stack([e, torch.zeros_like(e)]))
        trainer.zero_grad()
        loss, acc = trainer.loss_and_acc_for_batch(tok, 0, train=True)
        loss.backward()
        if step == 0:
            ops.side_join()
            torch.cuda.synchronize()
            w, s, _, _, z, _ = seen[0]
            ew, ez = G.rel_err(w.detach().cpu(), fx[f"step_{mode}_weights"]), G.rel_err(z.detach().cpu(), fx[f"step_{mode}_z"])
            errs = {k: _grad_err(model.param_grad(k).cpu().numpy(), fx, f"step_{mode}_", k) for k, _ in model.named_parameters()}
            worst = max(errs, key=errs.get)
            print(f"HIP model vae_{name}_drop {mode} overlap={overlap}: weights {ew:.2e} z {ez:.2e} worst gradient {worst} "
                  f"{errs[worst]:.2e}")
            assert ew < 1e-4 and ez < 1e-4
            ok = G.unique_rows(fx[f"step_{mode}_margin"])
            assert np.array_equal(s.cpu().numpy()[:, 0][ok], fx[f"step_{mode}_samples"][:, 0][ok])
            assert errs[worst] < 5e-4, sorted(errs.items(), key=lambda kv: -kv[1])[:5]
        trainer.step()
        el = abs(float(loss.detach()) - ref[step][0]) / abs(ref[step][0])
        print(f"HIP model vae_{name}_drop {mode} overlap={overlap} step {step}: loss {el:.2e} "
              f"accuracy {abs(float(acc.detach()) - ref[step][3]):.1e}")
        assert el <= 1e-4, (step, float(loss.detach()), ref[step][0])
        assert abs(float(acc.detach()) - ref[step][3]) < 1e-6
        if step in (0, 4):
            ops.side_join()
            for k, v in model.state_dict().items():
                pv = v.cpu().numpy()
                if name == "small":
                    assert np.abs(pv - fx[f"step_{mode}_after{step + 1}/{k}"]).max() < 1e-5, (k, step)
                else:
                    assert np.abs(pv.reshape(-1)[:64] - fx[f"step_{mode}_after{step + 1}/head/{k}"]).max() < 1e-5, (k, step)
    ops.side_defer(False)
    server.done()
    assert ops.chain_status() == 0


# ----------------------------------------------------------------------------------------------------------------------
# LatentRNN over the training-mode frozen VAE
# ----------------------------------------------------------------------------------------------------------------------
def _latent_inputs(name, variant):
    fx = G.load(f"latent_{name}_{variant}_drop")
    auto_reg, tf = variant.startswith("ar"), variant.endswith("tf")
    score = torch.from_numpy(fx["score"])
    n_past, n_target, n_future = [int(x) for x in fx["split"]]
    g = G.latent_mask_groups(fx, auto_reg, tf, score.shape[0], n_past, n_target, n_future)
    return fx, auto_reg, tf, score, (n_past, n_target, n_future), g


@pytest.mark.parametrize("variant", ["nar_fr", "ar_tf"])
def test_latent_kernels_with_reference_masks(variant):
    """The frozen encoder, the two context bi-GRUs, the generator bi-GRU (scalar x_0 input for the non-auto-regressive model) and the
    frozen decoder through the C-ABI, each under the reference's mask for that call (time-major as drawn): generated latents and
    logits against the fixture."""
    name = "small"
    fx, auto_reg, tf, score, (n_past, n_target, n_future), g = _latent_inputs(name, variant)
    c = G.CFGS[name]
    H, Z, B = c["H"], c["Z"], score.shape[0]
    P = G.latent_params(name, auto_reg)
    cfg = ops.vae_config(c["V"], c["E"], H, Z, H)
    vtable, vtotal = ops.vae_param_table(cfg)
    vparams = pack(vtable, vtotal, P, prefix="vae_model.")
    ltable, ltotal = ops.latent_param_table(LatentConfig(Z, H, int(auto_reg)))
    lparams = pack(ltable, ltotal, P)
    off = {n: o for n, o, _ in ltable}
    past, future, target = (t.to(DEV) for t in LatentRNNTrainer.split_score(score, n_past, n_future, n_target, 24))

    def encode(measures, eps_key, mask):
        rows = measures.reshape(-1, 24).contiguous()
        assert mask.shape == (24, rows.shape[0], 2 * H)
        mu, ls, _ = ops.encoder_fwd(cfg, rows, vparams, mask=mask.contiguous().to(DEV))
        z, _ = ops.reparam_kl(mu, ls, torch.from_numpy(fx[eps_key]).to(DEV))
        return z.view(B, -1, Z)
    zp, zf = encode(past, "eps_past", g["enc_past"]), encode(future, "eps_future", g["enc_future"])
    zt = encode(target, "eps_target", g["enc_target"])

    def bigru(prefix, x, x_scalar, h0, Hh, K, T, mask):
        assert mask.shape == (T, B, 2 * Hh)
        return ops.bigru2_fwd(x, x_scalar, lparams[off[prefix + ".weight_ih_l0"]:], Hh, B, T, K, h0=h0,
                              mask=mask.contiguous().to(DEV))
    _, cp, _ = bigru("context_rnn_past", zp.contiguous(), None, None, H, Z, n_past, g["ctx_past"])
    _, cf, _ = bigru("context_rnn_future", zf.contiguous(), None, None, H, Z, n_future, g["ctx_future"])
    ctx = torch.cat((cp, cf), 2).contiguous()
    if auto_reg:
        seed = torch.cat((zp[:, -1:], zt[:, :-1]), 1).contiguous()
        out, _, _ = bigru("generation_rnn", seed, None, ctx, 2 * H, Z, n_target, g["gen"])
    else:
        x0 = unpack(ltable, lparams, "x_0").reshape(1).contiguous()
        out, _, _ = bigru("generation_rnn", None, x0, ctx, 2 * H, 1, n_target, g["gen"])
    gz = ops.linear_fwd(out.reshape(B * n_target, 4 * H), unpack(ltable, lparams, "generation_linear.weight"),
                        unpack(ltable, lparams, "generation_linear.bias")).view(B, n_target, Z)
    # decoder rows ordered (sequence, measure), as the product decodes them: the per-measure masks interleaved accordingly
    mb = torch.stack([d["beat"] for d in g["dec"]], 2).reshape(4, B * n_target, H).contiguous().to(DEV)
    mt = torch.stack([d["tick"] for d in g["dec"]], 2).reshape(24, B * n_target, H).contiguous().to(DEV)
    w, s, _ = ops.decoder_fwd(cfg, gz.reshape(B * n_target, Z).contiguous(), None, False, vparams, mb, mt)
    w = w.view(B, n_target, 24, -1)
    egz, ew = relmax(gz, fx["gen_z"]), relmax(w, fx["weights"])
    print(f"HIP kernels latent_small_{variant}_drop: gen_z {egz:.2e} weights {ew:.2e}")
    assert egz < 2e-4
    assert ew < 2e-4
    ok = G.unique_rows(fx["margin"], 1e-3).reshape(B, -1)
    assert ok.mean() > 0.5
    assert np.array_equal(s.view(B, -1).cpu().numpy()[ok], fx["samples"][:, 0][ok])
    assert ops.chain_status() == 0


def _latent_queue(g, B, split, free_ar, encode_target, encode_last):
    """The reference's masks in the product's request order: ONE encoder mask (24, n*B, 2H) over all measures of a sequence that are
    read, rows ordered (sequence, measure) with measures past | target | future; the contexts; then
      not free-running AR: generator (nt, B, 4H); decoder beat (4, nt*B, H) and tick (24, nt*B, H), rows ordered (sequence, measure);
      free-running AR, per generated measure: generator (1, B, 4H); beat (4, B, H); tick (24, B, H); re-encoding (24, B, 2H).
    -> (queue, names of the recorded masks the product does not draw in this configuration)."""
    n_past, n_target, n_future = split
    p = g["p"]
    parts, unused = [("enc_past", n_past)], []
    if encode_target:
        parts.append(("enc_target", n_target))
    else:
        unused.append("enc_target")
    parts.append(("enc_future", n_future))
    enc = torch.cat([g[k].reshape(24, B, n, -1) for k, n in parts], 2)
    q = [((24, enc.shape[2] * B, enc.shape[3]), p, enc.reshape(24, enc.shape[2] * B, -1))]
    q += [(tuple(g[k].shape), p, g[k]) for k in ("ctx_past", "ctx_future")]
    if not free_ar:
        H = g["dec"][0]["beat"].shape[2]
        q.append((tuple(g["gen"].shape), p, g["gen"]))
        q.append(((4, n_target * B, H), p, torch.stack([d["beat"] for d in g["dec"]], 2).reshape(4, n_target * B, H)))
        q.append(((24, n_target * B, H), p, torch.stack([d["tick"] for d in g["dec"]], 2).reshape(24, n_target * B, H)))
    else:
        for i in range(n_target):
            q += [(tuple(m.shape), p, m) for m in (g["gen"][i], g["dec"][i]["beat"], g["dec"][i]["tick"])]
            if i + 1 < n_target or encode_last:
                q.append((tuple(g["enc_ar"][i].shape), p, g["enc_ar"][i]))
            else:
                unused.append("enc_ar[last]")
    return q, unused


def _latent_pass(name, variant, encode_all, monkeypatch, mutate=None):
    """Build LatentRNN over a VAE with dropout 0.5 (both in training mode), serve the fixture's masks -- `mutate`d first, for the
    controls -- and run forward.  -> everything the comparisons need."""
    fx, auto_reg, tf, score, split, g = _latent_inputs(name, variant)
    if mutate is not None:
        g = mutate(g)
    n_past, n_target, n_future = split
    free_ar = auto_reg and not tf
    c = G.CFGS[name]
    B = score.shape[0]
    ds = synthetic.SyntheticFolkDataset(num_notes=c["V"])
    vae = MV.MeasureVAE(ds, note_embedding_dim=c["E"], encoder_hidden_size=c["H"], latent_space_dim=c["Z"],
                        decoder_hidden_size=c["H"], encoder_dropout_prob=0.5, decoder_dropout_prob=0.5)
    model = LR.LatentRNN(ds, vae, num_rnn_layers=2, rnn_hidden_size=c["H"], dropout=0.5, rnn_class=torch.nn.GRU,
                         auto_reg=auto_reg, teacher_forcing=True)
    model.load_state_dict(G.latent_params(name, auto_reg))
    model.encode_unused_target = encode_all
    trainer = LatentRNNTrainer(ds, model, lr=1e-4)
    model.train()
    assert vae.training
    queue, unused = _latent_queue(g, B, split, free_ar, encode_target=encode_all or tf, encode_last=encode_all)
    assert unused == ([] if encode_all else ["enc_target"] + (["enc_ar[last]"] if free_ar else []))
    server = MaskServer(queue)
    monkeypatch.setattr(ops, "dropout_mask", server)
    monkeypatch.setattr(LR.random, "random", lambda: 0.0 if tf else 0.9)
    past, future, target = LatentRNNTrainer.split_score(score, n_past, n_future, n_target, 24)
    eps = tuple(torch.from_numpy(fx[k]).cuda() for k in ("eps_past", "eps_future", "eps_target"))
    eps_ar = [torch.from_numpy(fx[f"eps_ar{i}"]).cuda() for i in range(n_target)] if free_ar else None
    trainer.zero_grad()
    w, s, gz = model(past, future, target, n_target, train=True, eps=eps, eps_ar=eps_ar)
    server.done()
    return fx, free_ar, B, n_target, vae, model, trainer, target, w, s, gz


@pytest.mark.parametrize("what", ["re-encoding masks omitted", "first re-encoding mask batch-major",
                                  "generator masks of measures 1.. unscaled", "decoder tick masks of measures 1.. shifted"])
def test_latent_free_running_comparison_rejects_a_misplaced_mask(what, monkeypatch):
    """The control for the free-running cases below, on the HIP path: the server hands out ONE kind of mask of measures 1..3 wrong
    (measure 0 sees none of them and stays right).  The comparison the test below makes must then fail -- the first token difference
    is not a near-tie of the reference (comparable_ticks), or the comparable prefix is off by 100 tolerances."""
    def mutate(g):
        p = g["p"]
        if what == "re-encoding masks omitted":
            return dict(g, enc_ar=[G.mut_omit(m, p) for m in g["enc_ar"][:-1]] + g["enc_ar"][-1:])
        if what == "first re-encoding mask batch-major":
            return dict(g, enc_ar=[G.mut_batch_major(g["enc_ar"][0], p)] + g["enc_ar"][1:])
        if what == "generator masks of measures 1.. unscaled":
            return dict(g, gen=g["gen"][:1] + [G.mut_unscaled(m, p) for m in g["gen"][1:]])
        return dict(g, dec=g["dec"][:1] + [dict(d, tick=G.mut_shift(d["tick"], p)) for d in g["dec"][1:]])
    fx, free_ar, B, n_target, vae, model, trainer, target, w, s, gz = _latent_pass("small", "ar_fr", True, monkeypatch, mutate)
    assert G.rel_err(gz.detach().cpu()[:, 0], fx["gen_z"][:, 0]) < 2e-4                  # measure 0 alone notices nothing
    try:
        upto = G.comparable_ticks(s.cpu().numpy(), fx["samples"], fx["margin"], 1e-3)
    except AssertionError as e:
        print(f"HIP model latent_small_ar_fr_drop: {what}: rejected ({str(e)[:70]}...)")
        return
    ew, egz = G.prefix_errors(upto, w.detach().cpu(), fx["weights"], gz.detach().cpu(), fx["gen_z"])
    print(f"HIP model latent_small_ar_fr_drop: {what}: prefix errors weights {ew:.3f} gen_z {egz:.3f}")
    assert ew >= 100 * 2e-4 or egz >= 100 * 2e-4


@pytest.mark.parametrize("name,variant,encode_all", [("small", "nar_fr", True), ("small", "ar_tf", True), ("small", "ar_fr", True),
                                                     ("full", "ar_fr", True), ("small", "nar_fr", False), ("small", "ar_fr", False)])
def test_latent_rnn_step_with_reference_masks(name, variant, encode_all, monkeypatch):
    """LatentRNN.forward + LatentRNNTrainer step over a VAE built with dropout 0.5: LatentRNN.train() leaves the frozen VAE in training
    mode, so its encoder and decoder ask for masks too.  encode_all=True does the reference's work measure for measure
    (LatentRNN.encode_unused_target) and consumes every recorded mask; False is the product's default, which skips the two encodes
    nobody reads (the target's unless teacher-forced, the last generated measure's) -- exactly those masks stay behind."""
    fx, free_ar, B, n_target, vae, model, trainer, target, w, s, gz = _latent_pass(name, variant, encode_all, monkeypatch)
    # Everything is asserted.  On the free-running auto-regressive pass a sampled token is fed back (next tick, and through the
    # re-encoding the next measure): a sequence may leave the fixture's trajectory ONLY at a tick where the reference's own top two
    # logits are within the unique_rows floor (G.comparable_ticks asserts that of the first difference), and is compared up to there.
    sn = s.cpu().numpy()
    upto = G.comparable_ticks(sn, fx["samples"], fx["margin"], 1e-3) if free_ar else np.full(B, 24 * n_target)
    same_tokens = bool((upto == 24 * n_target).all())            # (comparable_ticks: then every token agrees)
    ew, egz = G.prefix_errors(upto, w.detach().cpu(), fx["weights"], gz.detach().cpu(), fx["gen_z"])
    print(f"HIP model latent_{name}_{variant}_drop encode_all={encode_all}: gen_z {egz:.2e} weights {ew:.2e} "
          f"comparable ticks per sequence {upto.tolist()} of {24 * n_target}")
    ok = G.unique_rows(fx["margin"], 1e-3).reshape(B, -1)
    assert ok.mean() > 0.5
    assert egz < 2e-4
    assert ew < 2e-4
    for b in range(B):
        n = int(upto[b])
        assert np.array_equal(sn[b, 0, :n][ok[b, :n]], fx["samples"][b, 0, :n][ok[b, :n]]), b
    loss, acc = trainer.mean_crossentropy_loss_and_accuracy(w, target)
    loss.backward()
    assert float(vae.grad.abs().max()) == 0.0                       # frozen VAE: no gradient reaches it
    if not same_tokens:
        print("a sequence left the fixture's trajectory at a near-tie: loss, gradients and the Adam step are not comparable")
    if same_tokens:                      # loss and gradients sum over every tick: comparable when no sequence left the trajectory
        errs = {}
        for k, _ in model.named_parameters():
            gk = model.param_grad(k).cpu().numpy()
            if name == "small":
                ref = fx["grad/" + k]
                errs[k] = float(np.abs(gk - ref).max() / (np.abs(ref).max() + 1e-7))
            else:
                rn = float(fx["gradnorm/" + k])
                errs[k] = abs(float(np.sqrt((gk.astype(np.float64) ** 2).sum())) - rn) / (rn + 1e-12)
        worst = max(errs, key=errs.get)
        el = abs(float(loss.detach()) - fx["loss_acc"][0]) / abs(fx["loss_acc"][0])
        print(f"HIP model latent_{name}_{variant}_drop encode_all={encode_all}: loss {el:.2e} worst gradient {worst} {errs[worst]:.2e}")
        assert el < 1e-4
        assert abs(float(acc) - fx["loss_acc"][1]) < 1e-6
        assert errs[worst] < 1e-3, sorted(errs.items(), key=lambda kv: -kv[1])[:5]
        trainer.step()
        for k, _ in model.named_parameters():
            v = model.param(k).cpu().numpy()
            if name == "small":
                assert np.abs(v - fx["after1/" + k]).max() < 1e-5, k
            else:
                assert np.abs(v.reshape(-1)[:64] - fx["after1head/" + k]).max() < 1e-5, k
    assert ops.chain_status() == 0


# ----------------------------------------------------------------------------------------------------------------------
# AnticipationRNN
# ----------------------------------------------------------------------------------------------------------------------
def _arnn_inputs(name):
    fx = G.load(f"arnn_{name}_drop")
    P = G.arnn_params_drop(name, fx)
    (tag, mask, p), = G.recorded_masks(fx)
    B, _, L = fx["score"].shape
    assert tag == "dropout_layer" and tuple(mask.shape) == (B, L, 1)
    return fx, P, mask[:, :, 0].t().contiguous(), p                      # the product scales time-major: (L, B)


@pytest.mark.parametrize("name", ["small", "full"])
def test_arnn_kernels_with_reference_mask(name):
    """Embedding (with the per-(tick, sequence) row scale that Dropout2d amounts to) + linear + LSTM entry points, forward, laid out as
    the reference's teacher-forced pass: backward constraint stack, forward generation stack WITHOUT anything between the layers
    (dropout_prob = 0.5 was set in the reference and does nothing there), the two-layer head."""
    fx, P, scale, p = _arnn_inputs(name)
    d = {k: v.to(DEV) for k, v in P.items()}
    score, md, loc = (torch.from_numpy(fx[k]).to(DEV) for k in ("score", "metadata", "constraints_loc"))
    B, _, L = score.shape
    V = d["note_embeddings.0.weight"].shape[0] - 1
    H = d["lstm_generation.0.weight_hh_l0"].shape[1]
    tok = score[:, 0].t().contiguous()                                                        # [L, B]
    md_tm = md[:, 0].permute(1, 0, 2)
    parts = [ops.embedding_fwd(d[f"metadata_embeddings.{i}.weight"], md_tm[..., i].contiguous().view(-1)) for i in range(3)]
    masked = (tok * loc[:, 0].t() + V * (1 - loc[:, 0].t())).contiguous()
    parts.append(ops.embedding_fwd(d["note_embeddings.0.weight"], masked.view(-1)))

    def stack(base, x, reverse):
        for l in range(2):
            gi = ops.linear_fwd(x.contiguous().view(L * B, -1), d[f"{base}.{l}.weight_ih_l0"], d[f"{base}.{l}.bias_ih_l0"])
            x = ops.lstm_fwd(gi.view(L, B, 4 * H), d[f"{base}.{l}.weight_hh_l0"], d[f"{base}.{l}.bias_hh_l0"], H, reverse=reverse)[0]
        return x
    oc = stack("lstm_constraint", torch.cat(parts, 1).view(L, B, -1), True)
    shifted = torch.cat((torch.zeros_like(tok[:1]), tok[:-1]), 0).contiguous()

    def logits(scale_lb):
        sc = scale_lb.to(DEV).clone()
        assert sc.shape == (L, B)
        sc[0] = 0.0                                                                          # the zero vector in front
        off = ops.embedding_fwd(d["note_embeddings.0.weight"], shifted.view(-1), sc.contiguous().view(-1)).view(L, B, -1)
        h = stack("lstm_generation", torch.cat((off, oc), 2), False)
        a = ops.linear_fwd(h.view(L * B, H), d["linear_1.weight"], d["linear_1.bias"], epi=2)
        return ops.linear_fwd(a, d["linear_ouput_notes.0.weight"], d["linear_ouput_notes.0.bias"]).view(L, B, -1).permute(1, 0, 2)
    w = logits(scale)
    ew = relmax(w, fx["tf_weights_all"])
    print(f"HIP kernels arnn_{name}_drop: weights {ew:.2e}")
    assert ew < 1e-4
    # the control: the mask wrong in one way at a time must move the kernels' logits by at least 100 tolerances
    wrong = {"input mask omitted": torch.ones_like(scale), "input mask unscaled": scale * (1.0 - p),
             "input mask read time-major": scale.t().reshape(L, B), "input mask one tick late": torch.roll(scale, 1, 0)}
    for what, m in wrong.items():
        moved = relmax(logits(m), fx["tf_weights_all"])
        print(f"HIP kernels arnn_{name}_drop: {what}: weights move by {moved:.3f}")
        assert moved >= 100 * 1e-4, what
    assert ops.chain_status() == 0


@pytest.mark.parametrize("name", ["small", "full"])
def test_arnn_trainer_step_with_reference_mask(name, monkeypatch):
    """ConstraintModelGaussianReg + AnticipationRNNGaussianRegTrainer, dropout_input_prob = 0.2 and dropout_prob = 0.5 as the fixture's
    reference model: the product asks for ONE (L, B) mask per pass (the reference draws (B, L): the server transposes)."""
    fx, P, scale, p = _arnn_inputs(name)
    c = G.ARNN_CFGS[name]
    ds = synthetic.SyntheticFolkDataset(num_notes=c["V"])
    ds.metadatas = [types.SimpleNamespace(num_values=6), types.SimpleNamespace(num_values=6)]
    model = ARNN.ConstraintModelGaussianReg(ds, note_embedding_dim=c["E"], metadata_embedding_dim=c["Em"],
                                            num_lstm_constraints_units=c["H"], num_lstm_generation_units=c["H"],
                                            linear_hidden_size=c["LH"], num_layers=2, dropout_input_prob=0.2,
                                            dropout_prob=0.5, unary_constraint=True, teacher_forcing=True)
    model.load_state_dict(P)
    trainer = ARNN.AnticipationRNNGaussianRegTrainer(ds, model, lr=1e-4)
    model.train()
    score, md, loc = (torch.from_numpy(fx[k]).cuda() for k in ("score", "metadata", "constraints_loc"))
    B, _, L = score.shape
    a, b = [int(x) for x in fx["ticks"]]
    server = MaskServer([((L, B), p, scale), ((L, B), p, scale)])
    monkeypatch.setattr(ops, "dropout_mask", server)
    monkeypatch.setattr(ARNN.random, "random", lambda: 0.0)                  # <= 0.5: teacher forcing
    with torch.no_grad():
        w_all, _ = model._forward_tf(score, md, loc)
    ew = G.rel_err(w_all[0].cpu(), fx["tf_weights_all"])
    trainer.zero_grad()
    loss, acc = trainer.loss_and_acc_for_batch((score, md, loc, a, b), 0, train=True)
    loss.backward()
    server.done()
    errs = {}
    for k, _ in model.named_parameters():
        gk = model.param_grad(k).cpu().numpy()
        if name == "small":
            key = "tf_grad/" + k
            ref = fx[key] if key in fx.files else np.zeros_like(gk)
            errs[k] = float(np.abs(gk - ref).max() / (np.abs(ref).max() + 1e-7))
        else:
            # as test_arnn_teacher_forced_step_golden: norm, first / last 64 elements against the tensor's own scale, signed sum
            key = "tf_gradnorm/" + k
            rn = float(fx[key]) if key in fx.files else 0.0
            flat = gk.reshape(-1).astype(np.float64)
            err = abs(float(np.sqrt((flat ** 2).sum())) - rn) / (rn + 1e-9)
            if key in fx.files:
                rms = rn / np.sqrt(flat.size) + 1e-12
                sc = max(float(np.abs(fx["tf_gradhead/" + k]).max()), float(np.abs(fx["tf_gradtail/" + k]).max()), rms)
                e_head = float(np.abs(flat[:64] - fx["tf_gradhead/" + k]).max()) / sc
                e_tail = float(np.abs(flat[-64:] - fx["tf_gradtail/" + k]).max()) / sc
                e_sum = abs(float(flat.sum()) - float(fx["tf_gradsum/" + k])) / (rn * np.sqrt(flat.size) + 1e-12)
                err = max(err, e_head, e_tail, e_sum)
            errs[k] = float(err)
    worst = max(errs, key=errs.get)
    el = abs(float(loss.detach()) - fx["tf_loss_acc"][0]) / abs(fx["tf_loss_acc"][0])
    print(f"HIP model arnn_{name}_drop: weights {ew:.2e} loss {el:.2e} worst gradient {worst} {errs[worst]:.2e}")
    assert ew < 1e-4
    assert el < 1e-4
    assert abs(float(acc) - fx["tf_loss_acc"][1]) < 1e-6
    assert errs[worst] < 1e-3, sorted(errs.items(), key=lambda kv: -kv[1])[:5]
    trainer.step()
    for k, _ in model.named_parameters():
        v = model.param(k).cpu().numpy()
        if name == "small":
            assert np.abs(v - fx["tf_after1/" + k]).max() < 1e-5, k
        else:
            assert np.abs(v.reshape(-1)[:64] - fx["tf_after1head/" + k]).max() < 1e-5, k
    assert ops.chain_status() == 0
