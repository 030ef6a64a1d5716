"""The CPU oracle (oracle/torch_ref.py) fed the masks the REFERENCE drew, against what the reference computed with them.

tests/golden/*_drop.npz hold the upstream models in train() with dropout on (0.5 in every GRU, the frozen VAE under
LatentRNN.train() included; Dropout2d(0.2) on the AnticipationRNN's inputs), every mask recorded in the reference's call order and
checked bit-exactly against the reference's own modules when the fixture was written (oracle/gen_golden.py, MaskRecorder).  The
HIP path was written against the oracle, so a mask the oracle misplaces would pass every HIP-vs-oracle test: this file is what
says the oracle places them as the reference does.

Tolerances are those of tests/test_oracle_golden.py for the same quantity at dropout 0.  Every placement is also pinned by a
mutation (one mask wrong at a time) that has to move the weights by at least 100 times the passing tolerance.
"""
import numpy as np
import pytest
import torch

from oracle import torch_ref as O
from tests import golden_util as G

torch.set_num_threads(4)

W_TOL_VAE, W_TOL_LATENT, W_TOL_ARNN = 5e-5, 1e-4, 5e-5      # tests/test_oracle_golden.py, weights at dropout 0
MOVE = 100.0


# ----------------------------------------------------------------------------------------------------------------------
# MeasureVAE
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small", "mid", "full"])
@pytest.mark.parametrize("mode", ["tf", "fr"])
def test_vae_train_steps_with_reference_masks(name, mode):
    """test_vae_train_steps of tests/test_oracle_golden.py, with fresh reference masks every step."""
    fx = G.load(f"vae_{name}_drop")
    P = G.vae_params(name)
    for p in P.values():
        p.requires_grad_(True)
    tok = torch.from_numpy(fx["tokens"])
    m = {k: torch.zeros_like(p) for k, p in P.items()}
    v = {k: torch.zeros_like(p) for k, p in P.items()}
    ref_losses = fx[f"step_{mode}_losses"]
    for step in range(5):
        eps = torch.from_numpy(fx[f"step_{mode}_eps{step}"])
        for p in P.values():
            p.grad = None
        masks = G.oracle_vae_masks(G.vae_step_masks(fx, mode, step))
        w, s, mu, ls, z = O.vae_forward(P, tok, eps, teacher_forced=(mode == "tf"), masks=masks)
        loss, ce, kl, acc = O.vae_loss(w, tok, mu, ls)
        loss.backward()
        got = np.array([loss.item(), ce.item(), kl.item(), acc.item()])
        assert np.allclose(got[:3], ref_losses[step][:3], rtol=2e-5, atol=1e-7), (step, got, ref_losses[step])
        if step == 0:
            ew, ez = G.rel_err(w.detach(), fx[f"step_{mode}_weights"]), G.rel_err(z.detach(), fx[f"step_{mode}_z"])
            print(f"vae_{name}_drop {mode}: weights {ew:.2e} z {ez:.2e}")
            assert ew < W_TOL_VAE
            assert ez < 5e-5
            ok = G.unique_rows(fx[f"step_{mode}_margin"])
            assert ok.mean() > 0.5
            assert np.array_equal(s.numpy()[:, 0][ok], fx[f"step_{mode}_samples"][:, 0][ok])
            assert abs(got[3] - ref_losses[0][3]) < 1e-6
            worst = 0.0
            for k, p in P.items():
                g = p.grad.numpy()
                if f"step_{mode}_grad/{k}" in fx.files:
                    ref = fx[f"step_{mode}_grad/{k}"]
                    worst = max(worst, np.abs(g - ref).max() / (np.abs(ref).max() + 1e-6))
                    assert np.abs(g - ref).max() <= 2e-4 * (np.abs(ref).max() + 1e-6), k
                else:
                    rn = fx[f"step_{mode}_gradnorm/{k}"]
                    gn = np.sqrt((g.astype(np.float64) ** 2).sum())
                    assert abs(gn - rn) <= 2e-4 * rn + 1e-9, k
                    ref = fx[f"step_{mode}_gradhead/{k}"]
                    got_h = g.reshape(-1)[:64]
                    worst = max(worst, np.abs(got_h - ref).max() / (np.abs(g).max() + 1e-9))
                    assert np.abs(got_h - ref).max() <= 2e-4 * (np.abs(g).max() + 1e-9), k
            print(f"vae_{name}_drop {mode}: worst gradient tensor {worst:.2e} of its max")
        with torch.no_grad():
            O.adam_step(P, {k: p.grad for k, p in P.items()}, m, v, step + 1)
        if step in (0, 4):
            for k, p in P.items():
                if name == "small":
                    ref = fx[f"step_{mode}_after{step + 1}/{k}"]
                    assert np.abs(p.detach().numpy() - ref).max() < 2e-6, (k, step)
                else:
                    ref = fx[f"step_{mode}_after{step + 1}/head/{k}"]
                    assert np.abs(p.detach().numpy().reshape(-1)[:64] - ref).max() < 5e-6, (k, step)


@pytest.mark.parametrize("name", ["small", "mid", "full"])
@pytest.mark.parametrize("mode", ["tf", "fr"])
def test_vae_every_mask_placement_is_observable(name, mode):
    fx = G.load(f"vae_{name}_drop")
    P = G.vae_params(name)
    tok = torch.from_numpy(fx["tokens"])
    eps = torch.from_numpy(fx[f"step_{mode}_eps0"])
    sm = G.vae_step_masks(fx, mode, 0)
    ref = fx[f"step_{mode}_weights"]
    with torch.no_grad():
        assert G.rel_err(O.vae_forward(P, tok, eps, mode == "tf", masks=G.oracle_vae_masks(sm))[0], ref) < W_TOL_VAE
        for what, mutate in G.VAE_MASK_MUTATIONS.items():
            w = O.vae_forward(P, tok, eps, mode == "tf", masks=G.oracle_vae_masks(mutate(sm)))[0]
            moved = G.rel_err(w, ref)
            print(f"vae_{name}_drop {mode}: {what}: weights move by {moved:.3f}")
            assert moved >= MOVE * W_TOL_VAE, f"mask placement not observable in vae_{name}_drop {mode}: {what} ({moved:.2e})"


# ----------------------------------------------------------------------------------------------------------------------
# LatentRNN over the training-mode frozen VAE
# ----------------------------------------------------------------------------------------------------------------------
LATENT = [("small", "nar_fr"), ("small", "ar_tf"), ("small", "ar_fr"), ("full", "ar_fr")]


def _latent_case(name, variant):
    fx = G.load(f"latent_{name}_{variant}_drop")
    auto_reg, tf = variant.startswith("ar"), variant.endswith("tf")
    P = G.latent_params(name, auto_reg)
    score = torch.from_numpy(fx["score"])
    n_past, n_target, n_future = [int(x) for x in fx["split"]]
    past, future, target = O.split_score(score, n_past, n_future, n_target)
    eps_ar = [torch.from_numpy(fx[f"eps_ar{i}"]) for i in range(n_target)] if auto_reg and not tf else None
    groups = G.latent_mask_groups(fx, auto_reg, tf, score.shape[0], n_past, n_target, n_future)

    def forward(g):
        return O.latent_forward(P, past, future, target, torch.from_numpy(fx["eps_past"]),
                                torch.from_numpy(fx["eps_future"]), torch.from_numpy(fx["eps_target"]), auto_reg=auto_reg,
                                teacher_forcing=tf, eps_ar=eps_ar, masks=G.oracle_latent_masks(g))
    return fx, P, target, groups, forward, auto_reg, tf


@pytest.mark.parametrize("name,variant", LATENT)
def test_latent_rnn_with_reference_masks(name, variant):
    """test_latent_rnn of tests/test_oracle_golden.py with the reference's masks, the frozen VAE's included."""
    fx, P, target, groups, forward, auto_reg, tf = _latent_case(name, variant)
    train_keys = [k for k in P if not k.startswith("vae_model.")]
    for k in train_keys:
        P[k].requires_grad_(True)
    w, s, gz = forward(groups)
    B, nt = target.shape[:2]
    free_ar = auto_reg and not tf
    # free-running AR feeds sampled tokens back through the encoder: a sequence may leave the fixture's trajectory only at a tick
    # where the reference's own top two logits are within the unique_rows floor (asserted), and is compared up to there
    upto = G.comparable_ticks(s.numpy(), fx["samples"], fx["margin"], 1e-3) if free_ar else np.full(B, 24 * nt)
    same = bool((upto == 24 * nt).all())
    ew, egz = G.prefix_errors(upto, w.detach(), fx["weights"], gz.detach(), fx["gen_z"])
    print(f"latent_{name}_{variant}_drop: gen_z {egz:.2e} weights {ew:.2e} comparable ticks per sequence {upto.tolist()}")
    assert egz < 1e-4
    assert ew < W_TOL_LATENT
    ok = G.unique_rows(fx["margin"], 1e-3).reshape(s.shape[0], -1)
    assert ok.mean() > 0.5
    for b in range(B):
        n = int(upto[b])
        assert np.array_equal(s.numpy()[b, 0, :n][ok[b, :n]], fx["samples"][b, 0, :n][ok[b, :n]]), b
    loss, acc = O.latent_loss(w, target)
    loss.backward()
    if same:                                  # loss and gradients sum over every tick
        assert abs(loss.item() - fx["loss_acc"][0]) < 2e-5 * abs(fx["loss_acc"][0])
        assert abs(acc.item() - fx["loss_acc"][1]) < 1e-6
        worst = 0.0
        for k in train_keys:
            g = P[k].grad.numpy()
            if name == "small":
                ref = fx["grad/" + k]
                worst = max(worst, np.abs(g - ref).max() / (np.abs(ref).max() + 1e-7))
                assert np.abs(g - ref).max() <= 5e-4 * (np.abs(ref).max() + 1e-7), k
            else:
                rn = fx["gradnorm/" + k]
                gn = np.sqrt((g.astype(np.float64) ** 2).sum())
                worst = max(worst, abs(gn - rn) / rn)
                assert abs(gn - rn) <= 5e-4 * rn + 1e-9, k
        print(f"latent_{name}_{variant}_drop: samples equal, worst gradient tensor {worst:.2e}")
        m = {k: torch.zeros_like(P[k]) for k in train_keys}
        v = {k: torch.zeros_like(P[k]) for k in train_keys}
        own = {k: P[k] for k in train_keys}
        with torch.no_grad():
            O.adam_step(own, {k: P[k].grad for k in train_keys}, m, v, 1)
        for k in train_keys:
            if name == "small":
                assert np.abs(P[k].detach().numpy() - fx["after1/" + k]).max() < 2e-6, k
            else:
                assert np.abs(P[k].detach().numpy().reshape(-1)[:64] - fx["after1head/" + k]).max() < 5e-6, k
    for k in P:
        if k.startswith("vae_model."):
            assert P[k].grad is None


def _each(g, key, f):
    """Mutation f on the mask (or on every mask of the list) g[key]."""
    m = g[key]
    return dict(g, **{key: [f(x, g["p"]) for x in m] if isinstance(m, list) else f(m, g["p"])})


def _dec(g, part, f):
    return dict(g, dec=[dict(d, **{part: f(d[part], g["p"])}) for d in g["dec"]])


def _latent_mutations(free_ar):
    M = {}
    for key in ("ctx_past", "ctx_future"):
        M[f"{key} omitted"] = lambda g, key=key: _each(g, key, G.mut_omit)
        M[f"{key} batch-major"] = lambda g, key=key: _each(g, key, G.mut_batch_major)
        M[f"{key} unscaled"] = lambda g, key=key: _each(g, key, G.mut_unscaled)
    M["gen omitted"] = lambda g: _each(g, "gen", G.mut_omit)
    M["gen unscaled"] = lambda g: _each(g, "gen", G.mut_unscaled)
    if not free_ar:                                        # the free-running path draws (1, B, 4H) per measure: no other order
        M["gen batch-major"] = lambda g: _each(g, "gen", G.mut_batch_major)
    # LatentRNN.train() leaves the frozen VAE in training mode: its encoder and decoder drop too
    M["frozen encoder omitted"] = lambda g: _each(_each(_each(g, "enc_past", G.mut_omit), "enc_future", G.mut_omit),
                                                 "enc_target", G.mut_omit)
    for key in ("enc_past", "enc_future"):
        M[f"{key} omitted"] = lambda g, key=key: _each(g, key, G.mut_omit)
        M[f"{key} batch-major"] = lambda g, key=key: _each(g, key, G.mut_batch_major)
        M[f"{key} unscaled"] = lambda g, key=key: _each(g, key, G.mut_unscaled)
    M["frozen decoder omitted"] = lambda g: _dec(_dec(g, "beat", G.mut_omit), "tick", G.mut_omit)
    M["frozen decoder beat omitted"] = lambda g: _dec(g, "beat", G.mut_omit)
    M["frozen decoder beat batch-major"] = lambda g: _dec(g, "beat", G.mut_batch_major)
    M["frozen decoder tick omitted"] = lambda g: _dec(g, "tick", G.mut_omit)
    M["frozen decoder tick unscaled"] = lambda g: _dec(g, "tick", G.mut_unscaled)
    M["frozen decoder tick shifted by one"] = lambda g: _dec(g, "tick", G.mut_shift)
    if free_ar:
        # the re-encoding of the LAST generated measure is drawn but its z is never read: not observable, left out on purpose
        M["re-encoding masks omitted"] = lambda g: dict(g, enc_ar=[G.mut_omit(m, g["p"]) for m in g["enc_ar"][:-1]]
                                                        + g["enc_ar"][-1:])
        M["first re-encoding mask batch-major"] = lambda g: dict(g, enc_ar=[G.mut_batch_major(g["enc_ar"][0], g["p"])]
                                                                 + g["enc_ar"][1:])
    return M


@pytest.mark.parametrize("name,variant", LATENT)
def test_latent_every_mask_placement_is_observable(name, variant):
    """One mask wrong at a time.  enc_target is observable only where the target's z is read (teacher-forced AR); elsewhere it
    is covered by 'frozen encoder omitted' through the past / future contexts."""
    fx, P, target, groups, forward, auto_reg, tf = _latent_case(name, variant)
    ref = fx["weights"]
    M = _latent_mutations(auto_reg and not tf)
    if auto_reg and tf:
        M["enc_target omitted"] = lambda g: _each(g, "enc_target", G.mut_omit)
        M["enc_target batch-major"] = lambda g: _each(g, "enc_target", G.mut_batch_major)
    with torch.no_grad():
        assert G.rel_err(forward(groups)[0], ref) < W_TOL_LATENT
        for what, mutate in M.items():
            moved = G.rel_err(forward(mutate(groups))[0], ref)
            print(f"latent_{name}_{variant}_drop: {what}: weights move by {moved:.3f}")
            assert moved >= MOVE * W_TOL_LATENT, \
                f"mask placement not observable in latent_{name}_{variant}_drop: {what} ({moved:.2e})"
        if auto_reg and not tf:
            last = dict(groups, enc_ar=groups["enc_ar"][:-1] + [G.mut_omit(groups["enc_ar"][-1], groups["p"])])
            assert G.rel_err(forward(last)[0], ref) < W_TOL_LATENT          # ... and indeed nobody reads it


@pytest.mark.parametrize("name", ["small", "full"])
def test_free_running_comparison_does_not_excuse_a_misplaced_mask(name):
    """The free-running AR comparison stops a sequence at its first token difference -- which a misplaced mask also produces.  It
    must not pass that way: with any mask of measures 1..3 wrong (generator, decoder, re-encoding; measure 0's are right, so a check
    of measure 0 alone would pass), either the first token difference is not a near-tie of the reference (comparable_ticks fails) or
    the comparable prefix is off by more than the tolerance."""
    fx, P, target, groups, forward, auto_reg, tf = _latent_case(name, "ar_fr")
    p = groups["p"]
    later = {
        "re-encoding masks omitted": dict(groups, enc_ar=[G.mut_omit(m, p) for m in groups["enc_ar"][:-1]] + groups["enc_ar"][-1:]),
        "first re-encoding mask batch-major": dict(groups, enc_ar=[G.mut_batch_major(groups["enc_ar"][0], p)] + groups["enc_ar"][1:]),
        "generator masks of measures 1.. unscaled": dict(groups, gen=groups["gen"][:1] + [G.mut_unscaled(m, p) for m in groups["gen"][1:]]),
        "decoder tick masks of measures 1.. shifted": dict(groups, dec=groups["dec"][:1] + [dict(d, tick=G.mut_shift(d["tick"], p))
                                                                                          for d in groups["dec"][1:]]),
    }
    with torch.no_grad():
        for what, g in later.items():
            w, s, gz = forward(g)
            assert G.rel_err(gz[:, 0], fx["gen_z"][:, 0]) < 1e-4              # measure 0 alone sees nothing
            try:
                upto = G.comparable_ticks(s.numpy(), fx["samples"], fx["margin"], 1e-3)
            except AssertionError as e:
                print(f"latent_{name}_ar_fr_drop: {what}: rejected ({str(e)[:70]}...)")
                continue
            ew, egz = G.prefix_errors(upto, w, fx["weights"], gz, fx["gen_z"])
            print(f"latent_{name}_ar_fr_drop: {what}: prefix errors weights {ew:.3f} gen_z {egz:.3f}")
            assert ew >= MOVE * W_TOL_LATENT or egz >= MOVE * 1e-4, what


# ----------------------------------------------------------------------------------------------------------------------
# AnticipationRNN
# ----------------------------------------------------------------------------------------------------------------------
def _arnn_case(name):
    fx = G.load(f"arnn_{name}_drop")
    P = G.arnn_params_drop(name, fx)
    (tag, mask, p), = G.recorded_masks(fx)
    assert tag == "dropout_layer" and p == 0.2 and tuple(mask.shape) == tuple(fx["score"].shape[::2]) + (1,)
    return fx, P, mask, p


@pytest.mark.parametrize("name", ["small", "full"])
def test_arnn_teacher_forced_step_with_reference_mask(name):
    """Dropout2d(0.2) on the shifted note embeddings: one keep flag per (sequence, tick), batch-major.  dropout_prob = 0.5 was
    set when the fixture was captured and does nothing in the reference (one-layer LSTMs, no dropout layer between them): the
    oracle reproduces the outputs without any mask between the LSTM layers."""
    fx, P, mask, p = _arnn_case(name)
    for q in P.values():
        q.requires_grad_(True)
    score, md, loc = (torch.from_numpy(fx[k]) for k in ("score", "metadata", "constraints_loc"))
    a, b = [int(x) for x in fx["ticks"]]
    w_all, _ = O.arnn_forward(P, score, md, loc, teacher_forcing=True, input_mask=mask)
    ew = G.rel_err(w_all.detach(), fx["tf_weights_all"])
    print(f"arnn_{name}_drop: weights {ew:.2e}")
    assert ew < W_TOL_ARNN
    loss, acc = O.arnn_loss(w_all[:, a:b], score[:, 0, a:b])
    assert abs(loss.item() - fx["tf_loss_acc"][0]) < 2e-5 * abs(fx["tf_loss_acc"][0])
    assert abs(acc.item() - fx["tf_loss_acc"][1]) < 1e-6
    loss.backward()
    m = {k: torch.zeros_like(q) for k, q in P.items()}
    v = {k: torch.zeros_like(q) for k, q in P.items()}
    seen, worst = 0, 0.0
    for k, q in P.items():
        g = q.grad.numpy() if q.grad is not None else np.zeros(q.shape, dtype=np.float32)
        if name == "small":
            key = "tf_grad/" + k
            if key in fx.files:
                ref = fx[key]
                seen += 1
                worst = max(worst, np.abs(g - ref).max() / (np.abs(ref).max() + 1e-7))
                assert np.abs(g - ref).max() <= 5e-4 * (np.abs(ref).max() + 1e-7), k
        else:
            key = "tf_gradnorm/" + k
            if key in fx.files:
                rn = float(fx[key])
                seen += 1
                gn = float(np.sqrt((g.astype(np.float64) ** 2).sum()))
                worst = max(worst, abs(gn - rn) / (rn + 1e-30))
                assert abs(gn - rn) <= 5e-4 * rn + 1e-9, k
    assert seen >= 20
    print(f"arnn_{name}_drop: worst gradient tensor {worst:.2e}")
    with torch.no_grad():
        O.adam_step(P, {k: (q.grad if q.grad is not None else torch.zeros_like(q)) for k, q in P.items()}, m, v, 1)
    for k, q in P.items():
        if name == "small":
            assert np.abs(q.detach().numpy() - fx["tf_after1/" + k]).max() < 2e-6, k
        else:
            assert np.abs(q.detach().numpy().reshape(-1)[:64] - fx["tf_after1head/" + k]).max() < 5e-6, k


@pytest.mark.parametrize("name", ["small", "full"])
def test_arnn_input_mask_placement_is_observable(name):
    fx, P, mask, p = _arnn_case(name)
    score, md, loc = (torch.from_numpy(fx[k]) for k in ("score", "metadata", "constraints_loc"))
    B, L = mask.shape[:2]
    ref = fx["tf_weights_all"]
    mutations = {
        "input mask omitted": torch.ones_like(mask),
        "input mask unscaled": mask * (1.0 - p),
        "input mask time-major": mask.reshape(L, B, 1).transpose(0, 1).contiguous(),     # the draw read as (L, B)
        "input mask one tick late": torch.roll(mask, 1, 1),
    }
    with torch.no_grad():
        for what, mm in mutations.items():
            moved = G.rel_err(O.arnn_forward(P, score, md, loc, teacher_forcing=True, input_mask=mm)[0], ref)
            print(f"arnn_{name}_drop: {what}: weights move by {moved:.3f}")
            assert moved >= MOVE * W_TOL_ARNN, f"mask placement not observable in arnn_{name}_drop: {what} ({moved:.2e})"


# ----------------------------------------------------------------------------------------------------------------------
# The masks themselves
# ----------------------------------------------------------------------------------------------------------------------
DROP_FIXTURES = ([(f"vae_{n}_drop", pre) for n in ("small", "mid", "full") for pre in ("step_tf_", "step_fr_")]
                 + [(f"latent_{n}_{v}_drop", "") for n, v in LATENT] + [("arnn_small_drop", ""), ("arnn_full_drop", "")])


@pytest.mark.parametrize("fixture,prefix", DROP_FIXTURES)
def test_recorded_masks_are_bernoulli_keep_flags(fixture, prefix):
    """Per module tag the pooled keep rate lies within four binomial standard deviations of 1 - p; values are 0 or 1/(1-p)."""
    pooled = {}
    for tag, m, p in G.recorded_masks(G.load(fixture), prefix):
        vals = torch.unique(m)
        assert all(float(x) in (0.0, float(np.float32(1.0) / np.float32(1.0 - p))) for x in vals), (tag, vals)
        n, kept, p0 = pooled.get(tag, (0, 0, p))
        assert p0 == p
        pooled[tag] = (n + m.numel(), kept + int((m != 0).sum()), p)
    assert pooled
    for tag, (n, kept, p) in pooled.items():
        sd = np.sqrt(p * (1 - p) / n)
        print(f"{fixture} {prefix}{tag}: {n} flags, keep rate {kept / n:.4f} (1 - p = {1 - p}, 4 sd = {4 * sd:.4f})")
        assert abs(kept / n - (1 - p)) <= 4 * sd, (tag, kept / n)
