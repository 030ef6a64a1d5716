"""The class-weighted, label-smoothed cross-entropy at the trainers' level: the three trainers' keywords
ce_weight / label_smoothing / ignore_index, _ElboWFn against the unfused expression, the defaults, the testers' class_report and the
training state -- on the small models of tests/test_gpu_mmd_trainer.py (MeasureVAE, B = 8), tests/test_gpu_latent.py and
tests/test_gpu_arnn.py (their "small" golden configurations).

A step's loss is compared with torch.nn.functional.cross_entropy in float64 ON THE STEP'S OWN LOGITS within the project's 1e-4
relative; gradient tensors of the fused and the unfused step within 5e-4 of their largest element, the bound tests/test_gpu_mmd_trainer.py
and tests/test_gpu_kl_schedule.py hold two steps over the same weights to; every integer of a report exactly."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import ce_w_ref as R
from tests import golden_util as G

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from inpaintnet_amd import ops, synthetic
    from inpaintnet_amd.latent_rnn_tester import LatentRNNTester
    from inpaintnet_amd.latent_rnn_trainer import LatentRNNTrainer
    from inpaintnet_amd.vae_tester import VAETester
    from inpaintnet_amd.vae_trainer import VAETrainer
    from tests.test_gpu_mmd_trainer import B, CFG, GRAD_TOL, LOSS_TOL, _np64, _step, _vae

CE_LABELS = ("class_counts", "cross_entropy_w", "cross_entropy_w_grad")
SMOOTH, IGN = 0.1, -100


def _cw(V):
    """Deterministic class weights with a zero, a heavy class and the rest near 1."""
    w = 0.5 + (torch.arange(V, dtype=torch.float32) * 0.37) % 1.0
    w[1] = 0.0
    w[V - 1] = 3.0
    return w


def _kw(V):
    return dict(ce_weight=_cw(V), label_smoothing=SMOOTH, ignore_index=IGN)


def _torch_ce(logits, targets, V):
    return float(F.cross_entropy(logits.detach().double().cpu().reshape(-1, V), targets.cpu().reshape(-1).long(), weight=_cw(V).double(),
                                 label_smoothing=SMOOTH, ignore_index=IGN))


def _record(model):
    """model.forward recorded: every call's (args, kwargs, outputs) is appended to the list returned."""
    seen, inner = [], model.forward

    def forward(*a, **k):
        out = inner(*a, **k)
        seen.append((a, k, out))
        return out
    model.forward = forward
    return seen


def _assert_last_ce(last, logits, targets, V):
    """last_ce against the restatement on the step's own logits: exact integers, denom to 1e-6."""
    assert set(last) == {"denom", "n_valid", "class_stats"} and all(t.is_cuda for t in last.values())
    assert last["denom"].dtype == torch.float64 and last["class_stats"].shape == (V, 3) and last["class_stats"].dtype == torch.int64
    e = R.evaluate(logits.detach().double().cpu().reshape(-1, V).numpy(), targets.cpu().reshape(-1).numpy(), _cw(V).numpy(), SMOOTH, IGN)
    assert int(last["n_valid"]) == e["n_valid"] and abs(float(last["denom"]) - e["denom"]) <= 1e-6 * e["denom"]
    assert np.array_equal(last["class_stats"].cpu().numpy(), e["stats"])
    return e


# =============================================================================== 1. one step of each trainer
def test_vae_step_is_torchs_weighted_cross_entropy_plus_the_kl_term():
    V = CFG["V"]
    _, model, trainer = _vae(**_kw(V))
    m = _step(trainer, model)
    weights, z_dist = m["out"][0], m["out"][2]
    from tests.test_gpu_mmd_trainer import _tokens
    ce = _torch_ce(weights, _tokens(), V)
    mu, ls = _np64(z_dist.loc), _np64(z_dist.log_scale)
    kl = float((0.5 * (np.exp(2.0 * ls) + mu * mu - 1.0) - ls).sum())
    want = ce + trainer.kl_beta / B * kl
    plain = float(F.cross_entropy(weights.detach().double().cpu().reshape(-1, V), _tokens().cpu().reshape(-1)))
    print(f"loss {float(m['loss']):.7f} = CE {ce:.7f} + KL term {trainer.kl_beta / B * kl:.7f} (plain CE {plain:.7f})")
    assert abs(float(m["loss"]) - want) <= LOSS_TOL * abs(want)
    # an untrained model's logits are nearly flat, so the settings move the loss little -- still ten tolerances, enough to tell the
    # weighted loss from the plain one
    assert abs(ce - plain) >= 10.0 * LOSS_TOL * abs(want)
    e = _assert_last_ce(trainer.last_ce, weights, _tokens(), V)
    assert e["stats"][:, 0].sum() == B * 24
    assert [l for l in m["labels"] if l in CE_LABELS] == ["class_counts", "cross_entropy_w", "cross_entropy_w_grad"]
    assert "cross_entropy" not in m["labels"]
    # validation uses the settings too, and launches no gradient
    v = _step(trainer, model, train=False)
    assert abs(float(v["loss"]) - (_torch_ce(v["out"][0], _tokens(), V) + trainer.kl_beta / B *
                                   float((0.5 * (np.exp(2.0 * _np64(v["out"][2].log_scale)) + _np64(v["out"][2].loc) ** 2 - 1.0)
                                          - _np64(v["out"][2].log_scale)).sum()))) <= LOSS_TOL * abs(float(v["loss"]))
    assert [l for l in v["labels"] if l in CE_LABELS] == ["class_counts", "cross_entropy_w"]


def test_latent_rnn_step_is_torchs_weighted_cross_entropy():
    from tests.test_gpu_latent import build
    V = G.CFGS["small"]["V"]
    fx = G.load("latent_small_nar_fr")
    ds, _, model = build("small", False)
    trainer = LatentRNNTrainer(ds, model, lr=1e-4, **_kw(V))
    model.train()
    n_past, n_target, n_future = [int(x) for x in fx["split"]]
    assert n_past + n_target + n_future == ds.n_bars
    batch = LatentRNNTrainer.split_score(torch.from_numpy(fx["score"]), n_past, n_future, n_target, 24)
    seen = _record(model)
    trainer.zero_grad()
    loss, acc = trainer.loss_and_acc_for_batch(batch, 0, train=True)
    loss.backward()
    ops.side_join()
    torch.cuda.synchronize()
    w, target = seen[0][2][0], batch[2]
    want = _torch_ce(w, target, V)
    print(f"latent: loss {float(loss):.7f} torch {want:.7f}")
    assert abs(float(loss) - want) <= 1e-4 * abs(want)
    e = _assert_last_ce(trainer.last_ce, w, target, V)
    assert abs(float(acc) - e["accuracy"]) <= 1e-6
    assert float(model.grad.abs().max()) > 0.0 and bool(torch.isfinite(model.grad).all())
    with torch.no_grad():
        vloss, _ = trainer.loss_and_acc_for_batch(batch, 0, train=False)
    assert abs(float(vloss) - _torch_ce(seen[1][2][0], target, V)) <= 1e-4 * abs(float(vloss))


def test_arnn_step_is_torchs_weighted_cross_entropy_per_voice():
    from inpaintnet_amd.arnn import AnticipationRNNGaussianRegTrainer
    from tests.test_gpu_arnn import build
    V = G.ARNN_CFGS["small"]["V"]
    fx = G.load("arnn_small")
    ds, model = build("small")
    trainer = AnticipationRNNGaussianRegTrainer(ds, model, lr=1e-4, **_kw(V))
    model.train()
    score, md, loc = (torch.from_numpy(fx[k]).cuda() for k in ("score", "metadata", "constraints_loc"))
    a, b = [int(x) for x in fx["ticks"]]
    seen = _record(model)
    trainer.zero_grad()
    loss, acc = trainer.loss_and_acc_for_batch((score, md, loc, a, b), 0, train=True)
    loss.backward()
    ops.side_join()
    torch.cuda.synchronize()
    weights = seen[0][2][0]
    from inpaintnet_amd.arnn import free_positions
    targets = score[:, :, free_positions(loc)].transpose(0, 1)
    want = sum(_torch_ce(w, targets[i], V) for i, w in enumerate(weights)) / len(weights)
    print(f"arnn: loss {float(loss):.7f} torch {want:.7f} over {len(weights)} voice(s)")
    assert abs(float(loss) - want) <= 1e-4 * abs(want)
    if len(weights) == 1:
        _assert_last_ce(trainer.last_ce, weights[0], targets[0], V)
    assert float(model.grad.abs().max()) > 0.0 and bool(torch.isfinite(model.grad).all())


# =============================================================================== 2. fused against unfused
def test_fused_elbo_gradients_equal_the_unfused_expression():
    """_ElboWFn against mean_crossentropy_loss_and_accuracy(..., weight=...) + compute_kld_loss: a subclass that overrides
    compute_kld_loss (with the same code) takes VAETrainer's unfused branch."""
    V = CFG["V"]

    class Unfused(VAETrainer):
        @staticmethod
        def compute_kld_loss(z_dist, prior_dist, beta=0.001):
            return VAETrainer.compute_kld_loss(z_dist, prior_dist, beta)

    _, mf, tf = _vae(**_kw(V))
    ds, mu, _ = _vae()
    tu = Unfused(ds, mu, lr=1e-3, **_kw(V))
    f, u = _step(tf, mf), _step(tu, mu)
    assert "cross_entropy_w" in u["labels"] and "cross_entropy_w_grad" in u["labels"]
    assert abs(float(f["loss"]) - float(u["loss"])) <= LOSS_TOL * abs(float(u["loss"]))
    assert np.array_equal(tf.last_ce["class_stats"].cpu().numpy(), tu.last_ce["class_stats"].cpu().numpy())
    worst = 0.0
    for k in u["grads"]:
        scale = float(u["grads"][k].abs().max())
        d = float((f["grads"][k] - u["grads"][k]).abs().max())
        worst = max(worst, d / (scale + 1e-30))
        assert d <= GRAD_TOL * scale + 1e-12, k
    print(f"fused vs unfused: worst gradient tensor differs by {worst:.2e} of its largest element")
    for name in ("dmu", "dls"):
        assert float((f[name] - u[name]).abs().max()) <= GRAD_TOL * float(u[name].abs().max()), name


# =============================================================================== 3. the defaults
def test_defaults_are_the_trainer_as_it_was(monkeypatch):
    """With the defaults last_ce stays None, the launches recorded are the default trainer's, and the weighted code is never reached
    (checked the way tests/test_gpu_attr_trainer.py checks attr_reg=None)."""
    from inpaintnet_amd import trainer as T

    def boom(*a, **k):
        raise AssertionError("a trainer with the default settings reached the weighted cross-entropy")
    _, m1, t1 = _vae()
    d1 = _step(t1, m1)
    _, m0, t0 = _vae(ce_weight=None, label_smoothing=0.0, ignore_index=None)
    monkeypatch.setattr(ops, "class_counts", boom)
    monkeypatch.setattr(ops, "cross_entropy_w", boom)
    monkeypatch.setattr(T._ElboWFn, "forward", staticmethod(boom))
    monkeypatch.setattr(T._CrossEntropyWFn, "forward", staticmethod(boom))
    z = _step(t0, m0)
    zv = _step(t0, m0, train=False)
    assert t0.last_ce is None and t1.last_ce is None
    assert not [l for l in z["labels"] + zv["labels"] if l in CE_LABELS]
    assert z["labels"] == d1["labels"]
    assert abs(float(z["loss"]) - float(d1["loss"])) <= LOSS_TOL * abs(float(d1["loss"]))
    for k in d1["grads"]:
        assert float((z["grads"][k] - d1["grads"][k]).abs().max()) <= GRAD_TOL * float(d1["grads"][k].abs().max()) + 1e-12, k
    w = torch.randn(4, 24, CFG["V"], device="cuda", requires_grad=True)
    t = torch.randint(0, CFG["V"], (4, 24), device="cuda")
    loss, _ = T.Trainer.mean_crossentropy_loss_and_accuracy(w, t)               # two arguments: the plain path
    loss.backward()
    assert abs(float(loss) - float(F.cross_entropy(w.detach().double().cpu().view(-1, CFG["V"]), t.cpu().view(-1)))) <= 1e-4 * float(loss)


def test_static_method_with_options_is_torchs_and_differentiable():
    V = CFG["V"]
    g = torch.Generator().manual_seed(5)
    w = torch.relu(torch.randn(6, 24, V, generator=g)).cuda().requires_grad_(True)
    t = torch.randint(0, V, (6, 24), generator=g)
    t[0, :5] = 7                                                                 # ignore_index inside the vocabulary: legal here
    from inpaintnet_amd.trainer import Trainer
    loss, acc = Trainer.mean_crossentropy_loss_and_accuracy(w, t.cuda(), weight=_cw(V).tolist(), label_smoothing=0.25, ignore_index=7)
    (loss * 3.0).backward()
    w64 = w.detach().double().cpu().requires_grad_(True)
    want = F.cross_entropy(w64.view(-1, V), t.view(-1), weight=_cw(V).double(), label_smoothing=0.25, ignore_index=7)
    (want * 3.0).backward()
    assert abs(float(loss) - float(want.detach())) <= 1e-4 * abs(float(want.detach()))
    assert float((w.grad.double().cpu() - w64.grad).abs().max()) <= 1e-5 * float(w64.grad.abs().max())
    e = R.evaluate(w64.detach().view(-1, V).numpy(), t.view(-1).numpy(), _cw(V).numpy(), 0.25, 7)
    assert abs(float(acc) - e["accuracy"]) <= 1e-6 and not w.grad[0, :5].any()


# =============================================================================== 4. the testers' report, the class counts
def _assert_report(rep, stats, conf):
    want = R.report(stats, conf)
    for k in ("counts", "hits", "predicted", "confusion"):
        assert rep[k].dtype == np.int64 and np.array_equal(rep[k], want[k]), k
    for k in ("recall", "precision", "f1"):
        assert np.array_equal(rep[k], want[k], equal_nan=True), k
    assert rep["accuracy"] == want["accuracy"] and rep["balanced_accuracy"] == want["balanced_accuracy"]


def test_vae_class_report_equals_the_restatement_on_its_own_logits():
    V = CFG["V"]
    ds, model, trainer = _vae()
    tester = VAETester(ds, model)
    tok = torch.from_numpy(synthetic.det_tokens("ce_w/report", (21, 24), V))
    loader = [(tok[:13], None), (tok[13:], None)]
    seen = _record(model)
    rep = tester.class_report(loader)
    assert len(seen) == 2 and rep["names"] == [str(i) for i in range(V)]
    stats, conf = np.zeros((V, 3), np.int64), np.zeros((V, V), np.int64)
    for (_, _, out), (t, _) in zip(seen, loader):
        e = R.evaluate(out[0].detach().double().cpu().reshape(-1, V).numpy(), t.reshape(-1).numpy())
        stats += e["stats"]
        conf += e["confusion"]
    _assert_report(rep, stats, conf)
    assert rep["counts"].sum() == 21 * 24 and 0.0 <= rep["balanced_accuracy"] <= 1.0
    # the histogram of the same loader, and the weights made of it
    counts = trainer.class_counts(loader)
    assert counts.dtype == torch.int64 and not counts.is_cuda and np.array_equal(counts.numpy(), np.bincount(tok.reshape(-1).numpy(), minlength=V))
    cw = trainer.class_weights(counts, "effective")
    assert abs(float((cw.double() * counts).sum()) - 21 * 24) <= 1e-5 * 21 * 24


def test_latent_rnn_class_report_equals_the_restatement_on_its_own_logits():
    from tests.test_gpu_latent import build
    V = G.CFGS["small"]["V"]
    fx = G.load("latent_small_nar_fr")
    ds, _, model = build("small", False)
    tester = LatentRNNTester(ds, model)
    score = torch.from_numpy(fx["score"])
    loader = [(score, None), (score[:2], None)]
    seen = _record(model)
    rep = tester.class_report(loader, fix_num_target=4)
    stats, conf = np.zeros((V, 3), np.int64), np.zeros((V, V), np.int64)
    for a, k, out in seen:
        target = k.get("target", a[2] if len(a) > 2 else None)
        e = R.evaluate(out[0].detach().double().cpu().reshape(-1, V).numpy(), target.cpu().reshape(-1).numpy())
        stats += e["stats"]
        conf += e["confusion"]
    _assert_report(rep, stats, conf)
    assert rep["counts"].sum() == (score.shape[0] + 2) * 4 * 24


# =============================================================================== 5. the training state
def test_training_state_round_trip_keeps_the_settings():
    V = CFG["V"]
    _, ma, a = _vae(**_kw(V))
    _, mb, b = _vae()
    b.load_training_state(a.training_state(1))
    assert torch.equal(b.ce_weight, _cw(V)) and (b.label_smoothing, b.ignore_index) == (SMOOTH, IGN)
    sa, sb = _step(a, ma), _step(b, mb)                                           # ... and the loaded trainer takes the weighted path
    assert "cross_entropy_w" in sb["labels"] and abs(float(sa["loss"]) - float(sb["loss"])) <= LOSS_TOL * abs(float(sa["loss"]))
    old = {k: v for k, v in a.training_state(1).items() if k not in a.CE_SETTINGS}
    _, _, c = _vae(label_smoothing=0.3)
    c.load_training_state(old)
    assert c.ce_weight is None and (c.label_smoothing, c.ignore_index) == (0.3, None)
