"""The attribute regularisation at the trainer's level: VAETrainer(attr_reg=, attr_gamma=, attr_delta=,
attr_spec=) on the small synthetic MeasureVAE of tests/test_gpu_mmd_trainer.py at B = 8 (its helpers pin eps, the prior draws and the
teacher-forcing coin), VAETester.measure_attributes / attribute_concordance / attribute_sweep.

Tolerances are that file's where a whole step is compared (a loss within 1e-4 of itself, a gradient tensor within 5e-4 of its largest
element) and the derived bounds of tests/attr_ref.py where the kernels' outputs are compared alone.  The vocabulary of the synthetic
model has 20 tokens: tests/attr_ref.py's SPEC names them."""
import numpy as np
import pytest
import torch

from tests import attr_ref as R
from tests import kl_fb_ref as K

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from inpaintnet_amd import ops
    from inpaintnet_amd.attributes import ATTRIBUTES, AttributeSpec
    from inpaintnet_amd.vae_tester import VAETester
    from tests.test_gpu_mmd_trainer import B, CFG, GRAD_TOL, LOSS_TOL, _eps, _np64, _same_bits, _step, _tokens, _vae

REG = {"note_range": 23, "num_notes": 0, "beat_strength": 5}                    # not in ATTRIBUTES' order, dims include 0 and Z - 1
ATTR_LABELS = ("measure_attrs", "attr_pair", "attr_pair_grad", "attr_finish")


def _kw(**more):
    return dict(attr_reg=dict(REG), attr_gamma=10.0, attr_delta=1.0, attr_spec=AttributeSpec(**R.SPEC), **more)


def _reference(out, trainer):
    """The restatement on the step's own z_tilde and tokens."""
    assert CFG["V"] == R.SPEC["num_tokens"]
    tok = _tokens().cpu().numpy()
    attrs = R.measure_attrs(tok, **R.SPEC)[:, [R.COLUMNS.index(k) for k in trainer.attr_reg]].astype(np.float32)
    dims = list(trainer.attr_reg.values())
    return attrs, dims, R.evaluate(out[4].detach().cpu().numpy(), dims, attrs, trainer.attr_delta, trainer.attr_gamma)


def _assert_attr_step(d, m, tm):
    """d: the step without the term, m: with it (same weights, tokens, eps, prior draws, coin)."""
    attrs, dims, e = _reference(m["out"], tm)
    last = tm.last_attr_reg
    A = len(dims)
    assert set(last) == {"value", "per_attr", "counts", "attrs"} and all(t.is_cuda for t in last.values())
    assert last["value"].shape == () and last["per_attr"].shape == (A,) and last["counts"].shape == (A, 3) and last["attrs"].shape == (B, A)
    assert np.array_equal(last["attrs"].cpu().numpy(), attrs)                   # (no logf among REG's attributes: equal bits)
    assert abs(float(last["value"]) - e["value"]) <= e["value_bound"]
    assert bool((np.abs(_np64(last["per_attr"]) - e["per_attr"]) <= e["per_bound"]).all())
    assert np.array_equal(last["counts"].cpu().numpy(), e["counts"])
    # the loss: the step's loss without the term, plus the term -- one float32 addition
    want = float(d["loss"]) + float(last["value"])
    print(f"loss {float(m['loss']):.7f} = {float(d['loss']):.7f} + {float(last['value']):.7f} (ref {e['value']:.7f}); "
          f"max |G| {np.abs(e['grad']).max():.3g} against max |dmu| {float(d['dmu'].abs().max()):.3g}")
    assert abs(float(m["loss"]) - want) <= LOSS_TOL * abs(want)
    assert abs(float(last["value"])) >= 100.0 * LOSS_TOL * abs(want)             # the term is far above that tolerance
    assert {"measure_attrs", "attr_pair_grad", "attr_finish"} <= set(m["labels"]) and "attr_pair" not in m["labels"]
    assert sorted(l for l in m["labels"] if l not in ATTR_LABELS) == sorted(d["labels"])     # nothing else is launched
    # what reaches the encoder: the default's dmu / dls plus what the reparameterisation's backward makes of dz = G, G scattered by
    # hand into the regularised columns of a [B, Z] zero
    dz = np.zeros((B, CFG["Z"]))
    dz[:, dims] = e["grad"]
    mu, ls = _np64(m["out"][2].loc), _np64(m["out"][2].log_scale)
    gmu, gls = K.backward(dz, mu, ls, _np64(_eps()), 0.0, None, np.ones(B, bool), "measure")
    other = [c for c in range(CFG["Z"]) if c not in dims]
    assert not gmu[:, other].any() and not gls[:, other].any()
    for name, extra in (("dmu", gmu), ("dls", gls)):
        want, got = _np64(d[name]) + extra, _np64(m[name])
        assert np.abs(extra).max() >= 0.01 * np.abs(want).max(), name             # the term is visible in what is compared
        assert np.abs(got - want).max() <= GRAD_TOL * np.abs(want).max(), name
        # ... and only through the regularised columns: elsewhere the two steps differ by no more than two default steps do
        assert np.abs(got[:, other] - _np64(d[name])[:, other]).max() <= GRAD_TOL * np.abs(want).max(), name
        assert np.abs(got[:, dims] - _np64(d[name])[:, dims]).max() >= 0.01 * np.abs(want).max(), name
    changed = [k for k in d["grads"] if k.startswith("encoder.") and not _same_bits(d["grads"][k], m["grads"][k])]
    assert len(changed) > 4                                                     # ... and it reaches the encoder's weights
    for k in d["grads"]:
        if k.startswith("decoder."):                                            # z_tilde is the same: the decoder sees no change
            assert float((d["grads"][k] - m["grads"][k]).abs().max()) <= GRAD_TOL * float(d["grads"][k].abs().max()) + 1e-12, k


def test_attr_term_adds_its_value_and_its_gradient():
    _, md, td = _vae()
    _, mm, tm = _vae(**_kw())
    d, m = _step(td, md), _step(tm, mm)
    assert td.last_attr_reg is None and tm.last_mmd is None and tm.last_kl is None
    _assert_attr_step(d, m, tm)


def test_attr_term_combines_with_free_bits_and_mmd():
    more = dict(kl_beta=0.5, free_nats=0.05, free_nats_per="dim", mmd_coeff=10)
    _, md, td = _vae(**more)
    _, mm, tm = _vae(**_kw(**more))
    d, m = _step(td, md), _step(tm, mm)
    assert tm.last_kl is not None and tm.last_mmd is not None
    assert _same_bits(tm.last_mmd["value"], td.last_mmd["value"]) and _same_bits(tm.last_kl["keep"], td.last_kl["keep"])
    assert "latent_bwd_fb" in m["labels"] and "mmd_pair_grad" in m["labels"]
    assert m["labels"].index("mmd_finish") < m["labels"].index("measure_attrs")  # added after the MMD term
    # the default of this comparison carries the floor and the MMD term itself: dmu / dls through the kept columns only
    attrs, dims, e = _reference(m["out"], tm)
    want = float(d["loss"]) + float(tm.last_attr_reg["value"])
    assert abs(float(m["loss"]) - want) <= LOSS_TOL * abs(want)
    assert abs(float(tm.last_attr_reg["value"]) - e["value"]) <= e["value_bound"]
    dz = np.zeros((B, CFG["Z"]))
    dz[:, dims] = e["grad"]
    mu, ls = _np64(m["out"][2].loc), _np64(m["out"][2].log_scale)
    gmu, gls = K.backward(dz, mu, ls, _np64(_eps()), 0.0, None, np.ones(CFG["Z"], bool), "dim")
    for name, extra in (("dmu", gmu), ("dls", gls)):
        want = _np64(d[name]) + extra
        assert np.abs(_np64(m[name]) - want).max() <= GRAD_TOL * np.abs(want).max(), name


def test_validation_adds_the_value_and_launches_no_gradient_phase():
    _, md, td = _vae()
    _, mm, tm = _vae(**_kw())
    d, m = _step(td, md, train=False), _step(tm, mm, train=False)
    _, _, e = _reference(m["out"], tm)
    assert abs(float(tm.last_attr_reg["value"]) - e["value"]) <= e["value_bound"]
    want = float(d["loss"]) + float(tm.last_attr_reg["value"])
    assert abs(float(m["loss"]) - want) <= LOSS_TOL * abs(want)
    assert abs(float(tm.last_attr_reg["value"])) >= 100.0 * LOSS_TOL * abs(want)
    assert {"measure_attrs", "attr_pair", "attr_finish"} <= set(m["labels"]) and "attr_pair_grad" not in m["labels"]
    assert [l for l in m["labels"] if l not in ATTR_LABELS] == d["labels"]


def test_attr_reg_none_is_the_default_trainer(monkeypatch):
    """With attr_reg=None the trainer launches exactly the default trainer's kernels, in the same order, and never reaches the
    attribute code.  Two default trainers do not repeat each other's last bits (float atomics in the KL sum and some weight gradients:
    tests/test_gpu_mmd_trainer.py measured it), so loss and gradients are held to that file's tolerances and the label lists and the
    absence of any call exactly."""
    from inpaintnet_amd import measure_vae

    def boom(*a, **k):
        raise AssertionError("a trainer with attr_reg=None reached the attribute code")
    _, m1, t1 = _vae()
    _, m0, t0 = _vae(attr_reg=None, attr_gamma=3.0, attr_delta=2.0, attr_spec=AttributeSpec(**R.SPEC))
    d1 = _step(t1, m1)
    monkeypatch.setattr(ops, "attr_reg", boom)
    monkeypatch.setattr(ops, "measure_attributes", boom)
    monkeypatch.setattr(measure_vae._AttrRegFn, "forward", staticmethod(boom))
    z = _step(t0, m0)
    zv = _step(t0, m0, train=False)
    assert t0.last_attr_reg is None and t1.last_attr_reg is None
    assert not [l for l in z["labels"] + zv["labels"] if l in ATTR_LABELS]
    assert z["labels"] == d1["labels"]
    same = 0
    for name, a, b, tol in [("loss", z["loss"], d1["loss"], LOSS_TOL)] + [(k, z["grads"][k], d1["grads"][k], GRAD_TOL) for k in d1["grads"]]:
        same += int(_same_bits(a, b))
        assert float((a - b).abs().max()) <= tol * float(b.abs().max()), name
    print(f"{same} of {1 + len(d1['grads'])} tensors have the default trainer's bits")
    assert same > 0


def test_training_state_round_trip_keeps_the_settings():
    spec = AttributeSpec(**R.SPEC)
    _, _, a = _vae(**_kw())
    _, _, b = _vae()
    b.load_training_state(a.training_state(1))
    assert (b.attr_reg, b.attr_gamma, b.attr_delta, b.attr_spec) == (REG, 10.0, 1.0, spec) and list(b.attr_reg) == list(REG)
    old = {k: v for k, v in a.training_state(1).items() if k not in a.ATTR_SETTINGS}
    _, _, c = _vae(attr_reg={"rhy_entropy": 2}, attr_spec=spec)
    c.load_training_state(old)
    assert (c.attr_reg, c.attr_gamma, c.attr_delta, c.attr_spec) == ({"rhy_entropy": 2}, 10.0, 10.0, spec)


def _tester():
    ds, model, _ = _vae()
    model.eval()
    return model, VAETester(ds, model)


def test_tester_concordance_agrees_with_the_restatement_on_one_batch():
    model, tester = _tester()
    spec = AttributeSpec(**R.SPEC)
    n = 21
    tok = torch.from_numpy(R.draw_tokens("tester", n, 24))
    attrs = tester.measure_attributes(tok, spec)
    want_attrs = R.measure_attrs(tok.numpy(), **R.SPEC)
    assert attrs.shape == (n, 4) and np.array_equal(attrs.cpu().numpy()[:, [0, 1, 3]], want_attrs[:, [0, 1, 3]].astype(np.float32))
    dims = [0, 5, 23, 7, 8, 9, 10, 11, 12]                                      # nine: a second call of the pair kernel
    got = tester.attribute_concordance([(tok, None)], dims, spec)
    assert got.shape == (len(dims), 4) and got.dtype == torch.float64 and got.is_cuda
    with torch.no_grad():
        loc = model.encoder(tok.cuda()).loc.cpu().numpy()
    want = np.zeros((len(dims), 4))
    for k in range(4):
        c = R.pair_counts(loc, dims, np.repeat(attrs.cpu().numpy()[:, k:k + 1], len(dims), 1))
        want[:, k] = (c[:, 0] - c[:, 1]) / (c[:, 0] + c[:, 1])
    diff = np.abs(got.cpu().numpy() - want).max()
    print(f"concordance: max |device - restatement| {diff:.3g}; range [{want.min():.3f}, {want.max():.3f}]")
    # two encoder passes may differ in their last bits (the project's 1e-5): that can flip a pair whose two means are that close, and
    # one flipped pair moves a concordance by 4 / (c + d) <= 4 / (n (n - 1) / 2): nothing else is allowed
    assert diff <= 4.0 / (n * (n - 1) / 2) + 1e-12
    assert np.abs(want).max() < 0.9 and len(set(np.round(want.ravel(), 6))) > 10   # an untrained model: neither trivial nor constant
    full = tester.attribute_concordance([(tok[:13], None), (tok[13:], None)], None, spec)
    assert full.shape == (CFG["Z"], 4)
    with pytest.raises(ValueError, match="empty"):
        tester.attribute_concordance([], dims, spec)
    with pytest.raises(ValueError, match="pitch name"):
        tester.attribute_concordance([(tok, None)], dims)                       # the synthetic dataset has no names: a spec is needed


def test_tester_sweep_returns_the_attributes_of_its_own_tokens():
    _, tester = _tester()
    spec = AttributeSpec(**R.SPEC)
    tok = torch.from_numpy(R.draw_tokens("sweep", 5, 24))
    values = [-2.0, 0.0, 1.5]
    attrs, tokens = tester.attribute_sweep(tok, 23, values, spec)
    assert attrs.shape == (3, 5, 4) and attrs.dtype == torch.float32 and tokens.shape == (3, 5, 24) and tokens.dtype == torch.int64
    t = tokens.cpu().numpy()
    assert t.min() >= 0 and t.max() < CFG["V"]
    want = R.measure_attrs(t.reshape(15, 24), **R.SPEC).reshape(3, 5, 4)
    got = attrs.cpu().numpy()
    assert np.array_equal(got[..., [0, 1, 3]], want[..., [0, 1, 3]].astype(np.float32))
    assert np.abs(got[..., 2] - want[..., 2]).max() <= R.LOG_ULP * np.spacing(np.float32(np.log(24)))
    assert tuple(ATTRIBUTES) == R.COLUMNS
    for bad in (lambda: tester.attribute_sweep(tok, CFG["Z"], values, spec), lambda: tester.attribute_sweep(tok, 0, [], spec),
                lambda: tester.attribute_sweep(tok, 1.0, values, spec)):
        with pytest.raises(ValueError, match="attribute_sweep"):
            bad()
