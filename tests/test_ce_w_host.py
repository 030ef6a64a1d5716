"""What can be said about the class-weighted, label-smoothed cross-entropy without a GPU: the float64
restatement tests/ce_w_ref.py against torch.nn.functional.cross_entropy, value and autograd gradient; Trainer.class_weights; the
trainers' keywords and the training state; the argument checks of the two C entries and of ops, which answer before any launch."""
import ctypes as C
import inspect
import itertools
import math

import numpy as np
import pytest
import torch

from inpaintnet_amd import _lib
from tests import ce_w_ref as R

ROWS, V = 11, 7


def _case(weights, ignore):
    g = torch.Generator().manual_seed(1234)
    x = torch.relu(torch.randn(ROWS, V, generator=g, dtype=torch.float64))
    x[::3] = 0.0
    t = torch.randint(0, V, (ROWS,), generator=g)
    t[0], t[-1] = 0, V - 1
    w = {"none": None, "random": torch.rand(V, generator=g, dtype=torch.float64) + 0.1,
         "zeros": torch.tensor([0.0, 1.5, 0.0, 0.25, 2.0, 0.0, 1.0], dtype=torch.float64)}[weights]
    ii = None
    if ignore == "some":
        ii, t[2], t[5] = -100, -100, -100
    elif ignore == "ends":
        ii, t[0], t[-1] = V + 3, V + 3, V + 3
    return x, t, w, ii


# =============================================================================== 1. the restatement is torch's definition
@pytest.mark.parametrize("weights,e,ignore", list(itertools.product(["none", "random", "zeros"], [0.0, 0.1, 1.0], ["none", "some", "ends"])))
def test_restatement_is_torchs_cross_entropy_in_float64(weights, e, ignore):
    x, t, w, ii = _case(weights, ignore)
    xt = x.clone().requires_grad_(True)
    want = torch.nn.functional.cross_entropy(xt, t, weight=w, label_smoothing=e, ignore_index=-100 if ii is None else ii)
    want.backward()
    want = want.detach()
    got = R.evaluate(x.numpy(), t.numpy(), None if w is None else w.numpy(), e, ii)
    assert abs(got["loss"] - float(want)) <= 1e-14 * abs(float(want))
    assert np.abs(got["grad"] - xt.grad.numpy()).max() <= 1e-15
    if ignore != "none":
        rows = np.nonzero(t.numpy() == ii)[0]
        assert len(rows) == 2 and not got["grad"][rows].any() and got["n_valid"] == ROWS - 2 and got["n_bad"] == 0
    c = R.counts(t.numpy(), V, None if w is None else w.numpy(), ii)
    assert abs(c["denom"] - got["denom"]) <= 1e-14 * got["denom"] and c["counts"].sum() == got["n_valid"]
    assert np.array_equal(got["stats"][:, 0], c["counts"]) and got["confusion"].sum() == got["n_valid"]
    assert np.array_equal(got["confusion"].sum(axis=1), got["stats"][:, 0]) and np.array_equal(got["confusion"].sum(axis=0), got["stats"][:, 2])
    assert np.array_equal(np.diag(got["confusion"]), got["stats"][:, 1])


def test_denominator_zero_is_nan_with_a_zero_gradient():
    x, t, _, _ = _case("none", "none")
    for w, ii, tt in ((None, 3, np.full(ROWS, 3)), (np.array([0.0, 0, 1, 1, 1, 1, 1]), None, np.arange(ROWS) % 2)):
        got = R.evaluate(x.numpy(), tt, w, 0.1, ii)
        assert math.isnan(got["loss"]) and not got["grad"].any() and got["denom"] == 0.0
        want = torch.nn.functional.cross_entropy(x, torch.from_numpy(tt), weight=None if w is None else torch.from_numpy(w),
                                                 label_smoothing=0.1, ignore_index=-100 if ii is None else ii)
        assert math.isnan(float(want))


def test_bad_targets_are_ignored_and_counted():
    x, t, _, _ = _case("none", "none")
    tt = t.numpy().copy()
    tt[1], tt[4], tt[6] = -1, V, -100
    got = R.evaluate(x.numpy(), tt, None, 0.0, -100)
    assert (got["n_bad"], got["n_valid"]) == (2, ROWS - 3) and not got["grad"][[1, 4, 6]].any()
    keep = np.ones(ROWS, bool)
    keep[[1, 4, 6]] = False
    assert abs(got["loss"] - R.evaluate(x.numpy()[keep], tt[keep])["loss"]) <= 1e-15


def test_argmax_is_the_first_of_equal_maxima():
    x = np.zeros((3, 4))
    x[1, 2] = x[1, 3] = 1.0
    got = R.evaluate(x, np.array([0, 3, 1]))
    assert got["stats"].tolist() == [[1, 1, 2], [1, 0, 0], [0, 0, 1], [1, 0, 0]] and got["accuracy"] == 1 / 3
    rep = R.report(got["stats"], got["confusion"])
    assert rep["recall"][0] == 1.0 and rep["recall"][1] == 0.0 and math.isnan(rep["recall"][2]) and math.isnan(rep["precision"][1])
    assert rep["balanced_accuracy"] == pytest.approx(1 / 3) and rep["f1"][0] == pytest.approx(2 / 3)


# =============================================================================== 2. class_weights
def _trainer_cls():
    from inpaintnet_amd.trainer import Trainer
    return Trainer


@pytest.mark.parametrize("scheme", ["inverse", "inverse_sqrt", "effective"])
@pytest.mark.parametrize("normalize", [True, False])
def test_class_weights_schemes(scheme, normalize):
    n = np.array([5000, 0, 12, 1, 300, 0, 77])
    got = _trainer_cls().class_weights(torch.from_numpy(n), scheme, beta=0.99, normalize=normalize)
    want = R.class_weights(n, scheme, 0.99, normalize)
    assert got.dtype == torch.float32 and got.shape == (7,)
    assert np.abs(got.double().numpy() - want).max() <= 1e-6 * want.max()
    assert got[1] == got[5] == got[3] == got.max()                              # count 0: the weight of the rarest present class
    if normalize:
        assert abs(float((got.double() * torch.from_numpy(n)).sum()) - n.sum()) <= 1e-6 * n.sum()
    else:
        raw = {"inverse": 1 / 12, "inverse_sqrt": 1 / math.sqrt(12), "effective": 0.01 / (1 - 0.99 ** 12)}[scheme]
        assert float(got[2]) == pytest.approx(raw, rel=1e-6)
    assert bool((got[:-1][n[:-1] > n[-1]] < got[-1]).all())                     # a more frequent class never weighs more


def test_class_weights_refuses_bad_arguments():
    T = _trainer_cls()
    for bad in (lambda: T.class_weights([0, 0]), lambda: T.class_weights([]), lambda: T.class_weights([3, -1]),
                lambda: T.class_weights([1, 2], "log"), lambda: T.class_weights([1, 2], "effective", beta=1.0),
                lambda: T.class_weights([1, 2], "effective", beta=-0.1)):
        with pytest.raises(ValueError, match="class_weights"):
            bad()
    assert T.class_weights([4, 4], "effective", beta=0.0).tolist() == [1.0, 1.0]


# =============================================================================== 3. the trainers' keywords and the training state
class _Untouchable:
    def __getattr__(self, name):
        raise AssertionError(f"the model was touched ({name}) before the keywords were checked")


class _HostModel:
    def __init__(self, n=8):
        self.flat = torch.arange(n, dtype=torch.float32)
        self.grad = torch.zeros(n)
        self._table = None
        self.free_bits = None
        self.latent_space_dim = 8


class _Dataset:
    n_bars, subdivision, num_beats_per_bar = 16, 6, 4

    def __init__(self, sizes=(V,)):
        self.note2index_dicts = [{i: i for i in range(n)} for n in sizes]


@pytest.fixture(autouse=True)
def _no_gc_freeze(monkeypatch):
    monkeypatch.setenv("INET_GC_FREEZE", "0")


def _classes():
    from inpaintnet_amd.arnn import AnticipationRNNGaussianRegTrainer
    from inpaintnet_amd.latent_rnn_trainer import LatentRNNTrainer
    from inpaintnet_amd.vae_trainer import VAETrainer
    return VAETrainer, LatentRNNTrainer, AnticipationRNNGaussianRegTrainer


BAD_KW = [{"ce_weight": [1.0] * (V - 1)}, {"ce_weight": [[1.0] * V]}, {"ce_weight": [1.0] * (V - 1) + [-0.5]},
          {"ce_weight": [1.0] * (V - 1) + [float("nan")]}, {"ce_weight": [1.0] * (V - 1) + [math.inf]}, {"ce_weight": "heavy"},
          {"ce_weight": []}, {"label_smoothing": -0.1}, {"label_smoothing": 1.5}, {"label_smoothing": float("nan")},
          {"label_smoothing": "0.1"}, {"label_smoothing": None}, {"label_smoothing": True}, {"ignore_index": 0}, {"ignore_index": V - 1},
          {"ignore_index": 1.0}, {"ignore_index": True}, {"ignore_index": "pad"}]


@pytest.mark.parametrize("kw", BAD_KW)
def test_trainers_reject_bad_keywords_before_touching_the_model(kw):
    for cls in _classes():
        with pytest.raises(ValueError, match="ce_weight|label_smoothing|ignore_index"):
            cls(_Dataset(), _Untouchable(), **kw)


def test_keyword_defaults_and_accepted_values():
    from inpaintnet_amd.trainer import Trainer
    for cls in _classes() + (Trainer,):
        prm = inspect.signature(cls.__init__).parameters
        assert [prm[k].default for k in Trainer.CE_SETTINGS] == [None, 0.0, None], cls
    prm = inspect.signature(Trainer.mean_crossentropy_loss_and_accuracy).parameters
    assert list(prm) == ["weights", "targets", "weight", "label_smoothing", "ignore_index"]
    assert [prm[k].default for k in list(prm)[2:]] == [None, 0.0, None]
    for cls in _classes():
        tr = cls(_Dataset(), _HostModel())
        assert tr._ce_plain() and tr.last_ce is None and tr.ce_weight is None and tr.ignore_index is None
        w = [0.0, 1.0, 2.0, 0.5, 1.0, 1.0, 3.0]                                  # a weight of 0 is legal
        for good in ({"ce_weight": w}, {"ce_weight": torch.tensor(w, dtype=torch.float64)}, {"ce_weight": np.array(w)},
                     {"label_smoothing": 0}, {"label_smoothing": 1.0}, {"ignore_index": -100}, {"ignore_index": V}, {"ignore_index": -1}):
            tr = cls(_Dataset(), _HostModel(), **good)
            assert tr._ce_plain() == (good == {"label_smoothing": 0})
        tr = cls(_Dataset(), _HostModel(), ce_weight=w, label_smoothing=0.1, ignore_index=-100)
        assert tr.ce_weight.dtype == torch.float32 and tr.ce_weight.tolist() == w and not tr.ce_weight.is_cuda
        assert isinstance(tr.label_smoothing, float) and tr._ce_args(torch.device("cpu"))[1:] == (0.1, -100)
        assert "free_nats_per='dim'" in Trainer.__init__.__doc__ and "no collective" in Trainer.__init__.__doc__
    # voices with different vocabularies: the length of ce_weight cannot be checked against one V
    assert _classes()[2](_Dataset((V, V + 2)), _HostModel(), ce_weight=[1.0] * 3).ce_weight.numel() == 3


def test_training_state_round_trip_carries_the_three_settings():
    for cls in _classes():
        w = [0.0, 1.0, 2.0, 0.5, 1.0, 1.0, 3.0]
        a = cls(_Dataset(), _HostModel(), ce_weight=w, label_smoothing=0.25, ignore_index=-100)
        st = a.training_state(3)
        assert st["ce_weight"].tolist() == w and (st["label_smoothing"], st["ignore_index"]) == (0.25, -100)
        b = cls(_Dataset(), _HostModel())
        assert b.load_training_state(st) == 3
        assert b.ce_weight.tolist() == w and (b.label_smoothing, b.ignore_index) == (0.25, -100) and not b._ce_plain()
        # a state written before the settings existed leaves this trainer's own
        old = {k: v for k, v in a.training_state(2).items() if k not in a.CE_SETTINGS}
        d = cls(_Dataset(), _HostModel(), label_smoothing=0.5, ignore_index=V)
        assert d.load_training_state(old) == 2 and (d.ce_weight, d.label_smoothing, d.ignore_index) == (None, 0.5, V)
        # ... a default trainer's state switches the settings off, and a bad state is refused
        assert d.load_training_state(cls(_Dataset(), _HostModel()).training_state(1)) == 1 and d._ce_plain()
        with pytest.raises(ValueError, match="label_smoothing"):
            d.load_training_state(dict(st, label_smoothing=2.0))


def test_training_state_survives_torch_save(tmp_path):
    VAETrainer = _classes()[0]
    a = VAETrainer(_Dataset(), _HostModel(), ce_weight=[1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0], label_smoothing=0.1)
    a.save_training_state(str(tmp_path / "state.pt"), 4)
    b = VAETrainer(_Dataset(), _HostModel())
    assert b.load_training_state(str(tmp_path / "state.pt")) == 4
    assert b.ce_weight.tolist() == [1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0] and b.label_smoothing == 0.1 and b.ignore_index is None


def test_report_helper_is_the_restatement():
    from inpaintnet_amd.trainer import class_report_from_counts, index_to_note_names
    x, t, _, _ = _case("none", "none")
    e = R.evaluate(x.numpy(), t.numpy())
    got = class_report_from_counts(torch.from_numpy(e["stats"]), torch.from_numpy(e["confusion"]), names=["a"] * V)
    want = R.report(e["stats"], e["confusion"])
    for k in ("counts", "hits", "predicted", "confusion"):
        assert got[k].dtype == np.int64 and np.array_equal(got[k], want[k]), k
    for k in ("recall", "precision", "f1"):
        assert np.array_equal(got[k], want[k], equal_nan=True), k
    assert got["accuracy"] == want["accuracy"] == e["accuracy"] and got["balanced_accuracy"] == want["balanced_accuracy"]
    assert got["names"] == ["a"] * V
    empty = class_report_from_counts(np.zeros((3, 3), np.int64), np.zeros((3, 3), np.int64))
    assert math.isnan(empty["accuracy"]) and math.isnan(empty["balanced_accuracy"]) and empty["names"] is None

    class DS:
        index2note_dicts = [{0: "__", 1: "rest", 2: "G4"}]
    assert index_to_note_names(DS(), 3) == ["__", "rest", "G4"] and index_to_note_names(DS(), 4) is None
    assert index_to_note_names(object(), 3) is None


# =============================================================================== 4. the C entries and ops refuse bad arguments
@pytest.fixture(scope="module")
def L():
    _lib.build(verbose=False)
    return _lib.lib()


X = C.c_void_p(16)                     # a pointer that is never followed: every call below is refused in front of the launch
NULL = None


def test_binding_has_the_headers_arity():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "inpaintnet_hip.h")).read()
    for name in ("inet_class_counts", "inet_cross_entropy_w_ws_bytes", "inet_cross_entropy_w"):
        proto = re.search(r"^int(?:64_t)? " + name + r"\(([^;]*)\);", hdr, re.M).group(1)
        assert len(proto.split(",")) == len(_lib._SIGNATURES[name][1]), name
    assert "ce.hip" in _lib.SOURCES
    from inpaintnet_amd import ops
    assert f"out, {ops.CE_META_WORDS} + V + extra_words int64 words" in hdr and f"out[{ops.CE_META_WORDS} + c] counts[c]" in hdr
    assert "ALL ZEROS" in hdr and "denom == 0" in hdr


def test_entries_refuse_bad_arguments_before_any_launch(L):
    ii = C.byref(C.c_int64(-100))

    def ce(weights=X, ld_w=4, rows=1, Vv=4, targets=X, cw=NULL, e=0.0, ign=NULL, meta=X, dW=NULL, ld_dw=4, scale_dev=NULL, loss=X,
           acc=X, add_term=NULL, add_scale=0.0, fwd_out=NULL, fwd_scale=0.0, stats=NULL, conf=NULL, ws=X, ws_bytes=1 << 20):
        return L.inet_cross_entropy_w(weights, ld_w, rows, Vv, targets, cw, e, ign, meta, dW, ld_dw, scale_dev, loss, acc, add_term,
                                      add_scale, fwd_out, fwd_scale, stats, conf, ws, ws_bytes, NULL)
    cases = {
        "counts targets": L.inet_class_counts(NULL, 4, 4, NULL, NULL, X, 0, NULL),
        "counts out": L.inet_class_counts(X, 4, 4, NULL, NULL, NULL, 0, NULL),
        "counts n": L.inet_class_counts(X, 0, 4, NULL, NULL, X, 0, NULL),
        "counts n huge": L.inet_class_counts(X, (1 << 40) + 1, 4, NULL, NULL, X, 0, NULL),
        "counts V": L.inet_class_counts(X, 4, 0, NULL, ii, X, 0, NULL),
        "counts extra": L.inet_class_counts(X, 4, 4, X, NULL, X, -1, NULL),
        "weights": ce(weights=NULL), "targets": ce(targets=NULL), "meta": ce(meta=NULL), "rows": ce(rows=0), "rows < 0": ce(rows=-2),
        "V": ce(Vv=0), "V < 0": ce(Vv=-1), "ld_w": ce(ld_w=3), "ld_dw": ce(dW=X, ld_dw=3),
        "no output": ce(loss=NULL, acc=NULL), "smoothing < 0": ce(e=-0.01), "smoothing > 1": ce(e=1.01), "smoothing nan": ce(e=float("nan")),
        "fwd_out without scale_dev": ce(dW=X, fwd_out=X), "add_term without loss": ce(loss=NULL, add_term=X),
        "ws null": ce(ws=NULL), "ws small": ce(ws_bytes=8), "ws null, accuracy alone": ce(loss=NULL, ws=NULL, ign=ii),
    }
    bad = {k: v for k, v in cases.items() if v != -1}
    assert not bad, bad
    assert L.inet_cross_entropy_w_ws_bytes(0) == -1 and L.inet_cross_entropy_w_ws_bytes(1) == 24
    # one partial per workgroup: four rows a workgroup up to 128 workgroups, a function of rows alone
    assert [L.inet_cross_entropy_w_ws_bytes(r) // 24 for r in (4, 5, 48, 512, 513, 6144)] == [1, 2, 12, 128, 128, 128]


def test_ops_refuse_bad_arguments():
    from inpaintnet_amd import ops
    t = torch.zeros(4, dtype=torch.int64)
    with pytest.raises(ValueError, match="device tensor"):
        ops.class_counts(t, 4)                                                  # (host tensors: refused in front of everything else)
    with pytest.raises(ValueError, match="label_smoothing"):
        ops._ce_common("x", 4, None, 1.5, None, t.device)
    with pytest.raises(ValueError, match="ignore_index"):
        ops._ce_common("x", 4, None, 0.0, 1.5, t.device)
    with pytest.raises(ValueError, match="weight"):
        ops._ce_common("x", 4, torch.ones(3), 0.0, None, t.device)
    with pytest.raises(ValueError, match="weight"):
        ops._ce_common("x", 4, torch.ones(4, dtype=torch.float64), 0.0, None, t.device)
    w, e, ii = ops._ce_common("x", 4, torch.ones(4), 1, 4, t.device)
    assert e == 1.0 and ii is not None and ops._ce_common("x", 4, None, 0.0, None, t.device) == (None, 0.0, None)
