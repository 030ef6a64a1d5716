"""The attribute regularisation without a GPU: the float64 restatement (tests/attr_ref.py) against what the
reference's own extractors returned (tests/golden/attr_reference.npz), note_range against hand-worked rows, the conditions the GPU
tests' inputs and bounds must meet, the descent check of the restatement, the binding of the new entries against the header, the
entries' refusals, AttributeSpec, and the VAETrainer keywords."""
import ast
import ctypes as C
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

from inpaintnet_amd import _lib
from tests import attr_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _attrs(tokens):
    return R.measure_attrs(tokens, **R.SPEC)


# =============================================================================== 1. the extractors
def test_restatement_reproduces_the_references_own_extractors():
    """num_notes: the reference divides in float32, one operation on one integer -- equal bits.  rhy_entropy and beat_strength: the
    reference adds 24 float64 terms (scipy's entropy of a 0/1 vector, a dot product with the weights); log(n) and milli / 1000 are
    within a few float64 roundings of that, far below half a float32 ulp: the float32 values are equal."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "attr_reference.npz"))
    tok = g["tokens"]
    assert tok.shape[1] == 24 and tok.shape[0] >= 40 and int((tok != R.SPEC["slur_index"]).sum(1).min()) >= 1
    assert np.array_equal(tok[:40], R.draw_tokens("golden", 40, 24))
    a = _attrs(tok)
    assert g["num_notes"].dtype == np.float32 and np.array_equal(a[:, 0].astype(np.float32), g["num_notes"])
    for col, name in ((2, "rhy_entropy"), (3, "beat_strength")):
        assert g[name].dtype == np.float64
        assert np.abs(a[:, col] - g[name]).max() <= 1e-13 * np.abs(g[name]).max(), name
        assert np.array_equal(a[:, col].astype(np.float32), g[name].astype(np.float32)), name
    assert len(set(a[:, 2])) > 5 and len(set(a[:, 3])) > 20                        # the fixture is not one value


def test_note_range_on_hand_worked_rows():
    e = R.edge_rows(24)
    rows = np.stack([e["no_pitch"], e["one_pitch"], e["full_range"], e["all_slur"], e["all_rest"]])
    a = _attrs(rows)
    assert list(a[:, 1]) == [0.0, 0.0, 1.0, 0.0, 0.0]                              # nothing pitched; D4 alone; G3..C6 = 29 / 29
    v = R.VOCAB.index
    row = np.array([v("START"), v(None), v("rest"), v("__"), v("C4"), v("__"), v("E5"), v("rest")] + [v("__")] * 16)
    assert _attrs(row[None])[0, 1] == (76 - 60) / 29                              # START / None / rest / slur are ignored
    # per row: a pitched row in front does not hand its flag to the unpitched row behind it (the reference's has_note is never reset)
    assert list(_attrs(np.stack([e["full_range"], e["no_pitch"]]))[:, 1]) == [1.0, 0.0]
    # the other three columns of the edge rows, by hand: all-slur is 0 notes, entropy 0 (n = 0), strength 0
    assert list(a[3]) == [0.0, 0.0, 0.0, 0.0]
    assert list(a[4]) == [0.0, 0.0, math.log(24), (4 * 1000 + 4 * 150 + 16 * 8) / 1000]
    # one_pitch: D4 at t % 6 == 0 and a rest at t % 6 == 3, slurs elsewhere: 4 notes of 24, 8 onsets
    assert list(a[1]) == [4 / 24, 0.0, math.log(8), (4 * 1000 + 4 * 150) / 1000]
    bad = e["one_pitch"].copy()
    bad[5] = R.SPEC["num_tokens"]
    out = _attrs(np.stack([e["one_pitch"], bad, e["one_pitch"]]))
    assert np.isnan(out[1]).all() and np.array_equal(out[0], out[2]) and not np.isnan(out[0]).any()


def test_depths_restate_the_launch_constants():
    src = open(os.path.join(ROOT, "inpaintnet_amd", "csrc", "attr.hip")).read()
    hdr = open(os.path.join(ROOT, "inpaintnet_amd", "csrc", "attr.h")).read()
    for text, name, want in ((src, "kAttrRows", R.ROWS), (src, "kAttrTile", R.TILE), (src, "kAttrFinishBlock", R.FINISH),
                             (src, "kAttrMeasureRows", R.MEASURE_ROWS), (hdr, "kAttrMaxT", R.MAX_T), (hdr, "kAttrMaxA", R.MAX_A),
                             (hdr, "kAttrColumns", len(R.COLUMNS))):
        assert int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1)) == want, name
    code = re.sub(r"//[^\n]*", "", src)
    assert "atomic" not in code.lower()                                         # no atomics of any kind
    assert "tanhf(delta * dz)" in code and "logf((float)onsets)" in code        # the device library's functions, not approximations
    assert "__tanhf" not in code and "__logf" not in code
    assert R.depth_s(256) == 4 + 1 + 9 + 1 + 9 and R.depth_s(4096) == 4 + 16 + 9 + 1 + 9 and R.depth_g(300) == 13


# =============================================================================== 2. the loss and the GPU tests' conditions
def test_closed_form_gradient_is_autograds():
    """What the kernel implements, (2 coeff delta / B^2) sum_j sgn(t - s) (1 - t^2), against autograd of the L1Loss expression --
    with duplicate z and tied attributes in the input (sign(0) = 0 on both sides)."""
    z, attrs = R.inputs(9, 3, 1, "tied")
    z = z.copy()
    z[4] = z[2]                                                                 # a duplicate row
    dims, delta, coeff = [2, 0], 3.0, 2.5
    attrs2 = np.concatenate([attrs, attrs[::-1]], 1)
    value, per, grad = R.loss_autograd(z, dims, attrs2, delta, coeff)
    B = z.shape[0]
    for a, r in enumerate(dims):
        x, ax = z[:, r].astype(np.float64), attrs2[:, a].astype(np.float64)
        t = np.tanh(delta * (x[:, None] - x[None, :]))
        s = np.sign(ax[:, None] - ax[None, :])
        assert abs(np.abs(t - s).mean() - per[a]) <= 1e-15
        want = 2.0 * coeff * delta / B ** 2 * (np.sign(t - s) * (1.0 - t * t)).sum(1)
        assert np.abs(want - grad[:, a]).max() <= 1e-14 * np.abs(want).max()
    assert abs(value - coeff * per.sum()) <= 1e-15 * value


@pytest.mark.parametrize("B,Z,A,kind", R.CASES)
def test_gpu_cases_meet_their_conditions(B, Z, A, kind):
    """What tests/test_gpu_attr_kernels.py asserts again next to the device's numbers: a wrong sign must not be able to hide."""
    for delta in R.DELTAS:
        for coeff in R.COEFFS:
            z, dims, attrs, e = R.case(B, Z, A, kind, delta, coeff)
            assert 0 in dims or Z - 1 in dims
            if kind == "cont" and B >= 16:
                assert float(e["untied"].min()) >= 0.9
            if kind == "tied":
                tied = 1.0 - e["untied"]
                assert float(tied.min()) >= 0.1 and float(e["untied"].min()) >= 0.5
            print(f"({B}, {Z}, {A}) {kind} delta {delta} coeff {coeff}: value {e['value']:.6g} bound / scale "
                  f"{e['value_bound'] / max(e['scale'], 1e-300):.3g}; grad bound / max |g| "
                  f"{e['grad_bound'].max() / max(np.abs(e['grad']).max(), 1e-300):.3g}")
            assert e["value_bound"] <= 1e-4 * e["scale"]
            assert bool((e["per_bound"] <= 1e-4 * e["per_attr"]).all())
            if B >= 2:
                assert e["value_bound"] > 0.0 and e["scale"] > 0.0
                # the gradient's bound is a bound, not a licence: below 1e-3 of the largest element
                assert e["grad_bound"].max() <= 1e-3 * np.abs(e["grad"]).max()
    if A > 1:
        assert 0 in dims and Z - 1 in dims


def test_case_list_covers_what_the_issue_names():
    Bs, Zs, As = ({c[i] for c in R.CASES} for i in range(3))
    assert {1, 2, 7, 8, 9, 256, 257, 300} <= Bs and {1, 3, 256} <= Zs and {1, 4, 8} == As
    assert {R.ROWS - 1, R.ROWS, R.ROWS + 1, 2 * R.ROWS + 1} <= Bs                 # the row block of this kernel
    assert any(k == "tied" for *_, k in R.CASES)
    assert R.dims_for(1, 1) == [0] and R.dims_for(256, 8)[:2] == [255, 0] and len(set(R.dims_for(256, 8))) == 8


def test_b1_and_all_equal_attributes():
    e = R.evaluate(np.ones((1, 3), np.float32), [1], np.ones((1, 1), np.float32), 10.0, 1.0)
    assert e["value"] == 0.0 and e["value_bound"] == 0.0 and e["counts"].tolist() == [[0, 0, 0]]
    z, _ = R.inputs(17, 256, 8, "cont")
    e = R.evaluate(z, [0, 5], np.full((17, 2), 0.25, np.float32), 10.0, 1.0)
    assert e["counts"].tolist() == [[0, 0, 17 * 16]] * 2 and e["value"] > 0.0      # every pair tied: the term pulls the z together


@pytest.mark.parametrize("seed", R.DESCENT["seeds"])
def test_restatement_descends_to_full_concordance(seed):
    """The GPU test runs 50 steps of z[:, dims] -= 4 G on the kernel's gradient and asks for concordance 1.0 on both attributes: the
    restatement's own gradient gets there within 25 steps, in float64 and in float32 -- 50 is twice that."""
    z, attrs = R.descent_inputs(seed)
    start = R.concordance(R.pair_counts(z, R.DESCENT["dims"], attrs))
    assert float(start.max()) < 0.75                                            # it does not start there: random is 0.5
    for dtype in (torch.float64, torch.float32):
        out, first = R.descend(z, attrs, dtype, 25)
        print(f"seed {seed} {dtype}: concordance {start} -> 1.0 after {first} steps")
        assert first is not None and first <= 25
        assert bool((R.concordance(R.pair_counts(out, R.DESCENT["dims"], attrs)) == 1.0).all())
        assert np.array_equal(out[:, 1:3], z[:, 1:3].astype(out.dtype))


# =============================================================================== 3. the binding and the entries
WANT = {"inet_measure_attrs": ("int", 12), "inet_attr_reg_ws_bytes": ("int64_t", 2), "inet_attr_reg": ("int", 14)}


def test_binding_has_the_headers_arity_and_types():
    text = open(os.path.join(ROOT, "include", "inpaintnet_hip.h")).read()
    from tests.test_integration_doc import quoted_argtypes
    quoted = dict(quoted_argtypes())
    for name, (res, arity) in WANT.items():
        proto = re.search(r"^(\w+)\s+%s\(([^)]*)\);" % name, text, re.M)
        assert proto and proto.group(1) == res, name
        params = [p.strip() for p in proto.group(2).split(",")]
        assert len(params) == arity, name
        r, argtypes = _lib._SIGNATURES[name]
        assert r is (C.c_int64 if res == "int64_t" else C.c_int) and len(argtypes) == arity and name in _lib.EXPORTS
        for prm, t in zip(params, argtypes):
            if "*" in prm:
                assert t is C.c_void_p, (name, prm)
            elif prm.startswith("int64_t"):
                assert t is C.c_int64, (name, prm)
            elif prm.startswith("float"):
                assert t is C.c_float, (name, prm)
            elif prm.startswith("double"):
                assert t is C.c_double, (name, prm)
            else:
                assert prm.startswith("int ") and t is C.c_int, (name, prm)
        assert name in quoted and [C.sizeof(t) for t in quoted[name]] == [C.sizeof(t) for t in argtypes], name
    from inpaintnet_amd import ops
    for fn, entry, n in ((ops.attr_reg, "inet_attr_reg", 14), (ops.measure_attributes, "inet_measure_attrs", 12)):
        calls = [c for c in ast.walk(ast.parse(inspect.getsource(fn)))
                 if isinstance(c, ast.Call) and isinstance(c.func, ast.Attribute) and c.func.attr == entry]
        assert len(calls) == 1 and len(calls[0].args) == n
    assert "attr.hip" in _lib.SOURCES and ops.ATTR_MAX_DIMS == R.MAX_A
    assert not [k for k in re.findall(r"INET_[A-Z0-9_]+", open(os.path.join(ROOT, "inpaintnet_amd", "attributes.py")).read())]


@pytest.fixture(scope="module")
def L():
    _lib.build(verbose=False)
    return _lib.lib()


X = C.c_void_p(16)                     # a pointer that is never followed: every call below is refused in front of the launch
NULL = None


def _dims(*d):
    return (C.c_int32 * len(d))(*d)


def test_entries_refuse_bad_arguments_before_any_launch(L):
    reg = lambda z=X, B=4, Z=4, dims=_dims(0, 3), A=2, attrs=X, delta=10.0, coeff=1.0, out=X, counts=X, grad=X, ws=X, nb=1 << 20: \
        L.inet_attr_reg(z, B, Z, dims, A, attrs, delta, coeff, out, counts, grad, ws, nb, NULL)
    calls = {
        "z": reg(z=NULL), "dims": reg(dims=NULL), "attrs": reg(attrs=NULL), "out": reg(out=NULL), "counts": reg(counts=NULL),
        "B 0": reg(B=0), "B < 0": reg(B=-2), "B > 2^24": reg(B=(1 << 24) + 1), "Z 0": reg(Z=0), "A 0": reg(A=0),
        "A 9": reg(dims=_dims(*range(9)), A=9, Z=16), "dup": reg(dims=_dims(1, 1)), "dim = Z": reg(dims=_dims(0, 4)),
        "dim < 0": reg(dims=_dims(-1, 2)), "delta nan": reg(delta=float("nan")), "delta inf": reg(delta=math.inf),
        "delta -inf": reg(delta=-math.inf), "coeff nan": reg(coeff=float("nan")), "coeff inf": reg(coeff=math.inf),
        "ws null": reg(ws=NULL), "ws small": reg(nb=31), "ws 0": reg(nb=0),
    }
    assert {k: v for k, v in calls.items() if v != -1} == {}
    assert L.inet_attr_reg_ws_bytes(0, 1) == -1 and L.inet_attr_reg_ws_bytes(4, 0) == -1 and L.inet_attr_reg_ws_bytes(4, 9) == -1
    assert L.inet_attr_reg_ws_bytes((1 << 24) + 1, 1) == -1
    # a float and three ints per attribute and row block
    assert L.inet_attr_reg_ws_bytes(4, 2) == 32 and L.inet_attr_reg_ws_bytes(256, 4) == 16 * 4 * 16
    assert L.inet_attr_reg_ws_bytes(17, 1) == 2 * 16 and L.inet_attr_reg_ws_bytes(4096, 8) == 256 * 8 * 16
    att = lambda tok=X, B=4, T=24, V=20, slur=0, rest=1, none=2, midi=X, lo=55, hi=84, out=X: \
        L.inet_measure_attrs(tok, B, T, V, slur, rest, none, midi, lo, hi, out, NULL)
    calls = {
        "tokens": att(tok=NULL), "midi": att(midi=NULL), "out": att(out=NULL), "B 0": att(B=0), "B > 2^24": att(B=(1 << 24) + 1),
        "T 7": att(T=7), "T 0": att(T=0), "T -6": att(T=-6), "T 102": att(T=102), "T 25": att(T=25), "V 0": att(V=0),
        "slur = V": att(slur=20), "rest < -1": att(rest=-2), "none = V": att(none=20), "hi = lo": att(lo=60, hi=60), "hi < lo": att(lo=84, hi=55),
    }
    assert {k: v for k, v in calls.items() if v != -1} == {}


def test_ops_refuse_bad_arguments():
    from inpaintnet_amd import ops
    from inpaintnet_amd.attributes import AttributeSpec
    for dims in ([], list(range(9)), [0, 0], [0, 16], [-1], [0.0], [True], 3, ["0"]):
        with pytest.raises(ValueError, match="attr_reg"):
            ops.attr_dims(dims, 16)
    assert ops.attr_dims((3, 0, 15), 16) == [3, 0, 15]
    z, a = torch.zeros(4, 6), torch.zeros(4, 2)
    with pytest.raises(ValueError, match="device tensor"):                      # (host tensors: refused in front of everything else)
        ops.attr_reg(z, [0, 1], a)
    spec = AttributeSpec(**R.SPEC)
    with pytest.raises(ValueError, match="device tensor"):
        ops.measure_attributes(torch.zeros(4, 24, dtype=torch.int64), spec)
    with pytest.raises(ValueError, match="AttributeSpec"):
        ops.measure_attributes(torch.zeros(4, 24, dtype=torch.int64), R.SPEC)
    src = inspect.getsource(ops.attr_reg)
    for word in ("delta must be finite", "coeff must be finite", "attrs must be", "z must be"):
        assert word in src, word
    assert "multiple of 6" in inspect.getsource(ops.measure_attributes)


# =============================================================================== 4. AttributeSpec
class _Dataset:
    def __init__(self, names):
        self.note2index_dicts = [{n: i for i, n in enumerate(names)}]


def test_pitch_names_are_parsed_without_music21():
    from inpaintnet_amd import ATTRIBUTES, AttributeSpec, attributes
    assert "import music21" not in inspect.getsource(attributes)
    assert ATTRIBUTES == R.COLUMNS and AttributeSpec is attributes.AttributeSpec
    for name, midi in (("G3", 55), ("F#4", 66), ("B-4", 70), ("C4", 60), ("C6", 84), ("E-4", 63), ("C##4", 62), ("D--4", 60),
                       ("A0", 21), ("C-1", 23), ("c4", 60)):
        assert attributes.pitch_midi(name) == midi, name
    for name in ("__", "rest", None, "START", "END", "H4", "G", "4", 7, "G3 ", "G#-4"):
        assert attributes.pitch_midi(name) is None, name
    spec = AttributeSpec.from_dataset(_Dataset(R.VOCAB))
    assert spec == AttributeSpec(**R.SPEC) and spec.midi.dtype == np.int32 and tuple(spec.midi) == R.VOCAB_MIDI
    assert (spec.slur_index, spec.rest_index, spec.none_index, spec.pitch_range) == (0, 1, 2, (55, 84))
    assert AttributeSpec(**spec.state()) == spec
    # a vocabulary without a rest or None: -1
    s2 = AttributeSpec.from_dataset(_Dataset(("C4", "__", "D4")))
    assert (s2.slur_index, s2.rest_index, s2.none_index) == (1, -1, -1) and list(s2.midi) == [60, -1, 62]
    ds = _Dataset(R.VOCAB)
    ds.pitch_range = [50, 90]
    assert AttributeSpec.from_dataset(ds).pitch_range == (50, 90)


def test_from_dataset_refuses_a_vocabulary_without_names():
    from inpaintnet_amd import AttributeSpec, synthetic
    with pytest.raises(ValueError, match="pitch name"):
        AttributeSpec.from_dataset(synthetic.SyntheticFolkDataset(num_notes=20))
    with pytest.raises(ValueError, match="note2index_dicts"):
        AttributeSpec.from_dataset(object())


@pytest.mark.parametrize("kw", [dict(num_tokens=0), dict(num_tokens=2.0), dict(slur_index=20), dict(rest_index=-2), dict(none_index=1.0),
                                dict(midi=(60,) * 19), dict(midi=[0.5] * 20), dict(midi=[128] * 20), dict(midi=[-2] * 20),
                                dict(pitch_range=(60, 60)), dict(pitch_range=(84, 55)), dict(pitch_range=55)])
def test_attribute_spec_refuses_bad_values(kw):
    from inpaintnet_amd import AttributeSpec
    with pytest.raises(ValueError, match="AttributeSpec"):
        AttributeSpec(**dict(R.SPEC, **kw))


def test_spec_never_gives_the_three_symbols_a_pitch():
    from inpaintnet_amd import AttributeSpec
    spec = AttributeSpec(20, 0, 1, 2, [60] * 20)
    assert list(spec.midi[:4]) == [-1, -1, -1, 60]


# =============================================================================== 5. the trainer's keywords
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


def _trainer(model=None, **kw):
    from inpaintnet_amd.vae_trainer import VAETrainer
    return VAETrainer(None, model or _HostModel(), **kw)


@pytest.fixture(autouse=True)
def _no_gc_freeze(monkeypatch):
    monkeypatch.setenv("INET_GC_FREEZE", "0")


@pytest.mark.parametrize("kw", [{"attr_reg": {}}, {"attr_reg": ["num_notes"]}, {"attr_reg": "num_notes"}, {"attr_reg": {"notes": 0}},
                                {"attr_reg": {"num_notes": -1}}, {"attr_reg": {"num_notes": 0.0}}, {"attr_reg": {"num_notes": True}},
                                {"attr_reg": {"num_notes": 1, "note_range": 1}}, {"attr_reg": {0: 0}},
                                {"attr_gamma": -1.0}, {"attr_gamma": float("nan")}, {"attr_gamma": math.inf}, {"attr_gamma": "10"},
                                {"attr_gamma": True}, {"attr_delta": 0.0}, {"attr_delta": -1.0}, {"attr_delta": float("nan")},
                                {"attr_delta": math.inf}, {"attr_delta": None}, {"attr_spec": R.SPEC}, {"attr_spec": 3}])
def test_trainer_rejects_bad_keywords_before_touching_the_model(kw):
    with pytest.raises(ValueError, match="attr_reg|attr_gamma|attr_delta|attr_spec"):
        _trainer(_Untouchable(), **kw)


def test_trainer_rejects_a_dimension_outside_z_dim_and_a_dataset_without_names():
    from inpaintnet_amd import AttributeSpec, synthetic
    from inpaintnet_amd.vae_trainer import VAETrainer
    spec = AttributeSpec(**R.SPEC)
    with pytest.raises(ValueError, match="z_dim"):
        _trainer(attr_reg={"num_notes": 8}, attr_spec=spec)
    assert _trainer(attr_reg={"num_notes": 7}, attr_spec=spec).attr_reg == {"num_notes": 7}
    with pytest.raises(ValueError, match="pitch name"):
        VAETrainer(synthetic.SyntheticFolkDataset(num_notes=20), _HostModel(), attr_reg={"num_notes": 0})
    assert VAETrainer(_Dataset(R.VOCAB), _HostModel(), attr_reg={"num_notes": 0}).attr_spec == spec


def test_defaults_leave_the_trainer_as_it_was():
    from inpaintnet_amd.vae_trainer import VAETrainer
    prm = inspect.signature(VAETrainer.__init__).parameters
    assert VAETrainer.ATTR_SETTINGS == ("attr_reg", "attr_gamma", "attr_delta", "attr_spec")
    assert [prm[k].default for k in VAETrainer.ATTR_SETTINGS] == [None, 10.0, 10.0, None]
    assert list(prm)[-4:] == list(VAETrainer.ATTR_SETTINGS)                     # appended: no positional argument moved
    tr = _trainer()
    assert tr.attr_reg is None and tr.last_attr_reg is None and tr.attr_spec is None
    # _add_attr_reg hands the loss through untouched and touches nothing else
    marker = object()
    assert tr._add_attr_reg(marker, None, None, True) is marker and tr.last_attr_reg is None
    src = inspect.getsource(VAETrainer.loss_and_acc_for_batch)
    assert src.count("self._add_attr_reg(self._add_mmd(loss, z_tilde, z_prior, train), z_tilde, score, train)") == 2


def test_training_state_round_trip_carries_the_four_settings():
    from inpaintnet_amd import AttributeSpec
    spec = AttributeSpec(**R.SPEC)
    a = _trainer(attr_reg={"note_range": 3, "num_notes": 0}, attr_gamma=2.5, attr_delta=4.0, attr_spec=spec, mmd_coeff=3.0)
    st = a.training_state(3)
    assert st["attr_reg"] == {"note_range": 3, "num_notes": 0} and list(st["attr_reg"]) == ["note_range", "num_notes"]
    assert (st["attr_gamma"], st["attr_delta"], st["attr_spec"]) == (2.5, 4.0, spec.state())
    assert all(type(v) in (int, list, tuple) for v in st["attr_spec"].values())  # plain values: torch.load needs no class of ours
    b = _trainer()
    assert b.load_training_state(st) == 3
    assert (b.attr_reg, b.attr_gamma, b.attr_delta, b.attr_spec, b.mmd_coeff) == ({"note_range": 3, "num_notes": 0}, 2.5, 4.0, spec, 3.0)
    # a state written before the settings existed leaves this trainer's own
    old = {k: v for k, v in a.training_state(2).items() if k not in a.ATTR_SETTINGS}
    d = _trainer(attr_reg={"beat_strength": 5}, attr_gamma=1.0, attr_spec=spec)
    assert d.load_training_state(old) == 2
    assert (d.attr_reg, d.attr_gamma, d.attr_delta, d.attr_spec) == ({"beat_strength": 5}, 1.0, 10.0, spec)
    # ... and a default trainer's state switches the term off
    assert d.load_training_state(_trainer().training_state(1)) == 1 and d.attr_reg is None
