"""The class-weighted, label-smoothed cross-entropy kernels alone (csrc/ce.hip through ops.class_counts / ops.cross_entropy_w,
DESIGN.md section 28) against the float64 restatement tests/ce_w_ref.py, which tests/test_ce_w_host.py holds equal to torch.

Shapes: the smallest at which a wave-per-row kernel with a finishing pass can go wrong -- V in {1, 2, 63, 64, 65, 130} (one, two and
three values a lane, around the 64-lane wrap), rows in {1, 5, 48, 1025} (one wave, less than a workgroup, several workgroups, the
grid-stride tail of the 128-workgroup launch) -- plus V = 300 (the row no longer fits the registers) and V = 1030 (class weights and
histograms no longer fit LDS), the two sizes at which the kernel takes another path.  Inputs are strided with NaN / inf in the
padding, dW with a sentinel in its padding; logits are post-ReLU (tests/test_gpu_pointwise.py's relu_logits).

Bounds: the plain kernel's there -- loss 1e-4 relative, dW relmax < 1e-5; denom 1e-6 relative (a double sum of at most V
float-times-integer products); every integer exactly."""
import math

import numpy as np
import pytest
import torch

from tests import ce_w_ref as R

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from inpaintnet_amd import ops
    from tests.test_gpu_pointwise import DEV, SENT, gen, relmax, relu_logits, strided

VS = [1, 2, 63, 64, 65, 130]
ROWS = [1, 5, 48, 1025]
IGN = -100


def _weights(V, g):
    """Random class weights in [0.1, 2.1) with a zero where the vocabulary has room for one."""
    w = torch.rand(V, generator=g) * 2.0 + 0.1
    if V > 1:
        w[V // 2] = 0.0
    return w


def _ignored(t, rows):
    """Every fifth row ignored, and the first and the last where there are five or more."""
    t = t.clone()
    t[3::5] = IGN
    if rows >= 5:
        t[0] = t[-1] = IGN
    return t


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def run(w, t, cw=None, e=0.0, ii=None, want=("loss", "acc", "dW", "stats", "conf"), counted=None, **glue):
    """ops.class_counts + ops.cross_entropy_w on strided logits into a strided dW; every output behind guard words."""
    rows, V = w.shape
    wv, _ = strided(w, 3, "poison")
    td = t.to(DEV)
    cwd = None if cw is None else cw.to(DEV)
    counted = ops.class_counts(td, V, cwd, ii) if counted is None else counted
    out = torch.full((5,), SENT, device=DEV)
    dv = dbuf = stats = conf = None
    if "dW" in want:
        dv, dbuf = strided(torch.full((rows, V), SENT), 2, SENT)
    if "stats" in want:
        stats = torch.zeros(V, 3, dtype=torch.int64, device=DEV)
    if "conf" in want:
        conf = torch.zeros(V, V, dtype=torch.int64, device=DEV)
    ops.cross_entropy_w(wv, td, counted, cwd, e, ii, loss=out[1:2] if "loss" in want else None,
                        accuracy=out[3:4] if "acc" in want else None, dW=dv, class_stats=stats, confusion=conf, **glue)
    torch.cuda.synchronize()
    o = out.cpu()
    assert o[0] == SENT and o[2] == SENT and o[4] == SENT
    assert ("loss" in want) or o[1] == SENT
    assert ("acc" in want) or o[3] == SENT
    if dv is not None:
        assert bool((dbuf[:, V:] == SENT).all()), "dW padding written"
    return dict(loss=o[1], acc=o[3], dW=None if dv is None else dv.cpu(), stats=None if stats is None else stats.cpu().numpy(),
                conf=None if conf is None else conf.cpu().numpy(), counted=counted)


def _assert_matches(got, ref, tag):
    c = got["counted"]
    denom, n_valid, n_bad = float(c.denom), int(c.n_valid), int(c.n_bad)
    print(f"{tag}: loss {float(got['loss'])} ref {ref['loss']}; dW {relmax(got['dW'], ref['grad']):.2e}; denom {denom} ref {ref['denom']}")
    assert abs(float(got["loss"]) - ref["loss"]) <= 1e-4 * abs(ref["loss"])
    assert relmax(got["dW"], ref["grad"]) < 1e-5
    assert abs(denom - ref["denom"]) <= 1e-6 * abs(ref["denom"])
    assert (n_valid, n_bad) == (ref["n_valid"], ref["n_bad"])
    assert np.array_equal(c.counts.cpu().numpy(), ref["counts"])
    assert np.array_equal(got["stats"], ref["stats"]) and np.array_equal(got["conf"], ref["confusion"])
    assert abs(float(got["acc"]) - ref["accuracy"]) <= 1e-6 * ref["accuracy"] + 1e-12        # one double division, one rounding to float


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("V", VS)
def test_weights_smoothing_and_ignored_rows_match_the_restatement(rows, V):
    g = gen(28, rows, V)
    w, t = relu_logits(rows, V, g)
    cw, t = _weights(V, g), _ignored(t, rows)
    if V > 1 and rows > 1:
        t[1] = V // 2                                                           # a target of weight 0: in the statistics, not in the loss
    ref = R.evaluate(w.numpy(), t.numpy(), cw.numpy(), 0.1, IGN)
    got = run(w, t, cw, 0.1, IGN)
    if ref["denom"] == 0.0:                                                     # rows = 1 with its only target at weight 0
        assert math.isnan(float(got["loss"])) and not got["dW"].any()
        return
    _assert_matches(got, ref, f"rows {rows} V {V}")
    ign = (t == IGN).numpy()
    assert not got["dW"][ign].any() and got["stats"][:, 0].sum() == rows - ign.sum() == got["conf"].sum()
    # the same bits across two calls, with or without dW, and from the gradient-only launch on the forward's count
    again = run(w, t, cw, 0.1, IGN)
    assert _same_bits(again["loss"], got["loss"]) and _same_bits(again["acc"], got["acc"]) and _same_bits(again["dW"], got["dW"])
    assert _same_bits(again["counted"].block[:3], got["counted"].block[:3])
    bare = run(w, t, cw, 0.1, IGN, want=("loss", "acc"))
    assert _same_bits(bare["loss"], got["loss"]) and _same_bits(bare["acc"], got["acc"])
    only = run(w, t, cw, 0.1, IGN, want=("dW",), counted=got["counted"])
    assert _same_bits(only["dW"], got["dW"])


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("V", VS)
def test_all_options_off_is_the_plain_kernel_bit_for_bit(rows, V):
    """weight=None, e = 0, nothing ignored: dW and the hit count are inet_cross_entropy_ex's bits (its scale = float32(1 / rows), the
    correctly rounded reciprocal of the denominator), the loss within the 1e-4 bound."""
    w, t = relu_logits(rows, V, gen(29, rows, V))
    got = run(w, t)
    wv, _ = strided(w, 3, "poison")
    dv, _ = strided(torch.zeros(rows, V), 2, SENT)
    acc = torch.zeros(2, device=DEV)
    ops.cross_entropy_ex(wv, t.to(DEV), loss_sum=acc[0:1], correct=acc[1:2], dW=dv, scale=1.0 / rows)
    torch.cuda.synchronize()
    assert _same_bits(got["dW"], dv.cpu())
    assert float(acc[1]) == float(got["stats"][:, 1].sum())
    ref = R.evaluate(w.numpy(), t.numpy())
    assert abs(float(got["loss"]) - ref["loss"]) <= 1e-4 * abs(ref["loss"])
    assert abs(float(got["loss"]) - float(acc[0]) / rows) <= 1e-4 * abs(ref["loss"])
    assert float(got["counted"].denom) == rows and np.array_equal(got["stats"], ref["stats"])
    assert float(got["acc"]) == float(np.float32(ref["stats"][:, 1].sum() / rows))


@pytest.mark.parametrize("V,cw_on,e", [(300, True, 0.1), (300, False, 0.0), (1030, True, 0.1), (1030, False, 0.0)])
def test_vocabularies_beyond_the_registers_and_beyond_lds(V, cw_on, e):
    rows = 5
    g = gen(30, V)
    w, t = relu_logits(rows, V, g)
    t[2] = IGN
    cw = _weights(V, g) if cw_on else None
    ref = R.evaluate(w.numpy(), t.numpy(), None if cw is None else cw.numpy(), e, IGN)
    got = run(w, t, cw, e, IGN)
    _assert_matches(got, ref, f"V {V}")
    assert not got["dW"][2].any()
    assert _same_bits(run(w, t, cw, e, IGN, want=("dW",), counted=got["counted"])["dW"], got["dW"])


@pytest.mark.parametrize("V", [2, 65])
def test_denominator_zero_gives_a_nan_loss_and_a_zero_gradient(V):
    rows = 48
    w, t = relu_logits(rows, V, gen(31, V))
    # every row ignored
    got = run(w, torch.full((rows,), IGN), None, 0.1, IGN)
    assert math.isnan(float(got["loss"])) and math.isnan(float(got["acc"])) and not got["dW"].any()
    assert float(got["counted"].denom) == 0.0 and int(got["counted"].n_valid) == 0 and not got["stats"].any() and not got["conf"].any()
    # every present target has weight 0: the rows are valid and counted, the loss is NaN, dW all zeros (torch: NaN)
    cw = torch.ones(V)
    cw[0] = 0.0
    got = run(w, torch.zeros(rows, dtype=torch.int64), cw, 0.1, None)
    ref = R.evaluate(w.numpy(), np.zeros(rows, np.int64), cw.numpy(), 0.1, None)
    assert math.isnan(float(got["loss"])) and not got["dW"].any() and float(got["counted"].denom) == 0.0
    assert int(got["counted"].n_valid) == rows and np.array_equal(got["stats"], ref["stats"]) and np.array_equal(got["conf"], ref["confusion"])
    assert abs(float(got["acc"]) - ref["accuracy"]) <= 1e-6


def test_a_target_outside_the_vocabulary_is_never_an_index():
    """-1, V, 2^40 and -2^62 among the targets: the rows are treated as ignored and counted in n_bad; the counting launch sets the
    token status word, as a bad embedding index does.  The count buffer is exactly 8 + V words and dW exactly rows x ld: a write
    through such a target would land in the guard words or fault."""
    rows, V = 48, 65
    w, t = relu_logits(rows, V, gen(32))
    t[5], t[6], t[7], t[8], t[9] = -1, V, 1 << 40, -(1 << 62), IGN
    ops.token_status(reset=True)
    try:
        ref = R.evaluate(w.numpy(), t.numpy(), None, 0.0, IGN)
        assert (ref["n_bad"], ref["n_valid"]) == (4, rows - 5)
        got = run(w, t, None, 0.0, IGN)
        _assert_matches(got, ref, "bad targets")
        assert not got["dW"][5:10].any() and ops.token_status() >= 1
        with pytest.raises(ops.TokenRangeError):
            ops.check_tokens("test")
    finally:
        ops.token_status(reset=True)
    # nothing ignored by index: the same targets, IGN is now a bad one too
    try:
        got = run(w, t, _weights(V, gen(33)), 0.1, None)
        assert int(got["counted"].n_bad) == 5 and not got["dW"][5:10].any()
    finally:
        ops.token_status(reset=True)


def test_folded_terms_and_null_outputs():
    rows, V = 48, 65
    g = gen(34)
    w, t = relu_logits(rows, V, g)
    cw, t = _weights(V, g), _ignored(t, rows)
    ref = R.evaluate(w.numpy(), t.numpy(), cw.numpy(), 0.1, IGN)
    # add_term / add_scale: folded into the loss once, in double, one rounding
    add = torch.tensor([1000.0], device=DEV)
    got = run(w, t, cw, 0.1, IGN, add_term=add, add_scale=0.5)
    assert abs(float(got["loss"]) - (ref["loss"] + 500.0)) <= 1e-4 * (ref["loss"] + 500.0) and float(add[0]) == 1000.0
    assert relmax(got["dW"], ref["grad"]) < 1e-5
    # the device scale on dW, fwd_out = fwd_scale * scale_dev exactly (one float32 product)
    sd = torch.tensor([0.8125 + 1.0 / 3.0])
    fwd = torch.full((3,), SENT, device=DEV)
    got = run(w, t, cw, 0.1, IGN, want=("dW",), scale_dev=sd.to(DEV), fwd_out=fwd[1:2], fwd_scale=0.3)
    assert relmax(got["dW"], ref["grad"] * float(sd[0])) < 1e-5
    assert torch.equal(fwd.cpu(), torch.tensor([SENT, float((torch.tensor([0.3]) * sd)[0]), SENT]))
    # each output alone
    for want in (("loss",), ("acc",), ("dW",), ("stats",), ("conf",)):
        one = run(w, t, cw, 0.1, IGN, want=want)
        if want == ("loss",):
            assert abs(float(one["loss"]) - ref["loss"]) <= 1e-4 * ref["loss"]
        if want == ("acc",):
            assert abs(float(one["acc"]) - ref["accuracy"]) <= 1e-6
        if want == ("dW",):
            assert relmax(one["dW"], ref["grad"]) < 1e-5
        if want == ("stats",):
            assert np.array_equal(one["stats"], ref["stats"])
        if want == ("conf",):
            assert np.array_equal(one["conf"], ref["confusion"])
    # the statistics accumulate: a second batch on the same tensors doubles them
    td, cwd = t.to(DEV), cw.to(DEV)
    stats = torch.zeros(V, 3, dtype=torch.int64, device=DEV)
    conf = torch.zeros(V, V, dtype=torch.int64, device=DEV)
    for _ in range(2):
        ops.cross_entropy_w(w.to(DEV), td, ops.class_counts(td, V, cwd, IGN), cwd, 0.1, IGN, class_stats=stats, confusion=conf)
    assert np.array_equal(stats.cpu().numpy(), 2 * ref["stats"]) and np.array_equal(conf.cpu().numpy(), 2 * ref["confusion"])
    with pytest.raises(ValueError):
        ops.cross_entropy_w(w.to(DEV), td, ops.class_counts(td, V, cwd, IGN), cwd, 0.1, IGN)       # no output at all


@pytest.mark.parametrize("V", [3, 130, 1030])
def test_class_counts_over_many_workgroups(V):
    """100 003 targets: the 64 workgroups of the counting launch, each with a tail; bad and ignored targets among them."""
    n = 100003
    g = gen(35, V)
    t = torch.randint(0, V, (n,), generator=g)
    t[::1000] = IGN
    t[7::5000] = V + 5
    cw = _weights(V, g)
    want = R.counts(t.numpy(), V, cw.numpy(), IGN)
    try:
        a = ops.class_counts(t.to(DEV), V, cw.to(DEV), IGN, extra=5)
        b = ops.class_counts(t.to(DEV), V, cw.to(DEV), IGN)
        torch.cuda.synchronize()
    finally:
        ops.token_status(reset=True)
    assert np.array_equal(a.counts.cpu().numpy(), want["counts"]) and (int(a.n_valid), int(a.n_bad)) == (want["n_valid"], want["n_bad"])
    assert abs(float(a.denom) - want["denom"]) <= 1e-6 * want["denom"]
    assert torch.equal(a.block[:8 + V], b.block) and not a.extra.any() and a.extra.numel() == 5
    assert a.block[3] == min((n + 255) // 256, 64) and a.block[4] == 0          # the tickets: every workgroup counted, the loss's at 0
