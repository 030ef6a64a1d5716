"""The attribute kernels alone (csrc/attr.hip through ops.measure_attributes / ops.attr_reg and the C entries)
against the float64 restatement tests/attr_ref.py: the extractors exactly (one float operation on one exact integer; logf within 2
ulp), the pair loss within the bounds derived there, the counts as integers, at every batch size at which a kernel takes another path."""
import numpy as np
import pytest
import torch

from tests import attr_ref as R

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from inpaintnet_amd import _lib, ops
    from inpaintnet_amd._lib import ptr, stream_ptr
    from inpaintnet_amd.attributes import AttributeSpec

SENT = -777.25
ISENT = -777


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _spec():
    return AttributeSpec(**R.SPEC)


def _assert_attrs(got, tokens, what):
    """got [B, 4] float32 from the device against the restatement cast to float32: equal, logf within 2 ulp, NaN rows NaN."""
    want = R.measure_attrs(tokens, **R.SPEC)
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.float32, what
    nan = np.isnan(want[:, 0])
    assert np.isnan(got[nan]).all() and not np.isnan(got[~nan]).any(), what
    w32 = want[~nan].astype(np.float32)
    g = got[~nan]
    for col in (0, 1, 3):
        assert np.array_equal(g[:, col], w32[:, col]), (what, R.COLUMNS[col])
    ulp = np.spacing(np.abs(w32[:, 2]))
    err = np.abs(g[:, 2].astype(np.float64) - want[~nan][:, 2])
    print(f"{what}: rhy_entropy max err {float((err / np.maximum(ulp, 1e-300)).max()) if len(err) else 0:.3g} ulp")
    assert bool((err <= R.LOG_ULP * ulp).all()), what
    assert bool((g[:, 2][want[~nan][:, 2] == 0.0] == 0.0).all())                 # logf(1) and the n = 0 rule: exactly 0


# =============================================================================== inet_measure_attrs
@pytest.mark.parametrize("T", [6, 24])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 257])
def test_extractors_are_exact_against_the_restatement(B, T):
    tok = R.draw_tokens(f"gpu/{B}x{T}", B, T)
    got = ops.measure_attributes(_dev(tok), _spec())
    _assert_attrs(got, tok, f"({B}, {T})")
    frac = [(tok == R.SPEC["slur_index"]).mean(), (tok == R.SPEC["rest_index"]).mean()]
    if B * T >= 6000:                                                           # (three standard deviations of a share are below 0.02 there)
        assert abs(frac[0] - 0.4) < 0.03 and abs(frac[1] - 0.1) < 0.03


@pytest.mark.parametrize("T", [6, 24])
def test_edge_rows_and_an_out_of_range_token(T):
    e = R.edge_rows(T)
    bad_hi, bad_lo = e["one_pitch"].copy(), e["full_range"].copy()
    bad_hi[T - 1] = R.SPEC["num_tokens"]
    bad_lo[0] = -1
    big = e["one_pitch"].copy()
    big[2] = 1 << 40                                                            # far outside int32: must not wrap into the table
    names = ["all_slur", "all_rest", "no_pitch", "one_pitch", "full_range"]
    rows = [e[k] for k in names] + [e["one_pitch"], bad_hi, e["one_pitch"], bad_lo, e["full_range"], big, e["all_rest"]]
    # ... in the middle of 70 drawn rows, so that the edge rows straddle the 64-row boundary of a workgroup
    drawn = R.draw_tokens(f"gpu/edge{T}", 70, T)
    tok = np.concatenate([drawn[:58], np.stack(rows), drawn[58:]], 0)
    got = ops.measure_attributes(_dev(tok), _spec())
    _assert_attrs(got, tok, f"edge rows T = {T}")
    g = got.cpu().numpy()[58:58 + len(rows)]
    assert list(g[0]) == [0.0, 0.0, 0.0, 0.0]                                   # all-slur: n = 0 gives entropy 0, not NaN
    assert g[1][0] == 0.0 and g[1][1] == 0.0 and g[2][1] == 0.0 and g[3][1] == 0.0 and g[4][1] == 1.0
    assert np.isnan(g[6]).all() and np.isnan(g[8]).all() and np.isnan(g[10]).all()
    assert np.array_equal(g[5], g[3]) and np.array_equal(g[7], g[3]) and np.array_equal(g[9], g[4]) and np.array_equal(g[11], g[1])


@pytest.mark.parametrize("B,T", [(1, 6), (65, 24)])
def test_extractor_output_stays_inside_its_buffer(B, T):
    tok = _dev(R.draw_tokens(f"gpu/sent{B}", B, T))
    spec = _spec()
    buf = torch.full((B * 4 + 2,), SENT, device="cuda")
    rc = _lib.lib().inet_measure_attrs(ptr(tok), B, T, spec.num_tokens, spec.slur_index, spec.rest_index, spec.none_index,
                                       ptr(spec.midi_table(tok.device)), 55, 84, ptr(buf[1:-1]), stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    b = buf.cpu()
    assert b[0] == SENT and b[-1] == SENT
    assert torch.equal(b[1:-1].view(B, 4), ops.measure_attributes(tok, spec).cpu())


def test_extractor_refuses_bad_shapes():
    spec = _spec()
    for bad in (lambda: ops.measure_attributes(torch.zeros(4, 7, dtype=torch.int64, device="cuda"), spec),
                lambda: ops.measure_attributes(torch.zeros(4, 102, dtype=torch.int64, device="cuda"), spec),
                lambda: ops.measure_attributes(torch.zeros(4, 24, dtype=torch.int32, device="cuda"), spec),
                lambda: ops.measure_attributes(torch.zeros(24, dtype=torch.int64, device="cuda"), spec),
                lambda: ops.measure_attributes(torch.zeros(4, 48, dtype=torch.int64, device="cuda")[:, ::2], spec),
                lambda: ops.measure_attributes(torch.zeros(0, 24, dtype=torch.int64, device="cuda"), spec)):
        with pytest.raises(ValueError, match="measure_attributes"):
            bad()


# =============================================================================== inet_attr_reg
def _check(out, counts, grad, e, what):
    o = out.double().cpu().numpy()
    err = abs(o[0] - e["value"])
    print(f"{what}: value {o[0]:.9g} ref {e['value']:.9g} err {err:.3g} bound {e['value_bound']:.3g}; per_attr worst err / bound "
          f"{float((np.abs(o[1:] - e['per_attr']) / np.maximum(e['per_bound'], 1e-300)).max()):.3g}")
    assert e["value_bound"] <= 1e-4 * e["scale"]                                # a wider bound would be vacuous
    assert err <= e["value_bound"], what
    assert bool((np.abs(o[1:] - e["per_attr"]) <= e["per_bound"]).all()), what
    assert counts.dtype == torch.int64 and np.array_equal(counts.cpu().numpy(), e["counts"]), what
    if grad is not None:
        g = grad.double().cpu().numpy()
        worst = float((np.abs(g - e["grad"]) / np.maximum(e["grad_bound"], 1e-300)).max())
        print(f"{what}: grad max |err| {np.abs(g - e['grad']).max():.3g} of max |g| {np.abs(e['grad']).max():.3g}; "
              f"worst err / bound {worst:.3g}")
        assert g.shape == e["grad"].shape and bool((np.abs(g - e["grad"]) <= e["grad_bound"]).all()), what


@pytest.mark.parametrize("B,Z,A,kind", R.CASES)
def test_attr_reg_against_float64_within_the_derived_bounds(B, Z, A, kind):
    z, attrs = R.inputs(B, Z, A, kind)
    zd, ad = _dev(z), _dev(attrs)
    for delta in R.DELTAS:
        for coeff in R.COEFFS:
            _, dims, _, e = R.case(B, Z, A, kind, delta, coeff)
            if kind == "cont" and B >= 16:
                assert float(e["untied"].min()) >= 0.9                          # a wrong sign cannot hide behind ties
            if kind == "tied":
                assert float((1.0 - e["untied"]).min()) >= 0.1 and float(e["untied"].min()) >= 0.5
            bits = None
            for want_grad in (False, True):
                out, counts, grad = ops.attr_reg(zd, dims, ad, delta, coeff, want_grad=want_grad)
                assert out.shape == (1 + A,) and counts.shape == (A, 3) and (grad is None) == (not want_grad)
                _check(out, counts, grad, e, f"({B}, {Z}, {A}) {kind} dims {dims} delta {delta} coeff {coeff} grad {want_grad}")
                if bits is not None:                                            # the value does not depend on the gradient phase
                    assert torch.equal(bits, out.view(torch.int32))
                bits = out.view(torch.int32).clone()


def test_one_measure_gives_zero():
    out, counts, grad = ops.attr_reg(torch.full((1, 3), 0.7, device="cuda"), [2], torch.full((1, 1), 0.3, device="cuda"), want_grad=True)
    assert out.tolist() == [0.0, 0.0] and counts.tolist() == [[0, 0, 0]] and grad.tolist() == [[0.0]]


def test_all_attributes_equal_ties_every_pair():
    B = 37
    z, _ = R.inputs(300, 256, 4, "cont")
    z = z[:B]
    attrs = np.full((B, 2), 0.25, np.float32)
    e = R.evaluate(z, [0, 255], attrs, 10.0, 1.0)
    out, counts, grad = ops.attr_reg(_dev(z), [0, 255], _dev(attrs), want_grad=True)
    assert counts.tolist() == [[0, 0, B * (B - 1)]] * 2
    _check(out, counts, grad, e, "all attributes equal")


def test_duplicate_latents_have_sign_zero():
    """Two measures with the same z and different attributes: neither concordant nor discordant, |0 - s| = 1 each way, and the two
    gradient terms sgn(0 - s)(1 - 0) cancel between them only through their own rows."""
    z = np.array([[0.5], [0.5], [-1.0]], np.float32)
    attrs = np.array([[1.0], [2.0], [3.0]], np.float32)
    e = R.evaluate(z, [0], attrs, 1.0, 1.0)
    out, counts, grad = ops.attr_reg(_dev(z), [0], _dev(attrs), 1.0, 1.0, want_grad=True)
    assert e["counts"].tolist() == [[0, 4, 0]]
    _check(out, counts, grad, e, "duplicate z")


def test_two_calls_give_identical_bits():
    B, Z, A, kind = 300, 256, 8, "tied"
    z, attrs = R.inputs(B, Z, A, kind)
    zd, ad, dims = _dev(z), _dev(attrs), R.dims_for(Z, A)
    o1, c1, g1 = ops.attr_reg(zd, dims, ad, 10.0, 10.0, want_grad=True)
    filler = torch.randn(1 << 20, device="cuda")                                 # other work in between, other workspace memory
    o2, c2, g2 = ops.attr_reg(zd, dims, ad, 10.0, 10.0, want_grad=True)
    o3, c3, _ = ops.attr_reg(zd, dims, ad, 10.0, 10.0)
    del filler
    assert torch.equal(o1.view(torch.int32), o2.view(torch.int32)) and torch.equal(g1.view(torch.int32), g2.view(torch.int32))
    assert torch.equal(o1.view(torch.int32), o3.view(torch.int32))               # the value does not depend on the gradient phase
    assert torch.equal(c1, c2) and torch.equal(c1, c3)


def test_a_nan_in_z_reaches_the_value():
    z, attrs = R.inputs(17, 256, 8, "cont")
    z = z.copy()
    z[16, 0] = np.nan                                                           # the one row of the second row block
    dims = [0, 255]
    out, counts, grad = ops.attr_reg(_dev(z), dims, _dev(attrs[:, :2]), want_grad=True)
    o = out.cpu().numpy()
    assert np.isnan(o[0]) and np.isnan(o[1]) and not np.isnan(o[2])             # ... through its own dimension only
    a = attrs.copy()
    a[3, 1] = np.nan
    o = ops.attr_reg(_dev(R.inputs(17, 256, 8, "cont")[0]), dims, _dev(a[:, :2]))[0].cpu().numpy()
    assert np.isnan(o[0]) and not np.isnan(o[1]) and np.isnan(o[2])


@pytest.mark.parametrize("B,Z,A", [(1, 1, 1), (7, 3, 1), (17, 256, 8), (257, 256, 4)])
def test_outputs_stay_inside_their_buffers(B, Z, A):
    """Guard words in front of and behind out, counts, grad and the workspace; without a gradient pointer grad's memory is not
    touched at all; every workspace row is written (nothing to zero in front)."""
    kind = "cont"
    z, dims, attrs, e = R.case(B, Z, A, kind, 10.0, 1.0)
    zd, ad = _dev(z), _dev(attrs)
    L = _lib.lib()
    nbytes = L.inet_attr_reg_ws_bytes(B, A)
    assert nbytes == R.cdiv(B, R.ROWS) * A * 16
    cdims = (_lib.C.c_int32 * A)(*dims)
    for want_grad in (True, False):
        obuf = torch.full((1 + A + 2,), SENT, device="cuda")
        cbuf = torch.full((3 * A + 2,), ISENT, dtype=torch.int64, device="cuda")
        gbuf = torch.full((B * A + 2,), SENT, device="cuda")
        ws = torch.full((nbytes // 4 + 2,), SENT, device="cuda")
        rc = L.inet_attr_reg(ptr(zd), B, Z, cdims, A, ptr(ad), 10.0, 1.0, ptr(obuf[1:-1]), ptr(cbuf[1:-1]),
                             ptr(gbuf[1:-1]) if want_grad else None, ptr(ws[1:-1]), nbytes, stream_ptr())
        assert rc == 0
        torch.cuda.synchronize()
        o, c, g, w = obuf.cpu(), cbuf.cpu(), gbuf.cpu(), ws.cpu()
        assert o[0] == SENT and o[-1] == SENT and c[0] == ISENT and c[-1] == ISENT and g[0] == SENT and g[-1] == SENT
        assert w[0] == SENT and w[-1] == SENT
        assert bool((w[1:-1].view(torch.int32) != torch.tensor(SENT).view(torch.int32)).all())
        _check(o[1:-1], c[1:-1].view(A, 3), g[1:-1].view(B, A) if want_grad else None, e, f"guarded ({B}, {Z}, {A}) grad {want_grad}")
        if not want_grad:
            assert bool((g == SENT).all())


def test_bad_arguments_are_refused():
    z, a = torch.zeros(4, 6, device="cuda"), torch.zeros(4, 2, device="cuda")
    for bad in (lambda: ops.attr_reg(z, [0, 0], a), lambda: ops.attr_reg(z, [0, 6], a), lambda: ops.attr_reg(z, [-1, 2], a),
                lambda: ops.attr_reg(torch.zeros(4, 16, device="cuda"), list(range(9)), torch.zeros(4, 9, device="cuda")),
                lambda: ops.attr_reg(z, [], torch.zeros(4, 0, device="cuda")), lambda: ops.attr_reg(z, [0, 1], a, delta=float("inf")),
                lambda: ops.attr_reg(z, [0, 1], a, delta=float("nan")), lambda: ops.attr_reg(z, [0, 1], a, delta=1e39),
                lambda: ops.attr_reg(z, [0, 1], a, coeff=float("nan")), lambda: ops.attr_reg(z, [0, 1], a[:, :1].contiguous()),
                lambda: ops.attr_reg(z, [0, 1], a[:3]), lambda: ops.attr_reg(z[0], [0], a), lambda: ops.attr_reg(z.double(), [0, 1], a),
                lambda: ops.attr_reg(z, [0, 1], torch.zeros(4, 4, device="cuda")[:, ::2])):
        with pytest.raises(ValueError, match="attr_reg"):
            bad()


# =============================================================================== descent on the kernel alone
@pytest.mark.parametrize("seed", R.DESCENT["seeds"])
def test_the_kernels_gradient_alone_sorts_the_dimensions(seed):
    """50 steps of z[:, dims] -= 4 G with the kernel's own G: both regularised dimensions end up ordering the measures exactly as
    their attributes do, and the other two columns keep their bits.  (The restatement gets there within 25 steps:
    tests/test_attr_host.py.)"""
    D = R.DESCENT
    z0, attrs = R.descent_inputs(seed)
    z, ad = _dev(z0), _dev(attrs)
    for _ in range(D["steps"]):
        _, _, G = ops.attr_reg(z, D["dims"], ad, D["delta"], D["coeff"], want_grad=True)
        z[:, D["dims"]] -= D["lr"] * G
    out, counts, _ = ops.attr_reg(z, D["dims"], ad, D["delta"], D["coeff"])
    c = counts.cpu().numpy()
    print(f"seed {seed}: counts {c.tolist()} per_attr {out[1:].tolist()}")
    assert np.array_equal(c, R.pair_counts(z.cpu().numpy(), D["dims"], attrs))
    assert bool((R.concordance(c) == 1.0).all())
    assert np.array_equal(z.cpu().numpy()[:, 1:3].view(np.int32), z0[:, 1:3].view(np.int32))
