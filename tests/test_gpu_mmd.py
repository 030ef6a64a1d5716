"""The MMD kernels alone (csrc/mmd.hip through ops.mmd / inet_mmd) against the float64 restatement
tests/mmd_ref.py within the bounds derived there: both kernels, the three estimators, with and without the gradient, at every shape
at which the kernel takes another path (one row, one row block, a ragged second block, a second column tile, one latent dimension past
a chunk and past the gradient's register span)."""
import numpy as np
import pytest
import torch

from tests import mmd_ref as M

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from inpaintnet_amd import _lib, ops
    from inpaintnet_amd._lib import ptr, stream_ptr

SENT = -777.25


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _check(out4, grad, e, what):
    o = out4.double().cpu().numpy()
    err = abs(o[0] - e["value"])
    print(f"{what}: value {o[0]:.9g} ref {e['value']:.9g} err {err:.3g} bound {e['value_bound']:.3g} "
          f"(bound / scale {e['value_bound'] / e['scale']:.3g})")
    assert e["value_bound"] <= 1e-4 * e["scale"]                                # a wider bound would be vacuous
    assert err <= e["value_bound"], what
    for i, name in ((1, "S_xx"), (2, "S_yy"), (3, "S_xy")):
        assert abs(o[i] - e[name]) <= e["b" + name], (what, name, o[i], e[name], e["b" + name])
    if grad is not None:
        g = grad.double().cpu().numpy()
        excess = np.abs(g - e["grad"]) - e["grad_bound"]
        worst = float((np.abs(g - e["grad"]) / np.maximum(e["grad_bound"], 1e-300)).max())
        print(f"{what}: grad max |err| {np.abs(g - e['grad']).max():.3g} of max |g| {np.abs(e['grad']).max():.3g}; "
              f"worst err / bound {worst:.3g}")
        assert g.shape == e["grad"].shape and bool((excess <= 0.0).all()), what


@pytest.mark.parametrize("kind", M.KERNELS)
@pytest.mark.parametrize("B,Z,var", M.CASES)
def test_mmd_against_float64_within_the_derived_bounds(B, Z, var, kind):
    x, y = M.inputs(B, Z)
    xd, yd = _dev(x), _dev(y)
    for estimator in M.ESTIMATORS:
        if B == 1 and estimator == "unbiased":
            with pytest.raises(ValueError, match="unbiased"):
                ops.mmd(xd, yd, kind, var, estimator)
            continue
        for coeff in (1.0, 10.0):
            _, _, v, e = M.case(B, Z, var, kind, estimator, coeff)
            if B >= 16:
                assert e["offdiag_share"] >= 0.9                                # a wrong off-diagonal term cannot hide behind the diagonal
            for want_grad in (False, True):
                out4, grad = ops.mmd(xd, yd, kind, var, estimator, coeff, want_grad=want_grad)
                assert out4.shape == (4,) and (grad is None) == (not want_grad)
                _check(out4, grad, e, f"{kind} {estimator} ({B}, {Z}) var {v} coeff {coeff} grad {want_grad}")


def test_bad_shapes_and_settings_are_refused():
    x = torch.zeros(4, 6, device="cuda")
    for bad in (lambda: ops.mmd(x, torch.zeros(4, 5, device="cuda")), lambda: ops.mmd(x, torch.zeros(3, 6, device="cuda")),
                lambda: ops.mmd(x[0], x[0]), lambda: ops.mmd(x, x, kernel="rbf"), lambda: ops.mmd(x, x, estimator="u"),
                lambda: ops.mmd(x, x, bandwidth=0.0), lambda: ops.mmd(x, x, bandwidth=float("nan")),
                lambda: ops.mmd(x, x, bandwidth=float("inf")), lambda: ops.mmd(x, x, coeff=float("inf"))):
        with pytest.raises(ValueError):
            bad()


@pytest.mark.parametrize("kind", M.KERNELS)
def test_two_calls_give_identical_bits(kind):
    B, Z = 300, 256
    x, y = M.inputs(B, Z)
    xd, yd = _dev(x), _dev(y)
    o1, g1 = ops.mmd(xd, yd, kind, None, "unbiased", 10.0, want_grad=True)
    filler = torch.randn(1 << 20, device="cuda")                                 # other work in between, other workspace memory
    o2, g2 = ops.mmd(xd, yd, kind, None, "unbiased", 10.0, want_grad=True)
    o3, _ = ops.mmd(xd, yd, kind, None, "unbiased", 10.0)
    del filler
    assert torch.equal(o1.view(torch.int32), o2.view(torch.int32)) and torch.equal(g1.view(torch.int32), g2.view(torch.int32))
    assert torch.equal(o1.view(torch.int32), o3.view(torch.int32))               # the value does not depend on the gradient phase


@pytest.mark.parametrize("kind", M.KERNELS)
@pytest.mark.parametrize("B,Z", [(2, 5), (37, 64), (300, 256)])
def test_unbiased_value_of_a_sample_against_itself(B, Z, kind):
    """x = y, the same tensor: every diagonal distance must be EXACTLY 0 and its kernel value exactly 1.  At a bandwidth so small that
    every off-diagonal kernel value vanishes (d / var > 1e4) only the diagonals are left, a (B - B) + a (B - B) - c B: the value is
    -2 coeff / B, the diagonal's share of the cross term, and the three sums are exactly B -- a diagonal distance of 1e-6 instead of 0
    would already lose a third of the value.  At the bandwidth 2 Z the off-diagonal terms do not cancel between the estimators'
    weights (2 off / (B^2 (B - 1)) is left, off = S - B): the value is -2 coeff / B + that, within the bound."""
    x, _ = M.inputs(B, Z)
    xd = _dev(x)
    coeff = 10.0
    tiny = 1e-6
    e = M.evaluate(x, x, kind, tiny, "unbiased", coeff)
    out4, grad = ops.mmd(xd, xd, kind, tiny, "unbiased", coeff, want_grad=True)
    o = out4.double().cpu().numpy()
    if kind == "gaussian":
        assert e["S_xx"] == B and o[1] == B and o[2] == B and o[3] == B           # exp(-1e4) = 0
        assert abs(o[0] - (-2.0 * coeff / B)) <= (M.U + 1e-12) * 2.0 * coeff / B        # one rounding of the value
        assert not bool(grad.any())
    assert abs(o[0] - e["value"]) <= e["value_bound"]
    assert abs(e["value"] - (-2.0 * coeff / B)) <= 1e-3 * coeff / B             # (imq: var / (var + d) < 1e-4 per pair is left)
    e = M.evaluate(x, x, kind, 2.0 * Z, "unbiased", coeff)
    out4, grad = ops.mmd(xd, xd, kind, None, "unbiased", coeff, want_grad=True)
    o = out4.double().cpu().numpy()
    off = e["S_xx"] - B
    want = coeff * (-2.0 / B + 2.0 * off / (B * B * (B - 1.0)))
    assert abs(e["value"] - want) <= 1e-12 * coeff
    assert abs(o[0] - want) <= e["value_bound"]
    assert o[1] == o[2] == o[3]                                                 # the same pairs in the same order: the same bits
    g = grad.double().cpu().numpy()
    assert bool((np.abs(g - e["grad"]) <= e["grad_bound"]).all())


@pytest.mark.parametrize("kind", M.KERNELS)
def test_misaligned_views_give_the_same_result(kind):
    B, Z = 37, 64
    x, y = M.inputs(B, Z)
    o0, g0 = ops.mmd(_dev(x), _dev(y), kind, None, "biased", 2.0, want_grad=True)
    bx = torch.full((B * Z + 1,), float("nan"), device="cuda")
    by = torch.full((B * Z + 3,), float("nan"), device="cuda")
    xv, yv = bx[1:].view(B, Z), by[3:].view(B, Z)                               # 4 and 12 bytes off a 16-byte boundary
    xv.copy_(_dev(x)); yv.copy_(_dev(y))
    assert xv.data_ptr() % 16 == 4 and yv.data_ptr() % 16 == 12
    o1, g1 = ops.mmd(xv, yv, kind, None, "biased", 2.0, want_grad=True)
    assert torch.equal(o0.view(torch.int32), o1.view(torch.int32)) and torch.equal(g0.view(torch.int32), g1.view(torch.int32))


@pytest.mark.parametrize("B,Z", [(1, 1), (3, 5), (17, 33), (65, 257)])
def test_outputs_stay_inside_their_buffers(B, Z):
    """Guard words in front of and behind out4 and grad; without a gradient pointer grad's memory is not touched at all."""
    x, y = M.inputs(B, Z)
    xd, yd = _dev(x), _dev(y)
    L = _lib.lib()
    nbytes = L.inet_mmd_ws_bytes(B, Z)
    assert nbytes == 2 * M.cdiv(B, M.ROWS) * 8
    ws = torch.full((nbytes // 4 + 2,), SENT, device="cuda")
    a, c, diag = ops.mmd_weights(B, "biased")
    for want_grad in (True, False):
        obuf = torch.full((4 + 2,), SENT, device="cuda")
        gbuf = torch.full((B * Z + 2,), SENT, device="cuda")
        ws.fill_(SENT)
        rc = L.inet_mmd(ptr(xd), ptr(yd), B, Z, 0, 2.0 * Z, a, c, diag, 1.0, ptr(obuf[1:5]), ptr(gbuf[1:-1]) if want_grad else None,
                        ptr(ws[1:-1]), nbytes, stream_ptr())
        assert rc == 0
        torch.cuda.synchronize()
        o, g, w = obuf.cpu(), gbuf.cpu(), ws.cpu()
        assert o[0] == SENT and o[5] == SENT and bool((o[1:5] != SENT).all())
        assert g[0] == SENT and g[-1] == SENT and w[0] == SENT and w[-1] == SENT
        assert bool((w[1:-1] != SENT).all())                                     # every workspace row is written: nothing to zero in front
        if want_grad:
            e = M.evaluate(x, y, "gaussian", 2.0 * Z, "biased", 1.0, key=(B, Z))
            assert bool((np.abs(g[1:-1].double().numpy().reshape(B, Z) - e["grad"]) <= e["grad_bound"]).all())
            assert abs(float(o[1]) - e["value"]) <= e["value_bound"]
        else:
            assert bool((g == SENT).all())
