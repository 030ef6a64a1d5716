"""The free-bits kernels alone (csrc/latent.hip: reparam_kl_fb_measure / _dim / _finish, latent_bwd_fb) through
ops.reparam_kl_fb / ops.latent_bwd_fb, both modes, against the float64 restatement and the bounds derived in tests/kl_fb_ref.py.

Shapes: the ones the kernels can go wrong at -- one element, one row, widths around the 64-lane wave and off the 16-byte path, more
rows than one workgroup, and 1037 rows: one full pass of both capped grids and a ragged second one.  Every test prints the share of
its bound the device used (DESIGN.md section 22 quotes them)."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import kl_fb_ref as K

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from inpaintnet_amd import _lib, ops
    from inpaintnet_amd._lib import ptr, stream_ptr

DEV = "cuda:0"
KSCALE, KDEV = 0.031, 0.75
SENT = -777.25


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def share(got, ref, bound):
    """max |got - ref| / bound over the elements (bound > 0 everywhere it is used)."""
    err = np.abs(got.detach().double().cpu().numpy().reshape(np.shape(ref)) - ref)
    return float(np.max(err / bound))


@functools.lru_cache(maxsize=None)
def reference(rows, Z, per):
    """The case's inputs on the device and its float64 reference: computed once, shared, never written to."""
    c = K.case(rows, Z, per)
    f = K.forward(c["mu"], c["ls"], c["eps"], c["free_nats"], per)
    b = K.bounds(c["mu"], c["ls"], c["eps"], c["free_nats"], per)
    d = {k: dev(c[k]) for k in ("mu", "ls", "eps", "dz")}
    return c, f, b, d


def run_fwd(d, free_nats, per, eps=True, want_z=True):
    z, parts, keep, kl, raw = ops.reparam_kl_fb(d["mu"], d["ls"], d["eps"] if eps else None, free_nats, per, want_z=want_z)
    torch.cuda.synchronize()
    return z, parts, keep, float(kl), float(raw)


@pytest.mark.parametrize("per", K.PER)
@pytest.mark.parametrize("shape", K.SHAPES)
def test_forward_and_backward_against_float64(shape, per):
    rows, Z = shape
    c, f, b, d = reference(rows, Z, per)
    assert c["margin"] > 0.0                          # the inputs' condition: no part within its bound of the threshold
    z, parts, keep, floored, raw = run_fwd(d, c["free_nats"], per)
    assert np.array_equal(keep.cpu().numpy() != 0.0, f["keep"]) and set(keep.cpu().tolist()) <= {0.0, 1.0}
    used = dict(parts=share(parts, f["parts"], b["parts"]), z=share(z, f["z"], b["z"]),
                floored=abs(floored - f["floored"]) / b["floored"], raw=abs(raw - f["raw"]) / b["raw"])
    kdev = torch.tensor([KDEV], device=DEV)
    dmu, dls = ops.latent_bwd_fb(d["dz"], d["mu"], d["ls"], d["eps"], KSCALE, keep, per, kscale_dev=kdev)
    torch.cuda.synchronize()
    rmu, rls = K.backward(c["dz"], c["mu"], c["ls"], c["eps"], KSCALE, KDEV, f["keep"], per)
    bmu, bls = K.backward_bounds(c["dz"], c["mu"], c["ls"], c["eps"], KSCALE, KDEV, f["keep"], per)
    used.update(dmu=share(dmu, rmu, bmu), dls=share(dls, rls, bls))
    print(f"{per} {shape}: share of the bound used: " + ", ".join(f"{k} {v:.3f}" for k, v in used.items()))
    assert all(v <= 1.0 for v in used.values()), used


@pytest.mark.parametrize("per", K.PER)
@pytest.mark.parametrize("shape", [(3, 5), (65, 257), (300, 256), K.SHAPES[-1]])
def test_all_kept_is_the_plain_pair_bit_for_bit(shape, per):
    """free_nats = 0 (every part of these inputs is positive): z is ops.reparam_kl's, dmu / dls are ops.latent_bwd's, floored == raw."""
    c, f, b, d = reference(*shape, per)
    z, parts, keep, floored, raw = run_fwd(d, 0.0, per)
    assert bool((keep == 1.0).all()) and floored == raw
    plain = torch.zeros(1, device=DEV)
    z0, _ = ops.reparam_kl(d["mu"], d["ls"], d["eps"], kl_sum=plain)
    assert same_bits(z, z0)
    assert abs(raw - float(plain)) <= b["raw"] + b["raw"]                        # two float32 sums of the same terms
    kdev = torch.tensor([KDEV], device=DEV)
    for dz, kd in ((d["dz"], kdev), (d["dz"], None), (None, kdev)):
        got = ops.latent_bwd_fb(dz, d["mu"], d["ls"], d["eps"], KSCALE, keep, per, kscale_dev=kd)
        want = ops.latent_bwd(dz, d["mu"], d["ls"], d["eps"], KSCALE, kscale_dev=kd)
        assert same_bits(got[0], want[0]) and same_bits(got[1], want[1])


@pytest.mark.parametrize("per", K.PER)
@pytest.mark.parametrize("shape", [(3, 5), (65, 257), (300, 256)])
def test_none_kept_hands_dz_on_bit_for_bit(shape, per):
    """free_nats above the largest part: dmu is dz, dls is (dz * eps) * sigma with the kernels' own sigma, floored = nparts * thr."""
    rows, Z = shape
    c, f, b, d = reference(rows, Z, per)
    top = float(f["parts"].max())
    lam = K.f32(2.0 * top if per == "measure" else 2.0 * top / rows)
    z, parts, keep, floored, raw = run_fwd(d, lam, per)
    assert bool((keep == 0.0).all())
    n, thr = parts.numel(), K.threshold(rows, lam, per)
    assert abs(floored - n * thr) <= n * K.U * n * thr                           # n equal float32 terms, added in a fixed order
    assert abs(raw - f["raw"]) <= b["raw"]
    dmu, dls = ops.latent_bwd_fb(d["dz"], d["mu"], d["ls"], d["eps"], KSCALE, keep, per, kscale_dev=torch.tensor([KDEV], device=DEV))
    _, sigma = ops.reparam_kl(d["mu"], d["ls"], None, want_sigma=True)
    assert same_bits(dmu, d["dz"])
    assert same_bits(dls, (d["dz"] * d["eps"]) * sigma)


@pytest.mark.parametrize("per", K.PER)
def test_one_nan_is_kept_and_stays_in_its_part(per):
    rows, Z = 37, 64
    c, f, b, d = reference(rows, Z, per)
    mu = d["mu"].clone()
    mu[5, 9] = float("nan")
    part = 5 if per == "measure" else 9
    dd = dict(d, mu=mu)
    z, parts, keep, floored, raw = run_fwd(dd, c["free_nats"], per)
    assert math.isnan(floored) and math.isnan(raw)
    assert math.isnan(float(parts[part])) and float(keep[part]) == 1.0
    z0, parts0, keep0, _, _ = run_fwd(d, c["free_nats"], per)
    others = torch.arange(parts.numel(), device=DEV) != part
    assert same_bits(parts[others], parts0[others]) and same_bits(keep[others], keep0[others])
    dmu, dls = ops.latent_bwd_fb(d["dz"], mu, d["ls"], d["eps"], KSCALE, keep, per)
    # (the clean inputs under the SAME keep vector: the NaN's part may have been floored without it)
    dmu0, dls0 = ops.latent_bwd_fb(d["dz"], d["mu"], d["ls"], d["eps"], KSCALE, keep, per)
    assert math.isnan(float(dmu[5, 9])) and int(torch.isnan(dmu).sum()) == 1 and not bool(torch.isnan(dls).any())
    clean = torch.ones(rows, Z, dtype=torch.bool, device=DEV)
    clean[5, 9] = False
    assert same_bits(dmu[clean], dmu0[clean]) and same_bits(dls, dls0)


@pytest.mark.parametrize("per", K.PER)
@pytest.mark.parametrize("shape", [(3, 5), (300, 256)])
def test_null_arguments(shape, per):
    rows, Z = shape
    c, f, b, d = reference(rows, Z, per)
    # eps null reads as 0: z is mu, parts do not depend on eps
    z, parts, keep, floored, raw = run_fwd(d, c["free_nats"], per, eps=False)
    _, parts1, keep1, _, _ = run_fwd(d, c["free_nats"], per)
    assert same_bits(z, d["mu"]) and same_bits(parts, parts1) and same_bits(keep, keep1)
    # z null: everything else as with it
    z2, parts2, keep2, floored2, _ = run_fwd(d, c["free_nats"], per, want_z=False)
    assert z2 is None and same_bits(parts2, parts1) and same_bits(keep2, keep1)
    assert abs(floored2 - f["floored"]) <= b["floored"]
    # dz null with and without kdev, eps null in the backward
    for kd in (KDEV, None):
        kdev = None if kd is None else torch.tensor([kd], device=DEV)
        dmu, dls = ops.latent_bwd_fb(None, d["mu"], d["ls"], None, KSCALE, keep1, per, kscale_dev=kdev)
        torch.cuda.synchronize()
        rmu, rls = K.backward(None, c["mu"], c["ls"], None, KSCALE, kd, f["keep"], per)
        bmu, bls = K.backward_bounds(None, c["mu"], c["ls"], None, KSCALE, kd, f["keep"], per)
        tiny = 1e-300                                                            # (floored elements: reference 0, bound 0, result 0)
        assert share(dmu, rmu, bmu + tiny) <= 1.0 and share(dls, rls, bls + tiny) <= 1.0
        floored_el = ~K.keep_of_elements(f["keep"], (rows, Z), per)
        assert not dmu.cpu().numpy()[floored_el].any() and not dls.cpu().numpy()[floored_el].any()


@pytest.mark.parametrize("per", K.PER)
def test_two_runs_give_the_same_parts_and_keep_bits(per):
    c, f, b, d = reference(*K.SHAPES[-1], per)
    a = run_fwd(d, c["free_nats"], per)
    again = run_fwd(d, c["free_nats"], per)
    assert same_bits(a[1], again[1]) and same_bits(a[2], again[2]) and same_bits(a[0], again[0])
    assert a[3:] == again[3:]                         # (no atomics: the two scalars repeat as well)


def test_scalars_are_added_onto_and_the_keep_length_is_checked():
    c, f, b, d = reference(37, 64, "dim")
    kl = torch.full((1,), 3.0, device=DEV)
    raw = torch.full((1,), -2.0, device=DEV)
    ops.reparam_kl_fb(d["mu"], d["ls"], d["eps"], c["free_nats"], "dim", kl_sum=kl, kl_raw=raw)
    assert abs(float(kl) - 3.0 - f["floored"]) <= b["floored"] + K.U * abs(f["floored"])
    assert abs(float(raw) + 2.0 - f["raw"]) <= b["raw"] + K.U * abs(f["raw"])
    with pytest.raises(ValueError):
        ops.latent_bwd_fb(None, d["mu"], d["ls"], None, 1.0, torch.ones(37, device=DEV), "dim")
    with pytest.raises(ValueError):
        ops.reparam_kl_fb(d["mu"], d["ls"], None, 1.0, "row")


def test_bad_arguments_return_minus_one_and_write_nothing():
    rows, Z = 8, 12
    L = _lib.lib()
    mu, ls = torch.zeros(rows, Z, device=DEV), torch.zeros(rows, Z, device=DEV)
    outs = [torch.full((rows * Z,), SENT, device=DEV) for _ in range(7)]         # z, parts, keep, kl, raw, dmu, dls
    ws = torch.full((4096,), SENT, device=DEV)
    z, parts, keep, kl, raw, dmu, dls = outs

    def fwd(mu_=mu, rows_=rows, Z_=Z, lam=1.0, per=1, parts_=parts, ws_=ws, nb=4096 * 4):
        return L.inet_reparam_kl_fb(ptr(mu_), ptr(ls), None, ptr(z), rows_, Z_, lam, per, ptr(parts_), ptr(keep), ptr(kl), ptr(raw),
                                    ptr(ws_), nb, stream_ptr())

    def bwd(keep_=parts, per=0, rows_=rows, Z_=Z, dmu_=dmu):
        return L.inet_latent_bwd_fb(None, ptr(mu), ptr(ls), None, 1.0, None, ptr(keep_), per, ptr(dmu_), ptr(dls), rows_, Z_, stream_ptr())
    rcs = [fwd(mu_=None), fwd(rows_=0), fwd(Z_=-1), fwd(lam=-1.0), fwd(lam=float("nan")), fwd(lam=math.inf), fwd(per=2), fwd(per=-1),
           fwd(parts_=None), fwd(ws_=None), fwd(nb=8), bwd(keep_=None), bwd(per=3), bwd(rows_=0), bwd(Z_=0), bwd(dmu_=None)]
    torch.cuda.synchronize()
    assert rcs == [-1] * len(rcs)
    assert all(bool((t == SENT).all()) for t in outs + [ws])
