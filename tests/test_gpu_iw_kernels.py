"""The three kernels of the importance-weighted log-likelihood (csrc/iw.hip), each alone through the C-ABI against
the float64 restatement of tests/iw_ref.py, within the bounds derived there.  Outputs lie between NaN-poisoned guard elements, which
must be untouched afterwards."""
import math

import numpy as np
import pytest
import torch

from tests import iw_ref as R

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from inpaintnet_amd import _lib, ops, synthetic
    from inpaintnet_amd._lib import ptr, stream_ptr

GUARD = 8                                # floats (or doubles) of NaN on either side of an output: keeps a 16-byte alignment


def guarded(n, dtype=torch.float32, shift=0):
    """-> (buffer, view of n elements behind GUARD + shift NaNs and in front of GUARD NaNs)"""
    buf = torch.full((2 * GUARD + shift + n,), float("nan"), dtype=dtype, device="cuda")
    return buf, buf[GUARD + shift:GUARD + shift + n]


def guards_intact(buf, n, shift=0):
    b = buf.cpu()
    return bool(torch.isnan(b[:GUARD + shift]).all()) and bool(torch.isnan(b[GUARD + shift + n:]).all())


def shifted(t, shift):
    """A copy of t that starts `shift` floats behind a 256-byte boundary (shift = 1: no 16-byte alignment)."""
    if not shift:
        return t
    buf = torch.empty(t.numel() + shift, dtype=t.dtype, device=t.device)
    v = buf[shift:].view(t.shape)
    v.copy_(t)
    return v


# =============================================================================== iw_draw
def draw_inputs(B, K, Z):
    tag = f"iw/draw/{B}x{K}x{Z}"
    mu = synthetic.det_normal(tag + "/mu", (B, Z))
    ls = (0.3 * synthetic.det_normal(tag + "/ls", (B, Z))).astype(np.float32)
    ls.flat[0] = -20.0
    ls.flat[-1] = 5.0
    eps = synthetic.det_normal(tag + "/eps", (B, K, Z))
    return mu, ls, eps


def raw_draw(mu, ls, eps_view, shift=0):
    """inet_iw_draw on device tensors, z and logr between guards; shift = 1 moves every pointer one float off its alignment."""
    B, Kc, Z = eps_view.shape
    mu_d, ls_d = shifted(mu, shift), shifted(ls, shift)
    if shift:
        full = torch.empty(eps_view.numel() + shift, dtype=torch.float32, device="cuda")
        e = full[shift:].view(B, Kc, Z)
        e.copy_(eps_view)
        eps_view = e
    stride_b = eps_view.stride(0) if B > 1 else Kc * Z
    zbuf, z = guarded(B * Kc * Z, shift=shift)
    rbuf, logr = guarded(B * Kc)
    rc = _lib.lib().inet_iw_draw(ptr(mu_d), ptr(ls_d), ptr(eps_view), stride_b, ptr(z), ptr(logr), B, Kc, Z, stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    assert guards_intact(zbuf, B * Kc * Z, shift) and guards_intact(rbuf, B * Kc)
    return z.view(B * Kc, Z).clone(), logr.clone()


def check_draw(z, logr, ref, what):
    B, Kc, Z = ref["z"].shape
    zerr = np.abs(z.cpu().double().numpy().reshape(B, Kc, Z) - ref["z"])
    rerr = np.abs(logr.cpu().double().numpy().reshape(B, Kc) - ref["logr"])
    print(what, "z error / bound %.3f, logr error / bound %.3f (bound / |logr| %.2g)"
          % ((zerr / ref["z_bound"]).max(), (rerr / ref["logr_bound"]).max(), (ref["logr_bound"] / np.abs(ref["logr"])).max()))
    assert (zerr <= ref["z_bound"]).all(), what
    assert (rerr <= ref["logr_bound"]).all(), what


@pytest.mark.parametrize("B,Kc", [(1, 1), (3, 2), (2, 7)])
@pytest.mark.parametrize("Z", [1, 3, 64, 65, 256, 260])
def test_iw_draw_against_float64(Z, B, Kc):
    """eps is the chunk [:, 1:1 + Kc] of a (B, Kc + 2, Z) tensor: eps_stride_b > Kc Z.  Z % 4 == 0 runs the 16-byte path (every
    pointer aligned), anything else the scalar one; ls holds -20 and +5."""
    K = Kc + 2
    mu, ls, eps = draw_inputs(B, K, Z)
    ref = R.draw(mu, ls, eps[:, 1:1 + Kc])
    mu_d, ls_d, eps_d = (torch.from_numpy(a).cuda() for a in (mu, ls, eps))
    view = eps_d[:, 1:1 + Kc]
    assert B == 1 or view.stride(0) > Kc * Z
    z, logr = raw_draw(mu_d, ls_d, view)
    check_draw(z, logr, ref, f"Z {Z} B {B} Kc {Kc}")
    z2, logr2 = raw_draw(mu_d, ls_d, view)
    assert torch.equal(z, z2) and torch.equal(logr, logr2)                      # two calls: equal bits
    zo, logro = ops.iw_draw(mu_d, ls_d, view)                                    # the ops wrapper is the same launch
    assert torch.equal(z, zo) and torch.equal(logr, logro)
    # eps = 0: z is mu, exactly
    z0, _ = raw_draw(mu_d, ls_d, torch.zeros_like(eps_d)[:, 1:1 + Kc])
    assert torch.equal(z0.view(B, Kc, Z), mu_d[:, None, :].expand(B, Kc, Z))


@pytest.mark.parametrize("Z", [64, 256, 260, 3])
def test_iw_draw_scalar_path_on_misaligned_pointers(Z):
    """Every pointer one float off a 16-byte boundary: Z = 256 takes the scalar path.  z is the same expression element by element, so
    its bits equal the aligned call's; logr is added in the other order and stays within its bound."""
    B, Kc = 3, 2
    mu, ls, eps = draw_inputs(B, Kc, Z)
    ref = R.draw(mu, ls, eps)
    mu_d, ls_d, eps_d = (torch.from_numpy(a).cuda() for a in (mu, ls, eps))
    z, logr = raw_draw(mu_d, ls_d, eps_d, shift=1)
    check_draw(z, logr, ref, f"misaligned Z {Z}")
    za, logra = raw_draw(mu_d, ls_d, eps_d)
    check_draw(za, logra, ref, f"aligned Z {Z}")
    assert torch.equal(z, za)


@pytest.mark.parametrize("Z", [3, 64, 65, 256])
def test_iw_draw_rows_do_not_depend_on_the_chunking_and_agree_with_reparam_kl(Z):
    B, K = 2, 7
    mu, ls, eps = draw_inputs(B, K, Z)
    mu_d, ls_d, eps_d = (torch.from_numpy(a).cuda() for a in (mu, ls, eps))
    z, logr = ops.iw_draw(mu_d, ls_d, eps_d)
    z, logr = z.view(B, K, Z), logr.view(B, K)
    sig = np.exp(ls.astype(np.float64))
    for k in range(K):
        zk, lk = ops.iw_draw(mu_d, ls_d, eps_d[:, k:k + 1])                      # Kc = 1: a chunk view, no copy
        assert torch.equal(zk, z[:, k]) and torch.equal(lk, logr[:, k]), (Z, k)
        zr, _ = ops.reparam_kl(mu_d, ls_d, eps_d[:, k].contiguous())
        tol = R.U * (np.abs(mu) + 2 * np.abs(eps[:, k].astype(np.float64) * sig))
        assert (np.abs(zk.cpu().double().numpy() - zr.cpu().double().numpy()) <= tol).all(), (Z, k)


# =============================================================================== nll_rows
NLL_CASES = [(1, 1, 1, 1), (2, 4, 5, 5), (20, 24, 5, 1), (63, 4, 70, 5), (64, 1, 5, 1), (65, 30, 70, 5), (130, 24, 5, 5), (20, 30, 1, 1)]


def test_nll_case_list_covers_what_it_must():
    assert {c[0] for c in NLL_CASES} == {1, 2, 20, 63, 64, 65, 130} and {c[1] for c in NLL_CASES} == {1, 4, 24, 30}
    assert {c[2] for c in NLL_CASES} == {1, 5, 70} and {c[3] for c in NLL_CASES} == {1, 5} and (65, 30, 70, 5) in NLL_CASES


def nll_inputs(V, T, Rr, big=True):
    tag = f"iw/nll/{V}x{T}x{Rr}"
    w = (3.0 * synthetic.det_normal(tag + "/w", (Rr, T, V))).astype(np.float32)
    if big:
        w.reshape(-1)[::7] = 80.0
        w.reshape(-1)[3::11] = -80.0
    tg = synthetic.det_tokens(tag + "/t", (Rr, T), V)
    logr = (5.0 * synthetic.det_normal(tag + "/r", (Rr,))).astype(np.float32)
    return w, tg, logr


def raw_nll(w, tg, logr, group, pad=3, want_nll=True, want_logw=True, ld_out=None):
    """inet_nll_rows with weights in rows of V + pad floats (NaN in the padding) and outputs between guards in rows of ld_out."""
    Rr, T, V = w.shape
    ld_w = V + pad
    wd = torch.full((Rr * T, ld_w), float("nan"), dtype=torch.float32, device="cuda")
    wd[:, :V] = torch.from_numpy(w).reshape(Rr * T, V)
    tgd = torch.from_numpy(np.asarray(tg, np.int64)).cuda().contiguous()
    lrd = None if logr is None else torch.from_numpy(logr).cuda()
    ld_out = group + 3 if ld_out is None else ld_out
    n = (Rr // group) * ld_out
    nbuf, nv = guarded(n)
    lbuf, lv = guarded(n)
    rc = _lib.lib().inet_nll_rows(ptr(wd), ld_w, ptr(tgd), ptr(lrd), ptr(nv) if want_nll else None, ptr(lv) if want_logw else None,
                                  ld_out, Rr, group, T, V, stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    assert guards_intact(nbuf, n) and guards_intact(lbuf, n)
    nv, lv = nv.view(Rr // group, ld_out).cpu(), lv.view(Rr // group, ld_out).cpu()
    for v, want in ((nv, want_nll), (lv, want_logw)):
        assert bool(torch.isnan(v[:, group:]).all())                             # the columns of other chunks are not written
        assert want or bool(torch.isnan(v).all())                                # a null output is not written at all
    return nv[:, :group].reshape(-1).double().numpy(), lv[:, :group].reshape(-1).double().numpy()


@pytest.mark.parametrize("V,T,Rr,group", NLL_CASES)
def test_nll_rows_against_float64(V, T, Rr, group):
    w, tg, logr = nll_inputs(V, T, Rr)
    ref = R.nll_rows(w, tg, logr)
    nll, logw = raw_nll(w, tg, logr, group)
    print(f"V {V} T {T} R {Rr}: nll error / bound %.3f, logw error / bound %.3f, bound / nll %.2g"
          % ((np.abs(nll - ref["nll"]) / ref["nll_bound"]).max(), (np.abs(logw - ref["logw"]) / ref["logw_bound"]).max(),
             (ref["nll_bound"] / np.maximum(ref["nll"], 1e-30)).max()))
    assert (np.abs(nll - ref["nll"]) <= ref["nll_bound"]).all()
    assert (np.abs(logw - ref["logw"]) <= ref["logw_bound"]).all()
    # each of nll / logw / logr null in turn: what is still written keeps its bits
    n2, l2 = raw_nll(w, tg, logr, group, want_nll=False)
    assert np.array_equal(l2, logw)
    n3, l3 = raw_nll(w, tg, logr, group, want_logw=False)
    assert np.array_equal(n3, nll)
    n4, l4 = raw_nll(w, tg, None, group)
    assert np.array_equal(n4, nll) and np.array_equal(l4, -nll)
    # the ops wrapper: the same launch, its own outputs
    wd = torch.from_numpy(w).cuda()
    on, ol = ops.nll_rows(wd, torch.from_numpy(tg).cuda(), torch.from_numpy(logr).cuda(), group=group, ld_out=group + 2)
    assert on.shape == (Rr // group, group) and on.stride(0) == group + 2
    assert np.array_equal(on.cpu().double().numpy().reshape(-1), nll) and np.array_equal(ol.cpu().double().numpy().reshape(-1), logw)


@pytest.mark.parametrize("V,T", [(2, 4), (20, 24), (65, 30), (130, 1)])
def test_nll_rows_all_equal_rows_give_t_log_v(V, T):
    w = np.full((5, T, V), 1.25, np.float32)
    tg = synthetic.det_tokens(f"iw/eq/{V}", (5, T), V)
    ref = R.nll_rows(w, tg)
    nll, _ = raw_nll(w, tg, None, 1)
    assert np.abs(ref["nll"] - T * math.log(V)).max() <= 1e-13 * T * math.log(V)
    assert (np.abs(nll - T * math.log(V)) <= ref["nll_bound"] + 1e-13 * T * math.log(V)).all()


def test_nll_rows_infinite_logits_and_targets_outside_the_vocabulary():
    V, T, Rr = 20, 24, 5
    w, tg, logr = nll_inputs(V, T, Rr, big=False)
    tg = tg.copy()
    # row 0: a -inf logit OFF the target; row 1: a -inf logit ON the target; row 2: a target of -1; row 4: a target of V; row 3: plain
    off = (tg[0, 5] + 1) % V
    w[0, 5, off] = -np.inf
    w[1, 7, tg[1, 7]] = -np.inf
    ref = R.nll_rows(w, tg, logr)
    bad = tg.copy()
    bad[2, 0] = -1
    bad[4, T - 1] = V
    nll, logw = raw_nll(w, bad, logr, 1)
    assert np.isfinite(ref["nll"][0]) and abs(nll[0] - ref["nll"][0]) <= ref["nll_bound"][0]
    assert nll[1] == np.inf and logw[1] == -np.inf and ref["nll"][1] == np.inf
    assert np.isnan(nll[2]) and np.isnan(logw[2]) and np.isnan(nll[4]) and np.isnan(logw[4])
    assert abs(nll[3] - ref["nll"][3]) <= ref["nll_bound"][3] and abs(logw[3] - ref["logw"][3]) <= ref["logw_bound"][3]
    # with group 5 the same rows land in one output row, the neighbours untouched by the NaNs
    nll5, logw5 = raw_nll(w, bad, logr, 5)
    assert np.array_equal(nll5, nll, equal_nan=True) and np.array_equal(logw5, logw, equal_nan=True)


def test_nll_rows_and_cross_entropy_meet_at_the_float64_mean():
    V, T, Rr = 65, 30, 70
    w, tg, _ = nll_inputs(V, T, Rr)
    mean, bound_ce, bound_nll = R.ce_mean(w, tg)
    nll, _ = raw_nll(w, tg, None, 5)
    wd = torch.from_numpy(w).cuda().reshape(Rr * T, V)
    out2 = torch.zeros(2, dtype=torch.float32, device="cuda")
    ops.cross_entropy(wd, torch.from_numpy(tg).cuda().reshape(-1), out2, out_scale=1.0 / (Rr * T))
    ce = float(out2[0])
    print("float64 mean %.9f; nll_rows mean error %.3g (bound %.3g); inet_cross_entropy error %.3g (bound %.3g)"
          % (mean, abs(nll.sum() / (Rr * T) - mean), bound_nll, abs(ce - mean), bound_ce))
    assert abs(nll.sum() / (Rr * T) - mean) <= bound_nll
    assert abs(ce - mean) <= bound_ce


# =============================================================================== iw_finish
def raw_finish(logw, nll, pad=3):
    B, K = logw.shape
    ld = K + pad
    lw = torch.full((B, ld), float("nan"), dtype=torch.float32, device="cuda")
    nl = torch.full((B, ld), float("nan"), dtype=torch.float32, device="cuda")
    lw[:, :K], nl[:, :K] = torch.from_numpy(logw), torch.from_numpy(nll)
    obuf, out = guarded(5 * B, dtype=torch.float64)
    rc = _lib.lib().inet_iw_finish(ptr(lw), ptr(nl), ld, B, K, ptr(out), stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0 and guards_intact(obuf, 5 * B)
    via_ops = ops.iw_finish(lw[:, :K], nl[:, :K])
    assert torch.equal(via_ops, out.view(B, 5)) or bool(torch.isnan(via_ops).any())
    return out.view(B, 5).cpu().numpy().copy()


def close(got, want):
    """1e-12 relative, 1e-12 absolute for ess (column 2); equal where the restatement is not finite."""
    fin = np.isfinite(want)
    assert np.array_equal(got[~fin], want[~fin], equal_nan=True)
    tol = R.FINISH_RTOL * np.abs(want)
    tol[:, 2] = R.FINISH_RTOL
    with np.errstate(invalid="ignore"):                                          # (inf - inf where both sides hold the same infinity)
        assert (np.abs(got - want)[fin] <= tol[fin]).all(), (got, want)


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("K", [1, 2, 63, 64, 65, 1000])
def test_iw_finish_against_numpy_float64(K, B):
    rng = np.random.default_rng(1000 * B + K)
    logw = (-30.0 + 2.0 * rng.standard_normal((B, K))).astype(np.float32)
    nll = (40.0 + rng.standard_normal((B, K))).astype(np.float32)
    got, want = raw_finish(logw, nll), R.finish(logw, nll)
    close(got, want)
    assert np.array_equal(got, raw_finish(logw, nll))                            # two calls: equal bits
    if K == 1:                                                                   # exactly
        assert np.array_equal(got[:, 0], logw[:, 0].astype(np.float64)) and np.array_equal(got[:, 1], got[:, 0])
        assert np.array_equal(got[:, 2], np.ones(B)) and np.array_equal(got[:, 3], nll[:, 0].astype(np.float64))


def test_iw_finish_special_values():
    lw = np.full((6, 7), -3.2699999809265137, np.float32)
    nl = np.ones((6, 7), np.float32)
    lw[1, 2] = np.nan                                                            # one NaN
    lw[2, :] = -np.inf                                                           # every weight zero
    lw[3, 1:] = -np.inf                                                          # one sample carries everything
    lw[4] = np.array([0.0, -800.0, -800.0, -800.0, -800.0, -800.0, -800.0], np.float32)      # a spread of 800 nats
    got = raw_finish(lw, nl)
    v = float(lw[0, 0])
    assert got[0, 0] == v and got[0, 1] == v and got[0, 2] == 7.0                # seven copies of one value: exactly
    assert np.isnan(got[1, :3]).all()
    assert got[2, 0] == -np.inf and got[2, 1] == -np.inf and got[2, 2] == 0.0
    assert got[3, 1] == -np.inf and got[3, 2] == 1.0 and abs(got[3, 0] - (v - math.log(7.0))) <= 1e-12 * abs(v - math.log(7.0))
    assert abs(got[4, 2] - 1.0) <= 1e-12 and abs(got[4, 0] + math.log(7.0)) <= 1e-12 * math.log(7.0)
    assert got[5, 0] == v and got[5, 1] == v and got[5, 2] == 7.0                # the measures next to the special ones are unaffected
    close(got, R.finish(lw, nl))
