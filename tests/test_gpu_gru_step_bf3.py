"""The bf16-pipe GRU step kernels (csrc/gru_step_bf3.hip: gru_step_bf3_kernel, gru_step_bf3_bwd_kernel) at shapes that take
milliseconds, against a float64 evaluation of the same two-layer bi-GRU.

The kernels are built for batches whose single time step fills the chip (B >= 1536 at H = 512); inet_set_option key 12 = 1 lowers
their tile threshold to one tile, and the chain kernels step aside with key 4 = 0 (or by themselves: H = 768, T = 1), so every
branch of the two launchers runs here at B <= 384: the initial state in ring slot 1, the zero-state step without a k loop, the
96-row and the 128-row tile with saves, the tail launch for dh0, T = 1 .. 3 (ring parity), both branches of the backward kernel's
workgroup remap, the piece outputs feeding gemm_bf3, the scalar input (a broadcast vector as the only input-side source) and the
mixed plan for B % 96 == 0 && B % 128 != 0 (step kernels forward, f32 per-step kernels backward over the step kernels' saves).
(The forward kernel's `tid = id` branch cannot be reached through the library: its grid is nd * tiles * H / 64 with nd = 2 and
H % 256 == 0, a multiple of 8 always.)

Rule for every compared tensor (the one test_chain_generations_against_float64 uses for "same products, other summation order"):
with err = max |got - ref| / max |ref| against float64, the step path must satisfy err_step <= 2 err_base + 3e-7 and err_step <
2e-5, where err_base is the identical call under key 12 = 0 (the f32 per-step kernels; for H = 768 / T = 1 with the chains on,
whatever the library then runs), and err_base itself must stay under 1e-5.

Measured on an MI355X: MEASURED below holds the worst tensor of every case; the worst pair of all is the 24-step piece case,
1.52e-06 on the step kernels against 1.33e-06 on the f32 per-step kernels (db_hh of layer 0, reverse) -- both at a few f32 ulp of
float64, a factor of 13 under the cap.  Under INET_TEST_POISON=1 (NaN-filled allocator pool) every case passes with the same step-path figures:
no ring slot, save or piece buffer is read before it is written.
"""
import numpy as np
import pytest
import torch

from oracle import torch_ref as O
from tests import bigru2_ref as R
from tests import golden_util as G

if torch.cuda.is_available():
    from inpaintnet_amd import ops

DEV = "cuda:0"
CAP, FLOOR = 2e-5, 3e-7

# (largest err_step, largest err_base) over the compared tensors of each case, as printed by the tests on an MI355X
MEASURED = {
    "b128-t3-h0": (5.89e-07, 5.28e-07), "b128-t3-zero": (4.56e-07, 3.72e-07), "b96-t2-scalar": (4.72e-07, 4.72e-07),
    "b192-t3-h0": (6.03e-07, 5.31e-07), "b256-t2-h512": (9.40e-07, 7.46e-07), "b384-t8-pieces": (1.18e-06, 1.04e-06),
    "b128-t24-pieces": (1.52e-06, 1.33e-06), "b128-t2-h768": (1.14e-06, 8.01e-07), "b128-t2-h1024-scalar": (1.11e-06, 8.90e-07),
    "b128-t1-h0": (5.46e-07, 5.23e-07), "b128-t1-zero": (3.78e-07, 3.50e-07),
    "encoder B128": (1.10e-06, 8.73e-07), "encoder B96": (9.16e-07, 9.01e-07),
}


_labels, _rel = R.labels, R.rel


def _check(tag, errs):
    """errs: {tensor: (err_step, err_base)}.  Prints every pair, then applies the rule of the module docstring."""
    R.check(tag, errs, "step", CAP, FLOOR)


# ------------------------------------------------------------------------------------------------ 1. inet_bigru2_fwd / _bwd
# (B, T, K, H, scalar x_0, chains (key 4), h0 given, dh0 wanted, mask)
CASES = {
    # 128-row tile, one row tile, backward grid 4 (no remap), odd T, tail launch
    "b128-t3-h0": (128, 3, 8, 256, False, 0, True, True, True),
    # the same shape on the zero-state branch: step 0 without a k loop, no tail launch
    "b128-t3-zero": (128, 3, 8, 256, False, 0, False, False, False),
    # 96-row tile; forward on the step kernels, backward on the f32 per-step kernels over their saves; vector-only input
    "b96-t2-scalar": (96, 2, 1, 256, True, 0, False, False, False),
    # 96-row tile with two row tiles, the same mixed forward / backward
    "b192-t3-h0": (192, 3, 8, 256, False, 0, True, True, True),
    # grids 32 / 16: the remap branch in both kernels, with the tail launch
    "b256-t2-h512": (256, 2, 4, 512, False, 0, True, True, True),
    # T B = 3072: both kernels write em.rows, layer 1's products run on gemm_bf3; 96-row forward tile, backward grid 12
    "b384-t8-pieces": (384, 8, 8, 256, False, 0, False, False, True),
    # the same piece path on the 128-row tile over 24 steps
    "b128-t24-pieces": (128, 24, 8, 256, False, 0, True, True, True),
    # the H the chain kernels never take: the default route of a real caller
    "b128-t2-h768": (128, 2, 8, 768, False, 1, True, True, False),
    # widest K of the backward contraction (3H = 3072)
    "b128-t2-h1024-scalar": (128, 2, 1, 1024, True, 0, True, True, False),
    # T = 1: no ring write, hlast from step 0, backward = first launch + tail only; with an initial state and without
    "b128-t1-h0": (128, 1, 8, 256, False, 1, True, True, False),
    "b128-t1-zero": (128, 1, 8, 256, False, 1, False, True, False),
}


def _bigru2_case(name):
    """Parameters, inputs and the float64 reference of one case (computed once per test)."""
    B, T, K, H, scalar, chains, with_h0, want_dh0, with_mask = CASES[name]
    return R.make_case(B, T, K, H, scalar, with_h0, want_dh0, with_mask, 1000 + sorted(CASES).index(name))


def _bigru2_run(name, c, key12, tmp_path, save=True):
    """One forward (+ backward) call under (key 4, key 12) = (the case's, key12): {tensor: error vs float64}, profile labels."""
    chains = CASES[name][5]
    return R.run(c, {4: chains, 12: key12}, tmp_path, f"{name}_{key12}_{int(save)}.csv", save)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_bigru2_on_the_step_kernels_against_float64(name, tmp_path):
    """inet_bigru2_fwd / _bwd on gru_step_bf3_kernel / gru_step_bf3_bwd_kernel against oracle.torch_ref.gru_stack in float64 on the
    same parameters, initial state and {0, 2} mask; loss (out * wo).sum() + (hn * wh).sum(); out, h_n, dx (dx_scalar), dh0 and all
    16 parameter gradients, by the rule of the module docstring.  The profile labels prove the route: 2 T forward launches (two
    layers), 2 (T + 1) backward launches with the tail launch for dh0 and 2 T without; for B % 128 != 0 no backward step launch and
    the f32 per-step kernels' instead; in the T B = 3072 cases a bf16-pipe product, and the forward-only build (save = 0: the pieces
    replace the masked output) as well.  Worst pair measured on an MI355X: 1.52e-06 (step kernels) / 1.33e-06 (f32 per-step kernels)
    at B = 128, T = 24; every case: MEASURED in this module."""
    B, T, K, H, scalar, chains, with_h0, want_dh0, with_mask = CASES[name]
    c = _bigru2_case(name)
    step, labels = _bigru2_run(name, c, 1, tmp_path)
    base, blabels = _bigru2_run(name, c, 0, tmp_path)
    fwd = f"gru_step_bf3 p9 np2 B{B} H{H} sv"
    bwd = f"gru_step_bf3_bwd p9 np2 B{B} H{H}"
    nf, nb = labels.count(fwd), labels.count(bwd)
    nstep_bwd = sum(l.startswith("gru_bwd ") for l in labels)
    print(f"{name}: {nf} forward step launches, {nb} backward step launches, {nstep_bwd} f32 per-step backward launches")
    assert nf == 2 * T, sorted(set(labels))
    if B % 128 == 0:
        assert nb == 2 * (T + 1 if want_dh0 else T) and nstep_bwd == 0, sorted(set(labels))
    else:
        assert nb == 0 and nstep_bwd == 2 * (T + 1 if want_dh0 else T), sorted(set(labels))
    assert not any(l.startswith("gru_step_bf3") for l in blabels), sorted(set(blabels))
    pieces = T * B >= 3072
    assert any("bf3p9" in l for l in labels) == pieces, sorted(set(labels))
    errs = {k: (step[k], base[k]) for k in step}
    if pieces:
        fstep, flabels = _bigru2_run(name, c, 1, tmp_path, save=False)
        fbase, _ = _bigru2_run(name, c, 0, tmp_path, save=False)
        assert flabels.count(fwd[:-3]) == 2 * T and any("bf3p9" in l for l in flabels), sorted(set(flabels))
        errs.update({k + " (save=0)": (fstep[k], fbase[k]) for k in fstep})
    _check(name, errs)
    torch.cuda.synchronize()
    assert ops.chain_status() <= 0


# ------------------------------------------------------------------------------------------------ 2. the encoder (gather table)
@pytest.mark.gpu
@pytest.mark.parametrize("B", [128, 96])
def test_encoder_on_the_step_kernels_against_float64(B, tmp_path):
    """MeasureVAE's encoder (the gather-table build of the forward kernel, the encoder's inter-layer mask, saves) at H = 256, T = 24
    against oracle.torch_ref.encoder_forward in float64: mu, logsigma and every encoder gradient for random dmu / dlogsigma.  B = 128:
    both step kernels and the piece outputs (3072 rows); B = 96: the table build on the 96-row tile with an f32 backward pass.  The
    float64 oracle follows the kernel's SELU branch within 1e-5 of the kink (oracle.torch_ref.selu_k).  Measured on an MI355X, worst
    tensor (dW of the log-sigma head's second layer): B = 128 1.10e-06 / 8.73e-07, B = 96 9.16e-07 / 9.01e-07 (step / base)."""
    from tests.test_gpu_kernels import pack
    c = G.CFGS["pk"]
    T, H, V, Z = 24, c["H"], c["V"], c["Z"]
    cfg = ops.vae_config(V, c["E"], H, Z, H)
    table, total = ops.vae_param_table(cfg)
    P = G.vae_params("pk")
    params = pack(table, total, P)
    g = torch.Generator().manual_seed(40 + B)
    tok = torch.randint(0, V, (B, T), generator=g)
    mask = ops.dropout_mask((T, B, 2 * H), 0.5, 321, 0, DEV)
    dmu, dls = torch.randn(B, Z, generator=g) * 1e-2, torch.randn(B, Z, generator=g) * 1e-2
    enc = [(n, off, shape) for n, off, shape in table if n.startswith("encoder.")]
    runs = {}
    for key12 in (1, 0):
        try:
            ops.set_option(4, 0)
            ops.set_option(12, key12)
            ops.prof_enable(True)
            grads = torch.zeros_like(params)
            mu, ls, ews = ops.encoder_fwd(cfg, tok.to(DEV), params, mask=mask, save=True)
            ops.encoder_bwd(cfg, tok.to(DEV), params, grads, mask, dmu.to(DEV), dls.to(DEV), ews)
            ops.side_join()
            torch.cuda.synchronize()
            labels = _labels(tmp_path, f"enc_{B}_{key12}.csv")
        finally:
            ops.prof_enable(False)
            ops.set_option(4, 1)
            ops.set_option(12, 256)
        kinks = {k: ops.ws_field(cfg, ews, B, 0, k).view(B, 2 * H).cpu() > 0 for k in ("a_mu", "a_ls")}
        got = {"mu": mu.cpu(), "logsigma": ls.cpu()}
        for n, off, shape in enc:
            got["d" + n] = grads[off:off + int(np.prod(shape))].reshape(shape).cpu()
        runs[key12] = (got, kinks, labels)
    labels, blabels = runs[1][2], runs[0][2]
    nf = labels.count(f"gru_step_bf3 p9 np2 B{B} H{H} sv")
    nb = labels.count(f"gru_step_bf3_bwd p9 np2 B{B} H{H}")
    nstep_bwd = sum(l.startswith("gru_bwd ") for l in labels)
    print(f"encoder B{B}: {nf} forward step launches, {nb} backward step launches, {nstep_bwd} f32 per-step backward launches")
    assert nf == 2 * T, sorted(set(labels))
    assert (nb, nstep_bwd) == ((2 * T, 0) if B == 128 else (0, 2 * T)), sorted(set(labels))      # (the encoder asks for no dh0)
    assert any("bf3p9" in l for l in labels) == (T * B >= 3072), sorted(set(labels))
    assert not any(l.startswith("gru_step_bf3") for l in blabels), sorted(set(blabels))
    # float64 reference, once per distinct set of SELU branches (the two runs agree unless a pre-activation sits on the kink)
    P64 = {k: v.double() for k, v in P.items() if k.startswith("encoder.")}
    refs = []
    for key12 in (1, 0):
        kinks = runs[key12][1]
        if refs and all(torch.equal(kinks[k], runs[1][1][k]) for k in kinks):
            refs.append(refs[0])
            continue
        for v in P64.values():
            v.requires_grad_(True)
            v.grad = None
        O.kink_stats_reset()
        m64, l64 = O.encoder_forward(P64, tok, [mask.cpu().double().permute(1, 0, 2)], kinks=kinks)
        st = dict(O.KINK_STATS)
        assert st["violations"] == 0 and st["flips"] <= 8 and st["max_abs_flip"] <= O.KINK_TOL, st
        ((m64 * dmu.double()).sum() + (l64 * dls.double()).sum()).backward()
        ref = {"mu": m64.detach(), "logsigma": l64.detach()}
        ref.update({"d" + n: P64[n].grad.clone() for n, _, _ in enc})
        refs.append(ref)
    errs = {k: (_rel(runs[1][0][k], refs[0][k]), _rel(runs[0][0][k], refs[1][k])) for k in refs[0]}
    _check(f"encoder B{B}", errs)
    assert ops.chain_status() <= 0


# ------------------------------------------------------------------------------------------------ 3. the -3 contract for key 12
def _contract_inputs():
    from inpaintnet_amd import layout
    B, T, K, H = 128, 3, 8, 256
    g = torch.Generator().manual_seed(3)
    offs, total = layout.arena_offsets(dict(layout._gru("g", K, H, 2, True)))
    flat = (torch.randn(total, generator=g) * 0.05).to(DEV)
    x = torch.randn(B, T, K, generator=g).to(DEV)
    wo, wh = torch.randn(B, T, 2 * H, generator=g).to(DEV), torch.randn(4, B, H, generator=g).to(DEV)
    return B, T, K, H, flat, x, wo, wh


@pytest.mark.gpu
def test_backward_refuses_a_workspace_written_under_another_step_threshold():
    """inet_set_option key 12 decides per shape whether the W_hh piece buffers of the step kernels exist: a workspace written by a
    forward call under key 12 = 1 is carved differently under the default 256, and the backward call must refuse it (rc -3) instead of
    running the f32 per-step kernels over a shifted workspace (the options snapshot once folded key 12 into two probe shapes that
    answer alike for 1 and 256).  With the threshold restored the same call succeeds -- the refused call wrote nothing into the
    workspace -- and its dx is that of an undisturbed forward + backward pair, bit for bit.  (Key 2 pins the f32 products to the
    64 x 64 LDS-tiled kernel without split-K for the length of the test: the cost model's split-K plans sum their k ranges with f32
    atomics, in an order that differs from run to run, and two undisturbed pairs then already differ in the last bit.)"""
    from inpaintnet_amd._lib import InetError
    B, T, K, H, flat, x, wo, wh = _contract_inputs()
    try:
        ops.set_option(2, 0)
        ops.set_option(4, 0)
        ops.set_option(12, 1)
        o, h, ws = ops.bigru2_fwd(x, None, flat, H, B, T, K, save=True)
        dx0, _ = ops.bigru2_bwd(x, None, flat, torch.zeros_like(flat), H, B, T, K, None, wo, wh, ws, want_dx=True)
        ops.side_join()
        torch.cuda.synchronize()
        o, h, ws = ops.bigru2_fwd(x, None, flat, H, B, T, K, save=True)
        ops.set_option(12, 256)
        with pytest.raises(InetError, match="rc=-3"):
            ops.bigru2_bwd(x, None, flat, torch.zeros_like(flat), H, B, T, K, None, wo, wh, ws, want_dx=True)
        ops.set_option(12, 1)
        dx1, _ = ops.bigru2_bwd(x, None, flat, torch.zeros_like(flat), H, B, T, K, None, wo, wh, ws, want_dx=True)
        ops.side_join()
        torch.cuda.synchronize()
    finally:
        ops.set_option(2, -1)
        ops.set_option(4, 1)
        ops.set_option(12, 256)
    assert bool(torch.isfinite(dx0).all()) and float(dx0.abs().max()) > 0.0
    assert torch.equal(dx0, dx1)
    assert ops.chain_status() <= 0


def test_step_threshold_changes_the_workspace_carve():
    """Host only: why the options snapshot must carry key 12's value -- at (B, T, K, H) = (128, 3, 8, 256) without the chain kernels
    the workspace holds the step kernels' W_hh pieces under key 12 = 1 and not under the default 256."""
    from inpaintnet_amd import _lib
    L = _lib.lib()
    try:
        assert L.inet_set_option(4, 0) == 0
        assert L.inet_set_option(12, 1) == 0
        low = L.inet_bigru2_ws_bytes(128, 3, 8, 256, 1)
        assert L.inet_set_option(12, 256) == 0
        default = L.inet_bigru2_ws_bytes(128, 3, 8, 256, 1)
    finally:
        L.inet_set_option(4, 1)
        L.inet_set_option(12, 256)
    assert default > 0 and low > default, (low, default)
