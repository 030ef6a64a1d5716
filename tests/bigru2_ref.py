"""Harness of the tests that hold inet_bigru2_fwd / _bwd (two directions, two layers) to a float64 evaluation of the same stack
(oracle.torch_ref.gru_stack): one case = parameters, inputs and the float64 reference, computed once; one run = the library call under
a set of options, every result as max |got - ref| / max |ref|, plus the profile labels of its launches.  Shared by
tests/test_gpu_gru_step_bf3.py (the bf16-pipe step kernels) and tests/test_gpu_gru_chain_tiles.py (the chain kernels)."""
import csv

import numpy as np
import torch

from oracle import torch_ref as O

DEV = "cuda:0"
# inet_set_option keys the runs change, and the library's defaults they go back to
DEFAULTS = {4: 1, 7: 9, 12: 256}


def labels(tmp_path, name):
    from inpaintnet_amd import ops
    path = str(tmp_path / name)
    ops.prof_dump(path)
    return [r["label"] for r in csv.DictReader(open(path))]


def rel(got, ref):
    """max |got - ref| / max |ref|; against an all-zero reference (dW_hh at T = 1 from a zero state) the absolute error."""
    ref = torch.as_tensor(ref).detach().double().cpu()
    scale = float(ref.abs().max())
    return float((got.detach().double().cpu() - ref).abs().max()) / (scale if scale > 0.0 else 1.0)


def check(tag, errs, what, cap, floor):
    """errs: {tensor: (err, err_base)}.  Prints every pair, then: err <= 2 err_base + floor, err < cap, err_base < cap / 2."""
    for k, (es, eb) in errs.items():
        print(f"{tag} {k}: {what} {es:.2e} base {eb:.2e}")
    ws = max(errs, key=lambda k: errs[k][0])
    print(f"{tag} WORST {what} {errs[ws][0]:.2e} ({ws}); worst base {max(e[1] for e in errs.values()):.2e}")
    bad = [(k, es, eb) for k, (es, eb) in errs.items()
           if not (es <= 2.0 * eb + floor and es < cap and eb < 0.5 * cap)]
    assert not bad, (tag, bad)


def make_case(B, T, K, H, scalar, with_h0, want_dh0, with_mask, seed):
    """Parameters, inputs and the float64 reference of one case."""
    from inpaintnet_amd import layout
    g = torch.Generator().manual_seed(seed)
    shapes = layout._gru("g", K, H, 2, True)
    offs, total = layout.arena_offsets(dict(shapes))
    # weights ~ N(0, 1/H), biases ~ 0.1: the recurrence stays contractive at every T
    P = {k: torch.randn(*s, generator=g) * ((1.0 / np.sqrt(H)) if "weight" in k else 0.1) for k, s in shapes}
    flat = torch.zeros(total)
    for k, (off, s) in offs.items():
        flat[off:off + P[k].numel()] = P[k].reshape(-1)
    h0 = torch.tanh(torch.randn(4, B, H, generator=g)) if with_h0 else None
    mask = (torch.rand(T, B, 2 * H, generator=g) > 0.5).float() * 2.0 if with_mask else None
    xs = torch.randn(1, generator=g) if scalar else None
    x = None if scalar else torch.randn(B, T, K, generator=g)
    wo = torch.randn(B, T, 2 * H, generator=g)
    wh = torch.randn(4, B, H, generator=g)
    # float64 reference
    P64 = {k: v.double().requires_grad_(True) for k, v in P.items()}
    h64 = (h0.double() if with_h0 else torch.zeros(4, B, H, dtype=torch.float64)).requires_grad_(True)
    if scalar:
        xs64 = xs.double().requires_grad_(True)
        x64 = xs64.view(1, 1, 1).expand(B, T, 1)
    else:
        x64 = x.double().requires_grad_(True)
    out, hn = O.gru_stack(x64, h64, P64, "g", 2, True, [mask.double().permute(1, 0, 2)] if with_mask else None)
    ((out * wo.double()).sum() + (hn * wh.double()).sum()).backward()
    ref = {"out": out.detach(), "hn": hn.detach(), "dx": (xs64 if scalar else x64).grad}
    if want_dh0:
        ref["dh0"] = h64.grad
    for k in P:
        ref["d" + k] = P64[k].grad
    dev = lambda t: None if t is None else t.to(DEV)
    return dict(spec=(B, T, K, H, scalar, want_dh0), P=P, offs=offs, flat=flat.to(DEV), x=dev(x), xs=dev(xs), h0=dev(h0),
                mask=dev(mask), wo=dev(wo), wh=dev(wh), ref=ref, fwd_ref={"out": ref["out"], "hn": ref["hn"]})


def run(c, options, tmp_path, csv_name, save=True, plan=None):
    """One forward (+ backward) call of case c under inet_set_option {key: value}: {tensor: error vs float64}, profile labels.
    plan: a callable evaluated while the options are in force (what a planner says about the call); its value is returned third."""
    from inpaintnet_amd import ops
    B, T, K, H, scalar, want_dh0 = c["spec"]
    planned = None
    try:
        for k, v in options.items():
            ops.set_option(k, v)
        if plan is not None:
            planned = plan()
        ops.prof_enable(True)
        o, h, ws = ops.bigru2_fwd(c["x"], c["xs"], c["flat"], H, B, T, K, h0=c["h0"], mask=c["mask"], save=save)
        got = {"out": o, "hn": h}
        if save:
            grads = torch.zeros_like(c["flat"])
            dxs = torch.zeros(1, device=DEV) if scalar else None
            dx, dh0 = ops.bigru2_bwd(c["x"], c["xs"], c["flat"], grads, H, B, T, K, c["mask"], c["wo"], c["wh"], ws,
                                     want_dx=not scalar, dx_scalar=dxs, want_dh0=want_dh0)
            ops.side_join()
            got["dx"] = dxs if scalar else dx
            if want_dh0:
                got["dh0"] = dh0
            for k, (off, sh) in c["offs"].items():
                got["d" + k] = grads[off:off + c["P"][k].numel()].reshape(sh)
        torch.cuda.synchronize()
        lab = labels(tmp_path, csv_name)
    finally:
        ops.prof_enable(False)
        for k in options:
            ops.set_option(k, DEFAULTS[k])
    ref = c["ref"] if save else c["fwd_ref"]
    assert set(got) == set(ref)
    for k, v in got.items():
        assert bool(torch.isfinite(v).all()), (csv_name, k)
    errs = {k: rel(got[k], ref[k]) for k in ref}
    return (errs, lab) if plan is None else (errs, lab, planned)
