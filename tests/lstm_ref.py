"""Harness of the tests that hold the LSTM layer (inet_lstm_fwd / _bwd) and the two-layer pipeline (inet_lstm2_fwd / _bwd) to a float64
evaluation of the same recurrence (oracle.torch_ref.lstm_cell / lstm_layer, autograd for the gradients): one case = parameters, inputs
and the float64 reference, computed once; one run = the library calls under a set of options, every result as
max |got - ref| / max |ref|, plus the (class, label) rows of its launches.  Modelled on tests/bigru2_ref.py; used by
tests/test_gpu_lstm_chain_tiles.py."""
import csv

import numpy as np
import torch

from oracle import torch_ref as O
from tests.bigru2_ref import check, rel  # noqa: F401  (the rule and the error measure are the GRU file's)

DEV = "cuda:0"
PROF_STEP_FWD, PROF_STEP_BWD = 1, 2     # profile classes of the recurrent launches (include/inpaintnet_hip.h inet_prof_read)


def launches(tmp_path, name):
    """The recurrent launches of a profile dump: (class, label) of every row of class 1 / 2.  The per-step LSTM kernels carry no label."""
    from inpaintnet_amd import ops
    path = str(tmp_path / name)
    ops.prof_dump(path)
    return [(int(r["class"]), r["label"]) for r in csv.DictReader(open(path)) if int(r["class"]) in (PROF_STEP_FWD, PROF_STEP_BWD)]


def _params(g, H, names):
    """weights ~ N(0, 1/H), biases ~ 0.1: the recurrence stays contractive at every T"""
    return {k: torch.randn(4 * H, H, generator=g) / np.sqrt(H) if k.startswith("W") else torch.randn(4 * H, generator=g) * 0.1
            for k in names}


def _layer64(gi, h, c, W_hh, b_hh, reverse):
    """oracle lstm_cell over gi [T,B,4H] (time-major, b_ih included) -> out [T,B,H], (hT, cT)"""
    T = gi.shape[0]
    outs = [None] * T
    for t in (range(T - 1, -1, -1) if reverse else range(T)):
        h, c = O.lstm_cell(gi[t], h, c, W_hh, b_hh)
        outs[t] = h
    return torch.stack(outs, 0), (h, c)


def make_single(B, T, H, reverse, with_state, seed, scale=0.5):
    """One layer: gi [T,B,4H] is the input (the caller's GEMM forms it), h0 / c0 random in (-1, 1) or absent; gradients flow in through
    the output sequence and the final state."""
    g = torch.Generator().manual_seed(seed)
    P = _params(g, H, ("W_hh", "b_hh"))
    gi = torch.randn(T, B, 4 * H, generator=g) * scale
    h0 = torch.rand(B, H, generator=g) * 2 - 1 if with_state else None
    c0 = torch.rand(B, H, generator=g) * 2 - 1 if with_state else None
    wo, wh, wc = torch.randn(T, B, H, generator=g), torch.randn(B, H, generator=g), torch.randn(B, H, generator=g)
    P64 = {k: v.double().requires_grad_(True) for k, v in P.items()}
    gi64 = gi.double().requires_grad_(True)
    h64 = (h0.double() if with_state else torch.zeros(B, H, dtype=torch.float64)).requires_grad_(True)
    c64 = (c0.double() if with_state else torch.zeros(B, H, dtype=torch.float64)).requires_grad_(True)
    out, (hT, cT) = _layer64(gi64, h64, c64, P64["W_hh"], P64["b_hh"], reverse)
    ((out * wo.double()).sum() + (hT * wh.double()).sum() + (cT * wc.double()).sum()).backward()
    ref = {"out": out.detach(), "hT": hT.detach(), "cT": cT.detach(), "dgi": gi64.grad, "dh0": h64.grad, "dc0": c64.grad,
           "dW_hh": P64["W_hh"].grad, "db_ih": P64["b_hh"].grad, "db_hh": P64["b_hh"].grad}
    dev = lambda t: None if t is None else t.to(DEV)
    return dict(spec=(B, T, H, reverse), P={k: dev(v) for k, v in P.items()}, gi=dev(gi), h0=dev(h0), c0=dev(c0), wo=dev(wo), wh=dev(wh),
                wc=dev(wc), ref=ref)


def make_pipeline(B, T, H, reverse, seed, scale=0.5):
    """Two stacked layers with zero initial states: gi0 [T,B,4H] is the input, layer 1 = oracle lstm_layer over layer 0's output."""
    g = torch.Generator().manual_seed(seed)
    P = _params(g, H, ("W_hh0", "b_hh0", "W_ih1", "b_ih1", "W_hh1", "b_hh1"))
    gi0 = torch.randn(T, B, 4 * H, generator=g) * scale
    wo = torch.randn(T, B, H, generator=g)
    P64 = {k: v.double().requires_grad_(True) for k, v in P.items()}
    gi64 = gi0.double().requires_grad_(True)
    z = torch.zeros(B, H, dtype=torch.float64)
    out0, _ = _layer64(gi64, z, z, P64["W_hh0"], P64["b_hh0"], reverse)
    L1 = {"l.weight_ih_l0": P64["W_ih1"], "l.bias_ih_l0": P64["b_ih1"], "l.weight_hh_l0": P64["W_hh1"], "l.bias_hh_l0": P64["b_hh1"]}
    out1, _ = O.lstm_layer(out0.permute(1, 0, 2), z, z, L1, "l", reverse=reverse)
    out1 = out1.permute(1, 0, 2)
    (out1 * wo.double()).sum().backward()
    ref = {"out0": out0.detach(), "out1": out1.detach(), "dgi0": gi64.grad, "dW_hh0": P64["W_hh0"].grad, "db_ih0": P64["b_hh0"].grad,
           "db_hh0": P64["b_hh0"].grad, "dW_ih1": P64["W_ih1"].grad, "dW_hh1": P64["W_hh1"].grad, "db_ih1": P64["b_ih1"].grad,
           "db_hh1": P64["b_hh1"].grad}
    return dict(spec=(B, T, H, reverse), P={k: v.to(DEV) for k, v in P.items()}, gi0=gi0.to(DEV), wo=wo.to(DEV), ref=ref)


def _single_calls(c):
    from inpaintnet_amd import ops
    B, T, H, reverse = c["spec"]
    P = c["P"]
    o, hT, cT, ws = ops.lstm_fwd(c["gi"], P["W_hh"], P["b_hh"], H, reverse=reverse, h0=c["h0"], c0=c["c0"], save=True, want_state=True)
    dW, dbi, dbh = torch.zeros_like(P["W_hh"]), torch.zeros_like(P["b_hh"]), torch.zeros_like(P["b_hh"])
    dgi, dh0, dc0 = ops.lstm_bwd(P["W_hh"], o, c["wo"], H, reverse, ws, dW, dbi, dbh, h0=c["h0"], dhT=c["wh"], dcT=c["wc"],
                                 want_dstate=True)
    ops.side_join()
    return {"out": o, "hT": hT, "cT": cT, "dgi": dgi, "dh0": dh0, "dc0": dc0, "dW_hh": dW, "db_ih": dbi, "db_hh": dbh}


GRADS2 = ("dW_hh0", "db_ih0", "db_hh0", "dW_ih1", "dW_hh1", "db_ih1", "db_hh1")


def _pipeline_calls(c, layer_by_layer):
    """The pipeline (ops.lstm2_fwd / lstm2_bwd), or the same two layers one after the other -- the path a caller takes when the pipeline
    refuses the shape, which it must under key 4 = 0."""
    from inpaintnet_amd import ops
    B, T, H, reverse = c["spec"]
    P = c["P"]
    grads = [torch.zeros_like(P[k[1:]]) if k[1:] in P else torch.zeros_like(P["b_hh0"]) for k in GRADS2]
    if layer_by_layer:
        assert ops.lstm2_fwd(c["gi0"], P["W_hh0"], P["b_hh0"], P["W_ih1"], P["b_ih1"], P["W_hh1"], P["b_hh1"], H, reverse=reverse,
                             save=True) is None
        o0, _, _, ws0 = ops.lstm_fwd(c["gi0"], P["W_hh0"], P["b_hh0"], H, reverse=reverse, save=True)
        gi1 = ops.linear_fwd(o0.view(T * B, H), P["W_ih1"], P["b_ih1"]).view(T, B, 4 * H)
        o1, _, _, ws1 = ops.lstm_fwd(gi1, P["W_hh1"], P["b_hh1"], H, reverse=reverse, save=True)
        dgi1, _, _ = ops.lstm_bwd(P["W_hh1"], o1, c["wo"], H, reverse, ws1, grads[4], grads[5], grads[6])
        do0 = ops.linear_bwd(dgi1.view(T * B, 4 * H), o0.view(T * B, H), P["W_ih1"], grads[3], None, need_dx=True).view(T, B, H)
        dgi0, _, _ = ops.lstm_bwd(P["W_hh0"], o0, do0.contiguous(), H, reverse, ws0, grads[0], grads[1], grads[2])
    else:
        o0, o1, ws0, ws1 = ops.lstm2_fwd(c["gi0"], P["W_hh0"], P["b_hh0"], P["W_ih1"], P["b_ih1"], P["W_hh1"], P["b_hh1"], H,
                                         reverse=reverse, save=True)
        dgi0 = ops.lstm2_bwd(P["W_hh0"], P["W_ih1"], P["W_hh1"], o0, o1, c["wo"], H, reverse, ws0, ws1, grads=grads)
    ops.side_join()
    return dict({"out0": o0, "out1": o1, "dgi0": dgi0}, **dict(zip(GRADS2, grads)))


def run(c, chain, tmp_path, csv_name, pipeline):
    """One forward + backward of case c with the chain kernels on (key 4 = 1) or off: {tensor: error vs float64}, the recurrent launches
    as (class, label), and ops.lstm_chain_plan for the shape as it stood during the call (with the slow-wait recorder's summary of
    the call under "slow_waits": a hand-off that took milliseconds is what launches that were not resident together leave behind)."""
    from inpaintnet_amd import ops
    B, T, H, _ = c["spec"]
    try:
        ops.set_option(4, int(chain))
        plan = ops.lstm_chain_plan(B, T, H, pipeline)
        ops.slow_waits(reset=True)
        ops.prof_enable(True)
        got = _pipeline_calls(c, not chain) if pipeline else _single_calls(c)
        torch.cuda.synchronize()
        rows = launches(tmp_path, csv_name)
        plan["slow_waits"] = ops.slow_waits_summary(reset=True)
    finally:
        ops.prof_enable(False)
        ops.set_option(4, 1)
    assert set(got) == set(c["ref"])
    for k, v in got.items():
        assert bool(torch.isfinite(v).all()), (csv_name, k)
    return {k: rel(got[k], c["ref"][k]) for k in c["ref"]}, rows, plan
