#!/usr/bin/env python3
"""What the importance-weighted log-likelihood costs on the GPU:
    python tools/iw_cost.py [--batch 256] [--samples 16] [--z 256] [--rounds 5] [--iters 20] [--calls 5] [--kernels-only] [--out FILE.json]
1. The three kernels alone at (B, Kc, Z, V = the bench vocabulary, T = 24), by HIP events around `iters` calls, the median of `rounds`
   rounds: ops.iw_draw next to ops.reparam_kl on the same number of elements (B Kc x Z), ops.nll_rows next to ops.cross_entropy
   without dW on the same logits, ops.iw_finish on (B, K).
2. VAETester.log_likelihood on one batch of B measures at K samples (the bench's MeasureVAE, eval mode), next to the encoder and the
   teacher-forced decoder launches of the same call alone: the host clock around `calls` calls between two synchronisations, the
   median of `rounds` rounds, and the share of the wall time spent outside those launches; MeasureVAE.log_weights with and without
   reproducible=True (one k range per product against the planner's choice).
Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from inpaintnet_amd import ops, synthetic                       # noqa: E402
from inpaintnet_amd.measure_vae import MeasureVAE               # noqa: E402
from inpaintnet_amd.vae_tester import VAETester                 # noqa: E402

NUM_NOTES = 48
T = 24


def event_us(fn, rounds, iters):
    for _ in range(3):
        fn()
    us = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        us.append(1e3 * a.elapsed_time(b) / iters)
    return {"us_per_call": round(statistics.median(us), 2), "us_rounds": [round(v, 2) for v in us]}


def kernels_alone(B, Kc, Z, V, rounds, iters):
    dev = "cuda:0"
    rows = B * Kc
    mu = torch.from_numpy(synthetic.det_normal("iw_cost/mu", (B, Z))).to(dev)
    ls = torch.from_numpy(0.3 * synthetic.det_normal("iw_cost/ls", (B, Z))).float().to(dev)
    eps = torch.from_numpy(synthetic.det_normal("iw_cost/eps", (B, Kc, Z))).to(dev)
    mu_r, ls_r, eps_r = mu.repeat_interleave(Kc, 0).contiguous(), ls.repeat_interleave(Kc, 0).contiguous(), eps.reshape(rows, Z)
    kl = torch.zeros(1, device=dev)
    w = torch.from_numpy(3.0 * synthetic.det_normal("iw_cost/w", (rows, T, V))).float().to(dev)
    tg = torch.from_numpy(synthetic.det_tokens("iw_cost/t", (rows, T), V)).to(dev)
    logr = torch.from_numpy(synthetic.det_normal("iw_cost/r", (rows,))).to(dev)
    nll, logw = torch.empty(B, Kc, device=dev), torch.empty(B, Kc, device=dev)
    out2 = torch.zeros(2, device=dev)
    w2, tg1 = w.view(rows * T, V), tg.view(-1)
    res = {
        "iw_draw": event_us(lambda: ops.iw_draw(mu, ls, eps), rounds, iters),
        "reparam_kl_same_elements": event_us(lambda: ops.reparam_kl(mu_r, ls_r, eps_r, kl_sum=kl), rounds, iters),
        "reparam_kl_same_elements_no_kl": event_us(lambda: ops.reparam_kl(mu_r, ls_r, eps_r), rounds, iters),
        "nll_rows": event_us(lambda: ops.nll_rows(w, tg, logr, group=Kc, out_nll=nll, out_logw=logw), rounds, iters),
        "cross_entropy_no_dW": event_us(lambda: ops.cross_entropy(w2, tg1, out2, out_scale=1.0 / (rows * T)), rounds, iters),
        "iw_finish": event_us(lambda: ops.iw_finish(logw, nll), rounds, iters),
    }
    res["iw_draw"]["GB_per_s"] = round(4.0 * (2 * rows * Z + 2 * B * Z + rows) / res["iw_draw"]["us_per_call"] / 1e3, 1)
    res["nll_rows"]["GB_per_s"] = round(4.0 * rows * T * V / res["nll_rows"]["us_per_call"] / 1e3, 1)
    return res


def end_to_end(B, K, rounds, calls):
    ds = synthetic.SyntheticFolkDataset(num_notes=NUM_NOTES)
    model = MeasureVAE(ds)
    model.load_state_dict({k: torch.from_numpy(synthetic.det_param(k, tuple(v.shape))) for k, v in model.state_dict().items()})
    tester = VAETester(ds, model)
    tok = torch.from_numpy(synthetic.det_tokens("iw_cost/tokens", (B, T), NUM_NOTES)).cuda()
    loader = [(tok, None)]
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    rows = tok.repeat_interleave(K, 0)
    z = torch.from_numpy(synthetic.det_normal("iw_cost/z", (B * K, model.latent_space_dim))).cuda()

    def whole():
        return tester.log_likelihood(loader, num_samples=K, generator=g, max_rows=B * K)

    eps = torch.randn(B, K, model.latent_space_dim, device="cuda", generator=g)

    def model_only():
        with torch.no_grad(), ops.one_k_range():             # (the GEMM settings log_weights runs under)
            model.encoder(tok)
            model.decoder(z, rows, train=False, teacher_forced=True)

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / calls
    fns = {"log_likelihood": whole, "encoder_and_decoder": model_only,
           "log_weights_reproducible": lambda: model.log_weights(tok, K, eps=eps, max_rows=B * K),
           "log_weights_planner": lambda: model.log_weights(tok, K, eps=eps, max_rows=B * K, reproducible=False)}
    for fn in fns.values():
        fn()
        fn()
    ms = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            ms[k].append(clock(fn))
    res = {k: {"median_ms": round(statistics.median(v), 4), "rounds_ms": [round(y, 4) for y in v]} for k, v in ms.items()}
    whole_ms, model_ms = res["log_likelihood"]["median_ms"], res["encoder_and_decoder"]["median_ms"]
    res["share_outside_encoder_and_decoder"] = round(1.0 - model_ms / whole_ms, 4)
    res["measures_per_s"] = round(B / whole_ms * 1e3, 1)
    res["result"] = whole()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--z", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("iw_cost.py measures on the GPU; none found")
    res = {"shape": {"B": a.batch, "Kc": a.samples, "Z": a.z, "V": NUM_NOTES, "T": T},
           "kernels": kernels_alone(a.batch, a.samples, a.z, NUM_NOTES, a.rounds, a.iters)}
    if not a.kernels_only:
        res["end_to_end"] = end_to_end(a.batch, a.samples, a.rounds, a.calls)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
