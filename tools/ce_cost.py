#!/usr/bin/env python3
"""What the class-weighted, label-smoothed cross-entropy costs on the GPU:
    python tools/ce_cost.py [--measures 256] [--rounds 7] [--iters 50] [--out FILE.json]
At the headline shape -- `measures` x 24 rows of the benchmark's V = 48 post-ReLU logits -- by HIP events around `iters` calls, the
median of `rounds` rounds, the three variants alternating within every round:
  plain          the pair the default VAE step launches: inet_cross_entropy_ex forward (loss, accuracy, the KL term folded in) and
                 backward (dW times the device scalar, the forwarded KL gradient)
  w_off          the new trio with all options off: the counting launch, the loss launch (with the statistics), the gradient launch
  w_on           the trio with class weights and label smoothing 0.1
and each launch of the trio alone.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from inpaintnet_amd import ops                                  # noqa: E402

V = 48


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--measures", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ce_cost.py measures on the GPU; there is none here")
    dev = "cuda:0"
    rows = a.measures * 24
    g = torch.Generator().manual_seed(28)
    w = torch.relu(torch.randn(rows, V, generator=g)).to(dev)
    t = torch.randint(0, V, (rows,), generator=g)
    t[torch.rand(rows, generator=g) < 0.7] = 0                                  # one symbol dominates, as the hold token does
    t = t.to(dev)
    cw = (torch.rand(V, generator=g) + 0.5).to(dev)
    kl, gl = torch.tensor([3.0], device=dev), torch.tensor([1.0], device=dev)
    out2, dW, gkl = torch.zeros(2, device=dev), torch.empty(rows, V, device=dev), torch.empty(1, device=dev)

    def plain():
        out2.zero_()
        ops.cross_entropy_ex(w, t, loss_sum=out2[0:1], correct=out2[1:2], out_scale=1.0 / rows, add_term=kl, add_scale=1e-3)
        ops.cross_entropy_ex(w, t, dW=dW, scale=1.0 / rows, scale_dev=gl, fwd_out=gkl, fwd_scale=1e-3)

    def count(cwv):
        return ops.class_counts(t, V, cwv, None, extra=3 * V)

    def fwd(c, cwv, e):
        ops.cross_entropy_w(w, t, c, cwv, e, None, loss=out2[0:1], accuracy=out2[1:2], class_stats=c.extra.view(V, 3), add_term=kl,
                            add_scale=1e-3)

    def bwd(c, cwv, e):
        ops.cross_entropy_w(w, t, c, cwv, e, None, dW=dW, scale_dev=gl, fwd_out=gkl, fwd_scale=1e-3)

    def trio(cwv, e):
        c = count(cwv)
        fwd(c, cwv, e)
        bwd(c, cwv, e)

    c_off, c_on = count(None), count(cw)
    variants = {
        "plain": plain, "w_off": lambda: trio(None, 0.0), "w_on": lambda: trio(cw, 0.1),
        "plain_zero_fill": out2.zero_,
        "plain_fwd": lambda: ops.cross_entropy_ex(w, t, loss_sum=out2[0:1], correct=out2[1:2], out_scale=1.0 / rows, add_term=kl, add_scale=1e-3),
        "plain_bwd": lambda: ops.cross_entropy_ex(w, t, dW=dW, scale=1.0 / rows, scale_dev=gl, fwd_out=gkl, fwd_scale=1e-3),
        "count_off": lambda: count(None), "count_on": lambda: count(cw),
        "fwd_off": lambda: fwd(c_off, None, 0.0), "fwd_on": lambda: fwd(c_on, cw, 0.1),
        "bwd_off": lambda: bwd(c_off, None, 0.0), "bwd_on": lambda: bwd(c_on, cw, 0.1),
    }
    for fn in variants.values():
        for _ in range(5):
            fn()
    us = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(a.iters):
                fn()
            e1.record()
            e1.synchronize()
            us[k].append(1e3 * e0.elapsed_time(e1) / a.iters)
    res = {"rows": rows, "V": V, "iters": a.iters,
           "us_per_call": {k: {"median": round(statistics.median(v), 2), "rounds": [round(x, 2) for x in v]} for k, v in us.items()}}
    trio(cw, 0.1)
    res["loss_w_on"], res["accuracy"] = float(out2[0]), float(out2[1])
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
