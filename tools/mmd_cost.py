#!/usr/bin/env python3
"""What the MMD latent loss costs on the GPU:
    python tools/mmd_cost.py [--shapes 256x256,4096x256] [--batch 256] [--steps 40] [--rounds 5] [--iters 20] [--kernels-only] [--out FILE.json]
1. ops.mmd alone (its pair and finish launches) at every (B, Z) of --shapes, both kernels, with and without the gradient, by HIP
   events around `iters` calls, the median of `rounds` rounds.
2. The bench's MeasureVAE training step (every step from the seeded weights, as bench.py's) at --batch for the default trainer and for
   mmd_coeff = 10, in ONE process, alternating within every round; the median over rounds of the time per step (host clock around
   `steps` steps between two synchronisations).
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
from inpaintnet_amd.vae_trainer import VAETrainer               # noqa: E402

NUM_NOTES = 48


def kernels_alone(B, Z, rounds, iters):
    dev = "cuda:0"
    x = torch.from_numpy(0.6 * synthetic.det_normal("mmd_cost/x", (B, Z)) + 0.2).float().to(dev)
    y = torch.from_numpy(synthetic.det_normal("mmd_cost/y", (B, Z))).float().to(dev)
    out = {}
    for kernel in ("gaussian", "imq"):
        for want_grad in (False, True):
            fn = lambda: ops.mmd(x, y, kernel, None, "unbiased", 10.0, want_grad=want_grad)
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
            med = statistics.median(us)
            # the work: a subtraction and a fused multiply-add per pair and latent dimension, three sums, two more passes for a gradient
            flop = 3.0 * B * B * Z * (3 + (2 if want_grad else 0))
            out[f"{kernel}{'+grad' if want_grad else ''}"] = {"us_per_call": round(med, 2), "us_rounds": [round(v, 2) for v in us],
                                                            "GFLOP_per_s": round(flop / med / 1e3, 1)}
    out["value"] = float(ops.mmd(x, y, "gaussian", None, "unbiased", 10.0)[0][0])
    return out


class Workload:
    def __init__(self, batch, **kw):
        self.ds = synthetic.SyntheticFolkDataset(num_notes=NUM_NOTES)
        self.model = MeasureVAE(self.ds)
        self.model.load_state_dict({k: torch.from_numpy(synthetic.det_param(k, tuple(v.shape)))
                                    for k, v in self.model.state_dict().items()})
        self.trainer = VAETrainer(self.ds, self.model, lr=1e-4, **kw)
        self.trainer.overlap_backward = True
        self.model.train()
        self.tokens = torch.from_numpy(synthetic.det_tokens("mmd_cost", (batch, 24), NUM_NOTES)).cuda()
        self.start = self.model.flat.detach().clone()

    def step(self):
        self.model.flat.copy_(self.start)
        t = self.trainer
        t.zero_grad()
        loss, acc = t.loss_and_acc_for_batch(self.tokens, 0, train=True)
        loss.backward()
        t.step()

    def run(self, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            self.step()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="256x256,4096x256")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mmd_cost.py measures on the GPU; none found")
    res = {"kernels": {}}
    for shape in a.shapes.split(","):
        B, Z = (int(v) for v in shape.split("x"))
        res["kernels"][shape] = kernels_alone(B, Z, a.rounds, a.iters)
    if not a.kernels_only:
        wls = {"default": Workload(a.batch), "mmd": Workload(a.batch, mmd_coeff=10.0)}
        for w in wls.values():
            w.run(5)
        ms = {k: [] for k in wls}
        for _ in range(a.rounds):
            for k, w in wls.items():
                ms[k].append(w.run(a.steps))
        for w in wls.values():
            w.trainer.finish()
        res["batch"] = a.batch
        res["step_ms"] = {k: {"median": round(statistics.median(v), 4), "rounds": [round(y, 4) for y in v]} for k, v in ms.items()}
        res["last_mmd"] = {k: float(v) for k, v in wls["mmd"].trainer.last_mmd.items()}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
