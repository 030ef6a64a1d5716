#!/usr/bin/env python3
"""What gradient clipping costs on the GPU:
    python tools/clip_cost.py [--batch 256] [--steps 40] [--rounds 5] [--iters 20] [--out FILE.json]
1. grad_sqnorm, adam_clip and adam alone on arenas of the MeasureVAE's size, by HIP events around `iters` launches, the median of
   `rounds` rounds; GB/s from the launches' algorithmic bytes (4n; 28n + the partials; 28n).
2. The bench's MeasureVAE training step (every step from the seeded weights, as bench.py's) at --batch for max_grad_norm None, inf
   and a finite value that clips every step, in ONE process, alternating between the three within every round; the median over
   rounds of the time per step (host clock around `steps` steps between two synchronisations).
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


def kernels_alone(n, rounds, iters):
    dev = "cuda:0"
    g = torch.randn(n, device=dev) * 1e-3
    p, m, v = torch.randn(n, device=dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    part = ops.grad_sqnorm(g)
    flag = torch.zeros(2, device=dev)
    jobs = {
        "grad_sqnorm": (lambda: ops.grad_sqnorm(g, part), 4.0 * n),
        "adam_clip": (lambda: ops.adam_step_clip(p, g, m, v, 1e-4, 7, 1.0, part, step_flag=flag), 28.0 * n + 8.0 * part.numel()),
        "adam": (lambda: ops.adam_step(p, g, m, v, 1e-4, 7, step_flag=flag), 28.0 * n),
    }
    out = {}
    for name, (fn, nbytes) in jobs.items():
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
        out[name] = {"us": round(med, 2), "us_rounds": [round(x, 2) for x in us], "GB_per_s": round(nbytes / med / 1e3, 1)}
    return out


class Workload:
    def __init__(self, batch, max_grad_norm):
        self.ds = synthetic.SyntheticFolkDataset(num_notes=NUM_NOTES)
        self.model = MeasureVAE(self.ds)
        self.model.load_state_dict({k: torch.from_numpy(synthetic.det_param(k, tuple(v.shape)))
                                    for k, v in self.model.state_dict().items()})
        self.trainer = VAETrainer(self.ds, self.model, lr=1e-4, max_grad_norm=max_grad_norm)
        self.trainer.overlap_backward = True
        self.model.train()
        self.tokens = torch.from_numpy(synthetic.det_tokens("clip_cost", (batch, 24), NUM_NOTES)).cuda()
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
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("clip_cost.py measures on the GPU; none found")
    probe = Workload(a.batch, float("inf"))
    probe.run(3)
    probe.trainer.finish()
    norm = probe.trainer.last_grad_norm
    n = probe.model.flat.numel()
    res = {"arena_floats": n, "arena_MB": round(4e-6 * n, 1), "kernels": kernels_alone(n, a.rounds, a.iters),
           "batch": a.batch, "first_norm": norm, "max_grad_norm_finite": 0.01 * norm}
    wls = {"none": Workload(a.batch, None), "inf": probe, "finite": Workload(a.batch, 0.01 * norm)}
    for w in wls.values():
        w.run(5)
    ms = {k: [] for k in wls}
    for _ in range(a.rounds):
        for k, w in wls.items():
            ms[k].append(w.run(a.steps))
    for w in wls.values():
        w.trainer.finish()
    res["step_ms"] = {k: {"median": round(statistics.median(x), 4), "rounds": [round(y, 4) for y in x]} for k, x in ms.items()}
    res["clipped_steps"] = {k: w.trainer.clipped_steps for k, w in wls.items()}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
