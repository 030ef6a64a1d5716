#!/usr/bin/env python3
"""What decoupled weight decay and the EMA shadow weights cost on the GPU:
    python tools/adamw_cost.py [--batch 256] [--steps 40] [--rounds 5] [--iters 20] [--out FILE.json]
1. adamw alone on arenas of the MeasureVAE's size in its four forms (plain, with the mask, with the EMA, with both), and adam and
   adam_clip in the same process as the baseline, by HIP events around `iters` launches, the median of `rounds` rounds; GB/s from the
   launches' algorithmic bytes (28n + n/8 with the mask + 8n with the EMA + the partials).  Back-to-back launches over 71 MB arenas
   see the Infinity Cache: the figures compare the forms with each other, not with HBM's peak.
2. The bench's MeasureVAE training step (every step from the seeded weights, as bench.py's) at --batch with the options off, with
   weight decay, with the EMA and with both, in ONE process, alternating between the four within every round; the median over rounds
   of the time per step (host clock around `steps` steps between two synchronisations).
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


def kernels_alone(n, mask, rounds, iters):
    dev = "cuda:0"
    g = torch.randn(n, device=dev) * 1e-3
    p, m, v = torch.randn(n, device=dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    e = p.clone()
    part = ops.grad_sqnorm(g)
    flag = torch.zeros(2, device=dev)

    def adamw(**kw):
        return lambda: ops.adamw_step(p, g, m, v, 1e-4, 7, weight_decay=0.01, step_flag=flag, **kw)
    jobs = {
        "adam": (lambda: ops.adam_step(p, g, m, v, 1e-4, 7, step_flag=flag), 28.0 * n),
        "adam_clip": (lambda: ops.adam_step_clip(p, g, m, v, 1e-4, 7, 1.0, part, step_flag=flag), 28.0 * n + 8.0 * part.numel()),
        "adamw": (adamw(), 28.0 * n),
        "adamw_mask": (adamw(decay_mask=mask), 28.0 * n + n / 8.0),
        "adamw_ema": (adamw(ema=e, ema_decay=0.999), 36.0 * n),
        "adamw_mask_ema": (adamw(decay_mask=mask, ema=e, ema_decay=0.999), 36.0 * n + n / 8.0),
        "adamw_clip_mask_ema": (adamw(decay_mask=mask, ema=e, ema_decay=0.999, max_norm=1.0, partials=part),
                                36.0 * n + n / 8.0 + 8.0 * part.numel()),
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
    out["expected_full_from_bytes_us"] = round(out["adam"]["us"] * (36.0 * n + n / 8.0) / (28.0 * n), 2)
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
        self.tokens = torch.from_numpy(synthetic.det_tokens("adamw_cost", (batch, 24), NUM_NOTES)).cuda()
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
        sys.exit("adamw_cost.py measures on the GPU; none found")
    wls = {"off": Workload(a.batch), "decay": Workload(a.batch, weight_decay=0.01), "ema": Workload(a.batch, ema_decay=0.999),
           "decay_ema": Workload(a.batch, weight_decay=0.01, ema_decay=0.999)}
    n = wls["off"].model.flat.numel()
    res = {"arena_floats": n, "arena_MB": round(4e-6 * n, 1),
           "kernels": kernels_alone(n, wls["decay"].trainer._decay_mask, a.rounds, a.iters), "batch": a.batch}
    for w in wls.values():
        w.run(5)
    ms = {k: [] for k in wls}
    for _ in range(a.rounds):
        for k, w in wls.items():
            ms[k].append(w.run(a.steps))
    for w in wls.values():
        w.trainer.finish()
    res["step_ms"] = {k: {"median": round(statistics.median(x), 4), "rounds": [round(y, 4) for y in x]} for k, x in ms.items()}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
