#!/usr/bin/env python3
"""What the KL floor ("free bits") costs on the GPU:
    python tools/kl_fb_cost.py [--rows 4096] [--z 256] [--batch 256] [--steps 40] [--rounds 5] [--iters 20] [--kernels-only] [--out FILE.json]
1. The plain pair (ops.reparam_kl with a KL sum, ops.latent_bwd) and the floored forms of both modes alone at [rows, z], by HIP events
   around `iters` calls, the median of `rounds` rounds -- a call of a floored forward is its two launches.  For per-kernel device times
   run this part under a kernel trace of its own (--kernels-only keeps the trace to these launches).
2. The bench's MeasureVAE training step (every step from the seeded weights, as bench.py's) at --batch for the default trainer and for
   free_nats > 0 in both modes, in ONE process, alternating within every round; the median over rounds of the time per step (host
   clock around `steps` steps between two synchronisations).
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


def kernels_alone(rows, Z, rounds, iters):
    dev = "cuda:0"
    mu = torch.from_numpy(0.3 * synthetic.det_normal("kl_fb_cost/mu", (rows, Z))).to(dev)
    ls = torch.from_numpy(-0.5 + 0.3 * synthetic.det_normal("kl_fb_cost/ls", (rows, Z))).to(dev)
    eps = torch.from_numpy(synthetic.det_normal("kl_fb_cost/eps", (rows, Z))).to(dev)
    dz = torch.from_numpy(synthetic.det_normal("kl_fb_cost/dz", (rows, Z))).to(dev)
    acc = torch.zeros(2, device=dev)
    kdev = torch.ones(1, device=dev)
    n = rows * Z
    lam = {"measure": 69.0, "dim": 0.27}                                         # about half of the parts are kept
    keep = {per: ops.reparam_kl_fb(mu, ls, eps, lam[per], per)[2] for per in lam}
    jobs = {"reparam_kl": (lambda: ops.reparam_kl(mu, ls, eps, kl_sum=acc[0:1]), 16.0 * n),
            "latent_bwd": (lambda: ops.latent_bwd(dz, mu, ls, eps, 1e-3, kscale_dev=kdev), 24.0 * n)}
    for per in lam:
        jobs[f"reparam_kl_fb[{per}]"] = (lambda per=per: ops.reparam_kl_fb(mu, ls, eps, lam[per], per, kl_sum=acc[0:1], kl_raw=acc[1:2]),
                                         16.0 * n)
        jobs[f"latent_bwd_fb[{per}]"] = (lambda per=per: ops.latent_bwd_fb(dz, mu, ls, eps, 1e-3, keep[per], per, kscale_dev=kdev),
                                         24.0 * n)
    out = {"kept": {per: int(keep[per].sum()) for per in lam}}
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
        out[name] = {"us_per_call": round(med, 2), "us_rounds": [round(x, 2) for x in us], "GB_per_s": round(nbytes / med / 1e3, 1)}
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
        self.tokens = torch.from_numpy(synthetic.det_tokens("kl_fb_cost", (batch, 24), NUM_NOTES)).cuda()
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
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--z", type=int, default=256)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("kl_fb_cost.py measures on the GPU; none found")
    res = {"rows": a.rows, "z": a.z, "kernels": kernels_alone(a.rows, a.z, a.rounds, a.iters)}
    if not a.kernels_only:
        wls = {"default": Workload(a.batch), "measure": Workload(a.batch, kl_warmup_steps=1000, free_nats=48.0),
               "dim": Workload(a.batch, kl_warmup_steps=1000, free_nats=0.2, free_nats_per="dim")}
        for w in wls.values():
            w.run(5)
        ms = {k: [] for k in wls}
        for _ in range(a.rounds):
            for k, w in wls.items():
                ms[k].append(w.run(a.steps))
        for w in wls.values():
            w.trainer.finish()
        res["batch"] = a.batch
        res["step_ms"] = {k: {"median": round(statistics.median(x), 4), "rounds": [round(y, 4) for y in x]} for k, x in ms.items()}
        res["kept_last_step"] = {k: int(w.trainer.last_kl["keep"].sum()) for k, w in wls.items() if w.trainer.last_kl is not None}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
