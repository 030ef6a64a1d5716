#!/usr/bin/env python3
"""What the attribute regularisation costs on the GPU:
    python tools/attr_cost.py [--shapes 256x256,4096x256] [--batch 256] [--steps 40] [--rounds 5] [--iters 20] [--kernels-only] [--out FILE.json]
1. ops.measure_attributes alone (one launch) and ops.attr_reg alone (its pair and finish launches) at every (B, Z) of --shapes, with 1
   and 4 attributes, with and without the gradient, by HIP events around `iters` calls, the median of `rounds` rounds.
2. The bench's MeasureVAE training step (every step from the seeded weights, as bench.py's) at --batch for the default trainer and for
   attr_reg on all four attributes, in ONE process, alternating within every round; the median over rounds of the time per step
   (host clock around `steps` steps between two synchronisations).
Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from inpaintnet_amd import ops, synthetic                       # noqa: E402
from inpaintnet_amd.attributes import ATTRIBUTES, AttributeSpec  # noqa: E402
from inpaintnet_amd.measure_vae import MeasureVAE               # noqa: E402
from inpaintnet_amd.vae_trainer import VAETrainer               # noqa: E402

NUM_NOTES = 48


def spec():
    """The synthetic vocabulary read as: 0 the slur, 1 the rest, 2 None, 3 and 4 START / END, then 43 pitches from G3 up."""
    midi = np.full(NUM_NOTES, -1, np.int64)
    midi[5:] = 55 + np.arange(NUM_NOTES - 5) % 30
    return AttributeSpec(NUM_NOTES, 0, 1, 2, midi)


def timed(fn, rounds, iters):
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


def kernels_alone(B, Z, rounds, iters):
    dev = "cuda:0"
    z = torch.from_numpy(0.5 * synthetic.det_normal("attr_cost/z", (B, Z))).float().to(dev)
    tokens = torch.from_numpy(synthetic.det_tokens("attr_cost/tok", (B, 24), NUM_NOTES)).to(dev)
    sp = spec()
    out = {"measure_attrs": timed(lambda: ops.measure_attributes(tokens, sp), rounds, iters)}
    attrs4 = ops.measure_attributes(tokens, sp)
    for A in (1, 4):
        attrs = attrs4[:, :A].contiguous()
        dims = [0, Z - 1, 1, Z // 2][:A]
        for want_grad in (False, True):
            r = timed(lambda: ops.attr_reg(z, dims, attrs, 10.0, 10.0, want_grad=want_grad), rounds, iters)
            r["Mtanh_per_s"] = round(B * B * A / r["us_per_call"], 1)           # the work: one tanh per pair and attribute
            out[f"attr_reg A={A}{'+grad' if want_grad else ''}"] = r
    o, c, _ = ops.attr_reg(z, [0, Z - 1, 1, Z // 2], attrs4, 10.0, 10.0)
    out["value"], out["counts"] = float(o[0]), c.tolist()
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
        self.tokens = torch.from_numpy(synthetic.det_tokens("attr_cost", (batch, 24), NUM_NOTES)).cuda()
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
        sys.exit("attr_cost.py measures on the GPU; none found")
    res = {"kernels": {}}
    for shape in a.shapes.split(","):
        B, Z = (int(v) for v in shape.split("x"))
        res["kernels"][shape] = kernels_alone(B, Z, a.rounds, a.iters)
    if not a.kernels_only:
        reg = {name: d for name, d in zip(ATTRIBUTES, (0, 1, 2, 3))}
        wls = {"default": Workload(a.batch), "attr_reg": Workload(a.batch, attr_reg=reg, attr_spec=spec())}
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
        last = wls["attr_reg"].trainer.last_attr_reg
        res["last_attr_reg"] = {"value": float(last["value"]), "per_attr": last["per_attr"].tolist(), "counts": last["counts"].tolist()}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
