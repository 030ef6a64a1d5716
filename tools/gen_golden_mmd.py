#!/usr/bin/env python3
"""Golden vectors of the reference's MMD latent loss.  TEST INFRASTRUCTURE.

Runs where oracle/gen_golden.py runs (the upstream reference importable behind its stub modules) and writes
tests/golden/mmd_reference.npz: for (B, Z) in CASES the inputs z_tilde and z_prior (float32, from synthetic.det_normal: x = 0.6 n + 0.2,
y = n), and what the reference's own VAETrainer.compute_mmd_loss(z_tilde, z_prior, coeff=10) (MeasureVAE/vae_trainer.py:93-126: the
Gaussian kernel, var = 16) returns on them in float64, with d value / d z_tilde from torch autograd in float64.

    python tools/gen_golden_mmd.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import oracle.gen_golden as gg  # noqa: E402  (stubs music21 & co. and puts the reference on sys.path)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from MeasureVAE.vae_trainer import VAETrainer  # noqa: E402
from inpaintnet_amd import synthetic  # noqa: E402
from tools.gen_golden_arnn_generate import save_npz  # noqa: E402

CASES = ((1, 5), (2, 5), (37, 16), (16, 256))
COEFF = 10


def inputs(B, Z):
    tag = f"mmd/{B}x{Z}"
    x = (0.6 * synthetic.det_normal(tag + "/x", (B, Z)) + 0.2).astype(np.float32)
    y = synthetic.det_normal(tag + "/y", (B, Z)).astype(np.float32)
    return x, y


def main():
    fx = {"cases": np.array(CASES), "coeff": np.array(COEFF)}
    for B, Z in CASES:
        x, y = inputs(B, Z)
        zt = torch.from_numpy(x).double().requires_grad_(True)
        value = VAETrainer.compute_mmd_loss(zt, torch.from_numpy(y).double(), coeff=COEFF)
        value.backward()
        key = f"{B}x{Z}"
        fx[key + "/z_tilde"], fx[key + "/z_prior"] = x, y
        fx[key + "/value"] = np.array(float(value.detach()), dtype=np.float64)
        fx[key + "/grad"] = zt.grad.numpy().astype(np.float64)
        print(f"{key}: value {float(value.detach()):.12g} max |grad| {float(zt.grad.abs().max()):.6g}")
    path = os.path.join(gg.OUT, "mmd_reference.npz")
    save_npz(path, fx)
    print("wrote %s (%d arrays, %d bytes)" % (path, len(fx), os.path.getsize(path)))


if __name__ == "__main__":
    main()
