#!/usr/bin/env python3
"""Golden vectors of the decoder's temperature-sampled free-running decode.  TEST INFRASTRUCTURE.

Runs where oracle/gen_golden.py runs (the upstream reference importable behind its stub modules) and writes
tests/golden/decoder_sample.npz (arrays only).

The reference's HierarchicalDecoder (MeasureVAE/decoder.py:412-529) at the `small` configuration of tests/golden_util.CFGS, with
sampling = 'multinomial', teacher forcing off and dropout 0, decodes four latents in one call per temperature.  Its multinomial
branch (decoder.py:506-509) reads `F.softmax` and `torch.multinomial` through its module's names `F` and `torch`; inside this
process those two names are replaced by the project's sampling rule (csrc/sample.h) fed from stored uniforms:
    s = temperature * x in f32, e_v = expf(s_v - max s) in f32, inclusive prefix in f64, token = the first v with prefix_v > u * total
with u = uniforms[row, tick].  Everything else is the reference's own code: which logits reach the draw, that the drawn token is
embedded and fed into the next tick, and that it is the token `samples` reports.

Per temperature: the seed, the uniforms (RandomState(seed).random_sample((4, 24))), the reference's weights and tokens and the
per-tick distance of u from the nearest step of the CDF.  Seeds are searched until that distance is at least MIN_MARGIN on every
tick (the margin of arnn_generate.npz), so a restatement with other rounding picks the same tokens.

    python tools/gen_golden_decoder_sample.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import oracle.gen_golden as gg  # noqa: E402  (stubs music21 & co. and puts the reference on sys.path)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from inpaintnet_amd import synthetic  # noqa: E402
from tools.gen_golden_arnn_generate import save_npz  # noqa: E402

MIN_MARGIN = 2e-5
TEMPERATURES = (1.0, 1.5)
ROWS, T = 4, 24


class Names:
    """A module's namespace with some names replaced"""

    def __init__(self, base, **over):
        self._base, self._over = base, over

    def __getattr__(self, k):
        return self._over[k] if k in self._over else getattr(self._base, k)


class Rule:
    """Stands in for (F.softmax, torch.multinomial) of the reference's decoder module: the sampling rule on stored uniforms."""

    def __init__(self, temperature, uniforms):
        self.temperature, self.u, self.t, self.margins = np.float32(temperature), uniforms, 0, []

    def softmax(self, x, dim):
        assert dim == 1
        return x                                                 # the logits go on to `multinomial` as they are

    def multinomial(self, x, n):
        assert n == 1 and x.shape[0] == self.u.shape[0]
        out, mg = [], []
        for b, row in enumerate(x.numpy().astype(np.float32)):
            s = self.temperature * row                           # f32
            e = np.exp(s - s.max()).astype(np.float32)
            pre = np.cumsum(e.astype(np.float64))
            u = self.u[b, self.t]
            out.append(int(np.argmax(pre > u * pre[-1])))
            mg.append(np.abs(pre[:-1] / pre[-1] - u).min())
        self.t += 1
        self.margins.append(mg)
        return torch.tensor(out, dtype=torch.int64).view(-1, 1)


def main():
    c = gg.CFGS["small"]
    model = gg.build_vae(c, dropout=0.0)
    gg.load_det_weights(model)
    model.train()                                                # (train=False would force the argmax: decoder.py:435-436)
    dec = model.decoder
    dec.sampling = 'multinomial'
    dec.use_teacher_forcing = False
    z = torch.from_numpy(synthetic.det_normal("decoder_sample/z", (ROWS, c["Z"])))
    score = torch.zeros(ROWS, T, dtype=torch.int64)
    fx = {"z": z.numpy(), "temperatures": np.array(TEMPERATURES), "min_margin": np.array(MIN_MARGIN)}
    mod = gg.ref_decoder_mod
    real_F, real_torch = mod.F, mod.torch
    for ti, temp in enumerate(TEMPERATURES):
        for seed in range(1000 * (ti + 1), 1000 * (ti + 1) + 10000):
            u = np.random.RandomState(seed).random_sample((ROWS, T))
            rule = Rule(temp, u)
            mod.F, mod.torch = Names(real_F, softmax=rule.softmax), Names(real_torch, multinomial=rule.multinomial)
            try:
                with torch.no_grad():
                    w, s = dec(z, score, train=True)
            finally:
                mod.F, mod.torch = real_F, real_torch
            assert rule.t == T
            mg = np.array(rule.margins).T                        # [ROWS, T]
            if mg.min() >= MIN_MARGIN:
                break
        else:
            raise RuntimeError("no seed with a CDF margin >= %g" % MIN_MARGIN)
        key = f"t{ti}"
        fx[key + "/seed"] = np.array(seed)
        fx[key + "/uniforms"] = u
        fx[key + "/weights"] = w.numpy().astype(np.float32)
        fx[key + "/tokens"] = s.numpy()[:, 0].astype(np.int16)
        fx[key + "/margin"] = mg.astype(np.float32)
        print(f"{key}: T {temp} seed {seed} min margin {mg.min():.3g} tokens/row {[len(set(r)) for r in s.numpy()[:, 0]]}")
    path = os.path.join(gg.OUT, "decoder_sample.npz")
    save_npz(path, fx)
    print("wrote %s (%d arrays, %d bytes)" % (path, len(fx), os.path.getsize(path)))


if __name__ == "__main__":
    main()
