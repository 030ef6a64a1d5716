#!/usr/bin/env python3
"""Golden vectors of AnticipationRNN's temperature-sampled generation and of its tester.  TEST INFRASTRUCTURE.

Runs where oracle/gen_golden.py runs (the upstream reference importable behind its stub modules) and writes
tests/golden/arnn_generate.npz:

  * ConstraintModelGaussianReg.generate (AnticipationRNN/anticipation_rnn_gauss_reg_model.py:570-679), B = 1, for the
    small (V 12, H 16) and the full (V 48, H 256) configuration at temperatures 1.0 and 1.5, on four synthetic chorales
    with four constraint windows.  Per call: the numpy seed, the L uniforms that np.random.choice draws from
    RandomState(seed) (one random_sample() double per tick, nothing else), the reference's tokens and the per-tick
    distance between the uniform and the nearest step of the CDF.  Seeds are searched until that distance is at least
    MIN_MARGIN on every tick, so a restatement with other rounding of the softmax picks the same tokens.
  * AnticipationRNNTester (anticipation_rnn_tester.py) on the model of arnn_inpaint_small.npz: get_constraints_location
    (the default and the stochastic branch under torch.manual_seed), mean_crossentropy_loss / mean_accuracy on stored
    weights and targets, and loss_and_acc_test over a two-batch loader.

The full configuration's weights are stored as keys and shapes only; tests regenerate them with synthetic.det_param.

    python tools/gen_golden_arnn_generate.py
"""
import contextlib
import io
import os
import sys
import zipfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import oracle.gen_golden as gg  # noqa: E402  (stubs music21 & co. and puts the reference on sys.path)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from AnticipationRNN.anticipation_rnn_gauss_reg_model import AnticipationRNNBaseline, ConstraintModelGaussianReg  # noqa: E402
import AnticipationRNN.anticipation_rnn_gauss_reg_model as ref_arnn_mod  # noqa: E402
from AnticipationRNN.anticipation_rnn_tester import AnticipationRNNTester  # noqa: E402
from inpaintnet_amd import synthetic  # noqa: E402

L = 384
MIN_MARGIN = 2e-5
TEMPERATURES = (1.0, 1.5)
# (start_tick, end_tick) of the unconstrained window of each of the four chorales
WINDOWS = ((7 * 24, 9 * 24), (3 * 24, 8 * 24), (0, 2 * 24), (12 * 24, 16 * 24))


class GenDataset(gg.FakeDataset):
    def tensor_to_score(self, tensor):
        return None


def build(cls, c, ds):
    m = cls(ds, note_embedding_dim=c["E"], metadata_embedding_dim=c["Em"], num_lstm_constraints_units=c["H"],
            num_lstm_generation_units=c["H"], linear_hidden_size=c["LH"], num_layers=2, dropout_input_prob=0.0,
            dropout_prob=0.0, unary_constraint=True, teacher_forcing=True)
    gg.load_det_weights(m)
    m.eval()
    return m


def inputs(V, n):
    score = torch.from_numpy(synthetic.folk_score(n, V, seed=23)).long()
    md = torch.from_numpy(synthetic.folk_metadata(n)).long()
    md[..., 0] = torch.from_numpy(synthetic.det_tokens("arnn_generate/md0", (n, 1, L), 6))
    loc = torch.zeros_like(score)
    for i, (a, b) in enumerate(WINDOWS[:n]):
        loc[i, :, :a] = 1
        loc[i, :, b:] = 1
    return score, md, loc


class ChoiceRecorder:
    """Wraps np.random.choice inside the reference module: records the probabilities of every draw."""

    def __init__(self):
        self.ps = []
        self.orig = np.random.choice

    def __enter__(self):
        def choice(a, p=None, **kw):
            self.ps.append(np.asarray(p, dtype=np.float64).copy())
            return self.orig(a, p=p, **kw)
        ref_arnn_mod.np.random.choice = choice
        return self

    def __exit__(self, *a):
        ref_arnn_mod.np.random.choice = self.orig


def margins(ps, u):
    """per tick: distance of the uniform from the nearest CDF step (np.random.choice: cdf = cumsum(p) / sum, searchsorted right)"""
    out = np.empty(len(ps))
    for t, p in enumerate(ps):
        cdf = np.cumsum(p)
        cdf /= cdf[-1]
        out[t] = np.abs(cdf[:-1] - u[t]).min() if len(cdf) > 1 else 1.0
    return out


def gen_call(model, score, md, loc, temperature, seed0):
    for seed in range(seed0, seed0 + 10000):
        np.random.seed(seed)
        with ChoiceRecorder() as rec, contextlib.redirect_stdout(io.StringIO()), torch.no_grad():
            _, gen, _ = model.generate(tensor_score=score, tensor_metadata=md, constraints_location=loc, temperature=temperature)
        assert len(rec.ps) == L
        u = np.random.RandomState(seed).random_sample(L + 1)
        tok = gen[0].numpy().astype(np.int64)
        restated = np.array([np.searchsorted(np.cumsum(p) / np.cumsum(p)[-1], u[t], side="right") for t, p in enumerate(rec.ps)])
        assert np.array_equal(restated, tok), "one random_sample() double per tick no longer explains np.random.choice"
        assert np.random.random_sample() == u[L]                 # nothing else drew from numpy's global stream
        mg = margins(rec.ps, u[:L])
        if mg.min() >= MIN_MARGIN:
            return seed, u[:L], tok, mg
    raise RuntimeError("no seed with a CDF margin >= %g" % MIN_MARGIN)


def gen_generate(fx):
    for name in ("small", "full"):
        c = gg.ARNN_CFGS[name]
        ds = GenDataset(c["V"])
        model = build(ConstraintModelGaussianReg, c, ds)
        fx[f"{name}/param_keys"] = np.array(list(model.state_dict().keys()))
        fx[f"{name}/param_shapes"] = np.array([",".join(str(d) for d in v.shape) for v in model.state_dict().values()])
        score, md, loc = inputs(c["V"], len(WINDOWS))
        fx[f"{name}/score"] = score.numpy().astype(np.int16)
        fx[f"{name}/metadata"] = md.numpy().astype(np.int16)
        fx[f"{name}/constraints_loc"] = loc.numpy().astype(np.int8)
        for ti, temp in enumerate(TEMPERATURES):
            for i in range(len(WINDOWS)):
                seed, u, tok, mg = gen_call(model, score[i], md[i], loc[i], temp, 1000 * (ti + 1) + 100 * i)
                key = f"{name}/t{ti}/{i}"
                fx[key + "/seed"] = np.array(seed)
                fx[key + "/uniforms"] = u
                fx[key + "/tokens"] = tok.astype(np.int16)
                fx[key + "/margin"] = mg.astype(np.float32)
                print(f"{key}: T {temp} seed {seed} min margin {mg.min():.3g}")
    fx["temperatures"] = np.array(TEMPERATURES)
    fx["windows"] = np.array(WINDOWS)
    fx["min_margin"] = np.array(MIN_MARGIN)


def gen_tester(fx):
    c = gg.ARNN_CFGS["small"]
    ds = GenDataset(c["V"])
    model = build(AnticipationRNNBaseline, c, ds)
    tester = AnticipationRNNTester(ds, model)
    score = torch.from_numpy(synthetic.folk_score(3, c["V"], seed=11)).long()
    torch.manual_seed(7)
    loc, a, b = tester.get_constraints_location(score, is_stochastic=False)
    fx["tester/default_loc"], fx["tester/default_ticks"] = loc.numpy().astype(np.int8), np.array([a, b])
    loc, a, b = tester.get_constraints_location(score, is_stochastic=False, start_measure=3, num_measures=4)
    fx["tester/given_loc"], fx["tester/given_ticks"] = loc.numpy().astype(np.int8), np.array([a, b])
    stoch = []
    torch.manual_seed(5)
    for _ in range(4):
        loc, a, b = tester.get_constraints_location(score, is_stochastic=True)
        stoch.append([a, b])
        fx[f"tester/stochastic_loc{len(stoch) - 1}"] = loc.numpy().astype(np.int8)
    fx["tester/stochastic_seed"], fx["tester/stochastic_ticks"] = np.array(5), np.array(stoch)
    # the static loss / accuracy on stored weights and targets
    g = torch.Generator().manual_seed(3)
    w = [torch.randn(3, 48, c["V"], generator=g)]
    t = torch.randint(0, c["V"], (1, 3, 48), generator=g)
    fx["tester/w"], fx["tester/t"] = w[0].numpy(), t.numpy()
    fx["tester/ce_acc"] = np.array([AnticipationRNNTester.mean_crossentropy_loss(w, t).item(),
                                    AnticipationRNNTester.mean_accuracy(w, t).item()], dtype=np.float64)
    # loss_and_acc_test over two batches (the tester's default window: measures 8 and 9)
    batches = []
    for k in range(2):
        s = torch.from_numpy(synthetic.folk_score(3, c["V"], seed=40 + k)).long()
        m = torch.from_numpy(synthetic.folk_metadata(3)).long()
        m[..., 0] = torch.from_numpy(synthetic.det_tokens(f"arnn_generate/tester_md{k}", (3, 1, L), 6))
        batches.append((s, m))
        fx[f"tester/batch{k}_score"], fx[f"tester/batch{k}_metadata"] = s.numpy().astype(np.int16), m.numpy().astype(np.int16)
    with contextlib.redirect_stderr(io.StringIO()), torch.no_grad():
        lo, ac = tester.loss_and_acc_test(batches)
    fx["tester/loss_acc"] = np.array([float(lo), float(ac)], dtype=np.float64)
    print("tester: loss %.6f acc %.6f" % (float(lo), float(ac)))


def save_npz(path, fx):
    """np.savez_compressed with a fixed timestamp on every member: the file is a function of its arrays alone."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for k, v in fx.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(v), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def main():
    fx = {}
    gen_generate(fx)
    gen_tester(fx)
    path = os.path.join(gg.OUT, "arnn_generate.npz")
    save_npz(path, fx)
    print("wrote %s (%d arrays, %d bytes)" % (path, len(fx), os.path.getsize(path)))


if __name__ == "__main__":
    main()
