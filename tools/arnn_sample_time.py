#!/usr/bin/env python3
"""Times AnticipationRNN's temperature-sampled generation (ConstraintModelGaussianReg.generate) at the reference's shape
(L 384, V 48, H = U = 256) for R = 1, 2, 4, 8 independent rows, with device events after warm-up: the whole call (constraint
LSTMs, the 23-tick warm-up, the token pass, the synchronisation) and the sampling token pass alone (ops.arnn_sample on the
same inputs).  With --old-tree DIR it also times the argmax token pass (ops.arnn_generate, L 384) in child processes that
alternate between the inpaintnet_amd package (with its built library) under DIR -- e.g. the parent commit's -- and this tree's,
--rounds times each.

    python tools/arnn_sample_time.py [--iters 20] [--old-tree DIR] [--rounds 3]
"""
import argparse
import json
import os
import subprocess
import sys
import types

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

L, V, E, EM, H = 384, 48, 10, 2, 256


def _median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def _time(fn, iters, warm=3):
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return _median(out)


def _model():
    import torch
    from inpaintnet_amd import synthetic
    from inpaintnet_amd.arnn import ConstraintModelGaussianReg

    class Dataset(synthetic.SyntheticFolkDataset):
        def empty_score_tensor(self, length):
            return torch.zeros(self.num_voices, length, dtype=torch.long)

    ds = Dataset(num_notes=V)
    ds.metadatas = [types.SimpleNamespace(num_values=6), types.SimpleNamespace(num_values=6)]
    model = ConstraintModelGaussianReg(ds, note_embedding_dim=E, metadata_embedding_dim=EM, num_lstm_constraints_units=H,
                                       num_lstm_generation_units=H, linear_hidden_size=H, num_layers=2, dropout_input_prob=0.0,
                                       dropout_prob=0.0, unary_constraint=True, teacher_forcing=True)
    model.load_state_dict({k: torch.from_numpy(synthetic.det_param(k, tuple(v.shape))) for k, v in model.state_dict().items()})
    return model


def _weights(model):
    pr = model.param
    return [pr(k) for k in ("lstm_generation.0.weight_ih_l0", "lstm_generation.0.bias_ih_l0", "lstm_generation.0.weight_hh_l0",
                            "lstm_generation.0.bias_hh_l0", "lstm_generation.1.weight_ih_l0", "lstm_generation.1.bias_ih_l0",
                            "lstm_generation.1.weight_hh_l0", "lstm_generation.1.bias_hh_l0", "linear_1.weight", "linear_1.bias",
                            "linear_ouput_notes.0.weight", "linear_ouput_notes.0.bias")]


def sample_table(iters):
    import numpy as np
    import torch
    from inpaintnet_amd import ops, synthetic
    model = _model()
    emb = model.param("note_embeddings.0.weight")
    rows = []
    for R in (1, 2, 4, 8):
        s = torch.from_numpy(synthetic.folk_score(R, V, seed=R)).long().cuda()
        md = torch.from_numpy(synthetic.folk_metadata(R)).long().cuda()
        loc = torch.zeros_like(s)
        loc[:, :, :168] = 1
        loc[:, :, 216:] = 1
        np.random.seed(0)
        t_gen = _time(lambda: model.generate(s, md, loc, temperature=1.5), iters)
        oc = torch.randn(R, L, H, device="cuda") * 0.5
        u = torch.from_numpy(np.random.RandomState(1).random_sample((R, L))).cuda()
        hc = torch.zeros(R, 2, 2, H, device="cuda")
        t_pass = _time(lambda: ops.arnn_sample(emb, oc, *_weights(model), 1.5, u, hc_init=hc), iters)
        ops.check_chains("arnn_sample_time")
        rows.append({"R": R, "generate_ms": round(t_gen, 4), "sample_pass_ms": round(t_pass, 4),
                     "sample_pass_us_per_tick": round(1e3 * t_pass / L, 3)})
    return rows


def argmax_time(iters):
    import torch
    from inpaintnet_amd import ops
    model = _model()
    emb = model.param("note_embeddings.0.weight")
    oc = torch.randn(L, H, device="cuda") * 0.5
    t = _time(lambda: ops.arnn_generate(emb, oc, *_weights(model)), iters)
    ops.check_chains("arnn_sample_time")
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--old-tree", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--child-argmax", default=None, help=argparse.SUPPRESS)    # (the tree whose package a child imports)
    a = ap.parse_args()
    sys.path.insert(0, a.child_argmax or REPO)
    if a.child_argmax:
        print(json.dumps({"argmax_ms": argmax_time(a.iters)}))
        return
    out = {"L": L, "V": V, "H": H, "sample": sample_table(a.iters)}
    if a.old_tree:
        res = {"old": [], "new": []}
        for _ in range(a.rounds):
            for tag, tree in (("old", os.path.abspath(a.old_tree)), ("new", REPO)):
                env = {k: v for k, v in os.environ.items() if k != "INET_LIB_PATH"}
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-argmax", tree, "--iters", str(a.iters)],
                                   env=env, capture_output=True, text=True, timeout=300)
                if r.returncode != 0:
                    raise RuntimeError(f"argmax child ({tag}) failed with {r.returncode}: {r.stderr[-2000:]}")
                res[tag].append(json.loads(r.stdout.strip().splitlines()[-1])["argmax_ms"])
        out["argmax_pass_ms"] = {k: [round(x, 4) for x in v] for k, v in res.items()}
        out["argmax_pass_median_ms"] = {k: round(_median(v), 4) for k, v in res.items()}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
