"""Helpers shared by the oracle and GPU parity tests."""
import os

import numpy as np
import torch

from inpaintnet_amd import layout, synthetic

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

CFGS = {
    "small": dict(V=12, E=4, H=16, Z=8),
    "mid": dict(V=20, E=6, H=48, Z=24),
    "full": dict(V=48, E=10, H=512, Z=256),
    # no fixture: H % 256 == 0 turns on the fragment-major operand path of the step kernels; used against the oracle
    "pk": dict(V=20, E=6, H=256, Z=24),
    # no fixture: a vocabulary / embedding wider than the token-sum kernels take (V > 64, E > 16): one-hot GEMM path
    "wide": dict(V=70, E=20, H=48, Z=24),
    # no fixture: vocabularies that are not a multiple of 16 (the real one is data-derived: MeasureVAE/measure_vae.py:56) on the
    # fragment-major path: the fused decode kernel pads its last 16-column block, the token segment-sum takes up to 128 rows
    "v61": dict(V=61, E=10, H=256, Z=24),
    "v93": dict(V=93, E=10, H=256, Z=24),
    # no fixture: beyond every fast path's limit (V > 128): per-tick decode, one-hot products for the embedding gradients
    "v140": dict(V=140, E=10, H=256, Z=24),
}


def load(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def vae_params(name, fx=None, prefix=""):
    """state_dict-keyed float32 torch tensors for the fixture's model (regenerated
    from the deterministic generator; cross-checked against stored copies when present)."""
    c = CFGS[name]
    shapes = layout.vae_param_shapes(c["V"], c["E"], c["H"], c["Z"], c["H"], prefix=prefix)
    P = {k: torch.from_numpy(synthetic.det_param(k, s)) for k, s in shapes.items()}
    if fx is not None:
        for k in P:
            key = "param/" + k
            if key in fx.files:
                assert np.array_equal(fx[key], P[k].numpy()), k
    return P


def latent_params(name, auto_reg):
    c = CFGS[name]
    P = vae_params(name, prefix="vae_model.")
    shapes = layout.latent_param_shapes(c["Z"], c["H"], auto_reg)
    for k, s in shapes.items():
        P[k] = torch.from_numpy(synthetic.det_param(k, s))
    return P


def unique_rows(margin, tol=1e-4):
    return margin > tol


def rel_err(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))

ARNN_CFGS = {
    "small": dict(V=12, E=4, Em=2, H=16, LH=16),
    "full": dict(V=48, E=10, Em=2, H=256, LH=256),
}


def arnn_params(name, fx=None):
    c = ARNN_CFGS[name]
    shapes = layout.arnn_param_shapes(c["V"], c["E"], c["Em"], c["H"], c["LH"])
    P = {k: torch.from_numpy(synthetic.det_param(k, s)) for k, s in shapes.items()}
    if fx is not None:
        assert list(fx["param_keys"]) == list(shapes)
        for k, shp in zip(fx["param_keys"], fx["param_shapes"]):
            assert tuple(int(d) for d in str(shp).split(",")) == tuple(shapes[str(k)]), k
        for k in P:
            if "param/" + k in fx.files:
                assert np.array_equal(fx["param/" + k], P[k].numpy()), k
    return P


def latent_params_from_fixture(fx, prefix="param/"):
    """state_dict of a fixture that stores its full weights (small configs)."""
    return {k[len(prefix):]: torch.from_numpy(fx[k]) for k in fx.files if k.startswith(prefix)}


def is_chain(label, kind, nprob, T, B, H=512):
    """A chain-kernel profile label of either generation: 'gru_chain_fwd ms4 np2 T24 B256 H512' (first: csrc/gru_chain.hip; 'ms4x2'
    = the build for two launches per CU) or 'gru_chain_fwd v2w4 p9 np2 T24 B256 H512' (second: csrc/gru_chain2.hip, waves per
    workgroup and piece products)."""
    return label.startswith(f"gru_chain_{kind} ") and label.endswith(f" np{nprob} T{T} B{B} H{H}")


# ----------------------------------------------------------------------------------------------------------------------
# *_drop fixtures: the reference in train() with dropout on, every mask it drew recorded in its own call order
# (oracle/gen_golden.py, MaskRecorder).  A recorded mask is in the REFERENCE's memory order: (T, B, D*H) time-major for a GRU
# (also for batch_first modules), (B, L, 1) for the AnticipationRNN's Dropout2d.
# ----------------------------------------------------------------------------------------------------------------------
def arnn_params_drop(name, fx):
    """arnn_params with the embedding tables at nn.Embedding's own N(0, 1) scale (what the reference keeps for this model and
    what arnn_*_drop.npz was captured with); checked against the copies the fixture stores."""
    P = arnn_params(name)
    for k in P:
        if "embeddings" in k:
            P[k] = P[k] * float(np.sqrt((P[k].shape[0] + P[k].shape[1]) / 2.0))
    stored = [k for k in P if "param/" + k in fx.files]
    assert any("embeddings" in k for k in stored)
    for k in stored:
        assert np.array_equal(fx["param/" + k], P[k].numpy()), k
    return P


def recorded_masks(fx, prefix=""):
    """-> [(tag, mask, p)] in the reference's call order; mask float32 with values {0, 1/(1-p)}."""
    tags, shapes, ps = fx[prefix + "mask_tags"], fx[prefix + "mask_shapes"], fx[prefix + "mask_p"]
    sizes = [int(np.prod(s)) for s in shapes]
    bits = fx[prefix + "mask_bits"]
    assert bits.size == (sum(sizes) + 7) // 8
    keep = np.unpackbits(bits)[:sum(sizes)]
    out, at = [], 0
    for tag, shape, p, n in zip(tags, shapes, ps, sizes):
        k = torch.from_numpy(keep[at:at + n].reshape(tuple(int(d) for d in shape)).astype(np.float32))
        out.append((str(tag), k / (1.0 - float(p)), float(p)))
        at += n
    return out


def vae_step_masks(fx, mode, step):
    """The 26 masks of one MeasureVAE training pass: {'enc': (T, B, 2H), 'beat': (4, B, H), 'tick': (24, B, H)}, time-major as
    drawn (the 24 single-tick calls' (1, B, H) masks stacked in call order)."""
    pre = f"step_{mode}_"
    rec = [m for m, s in zip(recorded_masks(fx, pre), fx[pre + "mask_step"]) if int(s) == step]
    assert [t for t, _, _ in rec] == ["encoder.lstm", "decoder.rnn_beat"] + ["decoder.rnn_tick"] * 24
    return {"enc": rec[0][1], "beat": rec[1][1], "tick": torch.cat([m for _, m, _ in rec[2:]], 0), "p": rec[0][2]}


# Mutations: each takes a recorded mask (reference layout) and returns what a restatement that gets ONE thing wrong would use.
def mut_omit(m, p):
    return torch.ones_like(m)


def mut_unscaled(m, p):
    return m * (1.0 - p)


def mut_batch_major(m, p):
    """The same draw read as if it had been made in (B, T, F) order."""
    T, B, F = m.shape
    assert T > 1 and B > 1
    return m.reshape(B, T, F).transpose(0, 1).contiguous()


def mut_shift(m, p):
    """Step t gets the mask of step t + 1."""
    return torch.roll(m, -1, 0)


# one mask of a vae_step_masks dict wrong at a time (the CPU oracle and the HIP kernels are both put through these)
def _swap_beat_tick(sm):
    """The beat mask and the masks of the first four ticks change places (both (4, B, H))."""
    out = dict(sm)
    out["beat"], out["tick"] = sm["tick"][:4].clone(), torch.cat((sm["beat"], sm["tick"][4:]), 0)
    return out


VAE_MASK_MUTATIONS = {
    "enc omitted": lambda sm: dict(sm, enc=mut_omit(sm["enc"], sm["p"])),
    "enc batch-major": lambda sm: dict(sm, enc=mut_batch_major(sm["enc"], sm["p"])),
    "enc unscaled": lambda sm: dict(sm, enc=mut_unscaled(sm["enc"], sm["p"])),
    "beat omitted": lambda sm: dict(sm, beat=mut_omit(sm["beat"], sm["p"])),
    "beat batch-major": lambda sm: dict(sm, beat=mut_batch_major(sm["beat"], sm["p"])),
    "beat unscaled": lambda sm: dict(sm, beat=mut_unscaled(sm["beat"], sm["p"])),
    "tick omitted": lambda sm: dict(sm, tick=mut_omit(sm["tick"], sm["p"])),
    # all 24 single-tick draws read as one (B, 24, H) draw
    "tick batch-major": lambda sm: dict(sm, tick=mut_batch_major(sm["tick"], sm["p"])),
    "tick unscaled": lambda sm: dict(sm, tick=mut_unscaled(sm["tick"], sm["p"])),
    "tick shifted by one": lambda sm: dict(sm, tick=mut_shift(sm["tick"], sm["p"])),
    "beat and tick swapped": _swap_beat_tick,
}


def oracle_vae_masks(sm):
    """vae_step_masks -> what oracle.torch_ref.vae_forward takes (batch-first views)."""
    return {k: sm[k].permute(1, 0, 2) for k in ("enc", "beat", "tick")}


def latent_mask_groups(fx, auto_reg, tf, B, n_past, n_target, n_future):
    """The recorded masks of one LatentRNN pass, grouped by role, each still time-major as drawn:
    enc_past / enc_future / enc_target (24, B*n, 2H) rows ordered (sequence, measure); ctx_past / ctx_future (n, B, 2H);
    gen: (nt, B, 4H), or a list of nt (1, B, 4H) on the free-running auto-regressive path; dec: list of nt {'beat' (4, B, H),
    'tick' (24, B, H)}; enc_ar: list of nt (24, B, 2H) (free-running auto-regressive path only)."""
    rec = recorded_masks(fx)
    tags = [t for t, _, _ in rec]
    ms = [m for _, m, _ in rec]
    dec_tags = ["vae_model.decoder.rnn_beat"] + ["vae_model.decoder.rnn_tick"] * 24
    free_ar = auto_reg and not tf
    per = 1 + 25 + 1 if free_ar else 25
    head = 5 if free_ar else 6
    assert tags[:5] == ["vae_model.encoder.lstm"] * 3 + ["context_rnn_past", "context_rnn_future"]
    assert len(rec) == head + per * n_target
    g = {"enc_past": ms[0], "enc_future": ms[1], "enc_target": ms[2], "ctx_past": ms[3], "ctx_future": ms[4],
         "dec": [], "p": rec[0][2]}
    if free_ar:
        g["gen"], g["enc_ar"] = [], []
    else:
        assert tags[5] == "generation_rnn"
        g["gen"] = ms[5]
    for i in range(n_target):
        at = head + per * i
        if free_ar:
            assert tags[at] == "generation_rnn" and tags[at + 26] == "vae_model.encoder.lstm"
            g["gen"].append(ms[at])
            g["enc_ar"].append(ms[at + 26])
            at += 1
        assert tags[at:at + 25] == dec_tags
        g["dec"].append({"beat": ms[at], "tick": torch.cat(ms[at + 1:at + 25], 0)})
    assert g["enc_past"].shape[1] == B * n_past and g["enc_future"].shape[1] == B * n_future
    assert g["enc_target"].shape[1] == B * n_target
    return g


def oracle_latent_masks(g):
    """latent_mask_groups -> what oracle.torch_ref.latent_forward takes (batch-first views)."""
    def bf(m):
        return [bf(x) for x in m] if isinstance(m, list) else m.permute(1, 0, 2)
    out = {k: bf(g[k]) for k in ("enc_past", "enc_future", "enc_target", "ctx_past", "ctx_future", "gen")}
    out["dec"] = [{"beat": bf(d["beat"]), "tick": bf(d["tick"])} for d in g["dec"]]
    if "enc_ar" in g:
        out["enc_ar"] = bf(g["enc_ar"])
    return out


def comparable_ticks(samples, ref_samples, margin, tol=1e-3):
    """How far a free-running pass can be held against the fixture, per sequence: samples, ref_samples (B, 1, n) tokens, margin (B, n)
    top-2 margin of the reference's logits.  A free-running pass feeds each sampled token back (into the next tick, and through the
    re-encoding into the next measure), so behind a token that differs nothing of that sequence is comparable -- but a token may only
    differ where the reference's own top two logits are closer than `tol` (the unique_rows floor): the FIRST differing tick of every
    sequence is asserted to be such a row, so a misplaced mask, which moves the logits by far more, cannot excuse itself this way.
    -> int array (B,): number of leading ticks whose logits are comparable (n where all tokens agree; else first differing tick + 1:
    the logits of that tick itself were computed from agreeing tokens)."""
    got, ref = np.asarray(samples)[:, 0], np.asarray(ref_samples)[:, 0]
    margin = np.asarray(margin).reshape(got.shape)
    upto = np.full(got.shape[0], got.shape[1], dtype=np.int64)
    for b in range(got.shape[0]):
        diff = np.nonzero(got[b] != ref[b])[0]
        if diff.size:
            t = int(diff[0])
            assert margin[b, t] <= tol, (f"sequence {b}: first token difference at tick {t}, where the reference's top-2 margin is "
                                         f"{margin[b, t]:.3g} > {tol}: not a near-tie, the pass itself is off")
            upto[b] = t + 1
    return upto


def prefix_errors(upto, weights, ref_weights, gen_z, ref_gen_z, ticks_per_measure=24):
    """Errors over the comparable prefix of every sequence (comparable_ticks), relative to the fixture tensors' maxima: logits of
    the first upto[b] ticks; generated latents of every measure that starts inside them (a measure's z is formed before its first
    tick is decoded)."""
    w, rw = np.asarray(weights, dtype=np.float64), np.asarray(ref_weights, dtype=np.float64)
    z, rz = np.asarray(gen_z, dtype=np.float64), np.asarray(ref_gen_z, dtype=np.float64)
    B, V = w.shape[0], w.shape[-1]
    w, rw = w.reshape(B, -1, V), rw.reshape(B, -1, V)
    ew = ez = 0.0
    for b in range(B):
        n = int(upto[b])
        nm = (n + ticks_per_measure - 1) // ticks_per_measure
        ew = max(ew, float(np.abs(w[b, :n] - rw[b, :n]).max()))
        ez = max(ez, float(np.abs(z[b, :nm] - rz[b, :nm]).max()))
    return ew / (np.abs(rw).max() + 1e-30), ez / (np.abs(rz).max() + 1e-30)
