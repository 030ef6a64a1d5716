"""The recorded launches of the decoder calls: the cases, one per route of csrc/vae.hip's dec_route, that
tools/record_decoder_launches.py writes into tests/golden/decoder_launches.json and tests/test_gpu_decoder_launches.py holds the
library to.

Per case the fixture holds the ordered launch labels (ops.prof_enable / ops.prof_dump) of the forward call -- and of the backward call
where the case has one -- next to the SHA-256 of the returned weights and samples as bytes.  Gradients are not digested: they stay with
the parity tests.  Nothing here imports the library at module level: the callers hand in the `ops` module they want exercised; the
inputs are synthetic.det_* values, which depend on their key alone.  Unless a case says otherwise the decoder is the full one
(H = 512, Z = 256, 4 x 6 ticks)."""
import csv
import functools
import hashlib
import json
import os
import tempfile

import numpy as np
import torch

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decoder_launches.json")
T = 24

# name -> the call.  tf: teacher-forced; save: with backward saves, followed by decoder_bwd; masks: "beat" / "both"; chains: option 4;
# calls: the (teacher_forced,) calls of a case that makes more than one
CASES = (
    ("01 B1 inference", dict(B=1)),
    ("02 B4 Z128 inference", dict(B=4, Z=128)),
    ("03 B2 beat mask inference", dict(B=2, masks="beat")),
    ("04 B17 inference", dict(B=17)),
    ("05 B768 inference", dict(B=768)),
    ("06 B17 chains off", dict(B=17, chains=0)),
    ("07 B17 V50 chains off", dict(B=17, V=50, chains=0)),
    ("08 B17 multinomial", dict(B=17, seed=5)),
    ("09 B17 temperature top_p", dict(B=17, temperature=6.0, top_p=0.9)),
    ("10 H64 B3 free and teacher-forced", dict(B=3, H=64, calls=(False, True))),
    ("11 B32 teacher-forced train", dict(B=32, tf=True, save=True, masks="both")),
    ("12 B256 teacher-forced train", dict(B=256, tf=True, save=True, masks="both")),
    ("13 B32 free-running train", dict(B=32, save=True, masks="both")),
    ("14 B1024 teacher-forced train", dict(B=1024, tf=True, save=True)),
    ("15 B32 teacher-forced train chains off", dict(B=32, tf=True, save=True, chains=0)),
    # (recorded from the revision in front of the sync-area ledger, DESIGN.md section 24: the odd-chunk form of case 05 in training)
    ("16 B768 free-running train", dict(B=768, save=True, masks="both")),
)


@functools.lru_cache(maxsize=None)
def _decoder(ops, synthetic, V, Z, H):
    """(cfg, flat device params) of a decoder; the full one through tests/test_gpu_decode_plans.py's helper"""
    if H == 512:
        from tests.test_gpu_decode_plans import decoder
        cfg, _, params = decoder(V, Z)
        return cfg, params
    from inpaintnet_amd import layout
    from tests.test_gpu_kernels import pack
    E = 10
    cfg = ops.vae_config(V, E, H, Z, H)
    table, total = ops.vae_param_table(cfg)
    P = {k: torch.from_numpy(synthetic.det_param(k, s)) for k, s in layout.vae_param_shapes(V, E, H, Z, H).items()}
    return cfg, pack(table, total, P)


def _labels(ops, fn):
    """Runs fn() with the launch profile on: (its result, the labels of its launches in order).  A chain status other than 0 fails."""
    ops.prof_enable(True)
    try:
        out = fn()
        torch.cuda.synchronize()
        with tempfile.TemporaryDirectory() as td:
            ops.prof_dump(os.path.join(td, "l.csv"))
            labels = [r["label"] for r in csv.DictReader(open(os.path.join(td, "l.csv")))]
    finally:
        ops.prof_enable(False)
    status = ops.chain_status()
    assert status == 0, (status, ops.slow_waits_summary())
    return out, labels


def run_case(ops, synthetic, name, B, V=48, Z=256, H=512, tf=False, save=False, masks=None, chains=1, seed=0, temperature=None,
             top_p=None, calls=None):
    """-> (forward labels, backward labels or None, digest of weights + samples) of case `name`"""
    cfg, params = _decoder(ops, synthetic, V, Z, H)
    key = f"decoder_launches/{name}"
    z = torch.from_numpy(synthetic.det_normal(f"{key}/z", (B, Z))).cuda()
    target = torch.from_numpy(synthetic.det_tokens(f"{key}/target", (B, T), V)).cuda()
    mb = ops.dropout_mask((4, B, H), 0.5, 11, 0, "cuda") if masks else None
    mt = ops.dropout_mask((T, B, H), 0.5, 11, 4 * B * H, "cuda") if masks == "both" else None
    kw = {}
    if temperature is not None:
        u = synthetic.det_uniform(f"{key}/u", (B, T), 0.0, 1.0).astype(np.float64)
        kw = dict(temperature=temperature, top_p=top_p, uniforms=torch.from_numpy(u).cuda())
    fwd, bwd, h = [], None, hashlib.sha256()
    ops.set_option(15, 4)
    ops.set_option(4, chains)
    try:
        for teacher in (calls or (tf,)):
            (w, s, ws), labels = _labels(ops, lambda: ops.decoder_fwd(cfg, z, target if teacher else None, teacher, params, mask_beat=mb,
                                                                      mask_tick=mt, save=save, multinomial_seed=seed, **kw))
            fwd += labels
            h.update(np.ascontiguousarray(w.cpu().numpy()).tobytes() + b"|samples|" + np.ascontiguousarray(s.cpu().numpy()).tobytes())
        if save:
            g = torch.zeros_like(params)
            dw = torch.from_numpy(synthetic.det_normal(f"{key}/dw", (B, T, V))).cuda() * 1e-3
            _, bwd = _labels(ops, lambda: ops.decoder_bwd(cfg, dw, w, s, params, g, mb, mt, ws))
    finally:
        ops.set_option(4, 1)
        ops.set_option(15, 4)
    return fwd, bwd, h.hexdigest()


def cases():
    """[(name, runner(ops, synthetic) -> (forward labels, backward labels or None, digest))] in the fixture's order"""
    return [(name, lambda o, s, name=name, kw=kw: run_case(o, s, name, **kw)) for name, kw in CASES]


def fixture():
    with open(FIXTURE) as f:
        return json.load(f)
