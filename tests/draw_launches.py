"""The recorded launches of the sampling calls: the cases, the five requests and the digest that
tools/record_draw_launches.py writes into tests/golden/draw_launches.json and tests/test_gpu_draw_launches.py holds the library to.

What a request is routed to is invisible in its tokens: a temperature request run by a truncating kernel returns the same tokens, only
slower.  So per case the fixture holds the ordered launch labels (ops.prof_enable / ops.prof_dump) next to the SHA-256 of the returned
tokens and log-probabilities, NaNs included, as bytes.  Nothing here imports the library at module level: the callers hand in the
`ops` module they want exercised; the inputs are synthetic.det_* values, which depend on their key alone."""
import csv
import hashlib
import json
import os
import tempfile

import numpy as np
import torch

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "draw_launches.json")
REQUESTS = ("argmax", "temperature", "truncated", "masked", "forced")     # each one the one before plus one thing
TOP_K, TOP_P = 3, 0.7
DEC_TEMP, ARNN_TEMP, ROWS_TEMP = 6.0, 1.5, 2.0
# decoder (B, V) at H = 512, Z = 256, 4 x 6 ticks: the register-resident launch with the beat path folded in; the first size past
# kDecodeB1MaxRows, tick by tick with the NV = 1 row kernels; the same with NV = 2, one token past a mask word
DECODER = ((1, 20), (17, 20), (17, 65))
# AnticipationRNN (R, V) at tests/arnn_trunc_ref.py's FULL shapes: the token pass in all builds; the sampling build with two chunks,
# whose truncated levels fall to the per-tick heads; the second launch of the eight-rows-per-launch split
ARNN = ((2, 48), (2, 65), (9, 48))
ROWS, ROWS_V = 5, 65                                                      # the row kernels through ops, NV = 2


def allow_mask(rows, T, V):
    """bool [rows, T, V]: three tokens of four allowed, another quarter banned from tick to tick and row to row"""
    r, t, v = np.ogrid[:rows, :T, :V]
    return (7 * v + 3 * t + r) % 4 != 0


def forced_words(rows, T, V):
    """int32 [rows, T]: a token on the even ticks, -1 (free) on the odd ones"""
    r, t = np.ogrid[:rows, :T]
    return np.where(t % 2 == 0, (3 * r + 5 * t + 1) % V, -1).astype(np.int32)


def labels_of(ops, fn):
    """Runs fn() with the launch profile on: (its result, the labels of its launches in order)."""
    ops.prof_enable(True)
    try:
        out = fn()
        torch.cuda.synchronize()
        with tempfile.TemporaryDirectory() as td:
            ops.prof_dump(os.path.join(td, "l.csv"))
            labels = [r["label"] for r in csv.DictReader(open(os.path.join(td, "l.csv")))]
    finally:
        ops.prof_enable(False)
    assert ops.chain_status() == 0
    return out, labels


def digest(tokens, logp):
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(tokens.detach().cpu().numpy()).tobytes())
    if logp is not None:
        h.update(b"|logp|" + np.ascontiguousarray(logp.detach().cpu().numpy()).tobytes())
    return h.hexdigest()


def _request_kw(req, rows, T, V, pack):
    """top_k / top_p / allowed / forced of request `req` from "truncated" up (device tensors in the layouts ops takes)"""
    kw = {"top_k": TOP_K, "top_p": TOP_P}
    if req in ("masked", "forced"):
        kw["allowed"] = pack(torch.from_numpy(allow_mask(rows, T, V))).cuda().contiguous()
    if req == "forced":
        kw["forced"] = torch.from_numpy(forced_words(rows, T, V)).cuda()
    return kw


def decoder_case(ops, synthetic, B, V, req):
    """-> (labels, digest) of the free-running decoder call of B measures under request `req`"""
    from tests.test_gpu_decode_plans import decoder
    cfg, _, params = decoder(V, 256)
    z = torch.from_numpy(synthetic.det_normal(f"draw_launches/z/{V}/{B}", (B, 256))).cuda()
    kw = {}
    lp = None
    if req != "argmax":
        kw = {"temperature": DEC_TEMP,
              "uniforms": torch.from_numpy(synthetic.det_uniform(f"draw_launches/u/{V}/{B}", (B, 24), 0.0, 1.0).astype(np.float64)).cuda()}
        if req != "temperature":
            lp = torch.full((B, 24), 7.0, dtype=torch.float32, device="cuda")
            kw.update(_request_kw(req, B, 24, V, ops.pack_allowed), logp=lp)
    (_, s, _), labels = labels_of(ops, lambda: ops.decoder_fwd(cfg, z, None, False, params, **kw))
    return labels, digest(s, lp)


def arnn_case(ops, synthetic, R, V, req):
    """-> (labels, digest) of AnticipationRNN's generation of R rows under request `req` (argmax: inet_arnn_generate, row 0 alone)"""
    from tests import arnn_trunc_ref as AR
    W = [torch.from_numpy(w).cuda() for w in AR.net(V, **AR.FULL)]
    oc, hc, u = AR.case(V, R, 0, **AR.FULL)
    oc, hc = torch.from_numpy(oc).cuda(), torch.from_numpy(hc).cuda()
    if req == "argmax":
        tok, labels = labels_of(ops, lambda: ops.arnn_generate(W[0], oc[0], *W[1:], hc_init=hc[0]))
        return labels, digest(tok, None)
    if req == "temperature":
        tok, labels = labels_of(ops, lambda: ops.arnn_sample(W[0], oc, *W[1:], ARNN_TEMP, u, hc_init=hc))
        return labels, digest(tok, None)
    kw = _request_kw(req, R, AR.L, V, ops.pack_allowed)
    (tok, lp, _), labels = labels_of(ops, lambda: ops.arnn_sample(W[0], oc, *W[1:], ARNN_TEMP, u, hc_init=hc, want_logp=True, **kw))
    return labels, digest(tok, lp)


def rows_case(ops, synthetic, req):
    """-> (labels, digest) of the row kernels at ROWS x ROWS_V through ops; "trunc_off" next to the five requests is
    sample_truncated(w, T, u, 0, 1.0), which must still run the truncating kernel; "argmax" is ops.argmax_rows"""
    w = torch.from_numpy(synthetic.det_normal("draw_launches/rows/w", (ROWS, ROWS_V))).cuda()
    u = torch.from_numpy(synthetic.det_uniform("draw_launches/rows/u", (ROWS,), 0.0, 1.0).astype(np.float64)).cuda()
    if req == "argmax":
        tok, labels = labels_of(ops, lambda: ops.argmax_rows(w))
        return labels, digest(tok, None)
    if req == "temperature":
        tok, labels = labels_of(ops, lambda: ops.sample_temperature(w, ROWS_TEMP, u))
        return labels, digest(tok, None)
    if req == "trunc_off":
        (tok, lp), labels = labels_of(ops, lambda: ops.sample_truncated(w, ROWS_TEMP, u, 0, 1.0))
        return labels, digest(tok, lp)
    kw = _request_kw(req, ROWS, 1, ROWS_V, ops.pack_allowed)
    kw = {k: (v[:, 0].contiguous() if isinstance(v, torch.Tensor) else v) for k, v in kw.items()}
    (tok, lp), labels = labels_of(ops, lambda: ops.sample_truncated(w, ROWS_TEMP, u, **kw))
    return labels, digest(tok, lp)


def cases():
    """[(name, runner(ops, synthetic) -> (labels, digest))] in the fixture's order"""
    out = []
    for B, V in DECODER:
        for req in REQUESTS:
            out.append((f"decoder B{B} V{V} {req}", lambda o, s, B=B, V=V, req=req: decoder_case(o, s, B, V, req)))
    for R, V in ARNN:
        for req in REQUESTS:
            out.append((f"arnn R{R} V{V} {req}", lambda o, s, R=R, V=V, req=req: arnn_case(o, s, R, V, req)))
    for req in REQUESTS + ("trunc_off",):
        out.append((f"rows {req}", lambda o, s, req=req: rows_case(o, s, req)))
    return out


def fixture():
    with open(FIXTURE) as f:
        return json.load(f)
