"""The decoder's truncated sampling rule (csrc/sample.h: truncate + pick + logp_of) restated in float64 on float32 inputs.

One (row, tick) with post-ReLU logits x[0..V), a temperature T, a uniform u, an integer top_k and a double top_p:
 1. s = T x in f32, m = max s.  Where the sampling rule does not apply (a NaN among s, m or the total not finite, u outside [0, 1) or
    NaN) the tick takes the argmax, lowest index among equals, and logp is NaN.
 2. e_v = expf(s_v - m) in f32.
 3. The tokens are ordered by (s_v descending, v ascending).
 4. K = top_k if 1 <= top_k < V, else V.
 5. A_i = the f64 sum of e over the first i tokens of the order; n = the smallest i <= K with A_i >= top_p A_K (top_p >= 1: n = K).
 6. Kept = the first n tokens of the order; token = the first v in INDEX order among the kept whose inclusive f64 prefix of kept e
    exceeds u S, S = the kept total.
 7. logp = (s_tok - m) - log(S), stored as f32.
Every draw comes with two margins: the distance of u from the nearest inner step of the kept CDF, and the distance of top_p from the
nearest A_i / A_K; a draw with one of them below MARGIN may go either way under another rounding of expf or another summation order."""
import numpy as np
import torch

from oracle import torch_ref as O
from tests import decoder_sample_ref as R

MARGIN = R.MARGIN        # 2e-5, for both margins
SETTINGS = ((1.0, 5, 1.0), (6.0, 0, 0.9), (6.0, 8, 0.7))        # (temperature, top_k, top_p) of the every-plan test


def pick(x, temperature, u, top_k=0, top_p=1.0, e_ulps=0):
    """x [V] f32 -> (token or -1 where the rule does not apply, logp f32 (NaN there), kept count n (0 there), CDF margin, nucleus margin)
    e_ulps: every e that is not exactly 1 moved by that many f32 ulps -- another expf's rounding (the tie rows' precondition)"""
    x = np.asarray(x, dtype=np.float32)
    V = x.size
    if not (0.0 < top_p <= 1.0):
        raise ValueError(f"top_p {top_p!r} outside (0, 1]")
    none = (-1, np.float32(np.nan), 0, np.inf, np.inf)
    with np.errstate(invalid="ignore", over="ignore"):
        s = (np.float32(temperature) * x).astype(np.float32)
    u = float(u)
    if np.isnan(s).any() or not np.isfinite(s.max()) or not (0.0 <= u < 1.0):
        return none
    m = s.max()
    d = (s - m).astype(np.float32)
    e32 = np.exp(d).astype(np.float32)
    for _ in range(abs(e_ulps)):
        e32 = np.where(e32 == 1.0, e32, np.nextafter(e32, np.float32(np.inf if e_ulps > 0 else 0.0))).astype(np.float32)
    e = e32.astype(np.float64)
    order = np.lexsort((np.arange(V), -s.astype(np.float64)))            # s descending, index ascending
    K = int(top_k) if 1 <= top_k < V else V
    A = np.cumsum(e[order][:K])
    bm = np.inf
    if top_p < 1.0:
        n = int(np.argmax(A >= top_p * A[-1])) + 1
        bm = float(np.abs(A / A[-1] - top_p).min())
    else:
        n = K
    keep = np.zeros(V, dtype=bool)
    keep[order[:n]] = True
    pre = np.cumsum(np.where(keep, e, 0.0))
    S = pre[-1]
    if not (S > 0.0 and np.isfinite(S)):
        return none
    hit = pre > u * S
    if not hit.any():
        return none
    idx = np.flatnonzero(keep)
    cm = float(np.abs(pre[idx][:-1] / S - u).min()) if idx.size > 1 else 1.0
    tok = int(np.argmax(hit))
    return tok, np.float32(np.float64(d[tok]) - np.log(S)), n, cm, bm


def pick_rows(w, temperature, u, top_k=0, top_p=1.0):
    """w [..., V] logits, u [...] uniforms -> tokens (the argmax where the rule does not apply), logp f32, kept counts, the two margins,
    and s_tok - m (what the logp tolerance scales with), all of u's shape"""
    w = np.asarray(w, dtype=np.float32)
    u = np.asarray(u, dtype=np.float64)
    flat = w.reshape(-1, w.shape[-1])
    N = flat.shape[0]
    tok, lp, n = np.empty(N, dtype=np.int64), np.empty(N, dtype=np.float32), np.empty(N, dtype=np.int64)
    cm, bm, d = np.empty(N), np.empty(N), np.zeros(N)
    for i, (row, ui) in enumerate(zip(flat, u.reshape(-1))):
        t, lp[i], n[i], cm[i], bm[i] = pick(row, temperature, ui, top_k, top_p)
        tok[i] = t if t >= 0 else R.argmax_first(row)
        if t >= 0:
            sr = (np.float32(temperature) * row).astype(np.float32)
            d[i] = float(sr[t] - sr.max())
    sh = u.shape
    return tok.reshape(sh), lp.reshape(sh), n.reshape(sh), cm.reshape(sh), bm.reshape(sh), d.reshape(sh)


def kept_rows(w, temperature, top_k=0, top_p=1.0):
    """w [..., V] -> bool [..., V]: the kept set of every row (all False where the rule does not apply); it does not depend on u"""
    w = np.asarray(w, dtype=np.float32)
    flat = w.reshape(-1, w.shape[-1])
    out = np.zeros(flat.shape, dtype=bool)
    for i, row in enumerate(flat):
        n = pick(row, temperature, 0.5, top_k, top_p)[2]
        s = (np.float32(temperature) * row).astype(np.float32)
        out[i, np.lexsort((np.arange(row.size), -s.astype(np.float64)))[:n]] = True
    return out.reshape(w.shape)


def firm(cm, bm):
    """draws that no rounding can move: both margins at least MARGIN"""
    return (np.asarray(cm) >= MARGIN) & (np.asarray(bm) >= MARGIN)


def logp_tol(d):
    """one f32 rounding each for s_tok - m, the total's expf terms and the final store: 8 ulp of max(1, |s_tok - m|)"""
    return 8.0 * 2.0 ** -23 * np.maximum(1.0, np.abs(d))


def trajectory(P64, z, choose, beats=4, ticks_per_beat=6, prefix="decoder"):
    """The float64 oracle's free-running decode (oracle.torch_ref.decoder_forward, no masks) with the fed-back token of tick t chosen by
    choose(t, logits [B,V] as f32 numpy) -> tokens [B]: one pass instead of decoder_sample_ref.sampled_trajectory's T + 1.
    -> (logits [B,T,V] float64 numpy, tokens [B,T])"""
    with torch.no_grad():
        B = z.shape[0]
        z = z.double()
        H = P64[f"{prefix}.rnn_beat.weight_hh_l0"].shape[1]
        hb0 = O.selu_k(z @ P64[f"{prefix}.z_to_beat_rnn_input.0.weight"].t() + P64[f"{prefix}.z_to_beat_rnn_input.0.bias"], None)
        h_beat = hb0.view(B, 2, H).transpose(0, 1).contiguous()
        beat_in = P64[f"{prefix}.b_0"].view(1, 1, 1).expand(B, beats, 1)
        beat_out, _ = O.gru_stack(beat_in, h_beat, P64, f"{prefix}.rnn_beat", 2, False, None)
        E = P64[f"{prefix}.note_embedding_layer.weight"]
        prev = P64[f"{prefix}.x_0"].view(1, -1).expand(B, -1)
        pf = f"{prefix}.rnn_tick"
        ws, toks = [], []
        for i in range(beats):
            o_i = beat_out[:, i]
            ht0 = O.selu_k(o_i @ P64[f"{prefix}.beat_emb_to_tick_rnn_hidden.0.weight"].t()
                           + P64[f"{prefix}.beat_emb_to_tick_rnn_hidden.0.bias"], None)
            hid = ht0.view(B, 2, H).transpose(0, 1)
            h0, h1 = hid[0], hid[1]
            c_i = O.selu_k(o_i @ P64[f"{prefix}.beat_emb_to_tick_rnn_input.0.weight"].t()
                           + P64[f"{prefix}.beat_emb_to_tick_rnn_input.0.bias"], None)
            for j in range(ticks_per_beat):
                t = i * ticks_per_beat + j
                gi0 = torch.cat((prev, c_i), 1) @ P64[f"{pf}.weight_ih_l0"].t() + P64[f"{pf}.bias_ih_l0"]
                h0 = O.gru_cell(gi0, h0, P64[f"{pf}.weight_hh_l0"], P64[f"{pf}.bias_hh_l0"])
                gi1 = h0 @ P64[f"{pf}.weight_ih_l1"].t() + P64[f"{pf}.bias_ih_l1"]
                h1 = O.gru_cell(gi1, h1, P64[f"{pf}.weight_hh_l1"], P64[f"{pf}.bias_hh_l1"])
                w_t = O.relu_k(h1 @ P64[f"{prefix}.tick_emb_to_note_emb.0.weight"].t() + P64[f"{prefix}.tick_emb_to_note_emb.0.bias"], None)
                tok = np.asarray(choose(t, w_t.numpy().astype(np.float32)), dtype=np.int64)
                prev = E[torch.from_numpy(tok)]
                ws.append(w_t)
                toks.append(tok)
        return torch.stack(ws, 1).numpy(), np.stack(toks, 1)


def truncated_trajectory(P64, z, temperature, u, top_k, top_p):
    """The truncated-sampling decode of the oracle -> (logits [B,T,V], tokens, kept counts, CDF margins, nucleus margins), [B,T] each"""
    B, T = u.shape
    n, cm, bm = (np.empty((B, T), dtype=np.int64), np.empty((B, T)), np.empty((B, T)))

    def choose(t, w):
        tok, _, n[:, t], cm[:, t], bm[:, t], _ = pick_rows(w, temperature, u[:, t], top_k, top_p)
        return tok
    w, tok = trajectory(P64, z, choose)
    return w, tok, n, cm, bm


# ---- the inputs the host test counts margins on and the GPU test runs: one definition ----
ALONE_V = (1, 2, 63, 64, 65, 128, 129, 512)                  # the 64-lane chunk edges
ALONE_ROWS = (1, 5, 70)
ALONE_TEMPS = (1.0, 6.0, -2.0)
ALONE_TOP_P = (1.0, 0.999, 0.5, 1e-9)                        # (the last keeps one token)
ALONE_SEED = 0                                               # (tests/test_decoder_trunc_host.py holds these rows to the margin caps)
PLAN_V, PLAN_Z, PLAN_B = (20, 48, 100), (256, 128), (1, 2, 4, 5, 7, 16)


def alone_top_k(V):
    return (0, 1, 2, V - 1, V, V + 5)


def alone_case(V, rows):
    """-> (x [rows, V + 3] post-ReLU logits with NaN in the padding, u [rows, 2] uniforms of which column 0 is used).
    A row is a floor of equal logits (1.0: ties, lowest index first) with one zero and a head of nine tokens around 20 at random places:
    a positive temperature ranks the head by value over the floor, a negative one the zero over the tied floor over the head.  The
    shape is forced by the margin caps, which are conditions on the inputs: among n tokens of comparable mass a uniform lies within
    2e-5 of a CDF step with probability 4e-5 n, and top_p within 2e-5 of a nucleus step wherever the steps around it are dense --
    which is every draw of a smooth 512-token row at top_p = 0.999, and, with two zeros, every draw at top_k = 2, top_p = 0.5 under a
    negative temperature (two equal masses: A_1 / A_2 = 0.5).  Here the steps are the head's, or the floor's equal ones whose distance
    from top_p is the same in every row, and the other group's mass is below 1e-7 of the total.  (V <= 12: every token is head.)"""
    from inpaintnet_amd import synthetic
    h = V if V <= 12 else 9
    g = synthetic.det_normal(f"decoder_trunc/alone/{ALONE_SEED}/{V}/{rows}", (rows, V + 3), 1.5)
    key = synthetic.det_uniform(f"decoder_trunc/alone/head/{ALONE_SEED}/{V}/{rows}", (rows, V), 0.0, 1.0)
    x = np.ones((rows, V + 3), dtype=np.float32)
    x[:, V:] = np.nan
    for r in range(rows):
        order = np.argsort(key[r], kind="stable")
        x[r, order[:h]] = np.maximum(20.0 + g[r, order[:h]], 0.0)
        if V > h:
            x[r, order[h]] = 0.0
    u = synthetic.det_uniform(f"decoder_trunc/alone/u/{ALONE_SEED}/{V}/{rows}", (rows, 2), 0.0, 1.0).astype(np.float64)
    return x, u


def tie_rows(V):
    """all equal | half zeros, the others one value | (V > 64) two tied maxima on lanes 63 and 64 above a floor of zeros"""
    rows = [np.full(V, 0.75, dtype=np.float32), np.where(np.arange(V) % 2 == 0, 0.0, 0.5).astype(np.float32)]
    if V > 64:
        r = np.zeros(V, dtype=np.float32)
        r[63] = r[64] = 1.25
        rows.append(r)
    return np.stack(rows)


def plan_inputs(V, Z, B, si):
    """z [B,Z] f32 and uniforms [B,24] of the every-plan test's call (V, Z, B) under SETTINGS[si]"""
    from inpaintnet_amd import synthetic
    z = synthetic.det_normal(f"decoder_trunc/z/{V}/{Z}/{B}", (B, Z))
    u = synthetic.det_uniform(f"decoder_trunc/u/{V}/{Z}/{B}/{si}", (B, 24), 0.0, 1.0).astype(np.float64)
    return z, u
