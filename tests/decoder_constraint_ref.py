"""The decoder's constrained sampling rule (csrc/sample.h: mask_words + mask_scores in front of truncate + pick + logp_of) restated in
float64 on float32 inputs.  The rule, as include/inpaintnet_hip.h, csrc/sample.h and DESIGN.md section 13 state it:

Mask layout.  `allow` is an array of 64-bit words [rows][T][NW], with NW = ceil(V / 64).  Token v is allowed iff bit v % 64 of word
v / 64 is set.  Bits at or above V are ignored.  A null `allow` means no constraint.

For one (row, tick), with logits x[0..V), temperature T, uniform u, top_k and top_p:
 0. Empty mask.  A mask with no bit set in [0, V) counts as all ones for that tick.  The Python surfaces refuse such a tick with
    ValueError before any launch.
 1. Scores.  s_v = T x_v in f32.  The NaN test of section 10 runs over all V values of s, as today.  The mask therefore does not change
    which ticks fall back.  Then s_v = -inf for every banned v, and m = the maximum over the allowed tokens.
 2. Truncation and draw.  Steps 2-7 of section 11 run unchanged on these s, with V and K = top_k unchanged.  Banned tokens tie at -inf
    and rank last.  Their e = expf(-inf - m) is 0, so they add no mass and cannot be the first prefix above u S.  A top_k above the
    number of allowed tokens keeps all of them.  logp is taken under the masked and truncated distribution.
 3. Fallback.  Where the rule does not apply (a NaN among s, m or S not finite, u outside [0, 1) or NaN), the tick takes today's argmax
    rule on the logits with every banned entry replaced by -inf.  The decode kernel may use its padding value -1 instead, which lies
    below every post-ReLU logit.  logp is NaN there.  The token is still an allowed one.

Here the mask is a bool vector [V] (True = allowed; None = no constraint); words() gives the kernel's layout without going through
ops.pack_allowed.  The functions return what decoder_trunc_ref.pick / pick_rows / kept_rows return, with both margins of every draw.
masked_argmax() is step 3 with "the token is still an allowed one" taken literally: np.argmax's rule (a NaN is the maximum, the lowest
index wins) over the ALLOWED entries alone -- np.argmax of the -inf-filled row wherever an allowed entry is above -inf or NaN."""
import numpy as np

from tests import decoder_trunc_ref as TR

MARGIN = TR.MARGIN


def effective(allow, V):
    """step 0: None or an empty mask -> all ones"""
    if allow is None:
        return np.ones(V, dtype=bool)
    allow = np.asarray(allow, dtype=bool)
    assert allow.shape == (V,), (allow.shape, V)
    return allow if allow.any() else np.ones(V, dtype=bool)


def words(allow):
    """bool [..., V] -> uint64 [..., ceil(V / 64)]: bit v % 64 of word v // 64 (plain Python integers: no packbits, no byte order)"""
    allow = np.asarray(allow, dtype=bool)
    V = allow.shape[-1]
    nw = (V + 63) // 64
    flat = allow.reshape(-1, V)
    out = np.zeros((flat.shape[0], nw), dtype=np.uint64)
    for i, row in enumerate(flat):
        for j in range(nw):
            out[i, j] = np.uint64(sum(1 << (v - 64 * j) for v in np.flatnonzero(row[64 * j:64 * j + 64]) + 64 * j))
    return out.reshape(allow.shape[:-1] + (nw,))


def masked_argmax(x, allow):
    """step 3: the argmax (a NaN is the maximum, lowest index among equals) over the allowed tokens"""
    x = np.asarray(x, dtype=np.float32)
    cand = np.flatnonzero(effective(allow, x.size))
    return int(cand[int(np.argmax(x[cand]))])


def pick(x, temperature, u, top_k=0, top_p=1.0, allow=None, e_ulps=0):
    """x [V] f32, allow bool [V] or None -> (token or -1 where the rule does not apply, logp f32 (NaN there), kept count n (0 there), CDF
    margin, nucleus margin): decoder_trunc_ref.pick's returns"""
    x = np.asarray(x, dtype=np.float32)
    V = x.size
    if not (0.0 < top_p <= 1.0):
        raise ValueError(f"top_p {top_p!r} outside (0, 1]")
    a = effective(allow, V)
    none = (-1, np.float32(np.nan), 0, np.inf, np.inf)
    with np.errstate(invalid="ignore", over="ignore"):
        s = (np.float32(temperature) * x).astype(np.float32)
    u = float(u)
    if np.isnan(s).any():                                       # over all V values: the mask does not change which ticks fall back
        return none
    s = np.where(a, s, np.float32(-np.inf)).astype(np.float32)
    m = s.max()                                                 # (= the maximum over the allowed tokens)
    if not np.isfinite(m) or not (0.0 <= u < 1.0):
        return none
    with np.errstate(invalid="ignore"):
        d = (s - m).astype(np.float32)
    e32 = np.exp(d).astype(np.float32)
    for _ in range(abs(e_ulps)):
        e32 = np.where((e32 == 1.0) | (e32 == 0.0), e32, np.nextafter(e32, np.float32(np.inf if e_ulps > 0 else 0.0))).astype(np.float32)
    e = e32.astype(np.float64)
    order = np.lexsort((np.arange(V), -s.astype(np.float64)))            # s descending, index ascending: the banned tie at -inf, last
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
    idx = np.flatnonzero(keep)                                  # (decoder_trunc_ref.pick's steps: a kept token without mass repeats one)
    cm = float(np.abs(pre[idx][:-1] / S - u).min()) if idx.size > 1 else 1.0
    tok = int(np.argmax(hit))
    return tok, np.float32(np.float64(d[tok]) - np.log(S)), n, cm, bm


def pick_rows(w, temperature, u, top_k=0, top_p=1.0, allow=None):
    """w [..., V] logits, u [...] uniforms, allow bool [..., V] or None -> tokens (the masked argmax where the rule does not apply), logp
    f32, kept counts, the two margins, and s_tok - m (what the logp tolerance scales with), all of u's shape"""
    w = np.asarray(w, dtype=np.float32)
    u = np.asarray(u, dtype=np.float64)
    V = w.shape[-1]
    flat = w.reshape(-1, V)
    al = None if allow is None else np.asarray(allow, dtype=bool).reshape(-1, V)
    N = flat.shape[0]
    tok, lp, n = np.empty(N, dtype=np.int64), np.empty(N, dtype=np.float32), np.empty(N, dtype=np.int64)
    cm, bm, d = np.empty(N), np.empty(N), np.zeros(N)
    for i, (row, ui) in enumerate(zip(flat, u.reshape(-1))):
        a = None if al is None else al[i]
        t, lp[i], n[i], cm[i], bm[i] = pick(row, temperature, ui, top_k, top_p, a)
        tok[i] = t if t >= 0 else masked_argmax(row, a)
        if t >= 0:
            sr = np.where(effective(a, V), (np.float32(temperature) * row).astype(np.float32), np.float32(-np.inf))
            d[i] = float(sr[t] - sr.max())
    sh = u.shape
    return tok.reshape(sh), lp.reshape(sh), n.reshape(sh), cm.reshape(sh), bm.reshape(sh), d.reshape(sh)


def kept_rows(w, temperature, top_k=0, top_p=1.0, allow=None):
    """w [..., V] -> bool [..., V]: the kept set of every row among its allowed tokens (all False where the rule does not apply)"""
    w = np.asarray(w, dtype=np.float32)
    V = w.shape[-1]
    flat = w.reshape(-1, V)
    al = None if allow is None else np.asarray(allow, dtype=bool).reshape(-1, V)
    out = np.zeros(flat.shape, dtype=bool)
    for i, row in enumerate(flat):
        a = effective(None if al is None else al[i], V)
        n = pick(row, temperature, 0.5, top_k, top_p, a)[2]
        with np.errstate(invalid="ignore", over="ignore"):
            s = np.where(a, (np.float32(temperature) * row).astype(np.float32), np.float32(-np.inf))
        out[i, np.lexsort((np.arange(V), -s.astype(np.float64)))[:n]] = True
        out[i] &= a
    return out.reshape(w.shape)


def free(allow):
    """allow bool [..., V] -> bool [...]: ticks with more than one allowed token (the margin caps count these; one-bit ticks are exact)"""
    a = np.asarray(allow, dtype=bool)
    c = a.sum(-1)
    return (c == 0) | (c > 1)


def constrained_trajectory(P64, z, temperature, u, top_k, top_p, allow):
    """The constrained decode of the oracle (decoder_trunc_ref.trajectory) -> (logits [B,T,V], tokens, kept counts, CDF margins, nucleus
    margins), [B,T] each; allow bool [B,T,V]"""
    B, T = u.shape
    n, cm, bm = (np.empty((B, T), dtype=np.int64), np.empty((B, T)), np.empty((B, T)))

    def choose(t, w):
        tok, _, n[:, t], cm[:, t], bm[:, t], _ = pick_rows(w, temperature, u[:, t], top_k, top_p, allow[:, t])
        return tok
    w, tok = TR.trajectory(P64, z, choose)
    return w, tok, n, cm, bm


# ---- the inputs the host test counts margins on and the GPU test runs: one definition ----
def plan_mask(V, B, T=24):
    """the every-plan mask: allow[r, t, v] = (v == (7 r + 3 t + 1) % V) where (r + t) % 4 == 0, else ((v + t + r) % 5 != 0)"""
    r, t, v = np.meshgrid(np.arange(B), np.arange(T), np.arange(V), indexing="ij")
    return np.where((r + t) % 4 == 0, v == (7 * r + 3 * t + 1) % V, (v + t + r) % 5 != 0)


def alone_mask(x):
    """the kernel-alone mask of rows x [rows, V]: allow[r, v] = ((v + r) % 3 != 0) or x[r, v] == 0; an empty row stays empty"""
    rows, V = x.shape
    r, v = np.meshgrid(np.arange(rows), np.arange(V), indexing="ij")
    return ((v + r) % 3 != 0) | (x == 0)
