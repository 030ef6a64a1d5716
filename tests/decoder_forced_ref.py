"""The decoder's forced tokens (csrc/sample.h: mask_scores + truncate + pick with u = 0 for S, then tok = f and logp_gap(s, m, f))
restated in float64 on float32 inputs, on top of decoder_constraint_ref.  The rule, as include/inpaintnet_hip.h, csrc/sample.h and
DESIGN.md section 15 state it:

Layout.
 - `forced` is an array of `int32` `[rows][T]`.
 - A value `f` with `0 <= f < V` forces that tick.
 - Every other value makes the tick free.  The Python surfaces write -1 for a free tick.
 - A null `forced` means no tick is forced.

At a free tick nothing changes.  Section 13's rule runs as it does today.

At a forced tick with token `f`:
 1. Scores and truncation.
    - Steps 0-2 of section 13 run unchanged on the tick's logits: s = T x in f32, the NaN test, the mask, m, and the top-k / nucleus
      truncation.
    - S is the kept total.
    - The tick's uniform is not used.  The rule is evaluated as with u = 0, so a uniform outside [0, 1) or NaN at a forced tick causes
      no fallback.
 2. Token.
    - The token is `f`.  It is reported in `samples` and fed back into tick t + 1.
    - This holds whether or not `f` is allowed or kept, and it holds on a fallback tick too.
 3. Log-probability.  logp = (s_f - m) - log S as f32.
    - It is exactly -inf when `f` is banned or truncated away (s_f = -inf).
    - It is NaN where the rule does not apply: a NaN among s, or m or S not finite.

Consequences.  The tests hold each of these exactly.
 (a) No forced tick.  A null `forced`, or one with no value in [0, V), gives inet_vae_decoder_sample_cx bit for bit in tokens, logits
     and logp.
 (b) Replay.  Force, at every tick, the tokens that a sampled, truncated or constrained call returned.  The replay uses the same
     temperature, top_k, top_p and mask, and any uniforms at all.  It returns that call's logits and logp bit for bit, with NaN where
     that call had NaN.
 (c) A banned forced token is still returned and fed back.  Its logp is -inf.
 (d) One-bit mask.  A forced tick whose mask has the single bit `f` set has logp exactly 0.0f.
 (e) Free ticks of a partly forced call follow section 13's rule on the trajectory behind the forced tokens.

pick() returns what decoder_constraint_ref.pick returns.  At a forced tick the token is f also where the rule does not apply (logp NaN,
kept count 0); the CDF margin is infinite (no uniform enters) and the nucleus margin is the tick's: whether f is kept may go either way
where top_p lies within MARGIN of a step of the ranking's cumulative mass."""
import numpy as np

from tests import decoder_constraint_ref as CR
from tests import decoder_trunc_ref as TR

MARGIN = TR.MARGIN
FORCED_SETTINGS = ((1.0, 0, 1.0), (6.0, 0, 0.9), (6.0, 8, 0.7))     # (temperature, top_k, top_p) of the every-plan test


def is_forced(f, V):
    return f is not None and 0 <= int(f) < V


def pick(x, temperature, u, top_k=0, top_p=1.0, allow=None, forced=None, e_ulps=0):
    """x [V] f32, allow bool [V] or None, forced an int or None -> (token, logp f32, kept count n, CDF margin, nucleus margin).  A free
    tick (forced None or outside [0, V)): decoder_constraint_ref.pick, token -1 where the rule does not apply.  A forced tick: the token
    is forced, logp NaN and n = 0 where the rule does not apply."""
    x = np.asarray(x, dtype=np.float32)
    V = x.size
    if not is_forced(forced, V):
        return CR.pick(x, temperature, u, top_k, top_p, allow, e_ulps)
    f = int(forced)
    if not (0.0 < top_p <= 1.0):
        raise ValueError(f"top_p {top_p!r} outside (0, 1]")
    a = CR.effective(allow, V)
    none = (f, np.float32(np.nan), 0, np.inf, np.inf)
    with np.errstate(invalid="ignore", over="ignore"):
        s = (np.float32(temperature) * x).astype(np.float32)
    if np.isnan(s).any():
        return none
    s = np.where(a, s, np.float32(-np.inf)).astype(np.float32)
    m = s.max()
    if not np.isfinite(m):
        return none
    with np.errstate(invalid="ignore"):
        d = (s - m).astype(np.float32)
    e32 = np.exp(d).astype(np.float32)
    for _ in range(abs(e_ulps)):
        e32 = np.where((e32 == 1.0) | (e32 == 0.0), e32, np.nextafter(e32, np.float32(np.inf if e_ulps > 0 else 0.0))).astype(np.float32)
    e = e32.astype(np.float64)
    order = np.lexsort((np.arange(V), -s.astype(np.float64)))
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
    S = np.where(keep, e, 0.0).sum()
    if not (S > 0.0 and np.isfinite(S)):
        return none
    # (the truncation writes s = -inf over a dropped token; a banned one holds it already)
    lp = np.float32(np.float64(d[f]) - np.log(S)) if keep[f] and a[f] else np.float32(-np.inf)
    return f, lp, n, np.inf, bm


def pick_rows(w, temperature, u, top_k=0, top_p=1.0, allow=None, forced=None):
    """w [..., V] logits, u [...] uniforms, allow bool [..., V] or None, forced int [...] or None -> tokens (a free tick outside the rule:
    the masked argmax), logp f32, kept counts, the two margins, and s_tok - m (what the logp tolerance scales with; 0 where logp is not
    finite), all of u's shape"""
    w = np.asarray(w, dtype=np.float32)
    u = np.asarray(u, dtype=np.float64)
    V = w.shape[-1]
    flat = w.reshape(-1, V)
    al = None if allow is None else np.asarray(allow, dtype=bool).reshape(-1, V)
    fo = None if forced is None else np.asarray(forced).reshape(-1)
    N = flat.shape[0]
    tok, lp, n = np.empty(N, dtype=np.int64), np.empty(N, dtype=np.float32), np.empty(N, dtype=np.int64)
    cm, bm, d = np.empty(N), np.empty(N), np.zeros(N)
    for i, (row, ui) in enumerate(zip(flat, u.reshape(-1))):
        a = None if al is None else al[i]
        f = None if fo is None else int(fo[i])
        t, lp[i], n[i], cm[i], bm[i] = pick(row, temperature, ui, top_k, top_p, a, f)
        tok[i] = t if t >= 0 else CR.masked_argmax(row, a)
        if t >= 0 and np.isfinite(lp[i]):
            sr = np.where(CR.effective(a, V), (np.float32(temperature) * row).astype(np.float32), np.float32(-np.inf))
            d[i] = float(sr[t] - sr.max())
    sh = u.shape
    return tok.reshape(sh), lp.reshape(sh), n.reshape(sh), cm.reshape(sh), bm.reshape(sh), d.reshape(sh)


def forced_trajectory(P64, z, temperature, u, top_k, top_p, allow, forced, **kw):
    """The forced decode of the oracle (decoder_trunc_ref.trajectory) -> (logits [B,T,V], tokens, logp f32, kept counts, CDF margins,
    nucleus margins, s_tok - m), [B,T] each; allow bool [B,T,V] or None, forced int [B,T] or None"""
    B, T = u.shape
    lp = np.empty((B, T), dtype=np.float32)
    n, cm, bm, d = np.empty((B, T), dtype=np.int64), np.empty((B, T)), np.empty((B, T)), np.empty((B, T))

    def choose(t, w):
        tok, lp[:, t], n[:, t], cm[:, t], bm[:, t], d[:, t] = pick_rows(w, temperature, u[:, t], top_k, top_p,
                                                                         None if allow is None else allow[:, t],
                                                                         None if forced is None else forced[:, t])
        return tok
    w, tok = TR.trajectory(P64, z, choose, **kw)
    return w, tok, lp, n, cm, bm, d


# ---- the inputs the host test counts margins on and the GPU test runs: one definition ----
def plan_forced(V, B, T=24):
    """the every-plan pattern: forced[r, t] = (5 r + 11 t + 2) % V where (r + 2 t) % 3 == 0, else -1 (used with
    decoder_constraint_ref.plan_mask: about 40 % of its forced tokens are banned)"""
    r, t = np.meshgrid(np.arange(B), np.arange(T), indexing="ij")
    return np.where((r + 2 * t) % 3 == 0, (5 * r + 11 * t + 2) % V, -1).astype(np.int32)


def alone_forced(rows, V):
    """the kernel-alone pattern: (3 r + 1) % V on every second row, else -1"""
    r = np.arange(rows)
    return np.where(r % 2 == 0, (3 * r + 1) % V, -1).astype(np.int32)
