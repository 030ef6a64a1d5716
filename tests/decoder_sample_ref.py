"""The decoder's temperature-sampling rule (csrc/sample.h) restated in float64, and what the tests build on it.

For post-ReLU logits x of one (row, tick), a temperature T and a uniform u:  s = T x,  e_v = exp(s_v - max s),  token = the first v
whose inclusive prefix of e exceeds u * sum(e) -- np.random.choice's order (searchsorted(cumsum(p) / sum(p), u, 'right')).  Where that
does not apply (max s or the sum not finite, a NaN among s, u outside [0, 1) or NaN, no prefix above u * sum) the tick takes the
argmax, lowest index among equals."""
import numpy as np
import torch

from oracle import torch_ref as O

MARGIN = 2e-5           # a draw whose uniform lies this close to a step of the CDF may go either way under another rounding


def pick(x, temperature, u):
    """x [V] -> (token, distance of u from the nearest inner step of the CDF); token -1 where the rule does not apply"""
    with np.errstate(invalid="ignore"):                        # (inf * 0: the NaN is what the next line looks for)
        s = float(temperature) * np.asarray(x, dtype=np.float64)
    u = float(u)
    if np.isnan(s).any() or not np.isfinite(s.max()) or not (0.0 <= u < 1.0):
        return -1, np.inf
    pre = np.cumsum(np.exp(s - s.max()))
    tot = pre[-1]
    if not (tot > 0.0 and np.isfinite(tot)):
        return -1, np.inf
    hit = pre > u * tot
    if not hit.any():
        return -1, np.inf
    margin = float(np.abs(pre[:-1] / tot - u).min()) if len(pre) > 1 else 1.0
    return int(np.argmax(hit)), margin


def argmax_first(x):
    """np.argmax's rule: a NaN is the maximum, the lowest index wins"""
    return int(np.argmax(np.asarray(x)))


def sample_rows(w, temperature, u):
    """w [..., V] logits, u [...] uniforms -> (tokens [...] with the argmax where the rule does not apply, margins [...])"""
    w = np.asarray(w)
    u = np.asarray(u, dtype=np.float64)
    flat = w.reshape(-1, w.shape[-1])
    tok = np.empty(flat.shape[0], dtype=np.int64)
    mg = np.empty(flat.shape[0])
    for i, (row, ui) in enumerate(zip(flat, u.reshape(-1))):
        t, mg[i] = pick(row, temperature, ui)
        tok[i] = t if t >= 0 else argmax_first(row)
    return tok.reshape(u.shape), mg.reshape(u.shape)


def oracle_logits(P64, z, feed, masks=None):
    """float64 logits [B,T,V] of the oracle's decoder with `feed` [B,T] fed back"""
    with torch.no_grad():
        w, _ = O.decoder_forward(P64, z.double(), None, False, masks=masks, feed_tokens=torch.as_tensor(feed, dtype=torch.int64))
    return w.numpy()


def sampled_trajectory(P64, z, temperature, u):
    """The sampled decode of the oracle: tick t's logits depend on the tokens before t alone, so feeding the picks back until they
    stop changing (at most T + 1 passes) gives the trajectory.  -> (logits [B,T,V], tokens [B,T], margins [B,T])"""
    B, T = u.shape
    tok = np.zeros((B, T), dtype=np.int64)
    for _ in range(T + 1):
        w = oracle_logits(P64, z, tok)
        new, mg = sample_rows(w, temperature, u)
        if np.array_equal(new, tok):
            return w, tok, mg
        tok = new
    raise AssertionError("the sampled trajectory did not settle")
