"""The float64 restatement of the importance-weighted log-likelihood kernels (include/inpaintnet_hip.h inet_iw_draw / inet_nll_rows /
inet_iw_finish), the end-to-end log weights through the float64 oracle, and the error bounds of the float32
kernels, derived here.  Shared by tests/test_iw_host.py (CPU) and tests/test_gpu_iw_kernels.py / tests/test_gpu_iw_model.py (GPU).

Nothing here imports the library: a reference that called the code under test would prove nothing.

The rule.  For a measure x_b (T = 24 tokens) the encoder gives mu_b, ls_b (log sigma), both [Z].  For k = 0..K-1 and eps[b,k,:]
standard normal:
  z[b,k,d]   = mu[b,d] + eps[b,k,d] * exp(ls[b,d])
  logr[b,k]  = log p(z) - log q(z|x) = sum_d ( 0.5 eps^2 - 0.5 z^2 + ls[b,d] )     (the 2*pi terms cancel)
  nll[b,k]   = - sum_t log softmax(weights[b,k,t,:])[ x[b,t] ]
               (weights come from the decoder run on z[b,k] with x_b's own tokens fed back: teacher-forced, eval mode, no dropout)
  logw[b,k]  = logr[b,k] - nll[b,k]
  m = max_k logw;  s1 = sum_k exp(logw - m);  s2 = sum_k exp(2 (logw - m))
  iwae[b] = m + log(s1 / K)         lower bound on log p(x_b), tight as K grows
  elbo[b] = (sum_k logw) / K        the single-sample bound, averaged
  ess[b]  = s1^2 / s2               effective sample size, in [1, K]
  rec[b]  = (sum_k nll) / K
  kl[b]   = -(sum_k logr) / K, the Monte-Carlo KL, formed as -(sum_k logw + sum_k nll) / K
A NaN anywhere in a measure's logw row: iwae, elbo and ess are NaN.  m == -inf: iwae = elbo = -inf, ess = 0.  A +inf: what IEEE gives.

The bounds, with u = 2^-24 (the unit roundoff of float32); first-order terms, the factor SLACK = 1.01 covers the higher orders.  expf
and logf are the device library's single-precision functions (NOT the hardware approximations), taken at 2 ulp = EXP_U u = 4 u, as
tests/mmd_ref.py takes expf.  Any fixed order of additions errs by at most depth u sum|terms| (Higham, Accuracy and Stability of
Numerical Algorithms, section 4.2), depth = the additions a term passes through.

iw_draw.  s^ = expf(ls) errs by EXP_U u s; the product eps s^ adds u, the sum mu + . adds u |z| (a fused multiply-add: one rounding
  less -- the bound allows both):
      |z^ - z| <= dz = u (|z| + (EXP_U + 1) |eps s|)
  The term t = 0.5 eps^2 - 0.5 z^2 + ls, mag = 0.5 eps^2 + 0.5 z^2 + |ls| >= |t|: the halvings are exact, the two squares, the
  difference and the sum round once each (fused: fewer), each by at most u mag: 3 u mag in all; z^ for z moves 0.5 z^2 by |z| dz.
  A lane adds its terms in ascending d -- ceil(Z / 64) of them on the scalar path, 4 ceil(Z / 256) <= ceil(Z / 64) + 3 on the 16-byte
  path -- and a xor tree of 6 levels adds the lanes:
      DEPTH_DRAW(Z) = ceil(Z / 64) + 3 + 6
      |logr^ - logr| <= sum_d ( (3 + DEPTH_DRAW) u mag_d + |z_d| dz_d )
nll_rows.  Per tick, m = max_v x_v is exact; fl(x_v - m) errs by u |x_v - m|, which is the RELATIVE error it causes in the
  exponential, expf adds EXP_U u, a result below the smallest normal float may be flushed (2^-126 absolute, V of them); a lane adds
  ceil(V / 64) exponentials, the xor tree 6 levels; all terms are >= 0 and se >= 1 (the maximum's own term):
      relse = ( sum_v e_v (EXP_U + |x_v - m|) / se + DEPTH_V ) u + V 2^-126,   DEPTH_V = ceil(V / 64) + 6
  logf(se^) errs by relse + EXP_U u |log se|;  lse = fl(m + .) by u |lse|;  the term c = fl(lse - x_target) by u |c|:
      err_t = relse + u (EXP_U |log se| + |lse| + |c|)
  Lane 0 of wave w adds its ticks w, w + 4, ... in ascending order (ceil(T / 4)), the four waves meet as (p0 + p1) + (p2 + p3) (2):
      DEPTH_T = ceil(T / 4) + 2
      |nll^ - nll| <= sum_t err_t + DEPTH_T u sum_t |c_t|
  logw = fl(logr - nll^):  |logw^ - logw| <= (the bound of nll) + u |logw|   (logr is an input here; after iw_draw its bound is added).
inet_cross_entropy on the same rows (the mean loss, for the comparison of the two kernels): the same err per row; a wave adds its
  rows (ceil(rows / (4 g)), g = min(ceil(rows / 4), 128) workgroups), the four waves in order (3), the product with out_scale (1), one
  atomic per workgroup in any order (g):   DEPTH_CE = ceil(rows / (4 g)) + 3 + 1 + g.
iw_finish runs in double: its tolerance is 1e-12 relative (1e-12 absolute for ess) against numpy float64 on the same float32 inputs."""
import numpy as np
import torch

U = 2.0 ** -24
EXP_U = 4                      # expf, logf: 2 ulp allowed = 4 u
SLACK = 1.01
TINY = 2.0 ** -126             # the smallest normal float32
FINISH_RTOL = 1e-12
COLUMNS = ("iwae", "elbo", "ess", "rec", "kl")


def cdiv(a, b):
    return -(-a // b)


def depth_draw(Z):
    return cdiv(Z, 64) + 3 + 6


def depth_v(V):
    return cdiv(V, 64) + 6


def depth_t(T):
    return cdiv(T, 4) + 2


def depth_ce(rows):
    g = min(cdiv(rows, 4), 128)
    return cdiv(rows, 4 * g) + 3 + 1 + g


def draw(mu, ls, eps):
    """mu, ls [B, Z], eps [B, K, Z] -> dict(z [B, K, Z], logr [B, K], z_bound [B, K, Z], logr_bound [B, K]), float64."""
    mu, ls, eps = (np.asarray(a, np.float64) for a in (mu, ls, eps))
    Z = mu.shape[1]
    s = np.exp(ls)[:, None, :]
    es = eps * s
    z = mu[:, None, :] + es
    lsb = np.broadcast_to(ls[:, None, :], z.shape)
    logr = (0.5 * eps * eps - 0.5 * z * z + lsb).sum(-1)
    dz = U * (np.abs(z) + (EXP_U + 1) * np.abs(es))
    mag = 0.5 * eps * eps + 0.5 * z * z + np.abs(lsb)
    bound = ((3 + depth_draw(Z)) * U * mag + np.abs(z) * dz).sum(-1)
    return dict(z=z, logr=logr, z_bound=SLACK * dz, logr_bound=SLACK * bound)


def nll_rows(weights, targets, logr=None):
    """weights [R, T, V] (float32 values), targets [R, T] ints in [0, V), logr [R] or None (0) -> dict(nll [R], logw [R], terms [R, T],
    nll_bound [R], logw_bound [R], term_err [R, T]) in float64.  -inf logits are allowed: exp(-inf) = 0 exactly on both sides."""
    x = np.asarray(weights, np.float64)
    tg = np.asarray(targets, np.int64)
    R, T, V = x.shape
    m = x.max(-1, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        d = x - m
        e = np.exp(d)
        se = e.sum(-1)
        ad = np.where(np.isfinite(d), np.abs(d), 0.0)                 # (a -inf logit: its exponential is 0 on both sides)
        relse = ((e * (EXP_U + ad)).sum(-1) / se + depth_v(V)) * U + V * TINY
        lse = m[..., 0] + np.log(se)
        xt = np.take_along_axis(x, tg[..., None], -1)[..., 0]
        c = lse - xt
        err = relse + U * (EXP_U * np.abs(np.log(se)) + np.abs(lse) + np.where(np.isfinite(c), np.abs(c), 0.0))
        nll = c.sum(-1)
        bound = SLACK * (err.sum(-1) + depth_t(T) * U * np.where(np.isfinite(c), np.abs(c), 0.0).sum(-1))
        lr = np.zeros(R) if logr is None else np.asarray(logr, np.float64)
        logw = lr - nll
        lb = bound + SLACK * U * np.where(np.isfinite(logw), np.abs(logw), 0.0)
    return dict(nll=nll, logw=logw, terms=c, nll_bound=bound, logw_bound=lb, term_err=SLACK * err)


def ce_mean(weights, targets):
    """The mean over all R * T rows of the cross-entropy terms, and the bound of inet_cross_entropy's float32 mean (out_scale = 1 /
    rows) and of the float64 mean of nll_rows' float32 outputs.  -> (mean, bound_ce, bound_nll_mean)."""
    r = nll_rows(weights, targets)
    rows = r["terms"].size
    mean = r["terms"].sum() / rows
    bound_ce = (r["term_err"].sum() + SLACK * (depth_ce(rows) + 1) * U * np.abs(r["terms"]).sum()) / rows
    return mean, bound_ce, r["nll_bound"].sum() / rows


def finish(logw, nll):
    """logw, nll [B, K] (float32 values) -> float64 [B, 5], the columns COLUMNS, with the special values of the rule."""
    lw, nl = np.asarray(logw, np.float64), np.asarray(nll, np.float64)
    B, K = lw.shape
    out = np.empty((B, 5))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for b in range(B):
            row = lw[b]
            sw, sn = row.sum(), nl[b].sum()
            if np.isnan(row).any():
                iwae = elbo = ess = np.nan
            else:
                m = row.max()
                if m == -np.inf:
                    iwae = elbo = -np.inf
                    ess = 0.0
                else:
                    d = row - m
                    s1, s2 = np.exp(d).sum(), np.exp(2.0 * d).sum()
                    iwae, elbo, ess = m + np.log(s1 / K), sw / K, s1 * s1 / s2
            out[b] = (iwae, elbo, ess, sn / K, -(sw + sn) / K)
    return out


def oracle_log_weights(P, tokens, eps):
    """The log weights end to end in float64 through oracle.torch_ref: P the state dict (tensors), tokens [B, 24] int64, eps [B, K, Z]
    -> (logw [B, K], nll [B, K], weights [B, K, 24, V]) as float64 arrays.  The decoder runs teacher-forced on x_b's own tokens, all
    B * K rows in one call (row b * K + k)."""
    from oracle import torch_ref as T
    P64 = {k: torch.as_tensor(v).double() for k, v in P.items()}
    tok = torch.as_tensor(tokens).long()
    e = torch.as_tensor(np.asarray(eps)).double()
    B, K, Z = e.shape
    with torch.no_grad():
        mu, ls = T.encoder_forward(P64, tok)
        z = (mu[:, None, :] + e * torch.exp(ls)[:, None, :]).reshape(B * K, Z)
        rows = tok.repeat_interleave(K, 0)
        w, _ = T.decoder_forward(P64, z, rows, True)
    d = draw(mu.numpy(), ls.numpy(), e.numpy())
    n = nll_rows(w.numpy(), rows.numpy())
    nll = n["nll"].reshape(B, K)
    return d["logr"] - nll, nll, w.numpy().reshape(B, K, w.shape[1], w.shape[2])
