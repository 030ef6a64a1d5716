"""The float64 restatement of the MMD latent loss (include/inpaintnet_hip.h inet_mmd), both kernels and the three
estimators, with its gradient from torch autograd -- and the error bounds of the float32 kernels, derived here.  Shared by
tests/test_mmd_host.py (CPU) and tests/test_gpu_mmd.py / tests/test_gpu_mmd_trainer.py (GPU).

Nothing here imports the library: a reference that called the code under test would prove nothing.  The gradient is autograd's, of
the value as written below -- not the closed form the kernel implements -- so that the kernel's formula is checked against something
that does not share it.

The rule.  x = z_tilde, y = z_prior, both [B, Z];  d(u, v) = sum_z (u_z - v_z)^2;  k = exp(-d / var) ('gaussian') or var / (var + d)
  ('imq');  S_xx = sum_ij k(x_i, x_j), S_yy = sum_pq k(y_p, y_q), S_xy = sum_pi k(y_p, x_i), diagonals included;
  value = coeff (a (S_xx - diag B) + a (S_yy - diag B) - c S_xy),  (a, c, diag) = weights(B, estimator).
  a, c, diag and coeff cross the C-ABI as doubles and var as a float: the restatement uses that float, so none carries an error.

The bounds, with u = 2^-24 (the unit roundoff of float32); first-order terms, the factor SLACK = 1.01 covers the higher orders (the
largest first-order factor here is below 1e-4).

A distance.  e = fl(u_z - v_z) errs by u |e|, so e^2 by 2u e^2; the kernel adds the squares in ascending z, one fused multiply-add
  each (one rounding per step; unfused there would be two -- the bound allows them): a term passes through at most Z additions.
      |d^ - d| <= DIST(Z) u d,   DIST(Z) = Z + 2          (all terms are >= 0: the sum of magnitudes IS d; d(u, u) = 0 exactly)
A kernel value.  The kernel calls expf, the device library's single-precision exp (NOT the hardware approximation __expf), taken
  at 2 ulp = EXP_U u = 4 u.
  gaussian: t = fl(-d^ / var) errs by (DIST + 1) u d / var in absolute terms, which is the RELATIVE error it causes in exp(t):
      |k^ - k| <= relk k,   relk = ((DIST + 1) d / var + EXP_U) u
  imq: s = fl(var + d^) errs by DIST u d + u (var + d), the quotient adds u:
      relk = (DIST d / (var + d) + 2) u
A sum S.  Per workgroup and thread: the 8 kernel values of a tile in a tree (3 levels), onto the thread's running share (one
  addition per tile: NT = ceil(B / 256)), the xor tree over the 64 lanes (6), the four waves in order (3); the finishing workgroup: a
  chain over ceil(NB / 256) workspace rows (NB = ceil(B / 8)), the xor tree (6), the four waves (3).  Any fixed order errs by at most
  depth u sum|terms| (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2):
      |S^ - S| <= sum_pairs relk k + DEPTH_S u S,   DEPTH_S = 3 + NT + 9 + ceil(NB / 256) + 9
The value is formed in double from the three float sums and rounded once:
      value_bound = |coeff| (a bS_xx + a bS_yy + c bS_xy) + u |value|
The gradient.  G_iz = ga A_iz - gc C_iz,  A_iz = sum_j k'(d_ij) (x_iz - x_jz),  C_iz = sum_p k'(d_pi) (x_iz - y_pz),
  ga = (float)(4 coeff a), gc = (float)(2 coeff c) (each within u of the exact product).
  k' = -k / var: relw = relk + u;   k' = -k^2 / var (imq): relw = 2 relk + 2 u.
  A term fl(x - col) (u) enters a chain of 64 fused multiply-adds (its lane c % 4 of the tile), the tree (p0 + p1) + (p2 + p3) (2),
  then acc = fma(coef, tile sum, acc), one rounding per tile of x and of y (2 NT):
      DEPTH_G = 1 + 64 + 2 + 2 NT + 1 (the coefficient's own rounding)
      grad_bound_iz = |ga| sum_j |k'_ij| |x_iz - x_jz| (relw_ij + DEPTH_G u) + |gc| sum_p |k'_pi| |x_iz - y_pz| (relw_pi + DEPTH_G u)"""
import functools

import numpy as np
import torch

U = 2.0 ** -24
EXP_U = 4                      # expf: 2 ulp allowed = 4 u
SLACK = 1.01
KERNELS = ("gaussian", "imq")
ESTIMATORS = ("unbiased", "biased", "reference")

# the launcher's constants (csrc/mmd.hip): rows of a workgroup's block, columns of a tile, threads of the finishing workgroup
ROWS, TILE, FINISH = 8, 256, 256


def f32(v):
    return float(np.float32(v))


def cdiv(a, b):
    return -(-a // b)


def weights(B, estimator):
    """(a, c, diag), the doubles that cross the ABI."""
    c = 2.0 / (B * B)
    if estimator == "unbiased":
        assert B >= 2
        return 1.0 / (B * (B - 1)), c, 1.0
    if estimator == "biased":
        return 1.0 / (B * B), c, 0.0
    assert estimator == "reference"
    return (1.0 / (B * (B - 1)) / 2 if B > 1 else 1.0), c, 0.0


def dist_u(Z):
    return Z + 2


def depth_s(B):
    return 3 + cdiv(B, TILE) + 9 + cdiv(cdiv(B, ROWS), FINISH) + 9


def depth_g(B):
    return 1 + 64 + 2 + 2 * cdiv(B, TILE) + 1


def _kernel(d, kind, var):
    return torch.exp(-d / var) if kind == "gaussian" else var / (var + d)


def _pair(rows, cols, kind, var, Z, B, grad_of=None):
    """One of the three sums, 32 rows of `rows` at a time (the B x B x Z differences never exist at once).  -> (S, bS without the
    depth term, dS / d grad_of from autograd or None, sum_j |k'| |row_z - col_z| (relw + DEPTH_G u) per row element)."""
    S, eS = 0.0, 0.0
    g = None if grad_of is None else torch.zeros_like(grad_of)
    gb = torch.zeros_like(rows)
    for i0 in range(0, rows.shape[0], 32):
        diff = rows[i0:i0 + 32, None, :] - cols[None, :, :]
        d = (diff * diff).sum(2)
        k = _kernel(d, kind, var)
        s = k.sum()
        if grad_of is not None:
            g += torch.autograd.grad(s, grad_of)[0]
        with torch.no_grad():
            dd, kk = d.detach(), k.detach()
            if kind == "gaussian":
                relk = ((dist_u(Z) + 1) * dd / var + EXP_U) * U
                w, relw = kk / var, relk + U
            else:
                relk = (dist_u(Z) * dd / (var + dd) + 2) * U
                w, relw = kk * kk / var, 2 * relk + 2 * U
            S += float(s)
            eS += float((kk * relk).sum())
            gb[i0:i0 + 32] = torch.einsum("ij,ijz->iz", w * (relw + depth_g(B) * U), diff.detach().abs())
    return S, eS, g, gb


@functools.lru_cache(maxsize=None)
def _sums_cached(key, kind, var):
    x, y = _INPUTS[key]
    return _sums(x, y, kind, var)


def _sums(x, y, kind, var):
    """Everything that depends on (x, y, kernel, var) alone, in float64: the sums, dS_xx / dx and dS_xy / dx from autograd, the
    bounds' parts.  var is the ABI's float."""
    var = f32(var)
    B, Z = x.shape
    xt = torch.from_numpy(np.asarray(x, np.float64)).requires_grad_(True)
    yt = torch.from_numpy(np.asarray(y, np.float64))
    Sxx, exx, gxx, gbA = _pair(xt, xt, kind, var, Z, B, grad_of=xt)
    Sxy, exy, gxy, gbC = _pair(xt, yt, kind, var, Z, B, grad_of=xt)
    Syy, eyy, _, _ = _pair(yt, yt, kind, var, Z, B)
    dep = depth_s(B) * U
    return dict(B=B, Z=Z, S_xx=Sxx, S_yy=Syy, S_xy=Sxy, offdiag_share=(Sxx - B) / Sxx,         # (the diagonal: B times k(0) = 1)
                bS_xx=SLACK * (exx + dep * Sxx), bS_yy=SLACK * (eyy + dep * Syy), bS_xy=SLACK * (exy + dep * Sxy),
                dS_xx=gxx.numpy(), dS_xy=gxy.numpy(), gbA=SLACK * gbA.detach().numpy(), gbC=SLACK * gbC.detach().numpy())


_INPUTS = {}


def evaluate(x, y, kind, var, estimator, coeff=1.0, key=None):
    """-> dict(value, S_xx, S_yy, S_xy, grad [B, Z] (autograd, float64), offdiag_share, value_bound, S bounds, grad_bound [B, Z],
    scale = |coeff| (a S_xx + a S_yy + c S_xy)).  key: a name under which (x, y) are remembered, so that the sums of one input are
    computed once for all estimators."""
    if key is not None:
        _INPUTS.setdefault(key, (x, y))
        s = _sums_cached(key, kind, f32(var))
    else:
        s = _sums(x, y, kind, var)
    B = s["B"]
    a, c, diag = weights(B, estimator)
    co = float(coeff)
    value = co * (a * (s["S_xx"] - diag * B) + a * (s["S_yy"] - diag * B) - c * s["S_xy"])
    # autograd's gradient of the value: the value is linear in the sums
    grad = co * (a * s["dS_xx"] - c * s["dS_xy"])
    ga, gc = abs(f32(4.0 * co * a)), abs(f32(2.0 * co * c))
    out = dict(s)
    out.update(value=value, grad=grad, a=a, c=c, diag=diag,
               value_bound=abs(co) * (a * s["bS_xx"] + a * s["bS_yy"] + c * s["bS_xy"]) + U * abs(value),
               scale=abs(co) * (a * s["S_xx"] + a * s["S_yy"] + c * s["S_xy"]),
               grad_bound=ga * s["gbA"] + gc * s["gbC"])
    return out


def value_autograd(x, y, kind, var, estimator, coeff=1.0):
    """The value written out whole in float64 torch with ONE backward through it (small shapes only: B x B x Z at once): what
    evaluate() must reproduce.  -> (value, grad)."""
    B = x.shape[0]
    a, c, diag = weights(B, estimator)
    xt = torch.from_numpy(np.asarray(x, np.float64)).requires_grad_(True)
    yt = torch.from_numpy(np.asarray(y, np.float64))

    def S(p, q):
        return _kernel(((p[:, None, :] - q[None, :, :]) ** 2).sum(2), kind, f32(var)).sum()
    value = float(coeff) * (a * (S(xt, xt) - diag * B) + a * (S(yt, yt) - diag * B) - c * S(yt, xt))
    value.backward()
    return float(value.detach()), xt.grad.numpy()


# ---- the cases of tests/test_gpu_mmd.py, checked on the CPU by tests/test_mmd_host.py
# (B, Z, var or None = 2 Z).  (17, 33): one row past two row blocks, one latent dimension past a chunk of Z.  (65, 257): one dimension
# past the 256 a workgroup's gradient registers span.  (300, 256): a second column tile, ragged.  (37, 16, 16.0): the reference's var.
CASES = [(1, 1, None), (1, 256, None), (2, 5, None), (3, 5, None), (37, 16, None), (37, 16, 16.0), (37, 64, None), (64, 63, None),
         (65, 257, None), (256, 256, None), (300, 256, None), (2 * ROWS + 1, 33, None)]


def inputs(B, Z):
    """x = 0.6 n + 0.2, y = n' (float32), the golden file's inputs for the shapes it holds."""
    from inpaintnet_amd import synthetic
    tag = f"mmd/{B}x{Z}"
    x = (0.6 * synthetic.det_normal(tag + "/x", (B, Z)) + 0.2).astype(np.float32)
    y = synthetic.det_normal(tag + "/y", (B, Z)).astype(np.float32)
    return x, y


def case(B, Z, var, kind, estimator, coeff=1.0):
    x, y = inputs(B, Z)
    v = 2.0 * Z if var is None else var
    return x, y, v, evaluate(x, y, kind, v, estimator, coeff, key=(B, Z))
