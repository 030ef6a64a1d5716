"""Plain references for the helper kernels of csrc/pointwise.hip, ce.hip, latent.hip, optim.hip and sample_rows.hip, shared by tests/test_pointwise_host.py (CPU) and
tests/test_gpu_pointwise.py (GPU): the counter-based generator mirrored in numpy uint64, everything else in float64.

Nothing here imports the library: a reference that called the code under test would prove nothing."""
import numpy as np
import torch

_U64 = np.uint64
_MASK64 = (1 << 64) - 1


def _u64(x):
    """Python int (any sign, any size) or array -> numpy uint64, modulo 2^64."""
    if isinstance(x, np.ndarray):
        return x.astype(np.uint64)
    return _U64(int(x) & _MASK64)


def mix64(x):
    """csrc/sample_rows.hip mix64 (the splitmix64 finaliser) on uint64 scalars or arrays; wraps modulo 2^64."""
    with np.errstate(over="ignore"):
        x = _u64(x) + _U64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> _U64(30))) * _U64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> _U64(27))) * _U64(0x94D049BB133111EB)
        return x ^ (x >> _U64(31))


def unmix64(h):
    """The inverse of mix64 (a bijection of 64-bit words), on Python ints: the counter whose hash is `h`.  Lets a test AIM a stream
    element at a chosen hash, e.g. one whose high word equals a dropout threshold."""
    M = _MASK64
    h = int(h) & M
    h ^= (h >> 31) ^ (h >> 62)
    h = (h * pow(0x94D049BB133111EB, -1, 1 << 64)) & M
    h ^= (h >> 27) ^ (h >> 54)
    h = (h * pow(0xBF58476D1CE4E5B9, -1, 1 << 64)) & M
    h ^= (h >> 30) ^ (h >> 60)
    return (h - 0x9E3779B97F4A7C15) & M


def dropout_threshold(p):
    """uint32(double(float32(p)) * 2^32): an element is kept when the high word of its hash is >= this."""
    return int(float(np.float32(p)) * 4294967296.0)


def offset_with_hash(seed, h):
    """The stream offset whose element 0 has hash h under `seed`."""
    return unmix64(h) ^ int(mix64(seed))


def _stream(n, seed, offset):
    """h[i] = mix64(mix64(seed) ^ (offset + i)), i < n, with offset + i modulo 2^64."""
    with np.errstate(over="ignore"):
        ctr = _u64(offset) + np.arange(int(n), dtype=np.uint64)
        return mix64(mix64(seed) ^ ctr)


def dropout_keep_value(p):
    """What a kept element holds: float32(1) / (float32(1) - float32(p))."""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def dropout_mask_ref(n, p, seed, offset):
    """inet_dropout_mask: out[i] = keep ? 1/(1-p) : 0 with keep = (high 32 bits of h[i]) >= uint32(double(float32(p)) * 2^32)."""
    p32 = np.float32(p)
    thr = np.uint32(int(float(p32) * 4294967296.0))
    keep = (_stream(n, seed, offset) >> _U64(32)).astype(np.uint32) >= thr
    return np.where(keep, dropout_keep_value(p), np.float32(0.0)).astype(np.float32)


def uniform24_ref(seed, counter):
    """The 24-bit numerator k of the uniform u = k / 2^24 that inet_sample_multinomial draws for the row whose counter
    (offset + row) is `counter` (scalar or uint64 array)."""
    with np.errstate(over="ignore"):
        h = mix64(mix64(seed) ^ _u64(counter))
    return (h >> _U64(40)).astype(np.uint32) if isinstance(h, np.ndarray) else int(h >> _U64(40))


# ------------------------------------------------------------------------------- float64 references
def argmax_first(w):
    """np.argmax per row: a NaN is the maximum, the lowest index wins among equals (Tensor.max(1) / np.argmax)."""
    return torch.from_numpy(np.argmax(torch.as_tensor(w).detach().cpu().double().numpy(), axis=1).astype(np.int64))


def cross_entropy_ref(w, tgt, scale=1.0):
    """w [rows, V] (any float dtype), tgt [rows] -> (loss sum, #rows whose argmax_first is the target,
    (softmax - onehot) * scale), all float64."""
    w = torch.as_tensor(w).detach().cpu().double()
    tgt = torch.as_tensor(tgt).cpu().long()
    lse = torch.logsumexp(w, dim=1)
    loss = (lse - w.gather(1, tgt[:, None])[:, 0]).sum()
    correct = float((argmax_first(w) == tgt).sum())
    dW = torch.softmax(w, dim=1)
    dW[torch.arange(w.shape[0]), tgt] -= 1.0
    return float(loss), correct, dW * float(scale)


def reparam_kl_ref(mu, ls, eps=None):
    """-> z = mu + eps * exp(ls) (eps None: z = mu), sigma = exp(ls), kl = sum 0.5 (sigma^2 + mu^2 - 1) - ls."""
    mu, ls = mu.detach().cpu().double(), ls.detach().cpu().double()
    sigma = ls.exp()
    z = mu if eps is None else mu + eps.detach().cpu().double() * sigma
    kl = (0.5 * (sigma * sigma + mu * mu - 1.0) - ls).sum()
    return z, sigma, float(kl)


def latent_bwd_ref(dz, mu, ls, eps, k):
    """Gradients of (mu, ls) of  sum(dz * z) + k * kl  by autograd in float64 (dz None: the KL term alone; eps None: z = mu)."""
    mu = mu.detach().cpu().double().requires_grad_(True)
    ls = ls.detach().cpu().double().requires_grad_(True)
    sigma = ls.exp()
    total = float(k) * (0.5 * (sigma * sigma + mu * mu - 1.0) - ls).sum()
    if dz is not None:
        z = mu if eps is None else mu + eps.detach().cpu().double() * sigma
        total = total + (dz.detach().cpu().double() * z).sum()
    total.backward()
    return mu.grad, ls.grad


def adam_ref(p, g, m, v, lr, step, b1=0.9, b2=0.999, eps=1e-8, gscale=1.0):
    """torch.optim.Adam, single-tensor form, in float64:  m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2;
    p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps).  The hyper-parameters are rounded to float32 first: the ABI takes them
    as `float`, so those are the values the step was asked to use (1 - float32(0.999) differs from 0.001 by 1.3e-5 of itself)."""
    lr, b1, b2, eps, gscale = (float(np.float32(x)) for x in (lr, b1, b2, eps, gscale))
    p, g, m, v = (t.detach().cpu().double() for t in (p, g, m, v))
    g = g * gscale
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    p = p - (lr / bc1) * (m / (v.sqrt() / np.sqrt(bc2) + eps))
    return p, m, v


def index_add_ref(dtable, idx, dout, row_scale=None, absolute=False):
    """dtable + sum over rows r of dout[r] * row_scale[r] landing on row idx[r], float64.  absolute=True: the sum of the
    terms' absolute values instead (dtable included): the scale of any summation order's rounding error."""
    t = dtable.detach().cpu().double().clone()
    d = dout.detach().cpu().double()
    if row_scale is not None:
        d = d * row_scale.detach().cpu().double()[:, None]
    if absolute:
        t, d = t.abs(), d.abs()
    return t.index_add_(0, idx.detach().cpu().long().reshape(-1), d)


def colsum_ref(x, out0=None):
    """(out0 +) sum over rows of x, float64."""
    x = x.detach().cpu().double()
    o = torch.zeros(x.shape[1], dtype=torch.float64) if out0 is None else out0.detach().cpu().double()
    return o + x.sum(0)
