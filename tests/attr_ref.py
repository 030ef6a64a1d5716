"""The float64 restatement of the attribute regularisation (include/inpaintnet_hip.h inet_measure_attrs / inet_attr_reg, DESIGN.md
section 27): the four extractors in numpy, the loss as ONE torch expression with its gradient from autograd, the pair counts -- and
the error bounds of the float32 kernels, derived here.  Shared by tests/test_attr_host.py (CPU) and tests/test_gpu_attr_kernels.py /
tests/test_gpu_attr_trainer.py (GPU).

Nothing here imports the library or the package's own AttributeSpec: a reference that called the code under test would prove nothing.
The gradient is autograd's, of L1Loss(tanh(delta D_z), sign(D_a)) as written -- not the closed form the kernel implements.

The rule.  x = z[:, dims[a]], D_z[i, j] = x_i - x_j, D_a[i, j] = attrs[i, a] - attrs[j, a];  t = tanh(delta D_z), s = sign(D_a);
  L_a = mean_ij |t - s| (diagonal included: it adds 0);  value = coeff sum_a L_a.
  delta crosses the C-ABI as a float: the restatement uses that float.  coeff crosses as a double.

The bounds, with u = 2^-24 (the unit roundoff of float32); first-order terms, SLACK = 1.01 covers the higher orders.

One pair.  d = fl(x_i - x_j) errs by u |d|, the argument fl(delta d) by another u: |dx| <= 2 u |x|, x = delta d, which moves tanh by
  tanh'(x) |dx| = (1 - t^2) 2 u |x|.  The kernel calls tanhf, the device library's; the library is built to the OpenCL limits, which
  give tanh 5 ulp = TANH_U u = 10 u:
      |t^ - t| <= E_t = (TANH_U |t| + 2 |x| (1 - t^2)) u
  w = fl(t^ - s) (s is -1, 0 or 1, exact: the sign of a float difference is the sign of the exact difference):
      | |w^| - |t - s| | <= E_t + u |t - s|
A sum S_a = sum_ij |t - s|.  Per workgroup and thread: the 16 values of a tile in a tree (4 levels), onto the thread's running share
  (one addition per tile: NT = ceil(B / 256)), the xor tree over the 64 lanes (6), the four waves in order (3); the finishing
  workgroup: a chain over ceil(NB / 256) workspace rows (NB = ceil(B / 16)), the xor tree (6), the four waves (3).  Any fixed order
  errs by at most depth u sum|terms| (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2):
      |S^ - S| <= bS = sum_pairs (E_t + u |t - s|) + DEPTH_S u S,   DEPTH_S = 4 + NT + 9 + ceil(NB / 256) + 9
  L_a and the value are formed in double from the float sums and rounded once each:
      per_bound_a = bS_a / B^2 + u L_a;   value_bound = |coeff| sum_a bS_a / B^2 + u |value|
The gradient.  G_ia = gcoef sum_j sgn(t - s) (1 - t^2), gcoef = (float)(2 coeff delta / B^2) (within u of the exact product).
  q = fma(-t^, t^, 1) has one rounding (u q) and inherits 2 |t| E_t from t^.  sgn(t^ - s) differs from sgn(t - s) only where t^ has
  rounded to s = +-1, and there 1 - t^2 <= 2 E_t is what is lost: inside the same term.  A term enters the thread's chain over the
  tiles (NT), the xor tree (6), the four waves (3), the product with gcoef (1), and gcoef's own rounding (1):
      DEPTH_G = NT + 11
      grad_bound_ia = |gcoef| sum_j (2 |t| E_t + u (1 - t^2) + DEPTH_G u (1 - t^2) [t != s])"""
import functools

import numpy as np
import torch

U = 2.0 ** -24
TANH_U = 10                    # tanhf: 5 ulp allowed = 10 u
LOG_ULP = 2                    # logf of the extractor: 2 ulp (the issue's figure)
SLACK = 1.01
COLUMNS = ("num_notes", "note_range", "rhy_entropy", "beat_strength")
COUNTS = ("concordant", "discordant", "tied")

# the launcher's constants (csrc/attr.hip): rows of a workgroup's block, columns of a tile, threads of the finishing workgroup,
# rows of a workgroup of the extractor, the most ticks it stages, the most dimensions of a call
ROWS, TILE, FINISH, MEASURE_ROWS, MAX_T, MAX_A = 16, 256, 256, 64, 96, 8


def f32(v):
    return float(np.float32(v))


def cdiv(a, b):
    return -(-a // b)


# ============================================================================================ the extractors
# the vocabulary of the tests: the reference's symbols, then pitches by music21's names with their MIDI numbers written out by hand
VOCAB = ("__", "rest", None, "START", "END", "G3", "A3", "B-3", "C4", "C#4", "D4", "E-4", "F#4", "G4", "A4", "B4", "C5", "E5", "G5", "C6")
VOCAB_MIDI = (-1, -1, -1, -1, -1, 55, 57, 58, 60, 61, 62, 63, 66, 67, 69, 71, 72, 76, 79, 84)
SPEC = dict(num_tokens=len(VOCAB), slur_index=0, rest_index=1, none_index=2, midi=VOCAB_MIDI, pitch_range=(55, 84))
BEAT_WEIGHTS_MILLI = (1000, 8, 8, 150, 8, 8)


def measure_attrs(tokens, num_tokens, slur_index, rest_index, none_index, midi, pitch_range=(55, 84)):
    """tokens [B, T] ints -> float64 [B, 4], the columns COLUMNS: each one operation on one exact integer.  A row with a token outside
    [0, num_tokens) is NaN."""
    tokens = np.asarray(tokens)
    B, T = tokens.shape
    assert T > 0 and T % 6 == 0
    lo, hi = pitch_range
    out = np.zeros((B, 4), np.float64)
    for b in range(B):
        row = tokens[b]
        if ((row < 0) | (row >= num_tokens)).any():
            out[b] = np.nan
            continue
        onset = row != slur_index
        pitches = [midi[k] for k in row if k not in (slur_index, rest_index, none_index) and midi[k] >= 0]
        n = int(onset.sum())
        milli = sum(BEAT_WEIGHTS_MILLI[t % 6] for t in range(T) if onset[t])
        out[b, 0] = (T - int((row == slur_index).sum()) - int((row == rest_index).sum())) / T
        out[b, 1] = (max(pitches) - min(pitches)) / (hi - lo) if pitches else 0.0
        out[b, 2] = np.log(n) if n > 0 else 0.0
        out[b, 3] = milli / 1000
    return out


def draw_tokens(tag, B, T, spec=SPEC, p_slur=0.4, p_rest=0.1):
    """[B, T] int64: the slur with probability 0.4, the rest with 0.1, else uniform over the other symbols."""
    from inpaintnet_amd import synthetic
    u = synthetic.det_uniform(f"attr/{tag}/u", (B, T), 0.0, 1.0)
    others = np.array([k for k in range(spec["num_tokens"]) if k not in (spec["slur_index"], spec["rest_index"])])
    tok = others[synthetic.det_tokens(f"attr/{tag}/k", (B, T), len(others))]
    tok = np.where(u < p_slur, spec["slur_index"], np.where(u < p_slur + p_rest, spec["rest_index"], tok))
    return tok.astype(np.int64)


def edge_rows(T, spec=SPEC):
    """name -> a row of T tokens: what the extractors must not get wrong."""
    slur, rest, none = spec["slur_index"], spec["rest_index"], spec["none_index"]
    g3, c6 = VOCAB.index("G3"), VOCAB.index("C6")
    rows = {
        "all_slur": [slur] * T,
        "all_rest": [rest] * T,
        "no_pitch": ([VOCAB.index("START"), none, rest, slur, VOCAB.index("END"), rest] * T)[:T],
        "one_pitch": ([VOCAB.index("D4"), slur, slur, rest, slur, slur] * T)[:T],
        "full_range": ([g3, slur, rest, c6, none, slur] * T)[:T],
    }
    return {k: np.array(v, np.int64) for k, v in rows.items()}


# ============================================================================================ the loss
def depth_s(B):
    return 4 + cdiv(B, TILE) + 9 + cdiv(cdiv(B, ROWS), FINISH) + 9


def depth_g(B):
    return cdiv(B, TILE) + 11


def loss_autograd(z, dims, attrs, delta, coeff, dtype=torch.float64):
    """The value as ONE torch expression, L1Loss(tanh(delta D_z), sign(D_a)) summed over the attributes, with autograd.
    -> (value, per_attr [A], grad [B, A] = d value / d z[:, dims])."""
    zt = torch.from_numpy(np.asarray(z)).to(dtype).requires_grad_(True)
    at = torch.from_numpy(np.asarray(attrs)).to(dtype)
    per = []
    for a, r in enumerate(dims):
        x = zt[:, r]
        Dz = x[:, None] - x[None, :]
        Da = at[:, a][:, None] - at[:, a][None, :]
        per.append(torch.nn.L1Loss()(torch.tanh(f32(delta) * Dz), torch.sign(Da)))
    value = float(coeff) * torch.stack(per).sum()
    value.backward()
    return float(value.detach()), np.array([float(p.detach()) for p in per]), zt.grad[:, list(dims)].double().numpy()


def pair_counts(z, dims, attrs):
    """[A, 3] ints over ordered pairs i != j: concordant, discordant, attribute-tied."""
    z, attrs = np.asarray(z, np.float64), np.asarray(attrs, np.float64)
    B = z.shape[0]
    off = ~np.eye(B, dtype=bool)
    out = np.zeros((len(dims), 3), np.int64)
    for a, r in enumerate(dims):
        sz = np.sign(z[:, r][:, None] - z[:, r][None, :])
        sa = np.sign(attrs[:, a][:, None] - attrs[:, a][None, :])
        out[a] = [int((off & (sa != 0) & (sz == sa)).sum()), int((off & (sa != 0) & (sz == -sa)).sum()), int((off & (sa == 0)).sum())]
    return out


def evaluate(z, dims, attrs, delta, coeff):
    """-> dict(value, per_attr [A], grad [B, A] (autograd, float64), counts [A, 3], value_bound, per_bound [A], grad_bound [B, A],
    scale = |coeff| sum_a L_a (every term is >= 0: the value's own magnitude), untied = the share of off-diagonal pairs whose
    attributes differ, per attribute)."""
    z, attrs = np.asarray(z, np.float32), np.asarray(attrs, np.float32)
    B = z.shape[0]
    d32, co = f32(delta), float(coeff)
    value, per, grad = loss_autograd(z, dims, attrs, d32, co)
    counts = pair_counts(z, dims, attrs)
    gcoef = abs(f32(2.0 * co * d32 / (B * B)))
    per_bound, grad_bound = np.zeros(len(dims)), np.zeros((B, len(dims)))
    for a, r in enumerate(dims):
        x = z[:, r].astype(np.float64)
        ax = attrs[:, a].astype(np.float64)
        X = d32 * (x[:, None] - x[None, :])
        t = np.tanh(X)
        s = np.sign(ax[:, None] - ax[None, :])
        q = 1.0 - t * t
        Et = (TANH_U * np.abs(t) + 2.0 * np.abs(X) * q) * U
        v = np.abs(t - s)
        bS = (Et + U * v).sum() + depth_s(B) * U * v.sum()
        per_bound[a] = SLACK * bS / (B * B) + U * per[a]
        grad_bound[:, a] = SLACK * gcoef * (2.0 * np.abs(t) * Et + U * q + depth_g(B) * U * q * (t != s)).sum(1)
    off = max(B * (B - 1), 1)
    return dict(B=B, value=value, per_attr=per, grad=grad, counts=counts, per_bound=per_bound, grad_bound=grad_bound,
                value_bound=abs(co) * float((per_bound - U * per).sum()) + U * abs(value), scale=abs(co) * float(per.sum()),
                untied=(counts[:, 0] + counts[:, 1] + (off - counts.sum(1))) / off)


# ---- the cases of tests/test_gpu_attr_kernels.py, checked on the CPU by tests/test_attr_host.py: (B, Z, A, kind)
# B: one row; two; one below, at and above half a row block (8) and a whole one (16); two blocks and a row; a full tile, a tile and a
# row, a ragged second tile.  Z: 1, 3, 256.  A: 1, 4, 8.  kind 'cont': continuous attributes; 'tied': iid integers 0..5.
CASES = [(1, 1, 1, "cont"), (2, 3, 1, "cont"), (7, 3, 1, "cont"), (8, 256, 4, "cont"), (9, 256, 8, "cont"), (15, 3, 1, "cont"),
         (16, 256, 4, "cont"), (17, 256, 8, "cont"), (33, 1, 1, "cont"), (256, 256, 4, "cont"), (257, 256, 8, "cont"),
         (300, 256, 4, "cont"), (300, 3, 1, "cont"), (9, 3, 1, "tied"), (257, 256, 4, "tied"), (300, 256, 8, "tied")]
DELTAS, COEFFS = (1.0, 10.0), (1.0, 10.0)


def dims_for(Z, A):
    """A distinct dimensions that include 0 and Z - 1 (A = 1: Z - 1, which is 0 at Z = 1), in no particular order."""
    if A == 1:
        return [Z - 1]
    rest = [d for d in (Z // 2, 1, Z - 2, 37, 100, Z // 2 + 1, 200) if 0 < d < Z - 1]
    dims = [Z - 1, 0] + list(dict.fromkeys(rest))[:A - 2]
    assert len(dims) == A and len(set(dims)) == A
    return dims


def inputs(B, Z, A, kind):
    """z = 0.5 n (float32); attrs uniform in [0, 1) ('cont') or iid integers 0..5 ('tied')."""
    from inpaintnet_amd import synthetic
    tag = f"attr/{B}x{Z}x{A}/{kind}"
    z = (0.5 * synthetic.det_normal(tag + "/z", (B, Z))).astype(np.float32)
    if kind == "cont":
        attrs = synthetic.det_uniform(tag + "/a", (B, A), 0.0, 1.0)
    else:
        attrs = synthetic.det_tokens(tag + "/a", (B, A), 6).astype(np.float32)
    return z, attrs


@functools.lru_cache(maxsize=None)
def case(B, Z, A, kind, delta=10.0, coeff=1.0):
    z, attrs = inputs(B, Z, A, kind)
    dims = dims_for(Z, A)
    return z, dims, attrs, evaluate(z, dims, attrs, delta, coeff)


# ---- the descent check: the kernel's gradient alone must sort two dimensions by two attributes
DESCENT = dict(B=32, Z=4, dims=[0, 3], delta=1.0, coeff=1.0, lr=4.0, steps=50, seeds=(0, 1, 2))


def descent_inputs(seed):
    rs = np.random.RandomState(seed)
    z = (0.1 * rs.randn(DESCENT["B"], DESCENT["Z"])).astype(np.float32)
    attrs = np.stack([rs.randint(0, 6, DESCENT["B"]) / 24, rs.randint(0, 30, DESCENT["B"]) / 29], 1).astype(np.float32)
    return z, attrs


def concordance(counts):
    c, d = np.asarray(counts, np.float64)[:, 0], np.asarray(counts, np.float64)[:, 1]
    return c / (c + d)


def descend(z, attrs, dtype, steps):
    """steps of z[:, dims] -= lr * G with the restatement's own gradient -> (z, the first step count at which both concordances were 1.0
    or None)."""
    z = np.array(z, dtype=np.float64 if dtype == torch.float64 else np.float32)
    dims, first = DESCENT["dims"], None
    for k in range(steps + 1):
        if first is None and bool((concordance(pair_counts(z, dims, attrs)) == 1.0).all()):
            first = k
        if k == steps:
            break
        G = loss_autograd(z, dims, attrs, DESCENT["delta"], DESCENT["coeff"], dtype)[2]
        z[:, dims] -= (DESCENT["lr"] * G).astype(z.dtype)
    return z, first
