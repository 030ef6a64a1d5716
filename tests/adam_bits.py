"""The recorded bits of the optimizer step: the inputs, the forms, the sizes and the digest that
tools/record_adam_bits.py writes into tests/golden/adam_step_bits.json and tests/test_gpu_adam_bits.py holds the library to.

The inputs come from integer arithmetic alone -- a splitmix64 of (key, i) in numpy uint64, mapped to float32 exactly -- so they depend
on no library's random numbers, and every other factor is built from IEEE multiplications in a fixed order.  Nothing here imports the
library: the callers hand in the `ops` module they want exercised."""
import functools
import hashlib
import json
import math
import os

import numpy as np
import torch

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "adam_step_bits.json")
DEV = "cuda:0"
LR = 1e-3
# the sizes of tests/test_gpu_adamw_ema.py, each another path of the kernel: tail only; around a mask word's edge; the 16-byte body
# plus a tail of 0..3; one size past a full pass of the grid
TAIL_N = [1, 3, 4, 5]
EDGE_N = [31, 32, 33, 63, 65]
BODY_N = [4 * 10007 + k for k in range(4)]
GRID_N = 4 * 4096 * 256 + 4 * 1000 + 3
SIZES = TAIL_N + EDGE_N + BODY_N + [GRID_N]
RANGES = [(0, 5), (37, 70), (4 * 5003 + 2, 4 * 5003 + 9)]          # the decay mask of tests/test_gpu_adamw_ema.py, clipped to n
REGIMES = {"zero": None, "tiny": -40, "big": 10}                    # the gradient's power of two (tests/test_gpu_pointwise.py adam_state)
FORMS = ("adam", "clip_inf", "clip_half", "w", "w_mask", "w_ema", "w_all")
PLAIN = ("adam", "clip_inf", "clip_half")                           # the forms with nothing of weight decay or EMA switched on
WEIGHT_DECAY, EMA_DECAY = 0.01, 0.999


def combos(n):
    """The parameter combinations of one size, in the order the digest covers them."""
    if n == GRID_N:
        return [(3, 1.0, "big")]
    return [(step, gscale, regime) for step in (1, 3, 1000) for gscale in (1.0, 0.125) for regime in REGIMES]


def splitmix64(key, n):
    """h[i] = the splitmix64 finalizer of key + (i + 1) * golden, i < n, in uint64 (wrapping)."""
    with np.errstate(over="ignore"):
        z = np.uint64(key) + (np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def stream(key, n, k):
    """n float32 in [-2^(k-1), 2^(k-1)): ((h >> 40) * 2^-24 - 0.5) * 2^k, every operation exact in float32."""
    j = (splitmix64(key, n) >> np.uint64(40)).astype(np.int64)                  # 24 bits
    return ((j - (1 << 23)).astype(np.float32) * np.float32(2.0 ** -24)) * np.float32(2.0 ** k)


def _key(which, n, step, gscale, regime):
    return ((((which << 40) + n) * 1024 + step) * 2 + (0 if gscale == 1.0 else 1)) * 4 + list(REGIMES).index(regime)


def _power(b, e):
    """b^e by e IEEE multiplications in float64: no libm in the inputs."""
    x = 1.0
    for _ in range(e):
        x *= b
    return x


@functools.lru_cache(maxsize=None)                                  # (all of them: 150 MB of host memory, generated once per process)
def inputs(n, step, gscale, regime):
    """(p, g, m, v, ema) as float32 numpy arrays nobody writes to: p of order 1, a gradient of the regime, the moments `step - 1` steps
    of that gradient leave behind (v >= 0), and an EMA arena that is a stream of its own."""
    k = REGIMES[regime]
    g = np.zeros(n, dtype=np.float32) if k is None else stream(_key(1, n, step, gscale, regime), n, k)
    p = stream(_key(2, n, step, gscale, regime), n, 2)
    e = stream(_key(3, n, step, gscale, regime), n, 1)
    b1, b2 = float(np.float32(0.9)), float(np.float32(0.999))
    ge = g.astype(np.float64) * gscale
    m = ((1.0 - _power(b1, step - 1)) * ge).astype(np.float32)
    v = ((1.0 - _power(b2, step - 1)) * (ge * ge)).astype(np.float32)
    for a in (p, g, m, v, e):
        a.setflags(write=False)
    return p, g, m, v, e


def inputs_digest(n):
    h = hashlib.sha256()
    for c in combos(n):
        for a in inputs(n, *c):
            h.update(a.astype("<f4").tobytes())
    return h.hexdigest()


def half_norm(n, step, gscale, regime):
    """What the recorder stores as clip_half's max_norm: half of |gscale| * sqrt(sum g^2) in float64 (exact squares, math.fsum); 1.0
    where the gradient is zero, since max_norm must be positive (nothing clips there)."""
    g = inputs(n, step, gscale, regime)[1].astype(np.float64)
    norm = abs(float(np.float32(gscale))) * math.sqrt(math.fsum((g * g).tolist()))
    return norm / 2.0 if norm > 0.0 else 1.0


def load_fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def _pinned(words):
    return torch.zeros(words, dtype=torch.int32).pin_memory()


def digest(ops, form, n, max_norms, through_w=False):
    """The SHA-256 of one (form, n): per combination, in combos(n)'s order, the little-endian bytes of p, m, v (ema where the form
    takes one) after the step and of the report words.  max_norms: clip_half's / w_all's max_norm per combination.
    through_w: a plain form through ops.adamw_step instead of ops.adam_step / ops.adam_step_clip -- same bits, the other entry point
    (its record has eight words; `adam`'s digest covers the four the form has and the rest must be zero)."""
    assert form in FORMS and (not through_w or form in PLAIN)
    h = hashlib.sha256()
    flag = torch.zeros(2, device=DEV)
    for c, half in zip(combos(n), max_norms):
        step, gscale, _ = c
        p, g, m, v, e = (torch.tensor(a, device=DEV) for a in inputs(n, *c))
        rep = _pinned(4 if form == "adam" and not through_w else 8)
        kw = dict(gscale=gscale, step_flag=flag, report=rep)
        clip = {}
        if form in ("clip_inf", "clip_half", "w_all"):
            clip = dict(max_norm=math.inf if form == "clip_inf" else half, partials=ops.grad_sqnorm(g))
        if form == "adam" and not through_w:
            ops.adam_step(p, g, m, v, LR, step, **kw)
        elif form in PLAIN and not through_w:
            ops.adam_step_clip(p, g, m, v, LR, step, clip["max_norm"], clip["partials"], **kw)
        elif form in PLAIN:
            ops.adamw_step(p, g, m, v, LR, step, **clip, **kw)
        else:
            mask = ops.pack_decay_mask(n, [(min(a, n), min(b, n)) for a, b in RANGES]) if form in ("w_mask", "w_all") else None
            ema = dict(ema=e, ema_decay=EMA_DECAY) if form in ("w_ema", "w_all") else {}
            ops.adamw_step(p, g, m, v, LR, step, weight_decay=WEIGHT_DECAY, decay_mask=mask, **ema, **clip, **kw)
        torch.cuda.synchronize()
        words = rep.tolist()
        if form == "adam" and through_w:
            assert words[4:] == [0, 0, 0, 0], (n, c, words)
            words = words[:4]
        for t in (p, m, v) + ((e,) if form in ("w_ema", "w_all") else ()):
            h.update(t.cpu().numpy().astype("<f4").tobytes())
        h.update(np.asarray(words, dtype="<i4").tobytes())
    return h.hexdigest()
