"""The float64 restatement of the clipping rule of inet_adam_step_clip (include/inpaintnet_hip.h), shared by
tests/test_clip_host.py (CPU) and tests/test_gpu_grad_clip.py (GPU).  Built on tests.pointwise_ref.adam_ref.

Nothing here imports the library: a reference that called the code under test would prove nothing."""
import math

import numpy as np
import torch

from tests import pointwise_ref as R


def sqnorm_ref(g):
    """S = sum g_i^2: the squares exact (a float32 squared fits float64: 24 x 24 bits in 53), the sum by math.fsum -- the correctly
    rounded value of the exact sum, whatever the order.  An inf or NaN element gives inf or NaN."""
    sq = torch.as_tensor(g).detach().cpu().double().reshape(-1).numpy() ** 2
    if not np.isfinite(sq).all():
        return float(sq.sum())                       # (fsum raises on inf - inf style inputs; the plain sum propagates)
    return math.fsum(sq.tolist())


def norm_ref(g, gscale=1.0):
    """norm = |gscale| * sqrt(S), gscale rounded to float32 first as the ABI takes it."""
    return abs(float(np.float32(gscale))) * math.sqrt(sqnorm_ref(g))


def clip_decision(g, max_norm, gscale=1.0):
    """-> (norm, nonfinite, clipped, scale): steps 1-3 of the rule.  scale is the float32 the kernel multiplies gscale by."""
    max_norm = float(np.float32(max_norm))
    assert max_norm > 0.0
    norm = norm_ref(g, gscale)
    if not math.isfinite(norm):
        return norm, True, False, 1.0
    c = max_norm / (norm + 1e-6)
    return norm, False, c < 1.0, float(np.float32(c)) if c < 1.0 else 1.0


def adam_clip_ref(p, g, m, v, lr, step, max_norm, b1=0.9, b2=0.999, eps=1e-8, gscale=1.0, skip=False, round_scale=True):
    """-> (p, m, v in float64, report words [executed, skipped, 0, 0, clipped, nonfinite], norm): steps 4-6 of the rule.  The applied
    step is adam_ref with gscale replaced by the ONE float32 product gscale * scale.

    round_scale=False leaves out the rule's two float32 roundings (scale = (float)c and the product): the coefficient stays the
    float64 c, which is what torch.nn.utils.clip_grad_norm_ applies to float64 gradients (tests/test_clip_host.py compares the two)."""
    same = tuple(t.detach().cpu().double() for t in (p, m, v))
    norm, nonfinite, clipped, scale = clip_decision(g, max_norm, gscale)
    if skip:
        return same + ([1, 1, 0, 0, 0, 0], norm)
    if nonfinite:
        return same + ([1, 0, 0, 0, 0, 1], norm)
    if round_scale:
        gs = float(np.float32(gscale) * np.float32(scale))
    else:
        gs = float(np.float32(gscale)) * (float(np.float32(max_norm)) / (norm + 1e-6) if clipped else 1.0)
    return _adam64(p, g, m, v, lr, step, b1, b2, eps, gs) + ([1, 0, 0, 0, int(clipped), 0], norm)


def _adam64(p, g, m, v, lr, step, b1, b2, eps, gs):
    """adam_ref with a gradient scale that is NOT rounded to float32 again (adam_ref rounds its gscale argument: a no-op for the float32
    product of the rule, a rounding too many for the float64 coefficient of round_scale=False): the scale goes into the gradient."""
    return R.adam_ref(p, g.detach().cpu().double() * gs, m, v, lr, step, b1, b2, eps, gscale=1.0)
