"""The float64 restatement of the rule of inet_adam_step_w (include/inpaintnet_hip.h): the optimizer step with
decoupled weight decay and EMA shadow weights, shared by tests/test_adamw_host.py (CPU) and tests/test_gpu_adamw_ema.py (GPU).  Built
on tests.pointwise_ref.adam_ref and tests.clip_ref.

Nothing here imports the library: a reference that called the code under test would prove nothing."""
import numpy as np
import torch

from tests import clip_ref as CR
from tests import pointwise_ref as R


def f32(x):
    return float(np.float32(x))


def decay_factor(lr, weight_decay, rounded=True):
    """decay = (float)(1.0 - (double)lr * (double)weight_decay), lr and weight_decay rounded to float32 first as the ABI takes them.
    rounded=False leaves the last rounding out: 1 - lr * wd in float64, which is what torch.optim.AdamW multiplies by."""
    d = 1.0 - f32(lr) * f32(weight_decay)
    return f32(d) if rounded else d


def one_minus(ema_decay):
    """omd = (float)(1.0 - (double)ema_decay), ema_decay rounded to float32 first."""
    return f32(1.0 - f32(ema_decay))


def warmup_decay(ema_decay, t):
    """The decay the trainer passes to the launch with step number t under ema_warmup."""
    return min(ema_decay, (1.0 + t) / (10.0 + t))


def mask_from_ranges(n, ranges):
    """The bool vector of the elements that decay: [start, stop) ranges, clipped to n."""
    mask = torch.zeros(n, dtype=torch.bool)
    for a, b in ranges:
        mask[min(a, n):min(b, n)] = True
    return mask


def adamw_ref(p, g, m, v, lr, step, weight_decay=0.0, mask=None, ema=None, ema_decay=0.0, max_norm=None, b1=0.9, b2=0.999,
              eps=1e-8, gscale=1.0, skip=False, round_decay=True):
    """-> (p, m, v, ema in float64 -- ema None if none was given --, the EIGHT report words without word 2, norm or None).
    max_norm None: no partials, only `skip` skips (adam_ref); else steps 1-6 of the clipping rule (clip_ref.adam_clip_ref).
    mask: a bool vector (None: every element decays).  An applied step: m, v as adam_ref; p1 = p * decay where the mask says so;
    p_new = p1 - update; e_new = ema_decay * e + omd * p_new.  A skipped or dropped step leaves all four alone."""
    p64, m64, v64 = (t.detach().cpu().double() for t in (p, m, v))
    e64 = None if ema is None else ema.detach().cpu().double()
    rep, norm, gs = [1, 0, 0, 0, 0, 0, 0, 0], None, f32(gscale)
    if max_norm is not None:
        norm, nonfinite, clipped, scale = CR.clip_decision(g, max_norm, gscale)
        if not skip:
            rep[4], rep[5] = int(clipped), int(nonfinite)
            gs = float(np.float32(gscale) * np.float32(scale))
        if nonfinite and not skip:
            return p64, m64, v64, e64, rep, norm
    if skip:
        rep[1] = 1
        return p64, m64, v64, e64, rep, norm
    decay = decay_factor(lr, weight_decay, round_decay)
    p1 = p64 * decay if mask is None else torch.where(mask, p64 * decay, p64)
    # adam_ref's update is p - u: apply it to p1 (the step itself does not read p)
    pn, mn, vn = R.adam_ref(p1, g.detach().cpu().double() * gs, m64, v64, lr, step, b1, b2, eps, gscale=1.0)
    if e64 is not None:
        e64 = f32(ema_decay) * e64 + one_minus(ema_decay) * pn
    return pn, mn, vn, e64, rep, norm
