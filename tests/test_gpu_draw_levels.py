"""The levels of csrc/sample.h's draw against one another, through inet_sample_temperature / _truncated / _constrained / _forced
(csrc/sample_rows.hip: sample_temperature_kernel, sample_truncated_kernel, sample_constrained_kernel and sample_forced_kernel, one kernel
per level): a level whose own step is switched off by its arguments returns the level below
bit for bit --
    level 4 with `forced` all -1                      = level 3,
    level 3 with a mask of all ones                   = level 2,
    level 2 with (top_k, top_p) = (0, 1.0)            = level 1 (tokens; level 1 has no logp) --
at the chunk edges of NV = 1, 2, 4, 8 (V = 1, 63, 64, 65, 129, 512), with exact ties, a row with a NaN (the argmax rule, logp NaN) and a
row with u = 1.0 (outside [0, 1): the argmax rule).  Each level runs its own instantiation: the four calls file four label prefixes."""
import csv
import os
import tempfile

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from inpaintnet_amd import ops

ROWS = 5
PREFIXES = ("sample_temperature ", "trunc_sample ", "cons_sample ", "force_sample ")


def inputs(V):
    """(logits [5, V] with a row stride of V + 3, uniforms [5]): small integers (exact ties, exact products with T = 0.5), a NaN in row
    2, u = 1.0 in row 3"""
    rng = np.random.default_rng(1000 + V)
    buf = torch.zeros(ROWS, V + 3)
    buf[:, :V] = torch.from_numpy(rng.integers(-3, 4, size=(ROWS, V)).astype(np.float32))
    buf[2, V // 2] = float("nan")
    u = rng.random(ROWS)
    u[3] = 1.0
    allow = rng.random((ROWS, V)) < 0.6
    allow[:, rng.integers(0, V)] = True                        # (no empty row)
    return buf.cuda()[:, :V], torch.from_numpy(u).cuda(), allow


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("V", [1, 63, 64, 65, 129, 512])
def test_a_level_switched_off_is_the_level_below(V):
    w, u, allow = inputs(V)
    assert w.stride(0) > V
    T, k, p = 0.5, 3, 0.7
    mask = ops.pack_allowed(allow).cuda()
    ones = ops.pack_allowed(np.ones((ROWS, V), dtype=bool)).cuda()
    free = torch.full((ROWS,), -1, dtype=torch.int32, device="cuda")

    ops.prof_enable(True)
    try:
        t1 = ops.sample_temperature(w, T, u)
        t2, l2 = ops.sample_truncated(w, T, u, k, p)
        t3, l3 = ops.sample_truncated(w, T, u, k, p, allowed=mask)
        t4, l4 = ops.sample_truncated(w, T, u, k, p, allowed=mask, forced=free)
        torch.cuda.synchronize()
        launches = ops.prof_read()["hbm_pointwise"][0]
        with tempfile.TemporaryDirectory() as td:
            ops.prof_dump(os.path.join(td, "l.csv"))
            with open(os.path.join(td, "l.csv"), newline="") as f:
                labels = [r["label"] for r in csv.DictReader(f)]
    finally:
        ops.prof_enable(False)
    # four launches, one per level, each under its own prefix
    assert launches == 4 and len(labels) == 4, (launches, labels)
    assert all(l.startswith(q) for l, q in zip(labels, PREFIXES)), labels

    assert torch.equal(t4, t3) and same_bits(l4, l3), (V, t4.tolist(), t3.tolist(), l4.tolist(), l3.tolist())
    t3o, l3o = ops.sample_truncated(w, T, u, k, p, allowed=ones)
    assert torch.equal(t3o, t2) and same_bits(l3o, l2), (V, t3o.tolist(), t2.tolist(), l3o.tolist(), l2.tolist())
    t2o, _ = ops.sample_truncated(w, T, u, 0, 1.0)
    assert torch.equal(t2o, t1), (V, t2o.tolist(), t1.tolist())

    # the rows outside the rule took the argmax rule (logp NaN), the others drew (logp finite or -inf never: a drawn token has mass)
    for lp in (l2, l3, l4):
        lp = lp.cpu().numpy()
        assert np.isnan(lp[[2, 3]]).all() and np.isfinite(lp[[0, 1, 4]]).all(), (V, lp)
    a = allow.copy()
    for tok, ok in ((t1, None), (t2, None), (t3, a), (t4, a)):
        tok = tok.cpu().numpy()
        assert tok.min() >= 0 and tok.max() < V
        if ok is not None:
            assert ok[np.arange(ROWS), tok].all(), (V, tok)
