"""The persistent LSTM chain kernels (csrc/lstm.hip lstm_chain_fwd_kernel<MS,SQ>, lstm_chain_bwd_kernel<MS,SQ>,
lstm_chain_fwd_tag_kernel<MS,4>) at every row tile and width, alone (inet_lstm_fwd / _bwd) and as the two-layer pipeline
(inet_lstm2_fwd / _bwd), against a float64 evaluation of the same recurrence (oracle.torch_ref.lstm_cell / lstm_layer with autograd):
the smallest shapes that reach each build on a chip of 256 CUs.  The ragged tails are chosen on purpose -- a last group with some,
one or no row blocks past the first exercises the min(rb0 + ms, rb_last) clamps of the contraction and the rb0 + p <= rb_last guards
of the publishing waves -- and the pipeline cases add the tagged hand-off at 32 rows per workgroup with its ring carried across
chunks, the counter hand-off with a prologue per chunk (ms4, H = 512), the minimum of two chunks, and more chunks than there are
per-chunk counter areas.

Rule for every compared tensor, the one of tests/test_gpu_gru_chain_tiles.py: with err = max |got - ref| / max |ref| against float64,
err_chain <= 2 err_base + 3e-7 and err_chain < 2e-5, where err_base is the identical call under inet_set_option(4, 0) (one launch per
step; for the pipeline the two layers one after the other, which is what a caller runs when inet_lstm2_fwd refuses), and
err_base < 1e-5.  Every run's outputs are finite, chain_status() stays 0, and its recurrent launches are exactly those that
inet_lstm_chain_plan reports: kernel family, ms, steps per launch, B, H, the " tag" suffix and the launch count.  ROUTES pins the
plans to the builds this file is about (tests/test_chain_plan.py checks ROUTES on the host).  No case runs the pipeline at a shape
its residency rule refuses; that (520, 70, 256) and (264, 70, 512) are refused is asserted on the host side.

MEASURED holds the worst (err_chain, err_base) of every case and direction as printed on an MI355X: the chain kernels sit between
4.3e-07 and 1.06e-06 (dgi0 of B = 264, T = 66, H = 256, reverse, against 9.41e-07 on the per-step kernels), the per-step base
between 4.3e-07 and 1.12e-06, a factor of 19 under the cap; no case needed a smaller input scale.  The single-layer pairs are
mostly dh0.  Under INET_TEST_POISON=1 (NaN-filled allocator pool) every case passes with the same figures -- no ring slot, counter,
save or carry buffer is read before it is written; only the base of the two B = 264, T = 66 runs moved (9.60e-07 / 8.91e-07), through
the f32 atomics of its split-K products.  No run left a slow-wait entry or a chain timeout.
"""
import pytest
import torch

from tests import lstm_ref as R

if torch.cuda.is_available():
    from inpaintnet_amd import ops

CAP, FLOOR = 2e-5, 3e-7

# name: (H, B, T, the direction that is given h0 / c0 -- the other starts from the zero state).  Every case runs in both directions.
SINGLE = {
    "h256-b40-t5": (256, 40, 5, False),         # ms1, 3 groups, 8-row tail
    "h256-b264-t5": (256, 264, 5, True),        # ms2: 8 x 32 + 8 rows (second sub-tile of the last group clamped)
    "h256-b536-t4": (256, 536, 4, False),       # ms4: 8 x 64 + 24 (two sub-tiles live, two clamped)
    "h256-b1024-t3": (256, 1024, 3, True),      # ms4, 16 full groups: the capacity boundary
    "h256-b1025-t2": (256, 1025, 2, False),     # refused: one launch per step
    "h512-b24-t5": (512, 24, 5, True),          # ms1
    "h512-b136-t4": (512, 136, 4, False),       # ms2: 4 x 32 + 8
    "h512-b296-t4": (512, 296, 4, True),        # ms4: 4 x 64 + 40 (last sub-tile clamped)
    "h512-b512-t3": (512, 512, 3, False),       # ms4, 8 full groups: the boundary
}
# name: (H, B, T); each in both directions
PIPELINE = {
    "h256-b136-t70": (256, 136, 70),     # fwd_tag<2,4>, chunks 32 / 32 / 6, ring continued across chunks (phase)
    "h256-b264-t66": (256, 264, 66),     # ms4, counter hand-off with a prologue per chunk
    "h512-b24-t70": (512, 24, 70),       # H = 512 in the pipeline, ms1
    "h512-b72-t64": (512, 72, 64),       # ms2, exactly two chunks (the minimum T)
    "h256-b7-t545": (256, 7, 545),       # 18 chunks > 16: the base counter area re-zeroed per chunk
}
REFUSED = ((520, 70, 256), (264, 70, 512))

# The plans on 256 CUs: (ok, MS, groups, tagged, steps per launch, launches per layer, per-chunk counter areas)
ROUTES = {
    "h256-b40-t5": (1, 1, 3, 0, 5, 1, 0), "h256-b264-t5": (1, 2, 9, 0, 5, 1, 0), "h256-b536-t4": (1, 4, 9, 0, 4, 1, 0),
    "h256-b1024-t3": (1, 4, 16, 0, 3, 1, 0), "h256-b1025-t2": (0, 0, 0, 0, 0, 0, 0),
    "h512-b24-t5": (1, 1, 2, 0, 5, 1, 0), "h512-b136-t4": (1, 2, 5, 0, 4, 1, 0), "h512-b296-t4": (1, 4, 5, 0, 4, 1, 0),
    "h512-b512-t3": (1, 4, 8, 0, 3, 1, 0),
    "h256-b136-t70": (1, 2, 5, 1, 32, 3, 1), "h256-b264-t66": (1, 4, 5, 0, 32, 3, 1), "h512-b24-t70": (1, 1, 2, 0, 32, 3, 1),
    "h512-b72-t64": (1, 2, 3, 0, 32, 2, 1), "h256-b7-t545": (1, 1, 1, 1, 32, 18, 0),
}

# worst (err_chain, err_base) over the compared tensors of each case and direction ("-fwd" / "-rev"), as printed by the test on an MI355X
MEASURED = {
    "h256-b40-t5-fwd": (4.30e-07, 4.30e-07), "h256-b40-t5-rev": (4.74e-07, 4.73e-07), "h256-b264-t5-fwd": (6.94e-07, 5.05e-07),
    "h256-b264-t5-rev": (5.09e-07, 4.91e-07), "h256-b536-t4-fwd": (5.16e-07, 5.27e-07), "h256-b536-t4-rev": (5.71e-07, 5.58e-07),
    "h256-b1024-t3-fwd": (8.61e-07, 9.02e-07), "h256-b1024-t3-rev": (6.31e-07, 5.92e-07), "h256-b1025-t2-fwd": (7.31e-07, 7.31e-07),
    "h256-b1025-t2-rev": (6.38e-07, 6.38e-07), "h512-b24-t5-fwd": (6.78e-07, 6.78e-07), "h512-b24-t5-rev": (9.24e-07, 7.22e-07),
    "h512-b136-t4-fwd": (7.55e-07, 7.55e-07), "h512-b136-t4-rev": (8.51e-07, 8.78e-07), "h512-b296-t4-fwd": (8.65e-07, 8.14e-07),
    "h512-b296-t4-rev": (7.05e-07, 7.88e-07), "h512-b512-t3-fwd": (7.56e-07, 8.31e-07), "h512-b512-t3-rev": (8.95e-07, 9.64e-07),
    "h256-b136-t70-fwd": (5.36e-07, 8.35e-07), "h256-b136-t70-rev": (5.83e-07, 8.41e-07), "h256-b264-t66-fwd": (8.04e-07, 7.54e-07),
    "h256-b264-t66-rev": (1.06e-06, 9.41e-07), "h512-b24-t70-fwd": (6.03e-07, 1.12e-06), "h512-b24-t70-rev": (5.23e-07, 7.31e-07),
    "h512-b72-t64-fwd": (8.49e-07, 9.21e-07), "h512-b72-t64-rev": (8.67e-07, 9.32e-07), "h256-b7-t545-fwd": (5.54e-07, 8.90e-07),
    "h256-b7-t545-rev": (6.31e-07, 7.80e-07),
}


def plan_key(p):
    """A plan of ops.lstm_chain_plan in the form of ROUTES."""
    return (p["ok"], p["MS"], p["groups"], p["tagged"], p["chunk_steps"], p["chunks"], p["areas"])


def expected_launches(p, B, T, H, layers, want_dstate):
    """{(class, label): launches} of `layers` LSTM layers under plan p.  One launch per step: T forward launches per layer, T backward
    ones and one more for dh0 where the initial state's gradient is asked for; they carry no label."""
    if not p["ok"]:
        return {(R.PROF_STEP_FWD, ""): layers * T, (R.PROF_STEP_BWD, ""): layers * (T + 1 if want_dstate else T)}
    want = {}
    for s_lo in range(0, T, p["chunk_steps"]):
        nt = min(p["chunk_steps"], T - s_lo)
        tail = f" ms{p['MS']} T{nt} B{B} H{H}"
        for key in ((R.PROF_STEP_FWD, "lstm_chain_fwd" + tail + (" tag" if p["tagged"] else "")), (R.PROF_STEP_BWD, "lstm_chain_bwd" + tail)):
            want[key] = want.get(key, 0) + layers
    return want


def check_launches(tag, rows, want):
    got = {}
    for r in rows:
        got[r] = got.get(r, 0) + 1
    print(f"{tag}: launches {sorted(got.items())}")
    assert got == want, (tag, got, want)


def compare(tag, name, c, pipeline, tmp_path, want_dstate):
    """Base run (key 4 = 0), chain run, launches of both against the planner, the rule of the module docstring."""
    H, B, T = (SINGLE if not pipeline else PIPELINE)[name][:3]
    layers = 2 if pipeline else 1
    base, brows, bplan = R.run(c, False, tmp_path, f"{tag}_base.csv", pipeline)
    assert not bplan["ok"], bplan
    check_launches(f"{tag} base", brows, expected_launches(bplan, B, T, H, layers, want_dstate))
    errs, rows, plan = R.run(c, True, tmp_path, f"{tag}_chain.csv", pipeline)
    assert ops.chain_status() == 0, tag
    print(f"{tag}: {plan['slow_waits']}")
    assert not plan["ok"] or (plan["side_by_side"] * plan["workgroups"] <= plan["chain_capacity"]), plan
    if plan["chain_capacity"] == 256:
        assert plan_key(plan) == ROUTES[name], (tag, plan)
        check_launches(tag, rows, expected_launches(plan, B, T, H, layers, want_dstate))
    else:
        print(f"{tag}: label check skipped, ROUTES and the case's shapes are chosen for 256 CUs and this chip has {plan['chain_capacity']}")
    R.check(tag, {k: (errs[k], base[k]) for k in errs}, "chain", CAP, FLOOR)
    assert ops.chain_status() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("name", list(SINGLE))
def test_lstm_layer_on_the_chain_kernels_against_float64(name, reverse, tmp_path):
    """inet_lstm_fwd (with saves) and inet_lstm_bwd (dW_hh, db_ih, db_hh, dh0, dc0; dhT / dcT given) of one case and direction: out, hT,
    cT, dgi, dh0, dc0, dW_hh, db_ih, db_hh against float64 by the rule of the module docstring.  Measured: MEASURED."""
    H, B, T, state_dir = SINGLE[name]
    c = R.make_single(B, T, H, reverse, reverse == state_dir, 3000 + 2 * sorted(SINGLE).index(name) + int(reverse))
    compare(f"{name}-{'rev' if reverse else 'fwd'}", name, c, False, tmp_path, True)


@pytest.mark.gpu
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("name", list(PIPELINE))
def test_lstm_pipeline_on_the_chain_kernels_against_float64(name, reverse, tmp_path):
    """inet_lstm2_fwd (with saves) and inet_lstm2_bwd of one case and direction: out0, out1, dgi0 and all seven weight / bias gradients
    against float64 by the rule of the module docstring; the base is the two layers one after the other on the per-step kernels.
    Measured: MEASURED."""
    H, B, T = PIPELINE[name]
    assert ops.lstm2_ok(B, T, H)
    c = R.make_pipeline(B, T, H, reverse, 4000 + 2 * sorted(PIPELINE).index(name) + int(reverse))
    compare(f"{name}-{'rev' if reverse else 'fwd'}", name, c, True, tmp_path, False)


@pytest.mark.gpu
def test_pipeline_refuses_what_cannot_be_resident_side_by_side():
    """Two launches of (520, ., 256) or (264, ., 512) do not fit the chip together at any tile: inet_lstm2_ok is 0 and inet_lstm2_fwd
    returns 1 without launching -- ops.lstm2_fwd gives None and the caller goes layer by layer."""
    for B, T, H in REFUSED:
        if ops.lstm_chain_plan(B, T, H, True)["chain_capacity"] > 256:
            continue                                 # (a larger chip takes them; the host test pins the rule per capacity)
        assert not ops.lstm2_ok(B, T, H), (B, T, H)
        gi0 = torch.zeros(T, B, 4 * H, device=R.DEV)
        W = torch.zeros(4 * H, H, device=R.DEV)
        b = torch.zeros(4 * H, device=R.DEV)
        assert ops.lstm2_fwd(gi0, W, b, W, b, W, b, H) is None, (B, T, H)
    assert ops.chain_status() == 0
