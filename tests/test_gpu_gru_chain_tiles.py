"""The persistent GRU chain kernels (csrc/gru_chain.hip gru_chain_fwd_kernel<MS,SQ,OCC>, gru_chain_bwd_kernel<MS,SQ[,EMR]>;
csrc/gru_chain2.hip gru_chain2_fwd_kernel<4,S,9,EM>) at every row tile, width and row chunk, against a float64 evaluation of the
same two-layer bi-GRU (oracle.torch_ref.gru_stack): the smallest shapes that reach each route of gru_layer_fwd / gru_layer_bwd on a
chip of 256 CUs -- one launch at 16 / 32 / 64 rows per workgroup with a ragged last tile, the two-tile BPTT build (ms8) over a ragged
batch with an empty second tile and over saves the per-step forward kernels wrote, row chunks of both generations on both ring
layouts with a backward pass, chunks two at a time on the 256-register builds <4,4,2> / <4,8,2>, and H = 1024 in one launch and in
chunks.

Rule for every compared tensor (out, h_n, dx or dx_scalar, dh0 where asked, all 16 parameter gradients), the one
test_chain_generations_against_float64 and the step-kernel tests use: with err = max |got - ref| / max |ref| against float64,
err_chain <= 2 err_base + 3e-7 and err_chain < 2e-5, where err_base is the identical call under inet_set_option(4, 0) (the per-step
kernels, which have tests of their own), and err_base < 1e-5.  The profile labels of every run must be the launches that
inet_gru_chain_plan reports for the shape under the same options, and ROUTES pins those plans to the routes this file is about
(tests/test_chain_plan.py checks ROUTES on the host).

MEASURED holds the worst (err_chain, err_base) of every case as printed on an MI355X: the worst pair of all is 2.55e-06 on the chain
kernels against 2.54e-06 on the per-step kernels (B = 768, T = 6, H = 512: db_hh of layer 0, reverse), a factor of 8 under the cap;
every other case sits between 3.7e-07 and 1.5e-06 on both sides.  Under INET_TEST_POISON=1 (NaN-filled allocator pool) every case
passes: no ring slot, save or piece buffer is read before it is written.  The figures of a second run differ in the last digits on
both sides alike (at most 1.4e-07 chain, 4.3e-07 base between the plain and the poisoned run; worst pair then 2.56e-06 / 2.60e-06):
the split-K products and the bias sums accumulate with f32 atomics, in an order that changes from run to run.
"""
import pytest
import torch

from tests import bigru2_ref as R

if torch.cuda.is_available():
    from inpaintnet_amd import ops

CAP, FLOOR = 2e-5, 3e-7
GEN1 = {7: 0}       # inet_set_option key 7 = 0: the first-generation forward kernels where the second generation would run

# name: (H, B, T, K, scalar x, h0 given, dh0 wanted, mask, modes).  modes: "chain" = the default options, "gen1" = key 7 = 0.
CASES = {
    # ---- H = 256
    "h256-b136-t7": (256, 136, 7, 8, False, False, False, False, ("chain", "gen1")),      # ms2: 4 x 32 + 8 rows
    "h256-b264-t6": (256, 264, 6, 8, False, False, False, False, ("chain", "gen1")),      # ms4: 4 x 64 + 8 rows
    "h256-b520-t3": (256, 520, 3, 8, False, True, True, True, ("chain",)),                 # ms8 BPTT over per-step saves
    "h256-b1024-t2": (256, 1024, 2, 8, False, False, False, False, ("chain",)),            # <4,4,2>: two 512-row chunks at a time
    "h256-b1024-t6": (256, 1024, 6, 8, False, False, False, False, ("chain",)),            # second-generation chunks, own rings
    # ---- H = 512
    "h512-b24-t7": (512, 24, 7, 8, False, False, False, False, ("chain",)),                # ms1 BPTT
    "h512-b24-t7-scalar": (512, 24, 7, 1, True, False, False, False, ("gen1",)),           # ms1 forward, vector-only input
    "h512-b72-t6": (512, 72, 6, 8, False, False, False, False, ("chain", "gen1")),         # ms2: 2 x 32 + 8 rows
    "h512-b200-t5": (512, 200, 5, 8, False, False, False, False, ("chain",)),              # ms4 below the generation boundary
    "h512-b200-t6": (512, 200, 6, 8, False, False, False, False, ("chain", "gen1")),       # ... and on it
    "h512-b300-t3": (512, 300, 3, 8, False, False, True, False, ("chain",)),               # ms8: the last workgroup's second tile is empty
    "h512-b448-t6": (512, 448, 6, 8, False, False, False, False, ("chain",)),              # seven 64-row second-generation chunks
    "h512-b768-t6": (512, 768, 6, 8, False, True, True, True, ("chain",)),                 # chunked BPTT on own rings
    "h512-b768-t2": (512, 768, 2, 8, False, False, False, False, ("chain",)),              # <4,8,2>; chunked BPTT on the full-batch ring
    # ---- H = 1024
    "h1024-b24-t3": (1024, 24, 3, 1, True, True, False, False, ("chain",)),                # ms1
    "h1024-b256-t2": (1024, 256, 2, 8, False, False, True, False, ("chain",)),             # two 128-row chunks, <4,16,1> one after the other
}

# The plans on 256 CUs, per (case, mode): forward (route, MS, OCC, rows per launch, launches, two at a time, ring), backward (MS, rows per
# launch, launches, ring).  MS of a second-generation launch is its four waves.
ROUTES = {
    ("h256-b136-t7", "chain"): (("chain2", 4, 1, 136, 1, 0, "full"), (2, 136, 1, "full")),
    ("h256-b136-t7", "gen1"): (("chain1", 2, 1, 136, 1, 0, "full"), (2, 136, 1, "full")),
    ("h256-b264-t6", "chain"): (("chain2", 4, 1, 264, 1, 0, "full"), (4, 264, 1, "full")),
    ("h256-b264-t6", "gen1"): (("chain1", 4, 1, 264, 1, 0, "full"), (4, 264, 1, "full")),
    ("h256-b520-t3", "chain"): (("step", 0, 0, 520, 3, 0, "full"), (8, 520, 1, "full")),
    ("h256-b1024-t2", "chain"): (("chain1", 4, 2, 512, 2, 1, "rows"), (8, 1024, 1, "full")),
    ("h256-b1024-t6", "chain"): (("chain2", 4, 1, 512, 2, 0, "own"), (8, 1024, 1, "full")),
    ("h512-b24-t7", "chain"): (("chain2", 4, 1, 24, 1, 0, "full"), (1, 24, 1, "full")),
    ("h512-b24-t7-scalar", "gen1"): (("chain1", 1, 1, 24, 1, 0, "full"), (1, 24, 1, "full")),
    ("h512-b72-t6", "chain"): (("chain2", 4, 1, 72, 1, 0, "full"), (2, 72, 1, "full")),
    ("h512-b72-t6", "gen1"): (("chain1", 2, 1, 72, 1, 0, "full"), (2, 72, 1, "full")),
    ("h512-b200-t5", "chain"): (("chain1", 4, 1, 200, 1, 0, "full"), (4, 200, 1, "full")),
    ("h512-b200-t6", "chain"): (("chain2", 4, 1, 200, 1, 0, "full"), (4, 200, 1, "full")),
    ("h512-b200-t6", "gen1"): (("chain1", 4, 1, 200, 1, 0, "full"), (4, 200, 1, "full")),
    ("h512-b300-t3", "chain"): (("step", 0, 0, 300, 3, 0, "full"), (8, 300, 1, "full")),
    ("h512-b448-t6", "chain"): (("chain2", 4, 1, 64, 7, 0, "own"), (8, 448, 1, "full")),
    ("h512-b768-t6", "chain"): (("chain2", 4, 1, 256, 3, 0, "own"), (4, 256, 3, "own")),
    ("h512-b768-t2", "chain"): (("chain1", 4, 2, 256, 3, 1, "rows"), (4, 256, 3, "rows")),
    ("h1024-b24-t3", "chain"): (("chain1", 1, 1, 24, 1, 0, "full"), (1, 24, 1, "full")),
    ("h1024-b256-t2", "chain"): (("chain1", 4, 1, 128, 2, 0, "rows"), (4, 128, 2, "rows")),
}

# worst (err_chain, err_base) over the compared tensors of each (case, mode), as printed by the test on an MI355X
MEASURED = {
    ("h256-b136-t7", "chain"): (6.97e-07, 6.62e-07), ("h256-b136-t7", "gen1"): (6.71e-07, 6.62e-07),
    ("h256-b264-t6", "chain"): (6.48e-07, 6.48e-07), ("h256-b264-t6", "gen1"): (6.78e-07, 6.48e-07),
    ("h256-b520-t3", "chain"): (9.16e-07, 9.16e-07), ("h256-b1024-t2", "chain"): (4.51e-07, 5.06e-07),
    ("h256-b1024-t6", "chain"): (1.45e-06, 1.45e-06), ("h512-b24-t7", "chain"): (5.27e-07, 5.07e-07),
    ("h512-b24-t7-scalar", "gen1"): (3.72e-07, 4.03e-07), ("h512-b72-t6", "chain"): (5.38e-07, 5.12e-07),
    ("h512-b72-t6", "gen1"): (4.33e-07, 5.12e-07), ("h512-b200-t5", "chain"): (5.60e-07, 5.39e-07),
    ("h512-b200-t6", "chain"): (9.74e-07, 1.01e-06), ("h512-b200-t6", "gen1"): (9.31e-07, 1.01e-06),
    ("h512-b300-t3", "chain"): (1.00e-06, 1.00e-06), ("h512-b448-t6", "chain"): (1.00e-06, 8.55e-07),
    ("h512-b768-t6", "chain"): (2.55e-06, 2.54e-06), ("h512-b768-t2", "chain"): (9.77e-07, 9.77e-07),
    ("h1024-b24-t3", "chain"): (5.62e-07, 5.86e-07), ("h1024-b256-t2", "chain"): (9.44e-07, 9.44e-07),
}


def plan_key(f, b):
    """A plan of ops.gru_chain_plan in the form of ROUTES."""
    return ((f["route"], f["MS"], f["OCC"], f["rows"], f["launches"], f["two_at_a_time"], f["ring"]),
            (b["MS"], b["rows"], b["launches"], b["ring"]))


def expected_labels(f, b, H, T, want_dh0):
    """{label prefix or label: launches} of the two layers' recurrent launches under the plans f, b (two directions per launch).
    A key that ends in a blank counts every label that starts with it; a tuple counts its members together (the build that writes
    piece outputs runs where the caller's workspace carries their buffers, which the plan of one layer does not know)."""
    want = {}
    if f["route"] == "step":
        want["gru_fwd "] = 2 * T
    elif f["route"] == "chain1":
        want[f"gru_chain_fwd ms{f['MS']}{'x2' if f['OCC'] == 2 else ''} np2 T{T} B{f['rows']} H{H}"] = 2 * f["launches"]
    elif f["route"] == "chain2":
        tail = f" p9 np2 T{T} B{f['rows']} H{H}"
        want[("gru_chain_fwd v2w4" + tail,) + (("gru_chain_fwd v2w4e" + tail,) if f["EMR"] else ())] = 2 * f["launches"]
    else:
        want["gru_step_bf3 "] = 2 * T
    if b["route"] == "step":
        want["gru_bwd "] = 2 * (T + 1 if want_dh0 else T)
    elif b["route"] == "chain1":
        tail = f" np2 T{T} B{b['rows']} H{H}"
        want[(f"gru_chain_bwd ms{b['MS']}" + tail,) + ((f"gru_chain_bwd ms{b['MS']}e" + tail,) if b["EMR"] else ())] = 2 * b["launches"]
    else:
        want["gru_step_bf3_bwd "] = 2 * (T + 1 if want_dh0 else T)
    return want


def check_labels(tag, labels, want):
    """The recurrent launches of a run are exactly those of `want`: every family of GRU launches that `want` does not name is absent."""
    rec = [l for l in labels if l.startswith(("gru_fwd ", "gru_bwd ", "gru_chain_fwd ", "gru_chain_bwd ", "gru_step_bf3 ", "gru_step_bf3_bwd "))]
    print(f"{tag}: launches {sorted(set(rec))}")
    counted = 0
    for key, n in want.items():
        if isinstance(key, tuple):
            got = sum(rec.count(k) for k in key)
        elif key.endswith(" "):
            got = sum(l.startswith(key) for l in rec)
        else:
            got = rec.count(key)
        assert got == n, (tag, key, got, n, sorted(set(rec)))
        counted += got
    assert counted == len(rec), (tag, want, sorted(set(rec)))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_bigru2_on_the_chain_kernels_against_float64(name, tmp_path):
    """inet_bigru2_fwd / _bwd of one case on the chain kernels (and, where the case says so, once more with the first-generation forward
    kernels) against float64 by the rule of the module docstring; the per-step kernels under key 4 = 0 are the base.  The launches of
    every run are those of inet_gru_chain_plan; on 256 CUs the plans are ROUTES.  chain_status() stays 0.  Measured: MEASURED."""
    H, B, T, K, scalar, with_h0, want_dh0, with_mask, modes = CASES[name]
    c = R.make_case(B, T, K, H, scalar, with_h0, want_dh0, with_mask, 2000 + sorted(CASES).index(name))
    plan = lambda: ops.gru_chain_plan(H, B, T, 2, True)
    base, blabels, (bf, bb) = R.run(c, {4: 0}, tmp_path, f"{name}_base.csv", plan=plan)
    assert bf["route"] in ("step", "step_bf3") and bb["route"] in ("step", "step_bf3"), (bf, bb)
    check_labels(f"{name} base", blabels, expected_labels(bf, bb, H, T, want_dh0))
    for mode in modes:
        tag = f"{name} {mode}"
        errs, labels, (f, b) = R.run(c, GEN1 if mode == "gen1" else {}, tmp_path, f"{name}_{mode}.csv", plan=plan)
        torch.cuda.synchronize()
        assert ops.chain_status() == 0, tag
        if f["chain_capacity"] == 256:
            assert plan_key(f, b) == ROUTES[(name, mode)], (tag, f, b)
            check_labels(tag, labels, expected_labels(f, b, H, T, want_dh0))
        else:
            print(f"{tag}: label check skipped, ROUTES and the case's shapes are chosen for 256 CUs and this chip has "
                  f"{f['chain_capacity']}")
        R.check(tag, {k: (errs[k], base[k]) for k in errs}, "chain", CAP, FLOOR)
    assert ops.chain_status() == 0
