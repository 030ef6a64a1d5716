"""The launch plans of the GRU layers (csrc/seq.hip gru_layer_fwd_plan / gru_layer_bwd_plan over csrc/gru_chain.hip chain_fwd_build /
chain_bwd_build, behind inet_gru_chain_plan), checked on the host: which kernel build, row tile, row chunk and ring layout a layer of
(H, B, T, nprob) lands on is pure arithmetic, gru_layer_fwd / gru_layer_bwd branch on these very functions, and a wrong pick is a
kernel contracting over the wrong width or two launches waiting for each other's CUs -- found here without a GPU."""
import ctypes as C
import os
import subprocess
import sys

import pytest

from inpaintnet_amd import _lib

KEYS = ("route", "rows", "launches", "gen", "MS", "SQ", "OCC", "EMR", "two", "ring", "groups", "members", "ring_floats", "ring_capacity",
        "capacity", "max_groups")
STEP, CHAIN1, CHAIN2, STEP_BF3 = range(4)
FULL, OWN, ROWS = range(3)
HS, NPROBS, TS = (256, 512, 1024), (1, 2, 4), (1, 2, 5, 6, 24)


def batches():
    """1..1100: every value next to a multiple of 16 (every tile of 16, 32, 64 and 128 rows and every chunk boundary is one) and a
    stride of 7 in between."""
    bs = set(range(1, 1101, 7))
    for m in range(16, 1101, 16):
        bs.update((m - 1, m, m + 1))
    return sorted(b for b in bs if 1 <= b <= 1100)


@pytest.fixture(scope="module")
def L():
    _lib.build(verbose=False)
    lib = _lib.lib()
    yield lib
    assert lib.inet_set_option(4, 1) == 0 and lib.inet_set_option(7, 9) == 0


def plan(L, H, B, T, nprob, save):
    out = (C.c_int64 * 32)()
    assert L.inet_gru_chain_plan(H, B, T, nprob, save, out) == 0, (H, B, T, nprob, save)
    f, b = dict(zip(KEYS, out[:16])), dict(zip(KEYS, out[16:]))
    return f, (b if save else None), list(out[16:])


def ceil_div(a, b):
    return (a + b - 1) // b


def pk(rows, K):
    return ceil_div(rows, 16) * 16 * K


def check_plan(p, H, B, T, nprob, K, backward, where):
    """Every invariant of one direction's plan; K = the width of the exchanged state (H forward, 3H backward)."""
    assert p["capacity"] > 0 and p["max_groups"] == 64 and p["ring_capacity"] == 3 * pk(B, K), (where, p)
    assert p["ring_floats"] <= p["ring_capacity"], (where, p)                  # the launches stay inside the workspace carve
    if p["route"] in (STEP, STEP_BF3):
        assert (p["rows"], p["launches"], p["gen"], p["two"], p["ring"]) == (B, T, 0, 0, FULL), (where, p)
        assert p["ring_floats"] == (3 if p["route"] == STEP_BF3 else 2) * pk(B, K), (where, p)
        return
    assert p["route"] in (CHAIN1, CHAIN2) and p["gen"] == (2 if p["route"] == CHAIN2 else 1), (where, p)
    assert T >= 2, (where, p)                                                   # a chain over one step is a step launch
    rows, n = p["rows"], p["launches"]
    assert rows >= 1 and B % rows == 0 and n == B // rows, (where, p)         # chunk rows divide B
    assert n == 1 or rows % 64 == 0, (where, p)
    assert p["members"] == H // 16, (where, p)
    if p["gen"] == 2:
        # second generation: forward only, T >= 6, H <= 512; four waves of one 16-row block each, S = H / 32; a counter per row block
        assert not backward and T >= 6 and H <= 512, (where, p)
        assert (p["MS"], p["SQ"], p["OCC"]) == (4, H // 32, 1), (where, p)
        assert p["groups"] == nprob * ceil_div(ceil_div(rows, 16), 4), (where, p)
        assert nprob * ceil_div(rows, 16) <= p["max_groups"], (where, p)
        slots = 3
    else:
        assert p["SQ"] == K // 64, (where, p)                                   # the build contracts over the layer's own width
        assert p["MS"] in ((1, 2, 4, 8) if backward else (1, 2, 4)), (where, p)
        assert p["MS"] != 8 or H <= 512, (where, p)
        assert p["groups"] == nprob * ceil_div(rows, 16 * p["MS"]), (where, p)
        assert p["OCC"] == (2 if p["two"] else 1), (where, p)                   # two at a time only on the build made for it
        assert p["OCC"] == 1 or (not backward and p["MS"] == 4 and H <= 512 and n >= 2), (where, p)
        if backward:
            assert p["EMR"] == 0 or (p["MS"], p["SQ"]) == (4, 24), (where, p)  # row pieces: <4,24,true> alone
        else:
            assert p["EMR"] == 0, (where, p)
        slots = 2
    # every workgroup of a launch resident at once, every group with a counter
    assert p["groups"] * p["members"] <= p["capacity"] and p["groups"] <= p["max_groups"], (where, p)
    # the ring floats the launches address, from the layout: the last chunk's last slot
    if p["ring"] == FULL:
        assert n == 1 and p["ring_floats"] == slots * pk(B, K), (where, p)
    elif p["ring"] == OWN:
        assert n >= 2 and p["ring_floats"] == (n - 1) * 3 * pk(rows, K) + slots * pk(rows, K), (where, p)
    else:
        assert p["ring"] == ROWS and n >= 2 and p["gen"] == 1, (where, p)
        assert p["ring_floats"] == (n - 1) * pk(rows, K) + pk(B, K) + pk(rows, K), (where, p)


def sweep(L):
    n = 0
    for H in HS:
        for nprob in NPROBS:
            for T in TS:
                for B in batches():
                    for save in (0, 1):
                        f, b, raw = plan(L, H, B, T, nprob, save)
                        where = (H, B, T, nprob, save)
                        check_plan(f, H, B, T, nprob, H, False, where)
                        if save:
                            check_plan(b, H, B, T, nprob, 3 * H, True, where)
                            # with saves a batch is chunked up to 1024 rows (beyond that one step fills the chip)
                            assert f["launches"] == 1 or f["route"] in (STEP, STEP_BF3) or B <= 1024, (where, f)
                        else:
                            assert raw == [-1] * 16, where
                        n += 1
    return n


def test_every_plan_of_the_grid_is_sound(L):
    """H x nprob x T x B x save: the build's SQ is the layer's width (H / 64 forward, 3H / 64 backward; H / 32 second generation), every
    launch fits the chip and the counters, two chunks run side by side only on an OCC = 2 build, chunk rows divide B, the ring floats
    the launches address follow from the layout and fit chain_ring_floats(B, .), the second generation runs only with T >= 6 and H <=
    512, and the row-piece BPTT build is <4,24,true> alone."""
    assert sweep(L) == len(HS) * len(NPROBS) * len(TS) * len(batches()) * 2


def test_the_same_under_the_first_generation_and_without_chains(L):
    """inet_set_option key 7 = 0: no second-generation launch anywhere, the rest still sound; key 4 = 0: step launches only."""
    try:
        assert L.inet_set_option(7, 0) == 0
        sweep(L)
        for H in HS:
            for B in (24, 136, 264, 448, 768, 1024):
                f, b, _ = plan(L, H, B, 6, 2, 1)
                assert f["route"] != CHAIN2 and f["gen"] != 2, (H, B, f)
                assert b["ring"] != OWN, (H, B, b)       # (own rings mirror a second-generation forward launch)
        assert L.inet_set_option(7, 9) == 0 and L.inet_set_option(4, 0) == 0
        for H in HS:
            for B in (24, 300, 768):
                f, b, _ = plan(L, H, B, 6, 2, 1)
                assert f["route"] in (STEP, STEP_BF3) and b["route"] in (STEP, STEP_BF3), (H, B, f, b)
    finally:
        L.inet_set_option(4, 1)
        L.inet_set_option(7, 9)


def test_h1024_chunks_run_the_h1024_build_one_after_the_other(L):
    """The defect this file was written for: a chunk launch of an H = 1024 layer (B = 256 rows, two directions: two 128-row chunks)
    once ran gru_chain_fwd_kernel<4,4,2>, the H = 256 build, beside its twin -- a contraction over 256 of the 1024 columns.  It is
    <4,16,1> (192 registers of W_hh per lane: a workgroup owns its CU), its chunks one after the other."""
    f, b, _ = plan(L, 1024, 256, 2, 2, 1)
    assert (f["route"], f["rows"], f["launches"], f["MS"], f["SQ"], f["OCC"], f["two"], f["ring"]) == (CHAIN1, 128, 2, 4, 16, 1, 0, ROWS), f
    assert (b["route"], b["rows"], b["launches"], b["MS"], b["SQ"], b["ring"]) == (CHAIN1, 128, 2, 4, 48, ROWS), b


def test_full_chip_chunks_never_run_side_by_side(L):
    """H = 512, B = 384, T = 5, two directions: three 128-row chunks at 32 rows per workgroup, 256 workgroups each on the one-per-CU
    build <2,8,1>.  Two such launches on two streams each wait for workgroups that cannot become resident while the other's spin."""
    f, _, _ = plan(L, 512, 384, 5, 2, 1)
    assert (f["route"], f["rows"], f["launches"], f["MS"], f["SQ"], f["OCC"], f["two"]) == (CHAIN1, 128, 3, 2, 8, 1, 0), f
    assert f["groups"] * f["members"] == f["capacity"] or f["capacity"] != 256, f


def test_routes_of_the_gpu_cases_on_256_cus(L):
    """tests/test_gpu_gru_chain_tiles.py ROUTES: the plan of every GPU case is the route the case was chosen for."""
    from inpaintnet_amd import ops
    from tests import test_gpu_gru_chain_tiles as G
    if plan(L, 256, 16, 2, 1, 1)[0]["capacity"] != 256:
        pytest.skip("ROUTES is written for a chain capacity of 256 workgroups (INET_CHAIN_CUS is set to another)")
    assert {(n, m) for n, c in G.CASES.items() for m in c[8]} == set(G.ROUTES)
    try:
        for (name, mode), want in G.ROUTES.items():
            H, B, T = G.CASES[name][:3]
            ops.set_option(7, 0 if mode == "gen1" else 9)
            f, b = ops.gru_chain_plan(H, B, T, 2, True)
            assert b["route"] == "chain1" and G.plan_key(f, b) == want, (name, mode, f, b)
    finally:
        ops.set_option(7, 9)


def test_plan_rejects(L):
    out = (C.c_int64 * 32)(*([7] * 32))
    for args in ((0, 8, 2, 2, 1), (256, 0, 2, 2, 1), (256, 8, 0, 2, 1), (256, 8, 2, 0, 1), (256, 8, 2, 5, 1), (-256, 8, 2, 2, 1)):
        assert L.inet_gru_chain_plan(*args, out) == -1, args
    assert L.inet_gru_chain_plan(256, 8, 2, 2, 1, None) == -1
    assert list(out) == [7] * 32
    # a width no chain kernel takes: step launches
    f, b, _ = plan(L, 768, 64, 6, 2, 1)
    assert f["route"] in (STEP, STEP_BF3) and b["route"] in (STEP, STEP_BF3)


@pytest.mark.parametrize("cus", [64, 304])
def test_other_chip_sizes(cus):
    """INET_CHAIN_CUS is read once per process: a fresh interpreter per capacity runs the sweep at a stride (H = 512 and 1024, two
    directions) -- the invariants hold for a quarter of the chip and for a larger one."""
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from tests import test_chain_plan as P\n"
            "from inpaintnet_amd import _lib\n"
            "L = _lib.lib()\n"
            "n = 0\n"
            "for H in (512, 1024):\n"
            "    for T in (2, 6):\n"
            "        for B in P.batches()[::3]:\n"
            "            f, b, _ = P.plan(L, H, B, T, 2, 1)\n"
            "            assert f['capacity'] == %d\n"
            "            P.check_plan(f, H, B, T, 2, H, False, (H, B, T))\n"
            "            P.check_plan(b, H, B, T, 2, 3 * H, True, (H, B, T))\n"
            "            n += 1\n"
            "print('plans', n)\n" % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))), cus))
    env = dict(os.environ, INET_CHAIN_CUS=str(cus))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "plans" in r.stdout, r.stdout + r.stderr


# ---- the LSTM planner (csrc/lstm.hip lstm_chain_plan behind inet_lstm_chain_plan) ----------------------------------------------------
LSTM_KEYS = ("ok", "MS", "groups", "members", "workgroups", "blocks", "tagged", "chunk", "chunks", "areas", "capacity", "side_by_side",
             "max_groups", "counter_stride", "counter_words")
LSTM_TS = (1, 63, 64, 65, 512, 513, 545)
LSTM_CHUNK, LSTM_MAX_CHUNKS = 32, 16           # lstm_chunk_steps() without INET_LSTM_CHUNK; kMaxChunks


def lstm_plan(L, B, T, H, pipeline):
    out = (C.c_int64 * 16)()
    assert L.inet_lstm_chain_plan(B, T, H, pipeline, out) == 0, (B, T, H, pipeline)
    return dict(zip(LSTM_KEYS, out[:15]))


def check_lstm_plan(p, B, T, H, pipeline, where):
    """Every invariant of one LSTM plan, from the shape, the capacity the plan reports and the chunk length alone."""
    side, cap = 2 if pipeline else 1, p["capacity"]
    assert cap > 0 and p["side_by_side"] == side and p["max_groups"] == 32, (where, p)
    assert p["max_groups"] * p["counter_stride"] <= p["counter_words"], (where, p)       # every group's counter inside the counter area
    fits = lambda ms: side * ceil_div(B, 16 * ms) * (H // 16) <= cap and ceil_div(B, 16 * ms) <= 32
    want_ms = next((ms for ms in (1, 2, 4) if fits(ms)), 0)
    want_ok = want_ms != 0 and not (pipeline and T < 2 * LSTM_CHUNK)
    assert p["ok"] == int(want_ok), (where, p)
    if not p["ok"]:
        assert all(p[k] == 0 for k in ("MS", "groups", "members", "workgroups", "blocks", "tagged", "chunk", "chunks", "areas")), (where, p)
        return
    assert p["MS"] == want_ms, (where, p)                                                # the smallest tile that fits
    assert p["members"] == H // 16 and p["groups"] == ceil_div(B, 16 * p["MS"]), (where, p)
    assert p["workgroups"] == p["groups"] * p["members"], (where, p)
    assert side * p["groups"] * p["members"] <= cap and p["groups"] <= 32, (where, p)   # all launches that run together resident at once
    assert p["groups"] * p["counter_stride"] <= p["counter_words"], (where, p)
    assert p["blocks"] == 8 * p["members"] * ceil_div(p["groups"], 8), (where, p)       # chain::blocks_for, members <= 32
    assert p["tagged"] == int(pipeline and H == 256 and p["MS"] <= 2), (where, p)
    if pipeline:
        assert T >= 2 * LSTM_CHUNK and p["chunk"] == LSTM_CHUNK and p["chunks"] == ceil_div(T, LSTM_CHUNK), (where, p)
        assert p["areas"] == int(p["chunks"] <= LSTM_MAX_CHUNKS), (where, p)
    else:
        assert (p["chunk"], p["chunks"], p["areas"]) == (T, 1, 0), (where, p)


def test_every_lstm_plan_of_the_grid_is_sound(L):
    """H x B (every batch of 1..1100) x T x {layer, pipeline}: ok implies that the launches which run side by side are resident together
    and every group has a counter, MS is the smallest tile with which they are, the tagged hand-off is the pipeline's at H = 256 and
    MS <= 2, per-chunk counter areas are used iff there are at most 16 chunks, and a pipeline shorter than two chunks is refused."""
    n = 0
    for H in (256, 512):
        for T in LSTM_TS:
            for B in range(1, 1101):
                for pipeline in (0, 1):
                    check_lstm_plan(lstm_plan(L, B, T, H, pipeline), B, T, H, pipeline, (B, T, H, pipeline))
                    n += 1
    assert n == 2 * len(LSTM_TS) * 1100 * 2


# (H, pipeline): ((last B of MS = 1, of MS = 2, of MS = 4); above the last one the plan is refused) on 256 CUs.  The single-layer rows
# are what chain_ms() / lstm_chain_ok() gave before there was a planner: smallest MS with ceil(B / 16 MS) * H / 16 <= 256.
LSTM_DOMAINS = {(256, 0): (256, 512, 1024), (512, 0): (128, 256, 512), (256, 1): (128, 256, 512), (512, 1): (64, 128, 256)}


def test_lstm_tile_boundaries_on_256_cus(L):
    """The single-layer plans are those of the parent commit at every B (boundaries 256 / 257, 512 / 513, 1024 / 1025 at H = 256 and
    128 / 129, 256 / 257, 512 / 513 at H = 512); the pipeline's domains are half as wide, and it refuses what the layer alone takes."""
    if lstm_plan(L, 1, 64, 256, 0)["capacity"] != 256:
        pytest.skip("the table is written for a chain capacity of 256 workgroups (INET_CHAIN_CUS is set to another)")
    for (H, pipeline), ends in LSTM_DOMAINS.items():
        for B in range(1, 1101):
            want = next((ms for ms, end in zip((1, 2, 4), ends) if B <= end), 0)
            p = lstm_plan(L, B, 64, H, pipeline)
            assert (p["ok"], p["MS"]) == (int(want != 0), want), (H, pipeline, B, p)
    pins = {(256, 0): ((256, 1), (257, 2), (512, 2), (513, 4), (1024, 4), (1025, 0)),
            (512, 0): ((128, 1), (129, 2), (256, 2), (257, 4), (512, 4), (513, 0)),
            (256, 1): ((128, 1), (129, 2), (256, 2), (257, 4), (512, 4), (513, 0)),
            (512, 1): ((64, 1), (65, 2), (128, 2), (129, 4), (256, 4), (257, 0))}
    for (H, pipeline), rows in pins.items():
        for B, ms in rows:
            assert lstm_plan(L, B, 64, H, pipeline)["MS"] == ms, (H, pipeline, B)
    # the benchmark's AnticipationRNN shape keeps its plan: two 16-row groups, tagged forward chunks of 32 steps, per-chunk areas
    p = lstm_plan(L, 32, 384, 256, 1)
    assert (p["ok"], p["MS"], p["groups"], p["tagged"], p["chunk"], p["chunks"], p["areas"]) == (1, 1, 2, 1, 32, 12, 1), p


def test_lstm_plan_rejects_and_switch(L):
    out = (C.c_int64 * 16)(*([7] * 16))
    for args in ((0, 8, 256, 0), (8, 0, 256, 0), (8, 8, 0, 1), (-8, 8, 256, 1), (8, -1, 256, 0)):
        assert L.inet_lstm_chain_plan(*args, out) == -1, args
    assert L.inet_lstm_chain_plan(8, 8, 256, 0, None) == -1
    assert list(out) == [7] * 16
    assert lstm_plan(L, 8, 64, 768, 0)["ok"] == 0 and lstm_plan(L, 8, 64, 128, 1)["ok"] == 0     # widths no chain kernel is built for
    assert L.inet_lstm2_ok(32, 64, 256) == 1 and L.inet_lstm2_ok(32, 63, 256) == 0
    try:
        assert L.inet_set_option(4, 0) == 0                                                      # chains off: nothing is ok
        assert lstm_plan(L, 32, 384, 256, 0)["ok"] == 0 and lstm_plan(L, 32, 384, 256, 1)["ok"] == 0
        assert L.inet_lstm2_ok(32, 384, 256) == 0
    finally:
        L.inet_set_option(4, 1)


def test_lstm_routes_of_the_gpu_cases_on_256_cus(L):
    """tests/test_gpu_lstm_chain_tiles.py ROUTES: the plan of every GPU case is the build the case was chosen for, no pipeline case sits
    in what the residency rule refuses, and the shapes that file expects to be refused are."""
    from inpaintnet_amd import ops
    from tests import test_gpu_lstm_chain_tiles as G
    if lstm_plan(L, 1, 64, 256, 0)["capacity"] != 256:
        pytest.skip("ROUTES is written for a chain capacity of 256 workgroups (INET_CHAIN_CUS is set to another)")
    assert set(G.ROUTES) == set(G.SINGLE) | set(G.PIPELINE) and not set(G.SINGLE) & set(G.PIPELINE)
    for name, want in G.ROUTES.items():
        pipeline = name in G.PIPELINE
        H, B, T = (G.PIPELINE if pipeline else G.SINGLE)[name][:3]
        p = ops.lstm_chain_plan(B, T, H, pipeline)
        assert G.plan_key(p) == want and (p["ok"] or not pipeline), (name, p)
    for B, T, H in G.REFUSED:
        assert not ops.lstm2_ok(B, T, H) and ops.lstm_chain_plan(B, T, H, False)["ok"], (B, T, H)


@pytest.mark.parametrize("cus", [64, 304])
def test_lstm_plans_on_other_chip_sizes(cus):
    """INET_CHAIN_CUS is read once per process: a fresh interpreter per capacity runs the LSTM sweep at a stride."""
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from tests import test_chain_plan as P\n"
            "from inpaintnet_amd import _lib\n"
            "L = _lib.lib()\n"
            "n = 0\n"
            "for H in (256, 512):\n"
            "    for T in (63, 64, 545):\n"
            "        for B in P.batches():\n"
            "            for pipeline in (0, 1):\n"
            "                p = P.lstm_plan(L, B, T, H, pipeline)\n"
            "                assert p['capacity'] == %d\n"
            "                P.check_lstm_plan(p, B, T, H, pipeline, (B, T, H, pipeline))\n"
            "                n += 1\n"
            "print('plans', n)\n" % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))), cus))
    env = dict(os.environ, INET_CHAIN_CUS=str(cus))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "plans" in r.stdout, r.stdout + r.stderr
