"""tests/gemm_cases.py against the planner, on the host (inet_gemm_plan needs no GPU): every case must land on the table entry it is
listed under -- family, cfg and layout -- with the splits, zero fill and epilogue pass the table says, under the case's options.  The
GPU test (tests/test_gpu_gemm_tables.py) launches exactly these rows, so a case that drifted to another kernel would silently test
that one; here it fails.  The set of entries that have cases is written out below: 51 of the 52 instantiations behind the five tables,
all but gemm_ks_kernel<4,6,true,true>, which plan_ks never picks."""
import ctypes as C

import pytest

from inpaintnet_amd import _lib
from tests import gemm_cases as GC

GEMV, TN_DIRECT, KC_DIRECT, KS, TILED = range(5)
CAP = 96
KEYS = ("family", "cfg", "tile_m", "tile_n", "splits", "k_per_split", "tiles_n", "tiles", "gx", "gy", "gz", "zero_fill", "two_pass",
        "launches", "products", "_")
LAYOUTS = ("NT", "NN", "TN", "TT")
TILES = ((64, 64), (128, 128), (192, 64), (192, 128), (192, 192))

ENTRIES = ([("gemv", m, "NT") for m in range(8)]
           + [("tiled", c, lay) for c in range(5) for lay in LAYOUTS]
           + [("tn_direct", c, "TN") for c in range(3)]
           + [("kc_direct", c, lay) for c in range(4) for lay in ("NT", "NN")]
           + [("ks", c, lay) for c in (0, 1, 2, 4) for lay in ("NT", "NN", "TN") if (c, lay) != (4, "TN")]
           + [("ks", 3, "TN")])


@pytest.fixture(scope="module")
def L():
    lib = _lib.lib()
    try:
        yield lib
    finally:
        options(lib)


def options(L, opt2=-1, opt3=0, opt5=1):
    assert L.inet_set_option(2, opt2) == 0 and L.inet_set_option(3, opt3) == 0 and L.inet_set_option(5, opt5) == 0


def plan(L, akm, bkm, M, N, K, lda, ldb, bias, epi, acc):
    out, work, label = (C.c_int32 * 16)(), (C.c_double * 2)(), C.create_string_buffer(CAP)
    assert L.inet_gemm_plan(akm, bkm, M, N, K, lda, ldb, int(bias), epi, int(acc), 1, out, work, label, CAP) == 0
    return dict(zip(KEYS, list(out)), label=label.value.decode())


def plan_case(L, c):
    options(L, c["opt2"], c["opt3"], c["opt5"])
    return plan(L, c["layout"][0], c["layout"][1], c["M"], c["N"], c["K"], c["lda"], c["ldb"], c["bias"], c["epi"], c["acc"])


def test_the_entries_that_have_cases():
    assert len(ENTRIES) == len(set(ENTRIES)) == 51
    assert set(GC.CASES) == set(ENTRIES)
    assert all(GC.CASES[e] for e in ENTRIES)


@pytest.mark.parametrize("entry", ENTRIES, ids=["%s-%d-%s" % e for e in ENTRIES])
def test_every_case_lands_on_its_entry(L, entry):
    family, cfg, lay = entry
    bad = []
    for c in GC.CASES[entry]:
        assert (GC.FAMILIES[c["family"]], c["cfg"], GC.LAYOUT_NAME[c["layout"]]) == entry, c
        p = plan_case(L, c)
        want = {k: c[k] for k in ("family", "cfg", "splits", "zero_fill", "two_pass")}
        if {k: p[k] for k in want} != want or p["products"] != 1 or p["launches"] != 1 + c["zero_fill"] + c["two_pass"]:
            bad.append((c, p))
    assert not bad, (len(bad), bad[:3])


def test_every_entry_has_operands_on_4_byte_aligned_rows():
    """Column offset 1 of a parent with an odd leading dimension, and a margin of 8 columns behind, on both operands."""
    for e in ENTRIES:
        odd = [c for c in GC.CASES[e] if c["aoff"] == 1 and c["boff"] == 1 and c["lda"] % 2 and c["ldb"] % 2]
        assert odd, e
    for cs in GC.CASES.values():
        for c in cs:
            acols = c["M"] if c["layout"][0] else c["K"]
            bcols = c["N"] if c["layout"][1] else c["K"]
            assert c["lda"] - c["aoff"] - acols >= 8 and c["ldb"] - c["boff"] - bcols >= 8, c
            assert (c["aoff"], c["boff"]) in ((1, 1), (8, 8)), c


def test_every_entry_runs_every_mode():
    """Plain store, bias + SELU, an aux epilogue and accumulation (the non-linear ones: wherever the entry takes them unsplit)."""
    for e in ENTRIES:
        cs = GC.CASES[e]
        assert any(not c["bias"] and c["epi"] == 0 and not c["acc"] for c in cs), e
        assert any(c["bias"] and c["epi"] == 1 for c in cs), e
        assert any(c["epi"] >= 3 for c in cs), e
        assert any(c["acc"] for c in cs), e
        assert any(c["strided"] for c in cs), e


@pytest.mark.parametrize("cfg", range(5))
@pytest.mark.parametrize("lay", LAYOUTS)
def test_every_tiled_entry_sees_its_edges(cfg, lay):
    tm, tn = TILES[cfg]
    cs = GC.CASES[("tiled", cfg, lay)]
    assert all(c["opt2"] == cfg for c in cs)
    assert any(c["M"] % tm and c["M"] > tm for c in cs), "a partial tile in M behind a whole one"
    assert any(c["N"] % tn and c["N"] > tn for c in cs), "a partial tile in N behind a whole one"
    assert any(c["M"] == tm and c["N"] == tn for c in cs) and any(c["M"] < tm and c["N"] < tn for c in cs)
    assert {c["K"] for c in cs if c["splits"] == 1} >= {1, 31, 32, 33, 70}
    assert any(c["K"] % 32 and c["K"] > 32 for c in cs), "a K tail behind full chunks"
    split = [c for c in cs if c["splits"] == 2]
    assert split and all(c["opt3"] == 2 and c["K"] == 70 for c in split)          # k_per_split 64: the second range is 6 deep
    assert any(c["zero_fill"] and c["strided"] for c in split) and any(c["acc"] and c["bias"] for c in split)
    assert any(c["bias"] and not c["acc"] and c["epi"] == 0 for c in split)
    assert any(c["two_pass"] and c["epi"] == 1 and c["bias"] for c in split) and any(c["two_pass"] and c["epi"] == 4 for c in split)


def test_split_tiled_cases_have_a_6_deep_second_range(L):
    for cfg in range(5):
        for lay in LAYOUTS:
            for c in GC.CASES[("tiled", cfg, lay)]:
                if c["splits"] == 2:
                    assert plan_case(L, c)["k_per_split"] == 64, c
    options(L)


def test_direct_entries_see_both_grid_orders(L):
    """The direct kernels renumber their workgroups when gridDim.x % 8 == 0: every TN-direct and kc-direct entry has a grid that is
    a multiple of 8 and one that is not; one of the latter has odd sub-view operands."""
    for e in ENTRIES:
        if e[0] not in ("tn_direct", "kc_direct"):
            continue
        grids = [(plan_case(L, c)["gx"], c["aoff"]) for c in GC.CASES[e]]
        assert any(g % 8 == 0 for g, _ in grids) and any(g % 8 and off == 1 for g, off in grids), (e, grids)
    options(L)


def test_ks_entries_see_their_smallest_k_and_a_split_grid(L):
    for e in ENTRIES:
        if e[0] != "ks":
            continue
        cs = GC.CASES[e]
        if e[2] != "TN":
            assert any(c["K"] == 64 for c in cs), e         # a k-contiguous A: one k group per wave
        else:
            assert any(c["K"] % 16 == 10 for c in cs), e     # a k-major A: K = 16 n - 6
            assert any(c["splits"] == 2 and c["opt3"] == 2 for c in cs), e
    options(L)


def test_no_plan_reaches_the_64x96_tile_with_a_kmajor_a(L):
    """gemm_ks_kernel<4,6,true,true>: built (kKsKernel[4][3]) and never planned.  Every key-5 mode, with and without a forced split,
    over the shapes that tile divides -- among them the shapes that give a k-contiguous A this tile."""
    shapes = [(64 * a, 96 * b, K) for a in (1, 2, 3, 9, 16, 19) for b in (1, 2, 3, 9, 16, 19) for K in (64, 74, 512, 2048, 4096)]
    for opt5 in range(5):
        for opt3 in (0, 1, 2, 4):
            options(L, -1, opt3, opt5)
            for (M, N, K) in shapes:
                for epi, acc in ((0, 0), (1, 0), (0, 1)):
                    p = plan(L, 1, 1, M, N, K, M, N, 0, epi, acc)
                    assert (p["family"], p["cfg"]) != (KS, 4), (opt5, opt3, M, N, K, epi, acc, p)
    options(L)
    assert plan(L, 0, 0, 576, 1824, 64, 64, 64, 0, 0, 0)["cfg"] == 4       # (the same shape, A k-contiguous: the tile is taken)
