"""The grouped GEMM launches (csrc/gemm.hip launch_gemm_group behind inet_gemm_group / ops.gemm_group) alone, against float64:
gemm_ks_group_kernel<TA,TB,AKM,BKM> -- the workgroup split-K body behind a workgroup -> product map, tiles 64x64, 64x32, 32x32 times
layouts NT, NN, TN -- and gemv_rows_group_kernel<M>, M = 1..8.  Every product of a group has its own shape, K, leading dimensions,
bias, epilogue and accumulation mode, so a wrong boundary in the first[] / tiles_n[] map, in the `v >= first[k]` selection or in the
per-product k range puts a plausible tile in the wrong place: every element of every product is compared.

Method: operands from a seeded generator, as column sub-views of wider parents; reference = epi(A . B^T + bias, aux) in float64 on the
CPU, plus the previous destination when accumulating; relmax (max abs error over max abs reference) < 2e-5, the bound
tests/test_gpu_kernels.py holds every f32 GEMM family to with K up to 6144 (K <= 1030 here).  Stored destinations are NaN beforehand
(an unwritten tile shows), every destination lies inside a larger buffer whose other elements must come back bit-unchanged, and the
profile of the call must show the launches ops.gemm_group_plan announces: one `groupN ...` label, or one label per product where the
group falls apart."""
import pytest
import torch

from tests.gemm_harness import DEV, LAYOUT_NAME, NN, NT, TN, TOL, TT, Product, dumped_labels, relmax, sub

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from inpaintnet_amd import ops


@pytest.fixture(autouse=True)
def default_gemm_options():
    """Whatever a test does with options 2, 3, 5 and the profiler, the next test finds the defaults."""
    try:
        yield
    finally:
        ops.set_option(2, -1)
        ops.set_option(3, 0)
        ops.set_option(5, 1)
        ops.prof_enable(False)


def P(M, N, K, bias=False, epi=0, acc=False, strided=False, boff=4, layout=None):
    """One product of a group: shape, modes, whether its destination is strided, the column offset of its B inside the parent (10:
    rows that start 8-byte aligned only, as rnn_tick.weight_ih_l0[:, E:]), its own layout where the group mixes them."""
    return dict(M=M, N=N, K=K, bias=bias, epi=epi, acc=acc, strided=strided, boff=boff, layout=layout)


def run_group(specs, layout, tmp_path, seed):
    """One ops.gemm_group call under the profiler.  Asserts that the launches followed the plan and that every product is right under
    its own modes; returns the plan rows of ops.gemm_group_plan and the products."""
    g = torch.Generator().manual_seed(seed)
    products = [Product(g, p, layout) for p in specs]
    calls = [p.call for p in products]
    rows = ops.gemm_group_plan(calls)
    ops.prof_enable(True)
    try:
        ops.gemm_group(calls)
        torch.cuda.synchronize()
        ops.prof_dump(str(tmp_path / "_inet_group.csv"))
    finally:
        ops.prof_enable(False)
    print("\n  %s" % " | ".join(r["label"] for r in rows if r["label"]))
    grouped = rows[0]["products"] == 1 and len(specs) > 1
    assert grouped == rows[0]["label"].startswith("group"), rows
    want = [rows[0]["label"]] if grouped else [r["label"] for r in rows]
    assert all(want) and dumped_labels(tmp_path / "_inet_group.csv") == want          # the launches followed the plan
    errs = [p.check() for p in products]
    assert all(e < TOL for e in errs), errs                # (a NaN fails: every product on its own)
    return rows, products


# ---- the workgroup split-K group: (tile, [products]); K per product for a k-contiguous A, and for TN (k-major A: any K, the rounded-up
# k range of a product reads the zero-returning buffer tail).  Modes are mixed inside every group; over the four groups every epilogue
# 0..5, bias and no bias, store and add, strided and dense destinations, n = 2, 3, 4 appear.
KS_GROUPS = {
    # 64 + 64 + 128 = 256 tiles of 64x64: the >= 192 rule is met at the first tile
    "64x64": ((64, 64), [P(512, 512, 80, bias=True, epi=1), P(256, 1024, 256, acc=True, boff=10),
                         P(512, 1024, 64, bias=True, epi=3, strided=True)], {0: 70}),
    # 120 + 48 + 28 = 196 tiles of 64x32; N % 64 == 32 rules 64x64 out
    "64x32": ((64, 32), [P(512, 480, 64, epi=4), P(1024, 96, 1024, bias=True, epi=2, strided=True, boff=10),
                         P(256, 224, 80, acc=True)], {1: 1000}),
    # 32x32 by divisibility: 15 + 1 + 14 + 19 tiles; the single-tile product sits between two others (both of its first[] boundaries)
    "32x32-divisible": ((32, 32), [P(96, 160, 1024, bias=True, epi=5), P(32, 32, 80, acc=True, boff=10),
                                   P(224, 64, 64, bias=True, epi=1, strided=True), P(32, 608, 256, bias=True, epi=2, acc=True)],
                        {0: 1000, 1: 70}),
    # 32x32 by smallness: every tile divides, 3 / 6 / 12 workgroups -- the planner ends on the smallest
    "32x32-small": ((32, 32), [P(64, 64, 1024, bias=True), P(128, 64, 64, epi=3, acc=True, strided=True, boff=10)], {0: 1000, 1: 70}),
}


@pytest.mark.parametrize("layout", [NT, NN, TN], ids=["NT", "NN", "TN"])
@pytest.mark.parametrize("case", list(KS_GROUPS))
def test_split_k_group(case, layout, tmp_path):
    """One instantiation of gemm_ks_group_kernel per (tile, layout), launched as ONE grouped launch."""
    tile, specs, tn_k = KS_GROUPS[case]
    specs = [dict(p, K=tn_k.get(i, p["K"])) if layout == TN else p for i, p in enumerate(specs)]
    rows, _ = run_group(specs, layout, tmp_path, seed=1000 + 10 * list(KS_GROUPS).index(case) + 2 * layout[0] + layout[1])
    p0, r = specs[0], rows[0]
    assert r["products"] == 1 and r["launches"] == 1 and r["family"] == ops.GEMM_FAMILIES.index("ks"), r
    assert (r["tile_m"], r["tile_n"]) == tile, r
    assert r["label"] == "group%d M%d N%d K%d %s k%dx%d e%d" % (len(specs), p0["M"], p0["N"], p0["K"], LAYOUT_NAME[layout], tile[0],
                                                                tile[1], p0["epi"]), r
    tiles = sum((p["M"] // tile[0]) * (p["N"] // tile[1]) for p in specs)
    assert (r["tiles"], r["grid_x"], r["grid_y"]) == (tiles, tiles, 1), r
    assert r["flops"] == sum(2.0 * p["M"] * p["N"] * p["K"] for p in specs)


@pytest.mark.parametrize("M", range(1, 9))
def test_few_row_group(M, tmp_path):
    """gemv_rows_group_kernel<M>: the grid is sized by the widest N (two N are no multiples of 4, the workgroups beyond a narrow
    product's N write nothing), K with a K % 4 tail and a K below one wave's stride of 4 x 64."""
    specs = [P(M, 1536, 512, bias=True, epi=1), P(M, 7, 5, epi=4, boff=10), P(M, 130, 1030, acc=True, strided=True)]
    rows, _ = run_group(specs, NT, tmp_path, seed=2000 + M)
    r = rows[0]
    assert r["products"] == 1 and r["launches"] == 1 and r["family"] == ops.GEMM_FAMILIES.index("gemv"), r
    assert r["label"] == "group3 M%d N1536 K512 NT gemv e1" % M and r["tile_m"] == M, r
    assert (r["grid_x"], r["grid_y"]) == (1536 // 4, 3), r


def test_interleaved_destinations_of_one_group(tmp_path):
    """Two products of one group write matrices 0 and 2 of one [M, 3, N] buffer (rows of one between the rows of the other: no element
    is shared); matrix 1 and a guard row on either side stay as they were."""
    g = torch.Generator().manual_seed(2100)
    M, N = 64, 96
    big = torch.randn(M + 2, 3, N, generator=g)
    calls, refs = [], []
    for slot, K, acc in ((0, 64, False), (2, 80, True)):
        (A, Ad), (B, Bd) = sub(g, M, K, 4), sub(g, N, K, 4)
        refs.append(A.double() @ B.double().t() + (big[1:M + 1, slot, :].double() if acc else 0.0))
        if not acc:
            big[1:M + 1, slot, :] = float("nan")
        calls.append(dict(A=Ad, B=Bd, M=M, N=N, K=K, accumulate=acc))
    bd = big.to(DEV)
    for c, slot in zip(calls, (0, 2)):
        c["out"] = bd[1:M + 1, slot, :]
    rows = ops.gemm_group_plan(calls)
    assert rows[0]["products"] == 1 and rows[0]["label"] == "group2 M64 N96 K64 NT k32x32 e0", rows
    ops.prof_enable(True)
    try:
        ops.gemm_group(calls)
        torch.cuda.synchronize()
        ops.prof_dump(str(tmp_path / "_inet_group.csv"))
    finally:
        ops.prof_enable(False)
    assert dumped_labels(tmp_path / "_inet_group.csv") == [rows[0]["label"]]           # the launch followed the plan
    after = bd.cpu()
    errs = [relmax(after[1:M + 1, slot, :], ref) for slot, ref in zip((0, 2), refs)]
    print("\n  interleaved destinations: relmax", errs)
    assert bool(torch.isfinite(after).all()) and all(e < TOL for e in errs), errs
    for t in (after, big):
        t[1:M + 1, 0, :] = 0
        t[1:M + 1, 2, :] = 0
    assert torch.equal(after, big)


def falls_apart(specs, layout, tmp_path, seed):
    rows, products = run_group(specs, layout, tmp_path, seed)
    assert all(r["products"] == len(specs) and not r["label"].startswith("group") for r in rows), rows
    return rows


def test_group_of_mixed_layouts_falls_apart(tmp_path):
    falls_apart([P(128, 256, 128, bias=True, epi=1, layout=NT), P(128, 256, 128, acc=True, strided=True, layout=NN),
                 P(64, 96, 70, epi=4, layout=TN)], None, tmp_path, 3001)


def test_group_of_kmajor_a_with_kcontiguous_b_falls_apart(tmp_path):
    """The (1,0) layout: only the LDS-tiled kernel reads it."""
    rows = falls_apart([P(96, 64, 70, epi=4), P(64, 128, 64, bias=True, epi=2, strided=True)], TT, tmp_path, 3002)
    assert all(r["family"] == ops.GEMM_FAMILIES.index("tiled") for r in rows), rows


def test_few_row_products_of_unequal_m_fall_apart(tmp_path):
    rows = falls_apart([P(8, 512, 512, bias=True, epi=1), P(7, 130, 1030, acc=True, strided=True)], NT, tmp_path, 3003)
    assert all(r["family"] == ops.GEMM_FAMILIES.index("gemv") for r in rows), rows


def test_nine_row_products_fall_apart(tmp_path):
    """One row more than the few-row kernel takes, and no split-K tile divides nine rows."""
    falls_apart([P(9, 130, 80, bias=True, epi=2), P(9, 64, 64, epi=5, acc=True)], NT, tmp_path, 3004)


def test_nt_group_with_a_k_off_the_16_deep_group_falls_apart(tmp_path):
    """A k-contiguous operand has no zero-returning K tail: K % 16 != 0 in one product keeps the whole group off the split-K kernel."""
    falls_apart([P(128, 128, 64, bias=True, epi=1), P(128, 128, 70, acc=True)], NT, tmp_path, 3005)


def test_group_beyond_2048_workgroups_falls_apart(tmp_path):
    """1056 = 33 x 32: only 32x32 divides, 2 x 1089 tiles > 2048."""
    falls_apart([P(1056, 1056, 64, bias=True, epi=1), P(1056, 1056, 64, acc=True, strided=True)], NT, tmp_path, 3006)


@pytest.mark.parametrize("key,value", [(5, 0), (5, 3), (2, 0)])
def test_group_falls_apart_under_options(key, value, tmp_path):
    """Option 5 = 0 (LDS-tiled kernels only) and 3 (no workgroup split-K): no split-K group.  Option 2 = 0 (a forced tile
    configuration): no group at all, few-row products go to the LDS-tiled kernel too."""
    ks = [P(64, 64, 256, bias=True), P(128, 64, 64, epi=3, acc=True, strided=True, boff=10)]
    rows, _ = run_group(ks, NT, tmp_path, 3100)
    assert rows[0]["products"] == 1 and rows[0]["label"].startswith("group2 "), rows          # (under the defaults: one launch)
    ops.set_option(key, value)
    rows = falls_apart(ks, NT, tmp_path, 3100)
    assert all(r["family"] != ops.GEMM_FAMILIES.index("ks") for r in rows), rows
    if key == 2:
        rows = falls_apart([P(4, 130, 70, bias=True, epi=1), P(4, 7, 5, acc=True, strided=True)], NT, tmp_path, 3101)
        assert all(r["family"] == ops.GEMM_FAMILIES.index("tiled") and r["cfg"] == 0 for r in rows), rows


def test_group_of_one_product(tmp_path):
    """n = 1 is the product's own plan: a split-K shape, a few-row shape."""
    rows = falls_apart([P(64, 64, 64, bias=True, epi=1, strided=True)], NT, tmp_path, 3201)
    assert rows[0]["label"] == ops.gemm_plan(64, 64, 64, lda=64 + 4 + 6, ldb=64 + 4 + 6, bias=True, epi=1)["label"]
    rows = falls_apart([P(3, 130, 1030, acc=True)], NT, tmp_path, 3202)
    assert rows[0]["family"] == ops.GEMM_FAMILIES.index("gemv"), rows
