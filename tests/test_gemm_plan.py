"""The launch planner of the f32 GEMM dispatcher (csrc/gemm.hip gemm_plan / gemm_group_plan behind inet_gemm_plan /
inet_gemm_group_plan), checked on the host: which kernel, tile and split a product of the training step lands on is pure arithmetic,
and a wrong pick is a performance regression that no numeric test sees.  tests/golden/gemm_plans.csv.gz holds what the dispatcher
launched on an MI355X for every case of tools/gemm_plan_record.py (recorded with the build in front of the planner / launcher split);
the planner has to give exactly those labels, FLOPs and bytes."""
import csv
import ctypes as C
import gzip
import itertools
import os

import pytest

from inpaintnet_amd import _lib

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_plans.csv.gz")
GEMV, TN, KC, KS, TILED = range(5)
GRANULE = {TN: 2, KS: 16, TILED: 32}                      # k_per_split is a multiple of it
KEYS = ("family", "cfg", "tile_m", "tile_n", "splits", "k_per_split", "tiles_n", "tiles", "gx", "gy", "gz", "zero_fill", "two_pass",
        "launches", "products", "_")
CAP = 96


@pytest.fixture(scope="module")
def L():
    _lib.build(verbose=False)
    lib = _lib.lib()
    yield lib
    options(lib)


def options(L, opt2=-1, opt3=0, opt5=1):
    assert L.inet_set_option(2, opt2) == 0 and L.inet_set_option(3, opt3) == 0 and L.inet_set_option(5, opt5) == 0


def plan(L, akm, bkm, M, N, K, lda=0, ldb=0, bias=0, epi=0, acc=0, nbatch=1):
    out, work, label = (C.c_int32 * 16)(), (C.c_double * 2)(), C.create_string_buffer(CAP)
    rc = L.inet_gemm_plan(akm, bkm, M, N, K, lda or (M if akm else K), ldb or (N if bkm else K), bias, epi, acc, nbatch, out, work,
                          label, CAP)
    p = dict(zip(KEYS, list(out)), flops=work[0], bytes=work[1], label=label.value.decode())
    return rc, p


def group_plan(L, descs):
    n = len(descs)
    d = (C.c_int64 * (10 * max(n, 1)))(*itertools.chain.from_iterable(descs))
    out, work, label = (C.c_int32 * (16 * max(n, 1)))(), (C.c_double * (2 * max(n, 1)))(), C.create_string_buffer(CAP * max(n, 1))
    rc = L.inet_gemm_group_plan(n, d, out, work, label, CAP)
    rows = []
    for i in range(n):
        p = dict(zip(KEYS, out[16 * i:16 * i + 16]), flops=work[2 * i], bytes=work[2 * i + 1])
        p["label"] = label.raw[CAP * i:CAP * (i + 1)].split(b"\0")[0].decode()
        rows.append(p)
    return rc, rows


@pytest.fixture(scope="module")
def rows():
    return [{k: (v if k == "launches" else int(v)) for k, v in r.items()} for r in csv.DictReader(gzip.open(FIXTURE, "rt"))]


def plan_row(L, r):
    options(L, r["opt2"], r["opt3"], r["opt5"])
    rc, p = plan(L, r["akm"], r["bkm"], r["M"], r["N"], r["K"], r["lda"], r["ldb"], 0, r["epi"], r["acc"], r["nbatch"])
    assert rc == 0, r
    return p


def test_the_planner_gives_what_the_dispatcher_launched(L, rows):
    """(a) every recorded case: the labels, FLOPs and bytes of the launches, in order."""
    assert len(rows) > 7000
    bad = []
    for r in rows:
        p = plan_row(L, r)
        got = "|".join(["%s;%.4f;%.4f" % (p["label"], p["flops"] * 1e-9, p["bytes"] * 1e-6)] * p["products"])
        if got != r["launches"]:
            bad.append((r, got))
    assert not bad, (len(bad), bad[:5])


def check_invariants(r, p):
    M, N, K, epi, acc, nb = r["M"], r["N"], r["K"], r["epi"], r["acc"], r["nbatch"]
    fam, tm, tn, splits, kps = p["family"], p["tile_m"], p["tile_n"], p["splits"], p["k_per_split"]
    assert fam in (GEMV, TN, KC, KS, TILED), (r, p)
    if fam in (TN, KC, KS):
        assert M % tm == 0 and N % tn == 0 and p["tiles"] == (M // tm) * (N // tn) and p["tiles_n"] == N // tn, (r, p)
    elif fam == TILED:
        assert p["tiles"] == -(-M // tm) * -(-N // tn) and p["tiles_n"] == -(-N // tn), (r, p)
    else:
        assert M <= 8 and tm == M and p["tiles"] == -(-N // 4) and not r["akm"] and not r["bkm"], (r, p)
    batch = nb if p["products"] == 1 else 1               # one launch took all the products, or each runs alone
    assert p["gx"] * p["gy"] * p["gz"] == p["tiles"] * splits * batch, (r, p)
    assert kps * splits >= K and kps * (splits - 1) < K, (r, p)
    if fam in GRANULE:
        assert kps % GRANULE[fam] == 0, (r, p)
    else:
        assert splits == 1 and kps == K, (r, p)
    assert p["zero_fill"] == int(splits > 1 and acc == 0), (r, p)
    assert p["two_pass"] == int(splits > 1 and epi != 0), (r, p)
    assert p["products"] in (1, nb) and p["launches"] == p["products"] * (1 + p["zero_fill"] + p["two_pass"]), (r, p)
    if epi != 0 and acc == 1:
        assert splits == 1, (r, p)                        # a non-linear accumulating call never splits
    if fam == KS and epi != 0:
        assert splits == 1, (r, p)
    if r["akm"] and not r["bkm"]:
        assert fam == TILED, (r, p)                       # k-major A with k-contiguous B: only the LDS-tiled kernel reads it
    if r["opt5"] == 0:
        assert fam in (GEMV, TILED), (r, p)
    if r["opt2"] >= 0:
        assert fam == TILED and p["cfg"] == r["opt2"], (r, p)
        assert (tm, tn) == ((64, 64), (128, 128), (192, 64), (192, 128), (192, 192))[r["opt2"]], (r, p)


def test_plan_invariants(L, rows):
    """(b) over the recorded sweep and the extremes of every size."""
    extremes = [dict(akm=a, bkm=b, M=M, N=N, K=K, lda=0, ldb=0, epi=e, acc=c, nbatch=1, opt2=-1, opt3=0, opt5=o5)
                for (M, N, K) in [(1, 1, 1), (1, 4096, 1), (4096, 1, 1), (1, 1, 1 << 20), (64, 64, 1 << 20), (1536, 512, 1 << 20),
                                  (100, 100, 1 << 20)]
                for a in (0, 1) for b in (0, 1) for e in (0, 1) for c in (0, 1) for o5 in range(5)]
    forced = [dict(x, opt2=o2, opt3=o3, opt5=1) for x in extremes[::5] for o2 in range(5) for o3 in (0, 2, 4)]
    for r in rows + extremes + forced:
        check_invariants(r, plan_row(L, r))


# ---- (c) the grouped launches of the MeasureVAE step (csrc/vae.hip), V = 48, E = 10, H = 512, Z = 256, four beats, B = 256 -----------
H, Z, B, NB = 512, 256, 256, 4


def fwd(M, N, K, epi):                                     # seq.h linear_fwd_args: x [M,K] . W [N,K]^T + b
    return (0, 0, M, N, K, K, K, 1, epi, 0)


def dgrad(M, N, K, epi):                                   # linear_dgrad_args: dx [M,K] = epi(dy [M,N] . W [N,K])
    return (0, 1, M, K, N, N, K, 0, epi, 0)


def wgrad(M, N, K):                                        # linear_wgrad_args: dW [N,K] += dy [M,N]^T . x [M,K]
    return (1, 1, N, K, M, N, K, 0, 0, 1)


VAE_GROUPS = {
    "encoder heads, first layer": ([fwd(B, 2 * H, 4 * H, 1)] * 2, "group2 M256 N1024 K2048 NT k64x32 e1"),
    "encoder heads, second layer": ([fwd(B, Z, 2 * H, 0)] * 2, "group2 M256 N256 K1024 NT k32x32 e0"),
    "encoder heads, data gradient": ([dgrad(B, Z, 2 * H, 3)] * 2, "group2 M256 N1024 K256 NN k64x32 e3"),
    "encoder heads, weight gradients of the second layer": ([wgrad(B, Z, 2 * H)] * 2, "group2 M256 N1024 K256 TN k64x32 e0"),
    "encoder heads, weight gradients of the first layer": ([wgrad(B, 2 * H, 4 * H)] * 2, "group2 M1024 N2048 K256 TN k64x64 e0"),
    "beat -> tick projections": ([fwd(NB * B, 2 * H, H, 1), fwd(NB * B, H, H, 1)], "group2 M1024 N1024 K512 NT k64x64 e1"),
    "beat path, four weight gradients": ([wgrad(NB * B, 2 * H, H), wgrad(NB * B, H, H), wgrad(NB * B, 3 * H, H),
                                          wgrad(NB * B, 3 * H, H)], "group4 M1024 N512 K1024 TN k64x64 e0"),
    "beat path, two weight gradients": ([wgrad(NB * B, 3 * H, H), wgrad(B, 2 * H, Z)], "group2 M1536 N512 K1024 TN k64x64 e0"),
}


@pytest.mark.parametrize("site", list(VAE_GROUPS))
def test_group_plans_of_the_vae_step(L, site):
    """The group* labels of a MeasureVAE step at B = 256 (recorded with the fixture's build), from the call sites' descriptors."""
    options(L)
    descs, label = VAE_GROUPS[site]
    rc, got = group_plan(L, descs)
    assert rc == 0
    assert got[0]["products"] == 1 and got[0]["launches"] == 1 and got[0]["label"] == label, got
    assert got[0]["family"] == KS and got[0]["flops"] == sum(2.0 * d[2] * d[3] * d[4] for d in descs)


def test_group_plans_that_fall_apart_or_go_to_the_gemv_group(L):
    options(L)
    rc, got = group_plan(L, [fwd(256, 512, 512, 0), dgrad(256, 512, 512, 0)])            # mixed layouts: one by one
    assert rc == 0 and [g["products"] for g in got] == [2, 2]
    assert [g["label"] for g in got] == [plan(L, 0, 0, 256, 512, 512, bias=1)[1]["label"], plan(L, 0, 1, 256, 512, 512)[1]["label"]]
    for M in range(1, 9):                                   # rows 1..8 of equal M: the gemv group, grid (widest N / 4, n)
        rc, got = group_plan(L, [fwd(M, 1536, 512, 0), fwd(M, 2048, 512, 1), fwd(M, 7, 5, 0)])
        assert rc == 0 and got[0]["products"] == 1 and got[0]["family"] == GEMV, got
        assert got[0]["label"] == "group3 M%d N1536 K512 NT gemv e0" % M and (got[0]["gx"], got[0]["gy"]) == (512, 3), got
    rc, got = group_plan(L, [fwd(8, 512, 512, 0), fwd(7, 512, 512, 0)])                  # unequal M
    assert rc == 0 and [g["products"] for g in got] == [2, 2] and all(g["family"] == GEMV for g in got)
    rc, got = group_plan(L, [fwd(9, 512, 512, 0)] * 2)                                    # nine rows: no gemv, no common tile
    assert rc == 0 and got[0]["products"] == 2
    # 2 x 1024 tiles of 64 x 64 are one launch, one tile more falls apart
    rc, got = group_plan(L, [fwd(2048, 2048, 256, 0)] * 2)
    assert rc == 0 and got[0]["products"] == 1 and got[0]["family"] == KS and got[0]["gx"] == 2048, got
    rc, got = group_plan(L, [fwd(2048, 2048, 256, 0), fwd(2048, 2112, 256, 0)])
    assert rc == 0 and [g["products"] for g in got] == [2, 2], got
    for opt5 in (0, 3):                                     # no workgroup split-K under these modes
        options(L, opt5=opt5)
        assert group_plan(L, [fwd(256, 512, 512, 0)] * 2)[1][0]["products"] == 2
    options(L, opt2=0)                                      # a forced tile configuration: the LDS-tiled kernel, one by one
    assert group_plan(L, [fwd(4, 512, 512, 0)] * 2)[1][0]["family"] == TILED
    options(L)


def test_calls_the_entries_reject(L):
    """(d) -1, and nothing written."""
    options(L)
    ok = dict(akm=0, bkm=0, M=64, N=64, K=64)
    assert plan(L, **ok)[0] == 0
    for bad in (dict(M=0), dict(N=0), dict(K=0), dict(M=-1), dict(N=-5), dict(K=-64), dict(epi=-1), dict(epi=6), dict(acc=-1), dict(acc=2),
                dict(nbatch=0), dict(nbatch=9), dict(nbatch=-1)):
        rc, p = plan(L, **dict(ok, **bad))
        assert rc == -1 and p["label"] == "" and p["tiles"] == 0, (bad, p)
    out, work, label = (C.c_int32 * 16)(), (C.c_double * 2)(), C.create_string_buffer(CAP)
    args = (0, 0, 64, 64, 64, 64, 64, 0, 0, 0, 1)
    assert L.inet_gemm_plan(*args, None, work, label, CAP) == -1
    assert L.inet_gemm_plan(*args, out, None, label, CAP) == -1
    assert L.inet_gemm_plan(*args, out, work, None, CAP) == -1
    assert L.inet_gemm_plan(*args, out, work, label, 0) == -1
    assert list(out) == [0] * 16 and label.value == b""
    one = fwd(64, 64, 64, 0)
    assert group_plan(L, [one])[0] == 0
    assert group_plan(L, [])[0] == -1 and group_plan(L, [one] * 5)[0] == -1
    for i, v in ((2, 0), (3, 0), (4, 0), (2, -3), (8, -1), (8, 6), (9, -1), (9, 2)):
        bad = list(one)
        bad[i] = v
        rc, got = group_plan(L, [one, tuple(bad)])
        assert rc == -1 and got[0]["label"] == "" and got[0]["tiles"] == 0, (i, v, got)
    d = (C.c_int64 * 10)(*one)
    assert L.inet_gemm_group_plan(1, None, out, work, label, CAP) == -1
    assert L.inet_gemm_group_plan(1, d, None, work, label, CAP) == -1
    assert L.inet_gemm_group_plan(1, d, out, None, label, CAP) == -1
    assert L.inet_gemm_group_plan(1, d, out, work, None, CAP) == -1


# ---- (e) the grouped launch behind the C-ABI: inet_gemm_group / ops.gemm_group, ops.gemm_group_plan -----------------------------------
def test_gemm_group_entry_rejects(L):
    """-1 before anything is launched (no device is touched: the pointers are not even memory)."""
    def desc(**bad):
        d = dict(A=0x1000, lda=64, a_kmajor=0, B=0x2000, ldb=64, b_kmajor=0, C=0x3000, ldc=64, M=64, N=64, K=64, bias=None, aux=None,
                 ldaux=0, epi=0, acc=0)
        d.update(bad)
        return _lib.GemmDesc(**d)
    two = (_lib.GemmDesc * 2)(desc(), desc())
    five = (_lib.GemmDesc * 5)(*[desc()] * 5)
    assert L.inet_gemm_group(0, two, None) == -1 and L.inet_gemm_group(-1, two, None) == -1
    assert L.inet_gemm_group(5, five, None) == -1
    assert L.inet_gemm_group(1, None, None) == -1 and L.inet_gemm_group(2, None, None) == -1
    for bad in (dict(A=None), dict(B=None), dict(C=None), dict(M=0), dict(N=0), dict(K=0), dict(M=-1), dict(N=-5), dict(K=-64),
                dict(epi=-1), dict(epi=6), dict(acc=-1), dict(acc=2)):
        for n, at in ((1, 0), (2, 0), (2, 1), (4, 3)):     # the bad product alone, first, last
            lst = (_lib.GemmDesc * n)(*[desc(**bad) if i == at else desc() for i in range(n)])
            assert L.inet_gemm_group(n, lst, None) == -1, (bad, n, at)


@pytest.mark.parametrize("site", list(VAE_GROUPS))
def test_ops_group_plan_is_the_raw_group_plan(L, site):
    """ops.gemm_group_plan over the call sites' descriptors: the dicts of ops.gemm_plan, value for value what the entry wrote."""
    from inpaintnet_amd import ops
    options(L)
    descs = VAE_GROUPS[site][0]
    rc, raw = group_plan(L, descs)
    names = ("a_kmajor", "b_kmajor", "M", "N", "K", "lda", "ldb", "bias", "epi", "accumulate")
    got = ops.gemm_group_plan([dict(zip(names, d)) for d in descs])
    rename = {"gx": "grid_x", "gy": "grid_y", "gz": "grid_z"}
    assert rc == 0 and len(got) == len(raw) == len(descs)
    for g, r in zip(got, raw):
        r = {rename.get(k, k): v for k, v in r.items() if k != "_"}
        assert g == r and tuple(g)[:15] == ops.GEMM_PLAN_KEYS and set(g) == set(ops.gemm_plan(64, 64, 64))
    assert got[0]["products"] == 1 and got[0]["label"] == VAE_GROUPS[site][1]


def test_ops_group_plan_of_a_group_that_falls_apart(L):
    from inpaintnet_amd import ops
    options(L)
    descs = [fwd(256, 512, 512, 0), dgrad(256, 512, 512, 0)]
    got = ops.gemm_group_plan([dict(M=256, N=512, K=512, bias=True), dict(M=256, N=512, K=512, b_kmajor=True)])
    assert [g["products"] for g in got] == [2, 2]
    assert [g["label"] for g in got] == [r["label"] for r in group_plan(L, descs)[1]]
    assert got[0] == dict(ops.gemm_plan(256, 512, 512, bias=True), products=2)
    with pytest.raises(ValueError):
        ops.gemm_group_plan([dict(M=64, N=64, K=64)] * 5)
