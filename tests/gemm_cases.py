"""The case table of tests/test_gemm_cases.py (host) and tests/test_gpu_gemm_tables.py (GPU): for every entry of the five single-product
kernel tables of csrc/gemm.hip -- kGemvKernel[8], kTiledKernel[5][4], kTnDirectKernel[3], kKcKernel[4][2], kKsKernel[5][4] -- that a
planner can reach, the smallest products the planner routes to it under options it documents, at the edges of that kernel.  No GPU and
no torch here: shapes and options are written out, nothing is searched at run time; the host test re-checks every row against
inet_gemm_plan (DESIGN.md section 30 has the table in words).

An entry is (family, cfg, layout): family as in ops.GEMM_FAMILIES, cfg the row of the family's table (gemv: M - 1), layout one of
"NT", "NN", "TN", "TT" (A k-major: T.; B k-major: .N).  A case is a dict:
  opt2, opt3, opt5          inet_set_option keys 2 (forced LDS tile), 3 (forced split), 5 (direct kernels) for the call
  layout, M, N, K
  aoff, lda, boff, ldb      column offset and leading dimension of each operand inside its parent.  Aligned cases: offset 8, a margin of 8
                            columns behind; odd cases: offset 1 and an ODD leading dimension (margin >= 8 behind), so the rows start
                            4-byte aligned only -- what common.h ld4u and the buffer loads of the direct kernels promise to take
  bias, epi, acc, strided   the call's modes (strided: the destination is the middle one of three interleaved matrices)
  family, cfg, splits, zero_fill, two_pass      what the planner has to answer

kKsKernel[4][TN] (gemm_ks_kernel<4,6,true,true>) is in the table of kernels, but plan_ks skips tile 4 for a k-major A: no case can
reach it, and the host test asserts that a sweep never gets it."""
NT, NN, TN, TT = (0, 0), (0, 1), (1, 1), (1, 0)
LAYOUT_NAME = {NT: "NT", NN: "NN", TN: "TN", TT: "TT"}
FAMILIES = ("gemv", "tn_direct", "kc_direct", "ks", "tiled")

# the modes every shape runs: plain store (into a strided destination), bias + SELU, one aux epilogue, bias + accumulate
STORE = dict(bias=False, epi=0, acc=False, strided=True)
SELU = dict(bias=True, epi=1, acc=False, strided=False)
ADD = dict(bias=True, epi=0, acc=True, strided=False)
BIAS = dict(bias=True, epi=0, acc=False, strided=False)


def AUX(epi):
    return dict(bias=False, epi=epi, acc=False, strided=False)


def modes(aux_epi):
    return (STORE, SELU, AUX(aux_epi), ADD)


LINEAR = (STORE, ADD)                                       # what a grid split of plan_ks takes
SPLIT = (STORE, ADD, BIAS, SELU, AUX(4))                    # a split LDS-tiled / TN-direct call: zero fill, atomics, bias once, two passes


def place(cols, odd):
    """(column offset, leading dimension) of an operand of `cols` columns."""
    if not odd:
        return 8, cols + 16
    ld = cols + 9
    return 1, ld + 1 - ld % 2


def case(family, cfg, layout, M, N, K, mode, opt2=-1, opt3=0, opt5=1, splits=1, odd=False):
    aoff, lda = place(M if layout[0] else K, odd)
    boff, ldb = place(N if layout[1] else K, odd)
    return dict(mode, opt2=opt2, opt3=opt3, opt5=opt5, layout=layout, M=M, N=N, K=K, aoff=aoff, lda=lda, boff=boff, ldb=ldb,
                family=FAMILIES.index(family), cfg=cfg, splits=splits, zero_fill=int(splits > 1 and not mode["acc"]),
                two_pass=int(splits > 1 and mode["epi"] != 0))


CASES = {}


def add(family, cfg, layout, shapes, mode_list, **kw):
    CASES.setdefault((family, cfg, LAYOUT_NAME[layout]), []).extend(
        case(family, cfg, layout, M, N, K, m, **kw) for (M, N, K) in shapes for m in mode_list)


# ---- gemv_rows_kernel<M>, M = 1..8: one wave per column, four columns per workgroup.  N = 1 and 7 (the waves beyond N write nothing);
# K = 1, 3 (scalar loop only), 4 (one 16-byte load), 261 (a second pass of the 256-stride loop and a scalar tail).  N = 7: odd operands.
for M in range(1, 9):
    for N in (1, 7):
        add("gemv", M - 1, NT, [(M, N, K) for K in (1, 3, 4, 261)], modes(3 + (M + N) % 3), odd=N == 7)

# ---- gemm_kernel<TM,TN,AKM,BKM>, forced with key 2: the whole tile, 2 x 2 tiles partial in M and in N (odd operands: the 16-byte loads
# of the fast path on 4-byte aligned rows), a product smaller than every tile; K = 1, 31 (one partial chunk), 32 (one full chunk), 33 and
# 70 (full chunks and a tail).  Key 3 = 2 at K = 70: k_per_split = 64, the second range is a 6-deep tail.
TILES = ((64, 64), (128, 128), (192, 64), (192, 128), (192, 192))
for cfg, (tm, tn) in enumerate(TILES):
    for li, layout in enumerate((NT, NN, TN, TT)):
        for si, (M, N) in enumerate(((tm, tn), (tm + 5, tn + 3), (5, 7))):
            add("tiled", cfg, layout, [(M, N, K) for K in (1, 31, 32, 33, 70)], modes(3 + (cfg + li + si) % 3), opt2=cfg, odd=si == 1)
            add("tiled", cfg, layout, [(M, N, 70)], SPLIT, opt2=cfg, opt3=2, splits=2, odd=si == 1)

# ---- gemm_tn_direct_kernel<TA,TB>, key 5 = 2 (without its size thresholds): one tile per configuration; K = 64 (the depth of the
# register pipeline), 65 and 131 (the k row of the upper half-wave past the range reads 0), K = 131 in two ranges of 66 + 65; a grid of
# 8 workgroups (the XCD renumbering, taken when gridDim.x % 8 == 0) next to the grids of 1 and 2.
for cfg, (M, N), (M8, N8) in ((0, (192, 128), (192, 1024)), (1, (128, 128), (256, 512)), (2, (192, 192), (1536, 192))):
    add("tn_direct", cfg, TN, [(M, N, 64)], modes(3 + cfg), opt5=2, odd=True)
    add("tn_direct", cfg, TN, [(M, N, 65), (M8, N8, 65)], modes(3 + (cfg + 1) % 3), opt5=2)
    add("tn_direct", cfg, TN, [(M, N, 131)], modes(3 + (cfg + 2) % 3), opt5=2, opt3=1)          # (one range: the cost model takes two)
    add("tn_direct", cfg, TN, [(M, N, 131)], SPLIT, opt5=2, opt3=2, splits=2)

# ---- gemm_kc_direct_kernel<TA,TB,BKM>, key 5 = 2, K = 64 (one block of the 4-group pipeline) and 128: tiles 192x64 and 128x128 alone and
# on a grid of 8; 192x192 and 192x128 are picked once the next smaller tile needs a second round of 256 workgroups (86 / 88 and 129 /
# 136 workgroups: grids that are no multiple of 8, with odd operands, and multiples of 8).
for layout in (NT, NN):
    for cfg, first, more in ((0, (384, 8256, 64), [(1536, 2112, 64)]), (1, (576, 5504, 64), [(3264, 1024, 64)]),
                             (2, (192, 64, 64), [(192, 512, 64), (192, 64, 128)]), (3, (128, 128, 64), [(256, 512, 64), (128, 128, 128)])):
        add("kc_direct", cfg, layout, [first], modes(3 + cfg % 3), opt5=2, odd=True)
        add("kc_direct", cfg, layout, more, modes(3 + (cfg + 1) % 3), opt5=2)

# ---- gemm_ks_kernel<TA,TB,AKM,BKM>, the defaults.  Tile 2 (32x32) alone and on a grid of 8; tile 1 (64x32) where 32x32 needs a second
# round; tile 0 (64x64) and tile 4 (64x96, k-contiguous A only) where the smaller ones need a third: all at K = 64, the smallest K the
# kernel takes (one k group per wave).  A k-major A also at K = 74 = 80 - 6 (the last group reads the zero-returning tail) and, with key
# 3 = 2 and K = 2048, on a grid split into two k ranges (plan_ks: k-major A, K / 2 >= 1024, no epilogue).
for layout in (NT, NN, TN):
    for cfg, (M, N), more, split in ((0, (192, 2752), [], (320, 832)), (1, (576, 576), [], (320, 416)),
                                       (2, (32, 32), [(64, 128, 64)], (32, 32)), (4, (576, 1824), [], None)):
        if cfg == 4 and layout == TN:
            continue                                        # plan_ks: tile 4 is for a k-contiguous A
        add("ks", cfg, layout, [(M, N, 64)], modes(3 + cfg % 3), odd=True)
        add("ks", cfg, layout, more, modes(4))
        if layout == TN:
            add("ks", cfg, layout, [(M, N, 74)], modes(5))
            add("ks", cfg, layout, [split + (2048,)], LINEAR, opt3=2, splits=2)
# tile 3 (96x64): a k-major A with K >= 2048, M no multiple of 64 (TN-direct does not take it).  The linear modes split the grid by
# themselves at 86 tiles, under the defaults and with the workgroup split-K kernel asked first (key 5 = 4); a non-linear epilogue keeps
# one range and needs 129 tiles; K = 2058 = 2064 - 6; key 3 = 2.
add("ks", 3, TN, [(96, 5504, 2048)], LINEAR, splits=2, odd=True)
add("ks", 3, TN, [(96, 5504, 2048)], LINEAR, opt5=4, splits=2)
add("ks", 3, TN, [(96, 5504, 2058)], LINEAR, splits=2)
add("ks", 3, TN, [(288, 2752, 2048)], (SELU, AUX(3)), odd=True)
add("ks", 3, TN, [(288, 2752, 2048)], (SELU, AUX(4)), opt5=4)
add("ks", 3, TN, [(288, 2752, 2058)], (SELU, AUX(5)))
add("ks", 3, TN, [(480, 832, 2048)], LINEAR, opt3=2, splits=2)
