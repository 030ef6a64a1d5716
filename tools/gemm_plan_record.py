#!/usr/bin/env python3
"""Record which kernel the f32 GEMM dispatcher (csrc/gemm.hip) picks for every case of a fixed list, on a GPU:
    python tools/gemm_plan_record.py [out.csv.gz]       (default tests/golden/gemm_plans.csv.gz; read it with zcat)
Each case is one ops.gemm / ops.gemm_batched call under ops.prof_enable; the row keeps the case, the option settings (inet_set_option
keys 2, 3, 5) and the `label;gflop;mbytes` of every GEMM launch the call made (a batched call that falls back makes several).
tests/test_gemm_plan.py holds inet_gemm_plan to these rows on the CPU.  The list lives here (cases()), so whoever changes a cost
constant or a threshold regenerates the fixture with the build they trust and reads the diff.  Only ops.gemm, ops.gemm_batched,
ops.set_option and ops.prof_* are used.  All operands are views of three zero-filled buffers: only the launch is of interest."""
import csv
import gzip
import io
import os
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

FIELDS = ("akm", "bkm", "M", "N", "K", "lda", "ldb", "epi", "acc", "nbatch", "opt2", "opt3", "opt5", "launches")
LAYOUTS = ((0, 0), (0, 1), (1, 1), (1, 0))

# the parametrisations of the f32 GEMM tests of tests/test_gpu_kernels.py
T_LAYOUTS = [(5, 12, 4), (70, 33, 10), (256, 1536, 512), (130, 200, 1000), (1536, 512, 6144), (48, 1536, 6144), (300, 7, 37)]
T_GEMV = [(1, 1024, 256), (4, 1536, 512), (4, 512, 512), (8, 130, 1030), (3, 48, 10), (2, 7, 5)]
T_TN = [(1536, 512, 6144), (1536, 1024, 1000), (384, 256, 131), (128, 128, 64), (576, 576, 777), (1024, 2048, 256)]
T_KC = [(6144, 1536, 1024), (6144, 1024, 1536), (6144, 512, 1536), (384, 256, 64), (192, 64, 192), (1152, 768, 320)]
T_KS = [(256, 1024, 2048), (1536, 512, 1024), (1024, 2048, 256), (256, 256, 1024), (64, 32, 64), (32, 32, 1008), (128, 96, 336),
        (1536, 512, 6144), (1536, 1024, 6144), (192, 128, 2064)]
T_BATCHED = [(1536, 512, 6144, 2), (1536, 1024, 6144, 2), (1536, 512, 1536, 2), (1536, 512, 6144, 3), (96, 40, 300, 2),
             (1536, 512, 6140, 2)]                                                # the last: K is no multiple of the split
# named in gemm.hip's comments and DESIGN.md sections 4 / 5
NAMED = [(12288, 1024, 256), (1024, 1536, 512), (6144, 3072, 1024), (6144, 1024, 3072)]
# one shape on each side of the planners' thresholds
EDGES = ([(384, 256, k) for k in (48, 64, 112, 128, 240, 256, 752, 768, 1008, 1024, 2032, 2048, 1000, 1040)] +   # K; K & 15, K & 63
         [(1536, 512, k) for k in (1536, 3072, 12288)] +                          # K / split against 768 (TN-direct), 1024 (ks)
         [(2304, 3072, 512), (2304, 2880, 512), (1152, 1152, 512),                # 192 / 180 / 36 workgroups of 192 x 192 (kc-direct)
          (768, 512, 6144), (384, 256, 6144), (192, 128, 6144),                   # tiles x splits around 192 (TN-direct)
          (2048, 2048, 256), (2048, 2112, 256),                                   # 1024 / 1056 tiles of 64 x 64 (ks)
          (8, 512, 512), (9, 512, 512), (8, 64, 64), (9, 64, 64)])                # gemv up to 8 rows
FORCED = [(5, 12, 4), (70, 33, 10), (256, 1536, 512), (130, 200, 1000), (1536, 512, 6144), (384, 256, 131), (128, 128, 64),
          (6144, 1536, 1024), (192, 64, 192), (256, 256, 1024), (12288, 1024, 256), (4, 512, 512)]
# leading dimensions on each side of the direct kernels' 2e9-byte operand guard: rows x ld x 4 with 6144 rows
LD_BELOW, LD_ABOVE, LD_ROWS = 81300, 81400, 6144


def shapes():
    seen, out = set(), []
    for s in T_LAYOUTS + T_GEMV + T_TN + T_KC + T_KS + NAMED + EDGES:
        if s not in seen:
            seen.add(s)
            out.append(s)
    return out


def case(akm, bkm, M, N, K, epi=0, acc=0, lda=0, ldb=0, nbatch=1, opt2=-1, opt3=0, opt5=1):
    return dict(akm=akm, bkm=bkm, M=M, N=N, K=K, lda=lda or (M if akm else K), ldb=ldb or (N if bkm else K), epi=epi, acc=acc,
                nbatch=nbatch, opt2=opt2, opt3=opt3, opt5=opt5)


def cases():
    out = []
    for M, N, K in shapes():
        for akm, bkm in LAYOUTS:
            for epi in (0, 1):
                for acc in (0, 1):
                    out += [case(akm, bkm, M, N, K, epi, acc, opt5=o5) for o5 in range(5)]
    for M, N, K in T_KS:                                     # the tests' K - 6 variants (k-major A)
        for bkm in (1, 0):
            for epi in (0, 1):
                for acc in (0, 1):
                    out += [case(1, bkm, M, N, K - 6, epi, acc, opt5=o5) for o5 in range(5)]
    # the 2e9 guard: A or B with 6144 rows of a long leading dimension; one family per layout and mode
    for akm, bkm in LAYOUTS:
        long_a = (1536, 512, LD_ROWS) if akm else (LD_ROWS, 512, 1024)       # A's rows are K (k-major) or M
        long_b = (1536, 512, LD_ROWS) if bkm else (1536, LD_ROWS, 1024)      # B's rows are K (k-major) or N
        for ld in (LD_BELOW, LD_ABOVE):
            for o5 in range(5):
                out.append(case(akm, bkm, *long_a, lda=ld, opt5=o5))
                out.append(case(akm, bkm, *long_b, ldb=ld, opt5=o5))
    for M, N, K in FORCED:
        for akm, bkm in LAYOUTS:
            for o2 in (-1, 0, 1, 2, 3, 4):
                for o3 in (0, 2, 4):
                    if o2 < 0 and o3 == 0:
                        continue
                    out += [case(akm, bkm, M, N, K, epi, 0, opt2=o2, opt3=o3) for epi in (0, 1)]
                    if (M, N, K) in FORCED[:3]:
                        out.append(case(akm, bkm, M, N, K, 1, 1, opt2=o2, opt3=o3))
    for M, N, K, nb in T_BATCHED:
        for o5 in range(5):
            out.append(case(1, 1, M, N, K, acc=1, lda=nb * M, nbatch=nb, opt5=o5))
    out.append(case(1, 1, 1536, 512, 6144, acc=1, lda=2 * 1536, nbatch=2, opt3=8))
    out.append(case(1, 1, 1536, 512, 6144, acc=1, lda=2 * 1536, nbatch=2, opt2=0))
    return out


def extent(rows, cols, ld):
    return (rows - 1) * ld + cols


def main():
    import torch
    from inpaintnet_amd import ops
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "tests", "golden", "gemm_plans.csv.gz")
    todo = cases()
    need = [0, 0, 0]
    for c in todo:
        nb = c["nbatch"]
        a = extent(c["K"], c["M"], c["lda"]) if c["akm"] else extent(c["M"], c["K"], c["lda"])
        b = extent(c["K"], c["N"], c["ldb"]) if c["bkm"] else extent(c["N"], c["K"], c["ldb"])
        if nb > 1:                                           # A interleaved (problem i at column i*M), B and C one after the other
            a = extent(c["K"], nb * c["M"], c["lda"])
            b, cc = nb * c["K"] * c["N"], nb * c["M"] * c["N"]
        else:
            cc = c["M"] * c["N"]
        need = [max(need[0], a), max(need[1], b), max(need[2], cc)]
    dev = torch.device("cuda", 0)
    bufA, bufB, bufC = (torch.zeros(n, dtype=torch.float32, device=dev) for n in need)

    def view(buf, rows, cols, ld):
        assert extent(rows, cols, ld) <= buf.numel()
        return buf.as_strided((rows, cols), (ld, 1))

    tmp = os.path.join(tempfile.mkdtemp(), "l.csv")
    rows = []
    try:
        for c in todo:
            M, N, K = c["M"], c["N"], c["K"]
            A = view(bufA, K, M, c["lda"]) if c["akm"] else view(bufA, M, K, c["lda"])
            B = view(bufB, K, N, c["ldb"]) if c["bkm"] else view(bufB, N, K, c["ldb"])
            Cv = view(bufC, M, N, N)
            ops.set_option(2, c["opt2"])
            ops.set_option(3, c["opt3"])
            ops.set_option(5, c["opt5"])
            ops.prof_enable(True)
            if c["nbatch"] > 1:
                ops.gemm_batched(A, B, Cv, M, N, K, c["nbatch"], M, K * N, M * N, a_kmajor=True, b_kmajor=True)
            else:
                ops.gemm(A, B, M, N, K, a_kmajor=bool(c["akm"]), b_kmajor=bool(c["bkm"]), epi=c["epi"], out=Cv,
                         accumulate=bool(c["acc"]))
            ops.prof_dump(tmp)
            ops.prof_enable(False)
            got = [r for r in csv.DictReader(open(tmp)) if r["class"] == "0"]
            rows.append(dict(c, launches="|".join(f"{r['label']};{r['gflop']};{r['mbytes']}" for r in got)))
    finally:
        ops.prof_enable(False)
        ops.set_option(2, -1)
        ops.set_option(3, 0)
        ops.set_option(5, 1)
    torch.cuda.synchronize()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    text = io.StringIO()
    w = csv.DictWriter(text, FIELDS, lineterminator="\n")
    w.writeheader()
    w.writerows(rows)
    with open(out_path, "wb") as f:                          # (no name, no time: the same rows give the same file)
        with gzip.GzipFile(filename="", mode="wb", fileobj=f, mtime=0) as z:
            z.write(text.getvalue().encode())
    print(f"{len(rows)} cases -> {out_path}")


if __name__ == "__main__":
    main()
