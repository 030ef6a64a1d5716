"""Every entry of the single-product kernel tables of csrc/gemm.hip -- kGemvKernel, kTiledKernel, kTnDirectKernel, kKcKernel, kKsKernel:
51 instantiations a planner can reach -- launched through ops.gemm at its edge shapes (tests/gemm_cases.py; tests/test_gemm_cases.py
checks on the host that every case lands on its entry) and compared with float64, element by element.

Method.  Operands are sub-views of parents in which every other element is NaN: the columns in front of and behind the operand and a
row in front and behind, so an element read from outside the operand and used shows as NaN in the result.  (The kernels' own
read-ahead -- the direct kernels fetch k groups past K that no MFMA uses, clamped rows of the LDS-tiled kernel -- stays inside the
parent by their stated contract.)  A stored destination is NaN beforehand (an unwritten element shows) and lies inside a larger buffer
whose other elements must come back bit-equal (tests/gemm_harness.py Product).  All cases of an entry run under one profile; its
labels must be the labels ops.gemm_plan gave, call by call: the launches followed the plan.  (run() opens ONE profile scope per call, behind
the zero fill and around the kernel and the epilogue pass: one label per call; the plan's `launches` is checked against its flags.)

Reference: epi(A . B^T + bias, aux) (+ C0) in float64 on the CPU.  Two bounds, both on every element:
  * the project's relmax < 2e-5 (max abs error over max abs reference);
  * |got - ref| <= bound, an element-wise worst case.  With u = 2^-24 and S = |A| . |B|^T + |bias| + |C0| in float64,
        bound_pre = 2 (K + 4) u S
    is twice the bound gamma_n S, n = K + 4, of a sum of K exact products, a bias, a previous value and up to two more partial sums in
    ANY order (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., section 4.2; the f32 products of v_mfma_f32_*_f32 are
    exact in the sense that each enters the sum with one rounding) -- twice, because the matrix core's internal accumulation is not
    documented as round-to-nearest after every step.  It passes the epilogue multiplied by the epilogue's Lipschitz factor -- 1 for
    none, ReLU and epi 5, SELU_SCALE * SELU_ALPHA for SELU, |selu'(aux)| for epi 3, |aux| for epi 4 -- and the epilogue's own
    arithmetic adds 4 u |out| (a multiply by aux, the f32 constant of selu') or, for SELU, 8 u (|out| + SELU_SCALE * SELU_ALPHA):
    selu_f calls expf, 1 ulp = 2 u at most (HIP math API, "Single precision mathematical functions", expf: maximum ulp error 1), on a
    value <= 1, then a subtraction and two multiplications.
No element is excluded.  The largest |got - ref| / bound of every entry is printed (`-s`); DESIGN.md section 30 has the maxima per
family as measured on an MI355X.  Above 0.5 an element would exceed the bound without its factor 2."""
import collections

import pytest
import torch

from oracle import torch_ref as O
from tests import gemm_cases as GC
from tests.gemm_harness import DEV, LAYOUT_NAME, Product, dumped_labels
from tests.test_gemm_cases import ENTRIES

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from inpaintnet_amd import ops

U = 2.0 ** -24
SA = O.SELU_SCALE * O.SELU_ALPHA
NAN = float("nan")
WORST = collections.defaultdict(float)                      # family -> largest err / bound seen in this session


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


def guarded(values, off, ld):
    """The device view of `values` at column `off` of a [rows + 2, ld] parent whose other elements are NaN."""
    rows, cols = values.shape
    parent = torch.full((rows + 2, ld), NAN)
    parent[1:rows + 1, off:off + cols] = values
    return parent.to(DEV)[1:rows + 1, off:off + cols]


class GuardedProduct(Product):
    """A case of tests/gemm_cases.py: NaN-guarded operands, and next to the float64 reference the element-wise bound.  The values of A
    and B, A . B^T and |A| . |B|^T depend on (layout, M, N, K) alone and are shared by the modes and options a shape runs under."""
    shared = {}

    def operands(self, g, p, akm, bkm):
        M, N, K = p["M"], p["N"], p["K"]
        key = (akm, bkm, M, N, K)
        if key not in self.shared:
            gs = torch.Generator().manual_seed(7 + 1000003 * M + 1009 * N + 13 * K + 2 * akm + bkm)
            A = torch.randn((K, M) if akm else (M, K), generator=gs)
            B = torch.randn((K, N) if bkm else (N, K), generator=gs)
            a, b = (A.t() if akm else A).double(), (B if bkm else B.t()).double()
            self.shared[key] = (A, B, a @ b, a.abs() @ b.abs())
        A, B, prod, self.absprod = self.shared[key]
        return guarded(A, p["aoff"], p["lda"]), guarded(B, p["boff"], p["ldb"]), prod

    def __init__(self, g, case):
        super().__init__(g, case, None)
        assert self.call["A"].stride(0) == case["lda"] and self.call["B"].stride(0) == case["ldb"]
        epi, K = case["epi"], case["K"]
        S = self.absprod
        if case["bias"]:
            S = S + self.call["bias"].cpu().double().abs()
        if case["acc"]:
            S = S + self.view(self.before).double().abs()
        aux = self.call["aux"].cpu().double() if epi >= 3 else None
        lip = 1.0                                           # none, ReLU, epi 5 (v or 0)
        if epi == 1:
            lip = SA
        elif epi == 3:
            lip = torch.where(aux > 0, torch.tensor(O.SELU_SCALE, dtype=torch.float64), aux + SA).abs()
        elif epi == 4:
            lip = aux.abs()
        # SELU: expf is good to 1 ulp = 2 u (HIP math API reference, single precision mathematical functions: expf, maximum ulp error 1)
        own = 8 * U * (self.ref.abs() + SA) if epi == 1 else 4 * U * self.ref.abs()
        self.bound = lip * (2 * (K + 4) * U * S) + own
        self.name += " opt %d/%d/%d a+%d/%d b+%d/%d" % (case["opt2"], case["opt3"], case["opt5"], case["aoff"], case["lda"],
                                                       case["boff"], case["ldb"])

    def check(self):
        """The harness's checks (written everywhere, relmax, nothing written outside), then every element against its own bound."""
        got = self.view(self.buffer.cpu()).double()
        assert bool(torch.isfinite(got).all()), self.name + ": NaN in the result -- an element left unwritten, or one read outside an operand"
        super().check(quiet=True)
        err = (got - self.ref).abs()
        ratio = err / self.bound
        worst = float(ratio.max())
        assert worst <= 1.0, (self.name, worst, int((ratio > 1.0).sum()), float(err.max()))
        return worst


@pytest.mark.parametrize("entry", ENTRIES, ids=["%s-%d-%s" % e for e in ENTRIES])
def test_table_entry(entry, tmp_path):
    """One instantiation: all its cases under one profile."""
    family, cfg, lay = entry
    GuardedProduct.shared.clear()
    g = torch.Generator().manual_seed(4000 + 97 * ENTRIES.index(entry))
    products, want = [], []
    ops.prof_enable(True)
    try:
        for c in GC.CASES[entry]:
            ops.set_option(2, c["opt2"])
            ops.set_option(3, c["opt3"])
            ops.set_option(5, c["opt5"])
            akm, bkm = c["layout"]
            plan = ops.gemm_plan(c["M"], c["N"], c["K"], a_kmajor=bool(akm), b_kmajor=bool(bkm), lda=c["lda"], ldb=c["ldb"],
                                 bias=c["bias"], epi=c["epi"], accumulate=c["acc"])
            assert (ops.GEMM_FAMILIES[plan["family"]], plan["cfg"], LAYOUT_NAME[c["layout"]]) == entry, (c, plan)
            assert (plan["splits"], plan["zero_fill"], plan["two_pass"]) == (c["splits"], c["zero_fill"], c["two_pass"]), (c, plan)
            assert plan["products"] == 1 and plan["launches"] == 1 + c["zero_fill"] + c["two_pass"], (c, plan)
            p = GuardedProduct(g, c)
            ops.gemm(p.call["A"], p.call["B"], c["M"], c["N"], c["K"], a_kmajor=bool(akm), b_kmajor=bool(bkm), bias=p.call.get("bias"),
                     epi=c["epi"], aux=p.call.get("aux"), out=p.call["out"], accumulate=c["acc"])
            products.append(p)
            want.append(plan["label"])
        torch.cuda.synchronize()
        ops.prof_dump(str(tmp_path / "_inet_tables.csv"))
    finally:
        ops.prof_enable(False)
        GuardedProduct.shared.clear()
    assert all(want) and dumped_labels(tmp_path / "_inet_tables.csv") == want              # the launches followed the plan
    worst = max(p.check() for p in products)
    WORST[family] = max(WORST[family], worst)
    print("\n  %s cfg %d %s: %d cases, largest err/bound %.3f (family so far: %.3f)" % (family, cfg, lay, len(products), worst,
                                                                                      WORST[family]))
