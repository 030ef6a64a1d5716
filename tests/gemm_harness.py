"""What the float64 tests of the f32 GEMM launches share (tests/test_gpu_gemm_group.py: the grouped launches; tests/test_gpu_gemm_tables.py:
every entry of the single-product kernel tables): the epilogues in float64, the project's relmax measure, the labels of a profile and
Product -- operands, float64 reference and guarded destination of one product.  Importing it needs no GPU; building a Product does."""
import torch

from oracle import torch_ref as O

DEV = "cuda:0"
TOL = 2e-5
NT, NN, TN, TT = (0, 0), (0, 1), (1, 1), (1, 0)
LAYOUT_NAME = {NT: "NT", NN: "NN", TN: "TN", TT: "TT"}


def relmax(a, b):
    a = a.detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def dumped_labels(path):
    """The labels of a prof_dump, launch by launch."""
    return [line.split(",")[1] for line in open(str(path)).read().strip().splitlines()[1:]]


def sub(g, rows, cols, off):
    """(CPU values, device view) of a [rows, cols] operand at column `off` of a wider parent with an even leading dimension."""
    parent = torch.randn(rows, off + cols + 6 + cols % 2, generator=g)
    return parent[:rows, off:off + cols], parent.to(DEV)[:rows, off:off + cols]


def epilogue(v, epi, aux):
    if epi == 1:
        return O.selu(v)
    if epi == 2:
        return torch.relu(v)
    if epi == 3:                                            # * selu'(x) from aux = selu(x)
        return v * torch.where(aux > 0, torch.tensor(O.SELU_SCALE), aux + O.SELU_SCALE * O.SELU_ALPHA).double()
    if epi == 4:
        return v * aux.double()
    if epi == 5:
        return v * (aux > 0).double()
    return v


class Product:
    """Operands, float64 reference and guarded destination of one product."""

    def operands(self, g, p, akm, bkm):
        """(device A, device B, A . B^T in float64): column sub-views of wider parents, B at column p["boff"]."""
        M, N, K = p["M"], p["N"], p["K"]
        A, Ad = sub(g, K, M, 4) if akm else sub(g, M, K, 4)
        B, Bd = sub(g, K, N, p["boff"]) if bkm else sub(g, N, K, p["boff"])
        return Ad, Bd, (A.t() if akm else A).double() @ (B if bkm else B.t()).double()

    def __init__(self, g, p, layout):
        akm, bkm = p["layout"] or layout
        M, N, K = p["M"], p["N"], p["K"]
        Ad, Bd, ref = self.operands(g, p, akm, bkm)
        self.call = dict(A=Ad, B=Bd, M=M, N=N, K=K, a_kmajor=bool(akm), b_kmajor=bool(bkm), epi=p["epi"], accumulate=p["acc"])
        if p["bias"]:
            bias = torch.randn(N, generator=g)
            ref = ref + bias.double()
            self.call["bias"] = bias.to(DEV)
        aux = None
        if p["epi"] >= 3:
            aux, self.call["aux"] = sub(g, M, N, 2)
        ref = epilogue(ref, p["epi"], aux)
        # the destination: rows 1..M of a buffer of M + 2 rows, and (strided) the middle one of three interleaved matrices
        self.view = (lambda t: t[1:M + 1, 1, :]) if p["strided"] else (lambda t: t[1:M + 1])
        self.before = torch.randn((M + 2, 3, N) if p["strided"] else (M + 2, N), generator=g)
        if p["acc"]:
            ref = ref + self.view(self.before).double()
        else:
            self.view(self.before).fill_(float("nan"))
        self.buffer = self.before.to(DEV)
        self.call["out"] = self.view(self.buffer)
        self.ref = ref
        self.name = "M%d N%d K%d %s%s e%d %s%s" % (M, N, K, LAYOUT_NAME[(akm, bkm)], " bias" if p["bias"] else "", p["epi"],
                                                  "add" if p["acc"] else "store", " strided" if p["strided"] else "")

    def check(self, quiet=False):
        """Every element of the product written and within the bound; the rest of the destination's buffer bit-unchanged."""
        after = self.buffer.cpu()
        err = relmax(self.view(after), self.ref)
        if not quiet:
            print("    %-48s relmax %.3g" % (self.name, err))
        assert bool(torch.isfinite(self.view(after)).all()), self.name + ": elements left unwritten (NaN)"
        assert err < TOL, (self.name, err)
        before = self.before.clone()
        self.view(after).zero_()
        self.view(before).zero_()
        assert torch.equal(after, before), self.name + ": written outside the destination"
        return err
