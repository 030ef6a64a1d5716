"""The helper kernels of csrc/pointwise.hip, ce.hip (ce_kernel), latent.hip, optim.hip and sample_rows.hip and the small entry points in front of them, each alone through the C-ABI and at its
edges: vocabulary widths around the 64-lane wave, one row more than the resident waves, strided operands with poisoned padding,
ties, NaN and infinities, null optional outputs, the tail of the float4 loops, both paths of the embedding gradient.

References are float64 (tests/pointwise_ref.py).  Where a kernel only ADDS, the inputs are integer-valued float32 in [-8, 8] and
row scales in {0, 2}: every partial sum stays below 2^24, any order of addition is exact, and the result must EQUAL the reference --
a dropped or doubled row, a wrong block boundary or a lost column shows at any size.  Elsewhere the bounds are the project's:
loss 1e-4 relative, dW 1e-5 of the tensor's maximum, z 1e-6, KL 1e-5, products 2e-5 of the maximum."""
import numpy as np
import pytest
import torch

from tests import pointwise_ref as R

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from inpaintnet_amd import _lib, ops
    from inpaintnet_amd._lib import check, ptr, stream_ptr

DEV = "cuda:0"
SENT = -777.25                      # what untouched padding and gaps hold
NAN, INF = float("nan"), float("inf")


def relmax(a, b):
    a = a.detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def gen(*key):
    return torch.Generator().manual_seed(hash(tuple(int(k) for k in key)) % (2 ** 31))


def ints(shape, g, lo=-8, hi=8):
    """Integer-valued float32 in [lo, hi]."""
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def sync():
    ops.side_join()
    torch.cuda.synchronize()


def strided(t, pad, fill):
    """A device copy of the 2-D tensor t whose rows are `pad` elements apart more than they are long, the padding holding `fill`
    (alternating with NaN / +inf where fill is the string "poison").  -> (view [rows, cols], whole buffer)."""
    rows, cols = t.shape
    buf = torch.empty(rows, cols + pad)
    if fill == "poison":
        buf[:, cols:] = torch.tensor([INF, NAN])[torch.arange(pad) % 2]
        buf[1::2, cols:] = torch.tensor([NAN, INF])[torch.arange(pad) % 2]
    else:
        buf[:, cols:] = fill
    buf[:, :cols] = t
    buf = buf.to(DEV)
    return buf[:, :cols], buf


# =============================================================================== 1. inet_argmax
def argmax_raw(w, V, out, stride=1):
    check(_lib.lib().inet_argmax(ptr(w), w.stride(0), w.shape[0], V, ptr(out), stride, stream_ptr()), "inet_argmax")


@pytest.mark.parametrize("rows", [1, 3, 4097])
@pytest.mark.parametrize("V", [1, 2, 63, 64, 65, 128, 129, 1000])
def test_argmax_rows_widths_and_padding(rows, V):
    """randn rows (no ties) and rows of three distinct values (ties everywhere: the lowest index wins), contiguous through
    ops.argmax_rows and with ld > V, the padding holding +inf and NaN.  4097 rows: one more than the 4096 waves of the launch."""
    g = gen(1, rows, V)
    for w in (torch.randn(rows, V, generator=g), ints((rows, V), g, 0, 2)):
        want = R.argmax_first(w)
        assert torch.equal(ops.argmax_rows(w.to(DEV)).cpu(), want)
        view, _ = strided(w, 5, "poison")
        assert torch.equal(ops.argmax_rows(view).cpu(), want)


def test_argmax_strided_output_leaves_the_gaps():
    g = gen(2)
    w = torch.randn(70, 65, generator=g)
    out = torch.full((70 * 3,), -7, dtype=torch.int64, device=DEV)
    argmax_raw(w.to(DEV), 65, out, stride=3)
    out = out.cpu().view(70, 3)
    assert torch.equal(out[:, 0], R.argmax_first(w))
    assert bool((out[:, 1:] == -7).all())


def special_rows(V):
    """Rows whose argmax is decided by a rule, not by the data."""
    g = gen(3, V)
    base = torch.randn(V, generator=g).clamp(-3, 3)
    rows = []
    r = base.clone(); r[0] = 5.0; rows.append(r)                                   # maximum first
    r = base.clone(); r[V - 1] = 5.0; rows.append(r)                               # maximum last
    r = base.clone(); r[V // 2] = 5.0; r[V - 1] = 5.0; rows.append(r)              # duplicated: the first wins
    r = base.clone(); r[0] = 5.0; r[V - 1] = 5.0; rows.append(r)
    if V > 64:
        r = base.clone(); r[63] = 5.0; r[64] = 5.0; rows.append(r)                 # across the lane wrap
        r = base.clone(); r[64] = 5.0; r[1] = 5.0; rows.append(r)                  # the later lane pass holds the lower index
    rows.append(torch.full((V,), 1.5))                                             # all equal
    rows.append(torch.full((V,), -INF))                                            # all -inf
    r = base.clone(); r[V - 1] = INF; rows.append(r)                               # +inf among finite values
    r = base.clone(); r[V // 2] = INF; r[V - 1] = INF; rows.append(r)
    r = torch.full((V,), -0.0); r[V - 1] = 0.0; rows.append(r)                     # -0.0 == +0.0: index 0
    r = torch.full((V,), 0.0); r[0] = -0.0; rows.append(r)
    return torch.stack(rows)


@pytest.mark.parametrize("V", [1, 2, 63, 64, 65, 128, 129, 1000])
def test_argmax_ties_infinities_and_signed_zeros(V):
    w = special_rows(V)
    want = R.argmax_first(w)
    assert torch.equal(ops.argmax_rows(w.to(DEV)).cpu(), want), (V, want)
    view, _ = strided(w, 3, "poison")
    assert torch.equal(ops.argmax_rows(view).cpu(), want)


def nan_rows(V):
    g = gen(4, V)
    base = torch.randn(V, generator=g)
    rows = [torch.full((V,), NAN)]                                                 # all NaN: index 0
    for at in sorted({0, V // 2, V - 1, min(64, V - 1), min(63, V - 1)}):
        r = base.clone(); r[at] = NAN; rows.append(r)                              # one NaN among finite values: the NaN
    r = base.clone(); r[V - 1] = NAN; r[0] = INF; rows.append(r)                   # NaN together with +inf: still the NaN
    r = base.clone(); r[0] = NAN; r[V - 1] = INF; rows.append(r)
    r = base.clone(); r[V // 2] = NAN; r[V - 1] = NAN; rows.append(r)              # two NaN: the first
    r = torch.full((V,), -INF); r[V - 1] = NAN; rows.append(r)
    return torch.stack(rows)


@pytest.mark.parametrize("V", [1, 2, 63, 64, 65, 128, 129, 1000])
def test_argmax_of_rows_with_nan_follows_numpy_and_stays_inside_the_vocabulary(V):
    """np.argmax's rule (the one csrc/arnn_gen.hip follows): a NaN is the maximum, the lowest index wins.  Whatever a row holds the
    result is an index of the row: the per-tick loops gather an embedding row with it on the next tick."""
    w = nan_rows(V)
    got = ops.argmax_rows(w.to(DEV)).cpu()
    assert int(got.min()) >= 0 and int(got.max()) < V, got
    assert torch.equal(got, R.argmax_first(w)), (got, R.argmax_first(w))


# =============================================================================== 2. inet_cross_entropy(_ex)
CE_SHAPES = ([(5, V) for V in (1, 2, 12, 63, 64, 65, 130, 300)] + [(1, V) for V in (1, 64, 65, 300)] +
             [(48, V) for V in (2, 12, 63, 130)] + [(6144, V) for V in (1, 12, 64, 65, 300)])


def relu_logits(rows, V, g):
    """Post-ReLU logits as the decoder produces them: about half zeros, every third row all zero; targets cover 0 and V - 1."""
    w = torch.relu(torch.randn(rows, V, generator=g))
    w[::3] = 0.0
    t = torch.randint(0, V, (rows,), generator=g)
    t[0] = 0
    t[-1] = V - 1
    return w, t


def run_ce(w, t, scale=1.0, out_scale=1.0, out0=(0.0, 0.0)):
    """inet_cross_entropy on strided weights (NaN / inf in the padding) into a strided dW (sentinel in the padding)."""
    rows, V = w.shape
    wv, _ = strided(w, 3, "poison")
    dv, dbuf = strided(torch.zeros(rows, V), 2, SENT)
    out = torch.tensor(out0, device=DEV)
    ops.cross_entropy(wv, t.to(DEV), out, dW=dv, scale=scale, out_scale=out_scale)
    torch.cuda.synchronize()
    assert bool((dbuf[:, V:] == SENT).all()), "dW padding written"
    return float(out[0]), float(out[1]), dv.cpu()


@pytest.mark.parametrize("rows,V", CE_SHAPES)
def test_cross_entropy_shapes_strides_and_accumulation(rows, V):
    w, t = relu_logits(rows, V, gen(5, rows, V))
    loss, correct, dW = R.cross_entropy_ref(w, t, scale=0.37)
    # sums: accumulated into live words; the count is a sum of ones, exact
    got_loss, got_correct, got_dW = run_ce(w, t, scale=0.37, out0=(3.0, 5.0))
    print(f"rows {rows} V {V}: loss {got_loss} ref {3.0 + loss}; correct {got_correct} ref {5.0 + correct}; dW {relmax(got_dW, dW):.2e}")
    assert abs(got_loss - (3.0 + loss)) <= 1e-4 * abs(3.0 + loss)
    assert got_correct == 5.0 + correct
    assert relmax(got_dW, dW) < 1e-5
    # means: out_scale = 1 / rows.  The count's partial sums are exact integers, each multiplied by float32(1 / rows) and added by at
    # most 128 atomics: 129 roundings of 2^-24 relative = 8e-6 of the result at worst
    got_loss, got_correct, _ = run_ce(w, t, scale=0.37, out_scale=1.0 / rows, out0=(0.5, 0.25))
    assert abs(got_loss - (0.5 + loss / rows)) <= 1e-4 * abs(0.5 + loss / rows)
    assert abs(got_correct - (0.25 + correct / rows)) <= 1e-5 * (0.25 + correct / rows)


@pytest.mark.parametrize("V", [1, 2, 64, 65, 300])
def test_cross_entropy_of_all_zero_rows(V):
    """A row ReLU has emptied: its argmax is index 0 and its loss log V."""
    rows = 7
    t = torch.arange(rows) % V
    got_loss, got_correct, got_dW = run_ce(torch.zeros(rows, V), t)
    assert abs(got_loss - rows * np.log(V)) <= 1e-4 * rows * np.log(V)
    assert got_correct == float((t == 0).sum())
    onehot = torch.nn.functional.one_hot(t, V).double()
    assert relmax(got_dW, 1.0 / V - onehot) < 1e-5


@pytest.mark.parametrize("V", [2, 65, 130, 300])
def test_cross_entropy_counts_only_the_first_of_tied_maxima(V):
    rows = 600
    g = gen(6, V)
    w = ints((rows, V), g, 0, 3)
    pairs = [(0, V - 1), (V // 2 - 1, V // 2)] + ([(63, 64), (1, 64)] if V > 64 else []) + ([(64, V - 1)] if V > 65 else [])
    t = torch.empty(rows, dtype=torch.int64)
    for r in range(rows):
        i, j = pairs[r % len(pairs)]
        w[r, i] = w[r, j] = 5.0
        t[r] = i if (r // len(pairs)) % 2 == 0 else j
    first = sum(1 for r in range(rows) if (r // len(pairs)) % 2 == 0)
    loss, correct, dW = R.cross_entropy_ref(w, t)
    assert correct == first
    got_loss, got_correct, got_dW = run_ce(w, t)
    assert got_correct == float(first)
    assert abs(got_loss - loss) <= 1e-4 * abs(loss) and relmax(got_dW, dW) < 1e-5


@pytest.mark.parametrize("rows,V", [(48, 12), (5, 65), (48, 300), (6144, 64)])
def test_cross_entropy_of_large_logits(rows, V):
    """Logits spread over +-80: exp(x - max) spans 70 orders of magnitude, nothing overflows, the small terms flush to zero."""
    g = gen(7, rows, V)
    w = (torch.rand(rows, V, generator=g) * 2.0 - 1.0) * 80.0
    t = torch.randint(0, V, (rows,), generator=g)
    loss, correct, dW = R.cross_entropy_ref(w, t)
    got_loss, got_correct, got_dW = run_ce(w, t)
    print(f"rows {rows} V {V}: loss {got_loss} ref {loss} dW {relmax(got_dW, dW):.2e}")
    assert abs(got_loss - loss) <= 1e-4 * abs(loss)
    assert got_correct == correct
    assert relmax(got_dW, dW) < 1e-5


def ce_ex_setup(rows, V, key):
    w, t = relu_logits(rows, V, gen(8, rows, V, key))
    wv, _ = strided(w, 3, "poison")
    dv, dbuf = strided(torch.zeros(rows, V), 2, SENT)
    return w, t, wv, t.to(DEV), dv, dbuf


@pytest.mark.parametrize("rows,V", [(48, 12), (6144, 65)])
def test_cross_entropy_ex_with_each_output_null(rows, V):
    w, t, wv, td, dv, dbuf = ce_ex_setup(rows, V, 0)
    loss, correct, dW = R.cross_entropy_ref(w, t, scale=2.0)
    # guard words around every scalar: a write through a pointer that was not given would land next to one that was
    for drop in ("loss_sum", "correct", "dW"):
        acc = torch.full((5,), SENT, device=DEV)
        acc[1] = 0.0
        acc[3] = 0.0
        dbuf[:, :V] = SENT
        ops.cross_entropy_ex(wv, td, loss_sum=None if drop == "loss_sum" else acc[1:2], correct=None if drop == "correct" else acc[3:4],
                             dW=None if drop == "dW" else dv, scale=2.0)
        torch.cuda.synchronize()
        a = acc.cpu()
        assert a[0] == SENT and a[2] == SENT and a[4] == SENT
        if drop == "loss_sum":
            assert a[1] == 0.0
        else:
            assert abs(float(a[1]) - loss) <= 1e-4 * abs(loss)
        assert a[3] == (0.0 if drop == "correct" else correct)
        if drop == "dW":
            assert bool((dbuf == SENT).all())
        else:
            assert relmax(dv, dW) < 1e-5 and bool((dbuf[:, V:] == SENT).all())


@pytest.mark.parametrize("rows,V", [(48, 12), (6144, 65)])
def test_cross_entropy_ex_device_scale_and_forwarded_gradient(rows, V):
    """dW is multiplied by scale * scale_dev[0]; fwd_out receives fwd_scale * scale_dev[0], one float32 product, exactly."""
    w, t, wv, td, dv, dbuf = ce_ex_setup(rows, V, 1)
    sd = torch.tensor([0.8125 + 1.0 / 3.0])
    fwd_scale = 0.3
    _, _, dW = R.cross_entropy_ref(w, t, scale=float(np.float32(1.0 / rows)) * float(sd[0]))
    fwd = torch.full((3,), SENT, device=DEV)
    ops.cross_entropy_ex(wv, td, dW=dv, scale=1.0 / rows, scale_dev=sd.to(DEV), fwd_out=fwd[1:2], fwd_scale=fwd_scale)
    torch.cuda.synchronize()
    assert relmax(dv, dW) < 1e-5 and bool((dbuf[:, V:] == SENT).all())
    want = torch.tensor([fwd_scale], dtype=torch.float32) * sd
    assert torch.equal(fwd.cpu(), torch.tensor([SENT, float(want[0]), SENT]))


def test_cross_entropy_ex_adds_the_extra_term_once():
    """6144 rows: 128 workgroups run, one of them adds add_scale * add_term[0]."""
    rows, V = 6144, 12
    w, t, wv, td, dv, dbuf = ce_ex_setup(rows, V, 2)
    loss, correct, _ = R.cross_entropy_ref(w, t)
    add = torch.tensor([1000.0], device=DEV)
    acc = torch.zeros(2, device=DEV)
    ops.cross_entropy_ex(wv, td, loss_sum=acc[0:1], correct=acc[1:2], add_term=add, add_scale=0.5)
    want = loss + 500.0
    print(f"loss {float(acc[0])} ref {want}")
    assert abs(float(acc[0]) - want) <= 1e-4 * abs(want)
    assert float(acc[1]) == correct and float(add[0]) == 1000.0
    # with the mean folded in
    acc.zero_()
    ops.cross_entropy_ex(wv, td, loss_sum=acc[0:1], correct=acc[1:2], out_scale=1.0 / rows, add_term=add, add_scale=0.5)
    assert abs(float(acc[0]) - (loss / rows + 500.0)) <= 1e-4 * abs(loss / rows + 500.0)


def test_cross_entropy_ex_extra_term_without_a_loss_word_writes_nothing():
    rows, V = 6144, 12
    w, t, wv, td, dv, dbuf = ce_ex_setup(rows, V, 3)
    _, correct, dW = R.cross_entropy_ref(w, t)
    add = torch.tensor([SENT, 1000.0, SENT], device=DEV)
    acc = torch.tensor([SENT, 0.0, SENT], device=DEV)
    ops.cross_entropy_ex(wv, td, correct=acc[1:2], dW=dv, add_term=add[1:2], add_scale=0.5)
    torch.cuda.synchronize()
    assert torch.equal(acc.cpu(), torch.tensor([SENT, correct, SENT]))
    assert torch.equal(add.cpu(), torch.tensor([SENT, 1000.0, SENT]))
    assert relmax(dv, dW) < 1e-5 and bool((dbuf[:, V:] == SENT).all())


# =============================================================================== 3. inet_reparam_kl, inet_latent_bwd
LATENT_N = [1, 255, 256, 257, 33 * 24, (1 << 20) + 3]


def latent_inputs(n, key):
    g = gen(9, n, key)
    mu = torch.randn(n, generator=g)
    ls = torch.rand(n, generator=g) * 9.0 - 6.0                 # [-6, 3]
    eps = torch.randn(n, generator=g)
    return mu, ls, eps


def reparam_raw(mu, ls, eps, z, sigma, kl):
    check(_lib.lib().inet_reparam_kl(ptr(mu), ptr(ls), ptr(eps), ptr(z), ptr(sigma), mu.numel(), ptr(kl), stream_ptr()),
          "inet_reparam_kl")
    torch.cuda.synchronize()


@pytest.mark.parametrize("n", LATENT_N)
def test_reparam_kl_sizes_null_outputs_and_accumulation(n):
    mu, ls, eps = latent_inputs(n, 0)
    md, ld, ed = mu.to(DEV), ls.to(DEV), eps.to(DEV)
    z_ref, s_ref, kl_ref = R.reparam_kl_ref(mu, ls, eps)
    # kl_sum starts at 0 in the first pass, where the 1e-5 is relative to the KL term alone (at n = 1 it is of order one), and at
    # 100 in the others, where one float32 word holds base + KL and the 1e-5 is relative to that word
    for drop in (None, "z", "sigma", "kl", "eps"):
        kl0 = 0.0 if drop is None else 100.0
        z = None if drop == "z" else torch.full((n + 2,), SENT, device=DEV)
        s = None if drop == "sigma" else torch.full((n + 2,), SENT, device=DEV)
        kl = None if drop == "kl" else torch.tensor([SENT, kl0, SENT], device=DEV)
        reparam_raw(md, ld, None if drop == "eps" else ed, None if z is None else z[1:], None if s is None else s[1:],
                    None if kl is None else kl[1:])
        if z is not None:
            assert float(z[0]) == SENT and float(z[-1]) == SENT
            if drop == "eps":
                assert torch.equal(z[1:-1].cpu(), mu)                      # z = mu + 0 * sigma
            else:
                assert relmax(z[1:-1], z_ref) < 1e-6
        if s is not None:
            assert float(s[0]) == SENT and float(s[-1]) == SENT and relmax(s[1:-1], s_ref) < 1e-6
        if kl is not None:
            got = kl.cpu()
            assert got[0] == SENT and got[2] == SENT
            print(f"n {n} drop {drop}: kl {float(got[1])} ref {kl0 + kl_ref}")
            assert abs(float(got[1]) - (kl0 + kl_ref)) <= 1e-5 * abs(kl0 + kl_ref)


@pytest.mark.parametrize("n", LATENT_N)
def test_latent_bwd_against_float64_autograd(n):
    """dmu = dz + k mu, dls = dz eps sigma + k (sigma^2 - 1): a handful of float32 roundings of terms no larger than the tensor's
    maximum -- the bound of z, 1e-6 of the maximum."""
    mu, ls, eps = latent_inputs(n, 1)
    dz = torch.randn(n, generator=gen(10, n))
    md, ld, ed, dd = mu.to(DEV), ls.to(DEV), eps.to(DEV), dz.to(DEV)
    kdev = torch.tensor([0.75], device=DEV)
    for use_dz, use_kdev in ((True, True), (True, False), (False, True), (False, False)):
        k = 0.031 * (0.75 if use_kdev else 1.0)
        dmu_ref, dls_ref = R.latent_bwd_ref(dz if use_dz else None, mu, ls, eps, float(np.float32(0.031)) * (0.75 if use_kdev else 1.0))
        dmu, dls = ops.latent_bwd(dd if use_dz else None, md, ld, ed, 0.031, kscale_dev=kdev if use_kdev else None)
        torch.cuda.synchronize()
        print(f"n {n} dz {use_dz} kdev {use_kdev} (k {k:.5f}): dmu {relmax(dmu, dmu_ref):.2e} dls {relmax(dls, dls_ref):.2e}")
        assert relmax(dmu, dmu_ref) < 1e-6 and relmax(dls, dls_ref) < 1e-6


# =============================================================================== 4. inet_adam_step_ex
ADAM_N = [1, 3, 4, 5] + [4 * 10007 + k for k in range(4)]
LR = 1e-3


def report_words():
    return torch.zeros(4, dtype=torch.int32).pin_memory()


def flag(a=0.0, b=0.0):
    """Every optimizer call of this file decides by an explicit step_flag: the process's own status word is never consulted."""
    return torch.tensor([a, b], device=DEV)


def adam_state(n, step, gscale, regime, key):
    """Parameters, a gradient of the regime, and the moments `step - 1` steps of that same gradient leave behind: the step under
    test then moves every parameter by lr or less (m_hat = g, v_hat = g^2), as a step of a training run does."""
    g = gen(11, n, step, key)
    p = torch.randn(n, generator=g)
    gr = torch.randn(n, generator=g) * {"zero": 0.0, "tiny": 1e-12, "big": 1e3}[regime]
    b1, b2 = float(np.float32(0.9)), float(np.float32(0.999))
    ge = gr.double() * gscale
    m = ((1.0 - b1 ** (step - 1)) * ge).float()
    v = ((1.0 - b2 ** (step - 1)) * ge * ge).float()
    return p, gr, m, v


@pytest.mark.parametrize("regime", ["zero", "tiny", "big"])
@pytest.mark.parametrize("step", [1, 2, 1000, 100000])
def test_adam_step_sizes_tails_and_gradient_regimes(step, regime):
    """Against float64 Adam.  m, v: 1e-6 of the tensor's maximum.  p: the update is ONE float32 subtraction of a step of about lr
    from p, so |dp| <= one ulp of p (2^-23 |p|) + the step's own relative error (a handful of float32 roundings, < 1e-6) times its
    size (<= lr).  n = 4 * 10007 + k: the float4 body plus a tail of k elements; n < 4: tail only."""
    for n in ADAM_N:
        for gscale in (1.0, 0.125):
            p, gr, m, v = adam_state(n, step, gscale, regime, 0)
            p_ref, m_ref, v_ref = R.adam_ref(p, gr, m, v, LR, step, gscale=gscale)
            pd, md, vd = p.to(DEV), m.to(DEV), v.to(DEV)
            rep = report_words()
            ops.adam_step(pd, gr.to(DEV), md, vd, LR, step, gscale=gscale, step_flag=flag(), report=rep)
            torch.cuda.synchronize()
            assert rep.tolist() == [1, 0, 0, 0], (n, rep)
            dp = (pd.cpu().double() - p_ref).abs()
            bound = 2.0 ** -23 * p_ref.abs() + 1e-6 * LR
            worst = float((dp / bound).max())
            assert relmax(md, m_ref) < 1e-6 and relmax(vd, v_ref) < 1e-6, (n, gscale, relmax(md, m_ref), relmax(vd, v_ref))
            assert worst <= 1.0, (n, gscale, worst)
            if regime == "zero":
                assert torch.equal(pd.cpu(), p)                     # the denominator is eps, the numerator 0
            elif regime == "big":
                assert bool((pd.cpu() != p).all())                  # m_hat / sqrt(v_hat) = +-1: every parameter moves by lr


@pytest.mark.parametrize("n", [5, 4 * 10007 + 3])
def test_adam_step_flag_decides_and_reports(n):
    p, gr, m, v = adam_state(n, 3, 1.0, "big", 1)
    p_ref, m_ref, v_ref = R.adam_ref(p, gr, m, v, LR, 3)
    for words, want_report in (((1.0, 0.0), [1, 1, 0, 0]), ((2.0, 1.0), [1, 1, 0, 1]), ((0.0, 1.0), [1, 0, 0, 1]), ((0.0, 0.0), [1, 0, 0, 0])):
        pd, md, vd = p.to(DEV), m.to(DEV), v.to(DEV)
        rep = report_words()
        ops.adam_step(pd, gr.to(DEV), md, vd, LR, 3, step_flag=flag(*words), report=rep)
        torch.cuda.synchronize()
        assert rep.tolist() == want_report, (words, rep)
        if words[0] != 0.0:                                         # skipped: bit-identical
            for got, was in ((pd, p), (md, m), (vd, v)):
                assert torch.equal(got.cpu().view(torch.int32), was.view(torch.int32)), words
        else:
            assert relmax(md, m_ref) < 1e-6 and relmax(vd, v_ref) < 1e-6
            assert bool(((pd.cpu().double() - p_ref).abs() <= 2.0 ** -23 * p_ref.abs() + 1e-6 * LR).all())
    # without report words the flag still decides
    pd, md, vd = p.to(DEV), m.to(DEV), v.to(DEV)
    ops.adam_step(pd, gr.to(DEV), md, vd, LR, 3, step_flag=flag(1.0))
    torch.cuda.synchronize()
    assert torch.equal(pd.cpu(), p) and torch.equal(md.cpu(), m) and torch.equal(vd.cpu(), v)


@pytest.mark.parametrize("at", ["body", "tail"])
def test_adam_reports_a_parameter_that_left_the_finite_range(at):
    n = 4 * 10007 + 1
    p, gr, m, v = adam_state(n, 1, 1.0, "big", 2)
    k = 4 * 5003 + 2 if at == "body" else n - 1
    gr[k] = INF
    pd, md, vd = p.to(DEV), m.to(DEV), v.to(DEV)
    rep = report_words()
    ops.adam_step(pd, gr.to(DEV), md, vd, LR, 1, step_flag=flag(), report=rep)
    torch.cuda.synchronize()
    assert rep.tolist() == [1, 0, 1, 0], rep
    bad = ~torch.isfinite(pd.cpu())
    assert int(bad.sum()) == 1 and bool(bad[k])
    # and a clean step of the same size reports nothing
    gr[k] = 1.0
    pd, md, vd = p.to(DEV), m.to(DEV), v.to(DEV)
    rep = report_words()
    ops.adam_step(pd, gr.to(DEV), md, vd, LR, 1, step_flag=flag(), report=rep)
    torch.cuda.synchronize()
    assert rep.tolist() == [1, 0, 0, 0], rep


# =============================================================================== 5. inet_epoch_stats_add_ex, inet_step_flag_export
def test_epoch_stats_add():
    sums = torch.tensor([SENT, 10.0, 20.0, 3.0, SENT], device=DEV)
    loss, acc = torch.tensor([4.0], device=DEV), torch.tensor([0.5], device=DEV)
    ops.epoch_stats_add(sums[1:], loss, acc, step_flag=flag())
    assert sums.tolist() == [SENT, 14.0, 20.5, 4.0, SENT]
    ops.epoch_stats_add(sums[1:], loss, None, step_flag=flag())                    # no accuracy: its sum stays
    assert sums.tolist() == [SENT, 18.0, 20.5, 5.0, SENT]
    for words in ((1.0, 0.0), (3.0, 1.0)):                                         # a skipped step stays out of the epoch means
        ops.epoch_stats_add(sums[1:], loss, acc, step_flag=flag(*words))
        assert sums.tolist() == [SENT, 18.0, 20.5, 5.0, SENT]
    ops.epoch_stats_add(sums[1:], loss, acc, step_flag=flag(0.0, 1.0))             # word 1 is the optimizer's business
    assert sums.tolist() == [SENT, 22.0, 21.0, 6.0, SENT]


def test_epoch_stats_ten_integer_adds_are_exact_and_real_ones_within_rounding():
    g = gen(12)
    sums = torch.zeros(3, device=DEV)
    vals = ints((10, 2), g)
    for lo, ac in vals:
        ops.epoch_stats_add(sums, lo.reshape(1).to(DEV), ac.reshape(1).to(DEV), step_flag=flag())
    assert sums.tolist() == [float(vals[:, 0].sum()), float(vals[:, 1].sum()), 10.0]
    # real values: ten float32 additions, each within 2^-24 of the running sum <= sum |terms|
    sums = torch.zeros(3, device=DEV)
    vals = torch.randn(10, 2, generator=g)
    for lo, ac in vals:
        ops.epoch_stats_add(sums, lo.reshape(1).to(DEV), ac.reshape(1).to(DEV), step_flag=flag())
    got = sums.cpu().double()
    for c in (0, 1):
        assert abs(float(got[c]) - float(vals[:, c].double().sum())) <= 10 * 2.0 ** -23 * float(vals[:, c].double().abs().sum())
    assert float(got[2]) == 10.0


def test_step_flag_export_on_a_clean_process():
    left = ops.token_status()
    assert left == 0, f"token status {left}: an earlier test met a token outside its vocabulary and did not clear the word"
    assert ops.chain_status() == 0
    dst = torch.full((4,), SENT, device=DEV)
    ops.step_flag_export(dst[1:3])
    assert dst.tolist() == [SENT, 0.0, 0.0, SENT]
    assert ops.token_status() == 0 and ops.chain_status() == 0


# =============================================================================== 6. inet_dropout_mask
@pytest.mark.parametrize("p", [0.0, 0.1, 0.2, 0.5, 0.999])
@pytest.mark.parametrize("n", [1, 255, 257, 2048 * 256 + 5])
def test_dropout_mask_is_the_counter_based_stream(n, p):
    """Bit-equal to the numpy mirror for every (seed, offset), offsets near 2^64 included; n = 2048 * 256 + 5 is past the grid cap:
    the stride loop runs.  (The mirror's own statistics and its offset contract: tests/test_pointwise_host.py.)"""
    keep = R.dropout_keep_value(p)
    for seed in (0, 0x5eed, 2 ** 64 - 1):
        for offset in (0, 2 ** 32 + 7, 2 ** 64 - 1000):
            got = ops.dropout_mask((n,), p, seed, offset, DEV).cpu()
            want = torch.from_numpy(R.dropout_mask_ref(n, p, seed, offset))
            assert torch.equal(got, want), (n, p, seed, offset, int((got != want).sum()))
            assert bool(((got == 0) | (got == float(keep))).all())
    if p == 0.0:
        assert bool((got == 1.0).all())


@pytest.mark.parametrize("p", [0.0, 0.1, 0.2, 0.5, 0.999])
def test_dropout_mask_threshold_is_inclusive(p):
    """Elements aimed (with the inverse hash) at the threshold itself and at its neighbours: `>=` keeps the first, `>` would not --
    a difference of one element in 2^32 that unaimed masks never meet."""
    thr = R.dropout_threshold(p)
    for seed in (0, 0x5eed):
        for hi in [thr, thr + 1] + ([thr - 1] if thr > 0 else []):
            off = (R.offset_with_hash(seed, (hi << 32) | 0x9abcdef0) - 1) & (2 ** 64 - 1)
            want = R.dropout_mask_ref(3, p, seed, off)
            assert (want[1] != 0) == (hi >= thr)
            got = ops.dropout_mask((3,), p, seed, off, DEV).cpu()
            assert torch.equal(got, torch.from_numpy(want)), (p, seed, hi, thr, got, want)


def test_dropout_mask_continues_across_calls():
    """What measure_vae.py and arnn.py rely on: a second call at offset + k continues the first call's stream."""
    n, k = 70000, 33333
    for off in (0, 2 ** 64 - 40000):
        whole = ops.dropout_mask((n,), 0.2, 0x5eed, off, DEV)
        rest = ops.dropout_mask((n - k,), 0.2, 0x5eed, off + k, DEV)
        assert torch.equal(whole[k:], rest)


# =============================================================================== 7. inet_sample_multinomial
def sample_raw(w, V, out, stride, seed, offset):
    check(_lib.lib().inet_sample_multinomial(ptr(w), w.stride(0), w.shape[0], V, ptr(out), stride, seed & (2 ** 64 - 1),
                                             offset & (2 ** 64 - 1), stream_ptr()), "inet_sample_multinomial")


@pytest.mark.parametrize("V", [1, 64, 65, 128, 129, 300])
def test_sample_multinomial_rows_are_counters(V):
    """Row r at offset o is row 0 at offset o + r ("rank-offsettable"); the row stride and the output stride are honoured."""
    rows = 300
    g = gen(13, V)
    w = torch.relu(torch.randn(rows, V, generator=g) * 2.0)
    wd = w.to(DEV)
    off = 2 ** 40 + 11
    whole = ops.sample_multinomial(wd, seed=99, offset=off).cpu()
    assert int(whole.min()) >= 0 and int(whole.max()) < V
    single = torch.full((rows,), -1, dtype=torch.int64, device=DEV)
    for r in range(0, rows, 7):
        sample_raw(wd[r:r + 1], V, single[r:r + 1], 1, 99, off + r)
    single = single.cpu()
    assert torch.equal(single[::7], whole[::7])
    view, _ = strided(w, 5, "poison")
    out = torch.full((rows * 3,), -7, dtype=torch.int64, device=DEV)
    sample_raw(view, V, out, 3, 99, off)
    out = out.cpu().view(rows, 3)
    assert torch.equal(out[:, 0], whole) and bool((out[:, 1:] == -7).all())
    if V > 1:
        assert len(set(whole.tolist())) > 1


@pytest.mark.parametrize("V", [64, 65, 128, 129, 300])
def test_sample_multinomial_never_draws_a_token_without_mass(V):
    """Logits 1e4 below the maximum have softmax mass exactly 0 (in float64 as well): at the head, in the middle, around the lane wrap
    and at the tail they are never drawn in 200 000 draws."""
    n = 200_000
    g = gen(14, V)
    row = torch.relu(torch.randn(V, generator=g) * 2.0) + 1.0
    dead = sorted({0, 1, V // 2, 62, 63, V - 2, V - 1} | ({64} if V > 65 else set()))
    row[dead] = float(row.max()) - 1e4
    p = torch.softmax(row.double(), 0)
    assert bool((p[dead] == 0).all()) and float(p.sum()) > 0.999
    draws = ops.sample_multinomial(row.repeat(n, 1).to(DEV), seed=1234, offset=5).cpu().numpy()
    counts = np.bincount(draws, minlength=V)
    assert counts.sum() == n and counts[dead].sum() == 0, {d: int(counts[d]) for d in dead}
    live = p > 0
    chi2 = float((((torch.from_numpy(counts).double() - n * p) ** 2)[live] / (n * p[live])).sum())
    k = int(live.sum())
    assert chi2 < k + 6.0 * np.sqrt(2.0 * k), (chi2, k)


# counters of seed 1234 whose 24-bit uniform is the largest (0xFFFFFF / 2^24, twice) and the smallest (0) among the first 2^26
# (tests/test_pointwise_host.py::test_the_aimed_uniforms holds the mirror to them)
AIMED = ((22982038, 0xFFFFFF), (50007773, 0xFFFFFF), (63355030, 0))


@pytest.mark.parametrize("counter,k24", AIMED)
def test_sample_multinomial_at_the_ends_of_the_uniform_range(counter, k24):
    """The draw compares an in-order prefix sum with u * total, and the total is summed in another order (lane-strided, then across
    the wave): the two can differ in the last bits, so for the largest u no prefix need exceed the target.  Whatever the rounding, the
    token drawn must be one with mass: near-equal masses followed by a tail of tokens without any, several mass vectors per shape."""
    assert R.uniform24_ref(1234, counter) == k24
    cases = [(V, tail, rep) for V in (65, 130, 300) for tail in (1, 7, 64, 70) for rep in range(8)]
    out = torch.full((len(cases),), -1, dtype=torch.int64, device=DEV)
    keep = []
    for i, (V, tail, rep) in enumerate(cases):
        g = gen(15, V, tail, rep)
        row = torch.cat([torch.randn(V, generator=g) * 0.01, torch.full((tail,), -1e4)]).reshape(1, -1).to(DEV)
        keep.append(row)
        sample_raw(row, V + tail, out[i:i + 1], 1, 1234, counter)
    torch.cuda.synchronize()
    wrong = []
    for (V, tail, rep), row, tok in zip(cases, keep, out.tolist()):
        p = torch.softmax(row[0].double().cpu(), 0)
        if not (0 <= tok < V + tail) or float(p[tok]) <= 0.0:
            wrong.append((V, tail, rep, tok))
        elif k24 == 0:
            assert tok == 0, (V, tail, rep, tok)                    # u = 0: the first token with mass
    assert not wrong, f"{len(wrong)} of {len(cases)} draws landed on a token without mass: {wrong[:8]}"


# =============================================================================== 8. inet_embedding_fwd / _bwd
@pytest.mark.parametrize("rows", [1, 1000, 100_003])
@pytest.mark.parametrize("E", [1, 10, 20, 33])
def test_embedding_fwd_is_one_gather_and_one_multiply(rows, E):
    g = gen(16, rows, E)
    W = 48
    table = torch.randn(W, E, generator=g)
    idx = torch.randint(0, W, (rows,), generator=g)
    idx[0] = 0
    idx[-1] = W - 1 if rows > 1 else 0
    td, idd = table.to(DEV), idx.to(DEV)
    assert torch.equal(ops.embedding_fwd(td, idd).cpu(), table[idx])
    scale = torch.randint(0, 3, (rows,), generator=g).float() * 0.7         # zeros, and factors that round
    assert torch.equal(ops.embedding_fwd(td, idd, row_scale=scale.to(DEV)).cpu(), table[idx] * scale[:, None])
    if rows > 1:
        last = torch.full((rows,), W - 1, dtype=torch.int64)
        assert torch.equal(ops.embedding_fwd(td, last.to(DEV)).cpu(), table[last])


EMB_ROWS = [1, 1023, 1024, 1025, 4096 + 17, 100_003]
EMB_W = [2, 6, 48, 128, 129]
EMB_E = [1, 10, 20, 32, 33, 64, 65, 300]
# every (rows, table size) pair with two of the widths, rotating, and the corners of the segment-sum path spelled out: each column
# template (E <= 32, <= 64, wider: more than one column block at 300) at the full 128-row LDS table and just past the switch
EMB_CASES = sorted({(r, w, EMB_E[(i + j + k) % 8]) for i, r in enumerate(EMB_ROWS) for j, w in enumerate(EMB_W) for k in (0, 3)} |
                   {(1024, 128, 32), (1024, 128, 64), (1024, 128, 65), (1024, 128, 300), (4096 + 17, 128, 33), (100_003, 128, 20),
                    (100_003, 128, 300), (1025, 2, 1), (1023, 128, 300), (100_003, 129, 10)})


def emb_case(rows, W, E, g, integer):
    absent = W // 2                                                 # a token that never occurs
    idx = torch.randint(0, W - 1, (rows,), generator=g)
    idx[idx >= absent] += 1
    if rows > 1 and absent != 0:
        idx[0] = 0
    if rows > 1 and absent != W - 1:
        idx[-1] = W - 1
    if integer:
        dout, dt0 = ints((rows, E), g), ints((W, E), g)
        scale = torch.randint(0, 2, (rows,), generator=g).float() * 2.0
    else:
        dout, dt0 = torch.randn(rows, E, generator=g), torch.randn(W, E, generator=g)
        scale = torch.rand(rows, generator=g) * torch.randint(0, 2, (rows,), generator=g).float()
    dt0[absent] = torch.randn(E, generator=g)                       # bits nobody has a reason to touch
    dt0[absent, 0] = -0.0
    return idx, dout, dt0, scale, absent


def run_emb_bwd(dout, idx, dt0, scale):
    dt = dt0.to(DEV)
    ops.embedding_bwd(dout.to(DEV), idx.to(DEV), dt, row_scale=None if scale is None else scale.to(DEV))
    sync()                                                          # the entry runs on a side stream
    return dt.cpu()


@pytest.mark.parametrize("rows,W,E", EMB_CASES)
def test_embedding_bwd_exact_sums_on_both_paths(rows, W, E):
    """rows >= 1024 and a table of at most 128 rows: the segment-sum kernel; else per-element atomics.  The table accumulates
    (non-zero on entry), a zero row scale drops the row, the row of a token that never occurs keeps its bits."""
    g = gen(17, rows, W, E)
    idx, dout, dt0, scale, absent = emb_case(rows, W, E, g, integer=True)
    for sc in (None, scale):
        got = run_emb_bwd(dout, idx, dt0, sc)
        want = R.index_add_ref(dt0, idx, dout, sc).float()
        assert torch.equal(got, want), (rows, W, E, sc is not None, int((got != want).sum()),
                                        (got != want).nonzero()[:4].tolist())
        assert torch.equal(got[absent].view(torch.int32), dt0[absent].view(torch.int32))


@pytest.mark.parametrize("rows,W,E", [(1023, 48, 20), (4096 + 17, 48, 20), (100_003, 6, 33), (100_003, 128, 300), (5000, 129, 10)])
def test_embedding_bwd_all_rows_on_one_token(rows, W, E):
    g = gen(18, rows, W, E)
    _, dout, dt0, scale, _ = emb_case(rows, W, E, g, integer=True)
    for tok in (0, W - 1):
        idx = torch.full((rows,), tok, dtype=torch.int64)
        got = run_emb_bwd(dout, idx, dt0, scale)
        want = R.index_add_ref(dt0, idx, dout, scale).float()
        assert torch.equal(got, want)
        others = torch.arange(W) != tok
        assert torch.equal(got[others].view(torch.int32), dt0[others].view(torch.int32))


@pytest.mark.parametrize("rows,W,E", [(1023, 48, 20), (777, 129, 65), (4096 + 17, 48, 20), (100_003, 128, 65), (100_003, 6, 300)])
def test_embedding_bwd_real_values_within_the_summation_bound(rows, W, E):
    """randn terms on both paths: |got - ref| <= n_v * 2^-23 * sum |terms| per table row, n_v the token's row count and the sum of
    absolute values formed in float64 by the same index_add -- the worst-case forward error of any order of n_v additions (and of the
    one product per term)."""
    g = gen(19, rows, W, E)
    idx, dout, dt0, scale, absent = emb_case(rows, W, E, g, integer=False)
    got = run_emb_bwd(dout, idx, dt0, scale).double()
    want = R.index_add_ref(dt0, idx, dout, scale)
    mag = R.index_add_ref(dt0, idx, dout, scale, absolute=True)
    n_v = torch.bincount(idx, minlength=W).double()[:, None]
    ratio = float(((got - want).abs() / (n_v * 2.0 ** -23 * mag + 1e-300)).max())
    print(f"rows {rows} W {W} E {E}: worst |err| / bound = {ratio:.3g}")
    assert ratio <= 1.0
    assert torch.equal(got[absent].float().view(torch.int32), dt0[absent].view(torch.int32))


# =============================================================================== 9. inet_relu_bwd
@pytest.mark.parametrize("n", [1, 257, (1 << 20) + 1])
def test_relu_bwd_passes_dy_where_y_is_positive(n):
    g = gen(20, n)
    pattern = torch.tensor([2.0, 0.0, -0.0, -1.0, NAN, 1e-30, -INF, INF])
    y = pattern[torch.arange(n) % len(pattern)]
    dy = torch.randn(n, generator=g)
    got = ops.relu_bwd(dy.to(DEV), y.to(DEV)).cpu()
    want = torch.where(y > 0, dy, torch.zeros(n))
    assert torch.equal(got, want)
    if n > 8:
        assert float(got[4]) == 0.0 and float(got[1]) == 0.0 and float(got[2]) == 0.0 and float(got[0]) == float(dy[0])


# =============================================================================== 10. inet_linear_fwd / _bwd
LINEAR_SHAPES = [(1, 1, 1), (7, 48, 10), (384, 1024, 266), (1024, 256, 276), (12288, 1024, 276)]


@pytest.mark.parametrize("M,N,K", LINEAR_SHAPES)
def test_linear_fwd_epilogues_against_float64(M, N, K):
    g = gen(21, M, N, K)
    x, W, b = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g), torch.randn(N, generator=g)
    xd, Wd, bd = x.to(DEV), W.to(DEV), b.to(DEV)
    prod = x.double() @ W.double().t()
    for bias in (None, b):
        pre = prod if bias is None else prod + b.double()
        for epi in (0, 1, 2):
            got = ops.linear_fwd(xd, Wd, None if bias is None else bd, epi=epi).cpu().double()
            want = (pre, torch.nn.functional.selu(pre), torch.relu(pre))[epi]
            if epi == 2:
                # a pre-activation within round-off of ReLU's kink may take either branch: left out, and they are few
                near = pre.abs() < 1e-6
                assert float(near.double().mean()) < 1e-3
                got, want = got.masked_fill(near, 0.0), want.masked_fill(near, 0.0)
            err = relmax(got, want)
            print(f"{M}x{N}x{K} bias {bias is not None} epi {epi}: {err:.2e}")
            assert err < 2e-5, (bias is not None, epi, err)


LINEAR_BWD_SHAPES = LINEAR_SHAPES + [(M, 96, K) for M in (1023, 1024) for K in (276, 266, 192, 130)]


@pytest.mark.parametrize("M,N,K", LINEAR_BWD_SHAPES)
def test_linear_bwd_all_outputs_against_float64(M, N, K):
    """dx (with M >= 1024 and K = 276, 266 or 130 through the split at K % 64; with 1023 rows, K = 192 or the small shapes not),
    dW and db accumulated into live tensors; then each output alone.  db with real terms is held to 2e-5 of the tensor maximum,
    the bound of test_gpu_kernels.py; test_bias_gradient_column_sums_are_exact has the integer terms."""
    g = gen(22, M, N, K)
    dy, x, W = torch.randn(M, N, generator=g), torch.randn(M, K, generator=g), torch.randn(N, K, generator=g)
    dW0, db0 = torch.randn(N, K, generator=g), torch.randn(N, generator=g)
    dyd, xd, Wd = dy.to(DEV), x.to(DEV), W.to(DEV)
    dx_ref = dy.double() @ W.double()
    dW_ref = dW0.double() + dy.double().t() @ x.double()
    db_ref = R.colsum_ref(dy, db0)

    def check_db(db):
        err = relmax(db, db_ref)
        assert err < 2e-5, err

    dW, db = dW0.to(DEV), db0.to(DEV)
    dx = ops.linear_bwd(dyd, xd, Wd, dW=dW, db=db)
    sync()
    print(f"{M}x{N}x{K}: dx {relmax(dx, dx_ref):.2e} dW {relmax(dW, dW_ref):.2e}")
    assert relmax(dx, dx_ref) < 2e-5 and relmax(dW, dW_ref) < 2e-5
    check_db(db)
    dW, db = dW0.to(DEV), db0.to(DEV)
    assert ops.linear_bwd(dyd, xd, Wd, dW=dW, db=db, need_dx=False) is None
    sync()
    assert relmax(dW, dW_ref) < 2e-5
    check_db(db)
    dx = ops.linear_bwd(dyd, xd, Wd)
    sync()
    assert relmax(dx, dx_ref) < 2e-5
    dW = dW0.to(DEV)
    ops.linear_bwd(dyd, xd, Wd, dW=dW, need_dx=False)
    sync()
    assert relmax(dW, dW_ref) < 2e-5
    db = db0.to(DEV)
    ops.linear_bwd(dyd, None, Wd, db=db, need_dx=False)
    sync()
    check_db(db)


@pytest.mark.parametrize("M", [1, 255, 257, 16385])
@pytest.mark.parametrize("N", [1, 64, 130])
def test_bias_gradient_column_sums_are_exact(M, N):
    """db through the column-sum kernel alone: integer terms, accumulated into a live vector; 16385 rows are past the cap of 64 row
    blocks, 130 columns leave a ragged third column block."""
    g = gen(23, M, N)
    dy, db0 = ints((M, N), g), ints((N,), g)
    W = torch.zeros(N, 4, device=DEV)
    db = torch.cat([torch.tensor([SENT]), db0, torch.tensor([SENT])]).to(DEV)
    ops.linear_bwd(dy.to(DEV), None, W, db=db[1:-1], need_dx=False)
    sync()
    got = db.cpu()
    assert got[0] == SENT and got[-1] == SENT
    assert torch.equal(got[1:-1], R.colsum_ref(dy, db0).float())
