"""Global-norm clipping and the non-finite skip of the optimizer step: grad_sqnorm_kernel and the step kernel
alone through ops.grad_sqnorm / ops.adam_step_clip, then through Trainer(max_grad_norm=...).  The reference is the float64
restatement of the rule, tests/clip_ref.py; the unclipped step must EQUAL ops.adam_step bit for bit -- two entry points of one kernel:
what holds the arithmetic itself in place is tests/test_gpu_adam_bits.py, against recorded bits.

Sizes: the optimizer tests' own (tail only, body + tail of 0..3), one just above one full pass of the norm kernel's grid (its
grid-stride loop runs twice, with a ragged end), one at which every workgroup of the Adam grid has work and the norm kernel's
four-loads-in-flight loop runs (more than four passes)."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import clip_ref as CR
from tests import pointwise_ref as R

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from inpaintnet_amd import ops
    import tests.test_gpu_pointwise as P            # adam_state / flag / relmax / LR: the optimizer tests' own helpers and bounds
    PARTS = ops.sqnorm_parts()
else:
    PARTS = 1024

DEV = "cuda:0"
INF, NAN = float("inf"), float("nan")
SMALL_N = [1, 3, 4, 5] + [4 * 10007 + k for k in range(4)]
TWO_PASS_N = PARTS * 256 * 4 * 2 + 4 * 257 + 3
ADAM_GRID_N = 4096 * 256 * 4 + 5
ALL_N = SMALL_N + [TWO_PASS_N, ADAM_GRID_N]
LR = 1e-3


def report8():
    return torch.zeros(8, dtype=torch.int32).pin_memory()


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def f32_bits(x):
    return int(np.float32(x).view(np.int32))


def norm_of_report(rep):
    return float(np.int32(rep[6]).view(np.float32))


def assert_norm_bits(rep, norm_ref, what):
    """(float)norm of the kernel against float32(norm_ref): one ulp (the kernel's f64 norm is within n * 2^-52 of the reference's,
    so the two can only fall on either side of ONE float32 rounding boundary)."""
    assert abs(int(rep[6]) - f32_bits(norm_ref)) <= 1, (what, norm_of_report(rep), norm_ref)


@functools.lru_cache(maxsize=None)
def regime_grad(n, regime):
    """(gradient, fsum reference of its sum of squares), computed once per (n, regime) and never written to."""
    g = torch.Generator().manual_seed(1000 + n % 9973 + 7 * len(regime))
    if regime == "zeros":
        x = torch.zeros(n)
    elif regime == "signs":
        x = torch.randint(0, 2, (n,), generator=g).float() * 2.0 - 1.0 + 0.25 * torch.randn(n, generator=g)
    else:
        x = torch.randn(n, generator=g) * {"tiny": 1e-12, "big": 1e3}[regime]
    return x, CR.sqnorm_ref(x)


def state(n, step, gscale, key, regime="big"):
    """P.adam_state: parameters, a gradient and the moments step - 1 steps of that gradient (times gscale) leave behind."""
    return P.adam_state(n, step, gscale, regime, key)


# =============================================================================== 1. the norm kernel alone
@pytest.mark.parametrize("regime", ["tiny", "big", "signs", "zeros"])
def test_sqnorm_partials_sum_to_the_exact_sum_of_squares(regime):
    """sum(partials) (added exactly, by fsum) against the fsum of the exact squares: relative error <= n * 2^-52 -- the first-order
    bound of ANY order of adding n non-negative exact terms in float64 is (n - 1) * 2^-53; one factor of two is slack.  Zeros give
    exactly 0.0; the buffer is NaN before the call, so an entry the kernel did not write shows; a second call gives the same bits."""
    for n in ALL_N:
        x, s_ref = regime_grad(n, regime)
        xd = x.to(DEV)
        part = torch.full((PARTS,), NAN, dtype=torch.float64, device=DEV)
        assert ops.grad_sqnorm(xd, part) is part
        first = part.cpu()
        assert bool(torch.isfinite(first).all()) and bool((first >= 0).all()), (n, regime)
        got = math.fsum(first.tolist())
        if regime == "zeros":
            assert got == 0.0 and bool((first == 0.0).all())
        else:
            err = abs(got - s_ref) / s_ref
            print(f"n {n} {regime}: relative error {err:.2e} (bound {n * 2.0 ** -52:.2e})")
            assert err <= n * 2.0 ** -52, (n, regime, err)
        again = ops.grad_sqnorm(xd)                                     # a buffer of the call's own
        assert again.dtype == torch.float64 and again.numel() == PARTS
        assert torch.equal(again.cpu().view(torch.int64), first.view(torch.int64)), (n, regime)


def test_sqnorm_workgroups_without_elements_write_zero():
    part = torch.full((PARTS,), NAN, dtype=torch.float64, device=DEV)
    ops.grad_sqnorm(torch.full((5,), 3.0, device=DEV), part)
    got = part.cpu()
    assert float(got[0]) == 45.0 and bool((got[1:] == 0.0).all())


def test_clip_entry_points_refuse_bad_arguments():
    p, g, m, v = (torch.zeros(8, device=DEV) for _ in range(4))
    part = ops.grad_sqnorm(g)
    for bad in (0.0, -1.0, NAN, -INF):
        with pytest.raises(ValueError):
            ops.adam_step_clip(p, g, m, v, LR, 1, bad, part)
    with pytest.raises(ValueError):
        ops.adam_step_clip(p, g, m, v, LR, 0, 1.0, part)                # step is 1-based
    torch.cuda.synchronize()
    assert float(p.abs().max()) == 0.0


# =============================================================================== 2. not clipped: bit-identical to inet_adam_step_ex
# (an entry-point check: both calls reach one kernel, so this holds scale == 1.0f and the argument plumbing; that the arithmetic is
# what it was is tests/test_gpu_adam_bits.py's to prove, against the recorded fixture)
@pytest.mark.parametrize("gscale", [1.0, 0.125])
@pytest.mark.parametrize("how", ["ten_times", "inf"])
def test_unclipped_step_is_bit_identical_to_adam_step(how, gscale):
    for n in ALL_N:
        p, gr, m, v = state(n, 3, gscale, 20)
        norm = CR.norm_ref(gr, gscale)
        max_norm = INF if how == "inf" else 10.0 * norm
        pa, ma, va, gd = p.to(DEV), m.to(DEV), v.to(DEV), gr.to(DEV)
        ops.adam_step(pa, gd, ma, va, LR, 3, gscale=gscale, step_flag=P.flag(), report=P.report_words())
        pb, mb, vb = p.to(DEV), m.to(DEV), v.to(DEV)
        rep = report8()
        ops.adam_step_clip(pb, gd, mb, vb, LR, 3, max_norm, ops.grad_sqnorm(gd), gscale=gscale, step_flag=P.flag(), report=rep)
        torch.cuda.synchronize()
        rep = rep.tolist()
        assert rep[:6] == [1, 0, 0, 0, 0, 0] and rep[7] == 0, (n, rep)
        assert_norm_bits(rep, norm, n)
        assert same_bits(pa, pb) and same_bits(ma, mb) and same_bits(va, vb), n
        assert not torch.equal(pb.cpu(), p)                              # (and the step was applied)


# =============================================================================== 3. clipped: against the restatement
@pytest.mark.parametrize("step", [1, 1000])
@pytest.mark.parametrize("divisor", [2.0, 1000.0])
def test_clipped_step_matches_the_restatement(divisor, step):
    """max_norm = norm / 2 and norm / 1000: far from c = 1, the decision cannot flip on rounding.  Bounds: the optimizer tests' own
    (tests/test_gpu_pointwise.py section 4): m, v within 1e-6 of the tensor's maximum, |dp| <= 2^-23 |p| + 1e-6 lr.  The moments are
    those `step - 1` steps of the CLIPPED gradient leave behind, so the step moves every parameter by lr or less, as there."""
    for n in ALL_N:
        for gscale in (1.0, 0.125):
            gr = state(n, step, gscale, 30)[1]
            norm = CR.norm_ref(gr, gscale)
            max_norm = float(np.float32(norm / divisor))
            _, nonfinite, clipped, scale = CR.clip_decision(gr, max_norm, gscale)
            assert clipped and not nonfinite and scale < 1.0
            p, gr2, m, v = state(n, step, float(np.float32(gscale) * np.float32(scale)), 30)
            assert torch.equal(gr, gr2)
            p_ref, m_ref, v_ref, rep_ref, _ = CR.adam_clip_ref(p, gr, m, v, LR, step, max_norm, gscale=gscale)
            pd, md, vd, gd = p.to(DEV), m.to(DEV), v.to(DEV), gr.to(DEV)
            rep = report8()
            ops.adam_step_clip(pd, gd, md, vd, LR, step, max_norm, ops.grad_sqnorm(gd), gscale=gscale, step_flag=P.flag(), report=rep)
            torch.cuda.synchronize()
            rep = rep.tolist()
            assert rep[:6] == rep_ref == [1, 0, 0, 0, 1, 0] and rep[7] == 0, (n, rep)
            assert_norm_bits(rep, norm, n)
            worst = float(((pd.cpu().double() - p_ref).abs() / (2.0 ** -23 * p_ref.abs() + 1e-6 * LR)).max())
            rm, rv = P.relmax(md, m_ref), P.relmax(vd, v_ref)
            print(f"n {n} gscale {gscale} /{divisor:g} step {step}: m {rm:.2e} v {rv:.2e} p {worst:.3f} of its bound")
            assert rm < 1e-6 and rv < 1e-6, (n, gscale, rm, rv)
            assert worst <= 1.0, (n, gscale, worst)
            assert bool((pd.cpu() != p).all())                          # every parameter moved


# =============================================================================== 4. one scale in every workgroup
def test_every_workgroup_applies_the_same_scale():
    """g = 1 everywhere, m = v = 0, step 1: m = (1 - b1) * gscale * scale and v likewise are the same float32 in every element iff
    every workgroup derived the same scale, to the last bit (a scale that is no power of two: its rounding is in play)."""
    n = ADAM_GRID_N
    g = torch.ones(n, device=DEV)
    p, m, v = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    max_norm = 3.0
    scale = float(np.float32(max_norm / (math.sqrt(n) + 1e-6)))         # S = n exactly, whatever the order
    assert scale < 1.0 and math.frexp(scale)[0] != 0.5
    rep = report8()
    ops.adam_step_clip(p, g, m, v, LR, 1, max_norm, ops.grad_sqnorm(g), step_flag=P.flag(), report=rep)
    torch.cuda.synchronize()
    assert rep.tolist()[:6] == [1, 0, 0, 0, 1, 0]
    assert_norm_bits(rep.tolist(), math.sqrt(n), "ones")
    assert bool((bits(m) == bits(m)[0]).all()) and bool((bits(v) == bits(v)[0]).all())
    b1 = np.float32(0.9)
    assert abs(float(m[0]) - float((np.float32(1) - b1) * np.float32(scale))) <= 2.0 ** -23 * float(m[0])
    assert bool((p == p[0]).all()) and float(p[0]) < 0.0


# =============================================================================== 5. non-finite gradients
@pytest.mark.parametrize("bad", [INF, -INF, NAN])
@pytest.mark.parametrize("where", ["body", "tail", "second_pass"])
def test_nonfinite_gradient_drops_the_step_and_a_clean_one_behind_it_applies(where, bad):
    n = TWO_PASS_N if where == "second_pass" else 4 * 10007 + 3
    k = {"body": 4 * 5003 + 2, "tail": n - 1, "second_pass": PARTS * 256 * 4 + 4 * 1001 + 1}[where]
    assert k < n and (where != "tail" or k >= (n // 4) * 4)
    p, gr, m, v = state(n, 2, 1.0, 50)
    clean = gr.to(DEV)
    dirty = clean.clone()
    dirty[k] = bad
    pd, md, vd = p.to(DEV), m.to(DEV), v.to(DEV)
    part = torch.empty(PARTS, dtype=torch.float64, device=DEV)
    for max_norm in (INF, 1.0):
        rep = report8()
        ops.adam_step_clip(pd, dirty, md, vd, LR, 2, max_norm, ops.grad_sqnorm(dirty, part), step_flag=P.flag(), report=rep)
        torch.cuda.synchronize()
        rep = rep.tolist()
        assert rep[:6] == [1, 0, 0, 0, 0, 1] and rep[7] == 0, (where, bad, rep)
        assert not math.isfinite(norm_of_report(rep))
        assert same_bits(pd, p) and same_bits(md, m) and same_bits(vd, v)
    rep = report8()
    ops.adam_step_clip(pd, clean, md, vd, LR, 2, INF, ops.grad_sqnorm(clean, part), step_flag=P.flag(), report=rep)
    torch.cuda.synchronize()
    assert rep.tolist()[:6] == [1, 0, 0, 0, 0, 0]
    p_ref, m_ref, v_ref = R.adam_ref(p, gr, m, v, LR, 2)
    assert P.relmax(md, m_ref) < 1e-6 and P.relmax(vd, v_ref) < 1e-6
    assert bool(((pd.cpu().double() - p_ref).abs() <= 2.0 ** -23 * p_ref.abs() + 1e-6 * LR).all())


# =============================================================================== 6. the flag wins
def test_step_flag_wins_over_a_nonfinite_gradient():
    n = 4 * 10007 + 1
    p, gr, m, v = state(n, 2, 1.0, 60)
    gd = gr.to(DEV)
    gd[77] = NAN
    for words, want in (((1.0, 0.0), [1, 1, 0, 0, 0, 0]), ((2.0, 1.0), [1, 1, 0, 1, 0, 0]), ((0.0, 1.0), [1, 0, 0, 1, 0, 1])):
        pd, md, vd = p.to(DEV), m.to(DEV), v.to(DEV)
        rep = report8()
        ops.adam_step_clip(pd, gd, md, vd, LR, 2, 1.0, ops.grad_sqnorm(gd), step_flag=P.flag(*words), report=rep)
        torch.cuda.synchronize()
        assert rep.tolist()[:6] == want and rep.tolist()[7] == 0, (words, rep)
        assert same_bits(pd, p) and same_bits(md, m) and same_bits(vd, v)
    # a clean gradient: word 1 of the flag still reaches word 3 of the report, and the step is applied; no report at all is fine too
    gd[77] = 1.0
    pd, md, vd = p.to(DEV), m.to(DEV), v.to(DEV)
    rep = report8()
    ops.adam_step_clip(pd, gd, md, vd, LR, 2, INF, ops.grad_sqnorm(gd), step_flag=P.flag(0.0, 1.0), report=rep)
    qd, nd, wd = p.to(DEV), m.to(DEV), v.to(DEV)
    ops.adam_step_clip(qd, gd, nd, wd, LR, 2, INF, ops.grad_sqnorm(gd), step_flag=P.flag())
    torch.cuda.synchronize()
    assert rep.tolist()[:6] == [1, 0, 0, 1, 0, 0]
    assert not torch.equal(pd.cpu(), p) and same_bits(pd, qd) and same_bits(md, nd) and same_bits(vd, wd)


# =============================================================================== 7. the head of the gradient store is not in the norm
def test_the_stores_head_stays_out_of_the_norm():
    n = 4 * 10007 + 2
    p, gr, m, v = state(n, 2, 1.0, 70)
    store = torch.empty(4 + n, device=DEV)
    store[:4] = 1e30
    store[4:] = gr.to(DEV)
    g = store[4:]
    norm = CR.norm_ref(gr)
    pd, md, vd = p.to(DEV), m.to(DEV), v.to(DEV)
    rep = report8()
    ops.adam_step_clip(pd, g, md, vd, LR, 2, 10.0 * norm, ops.grad_sqnorm(g), step_flag=P.flag(), report=rep)
    torch.cuda.synchronize()
    assert rep.tolist()[:6] == [1, 0, 0, 0, 0, 0]
    assert_norm_bits(rep.tolist(), norm, "head")


# =============================================================================== 8. Trainer(max_grad_norm=...)
def _vae(max_grad_norm):
    from inpaintnet_amd import synthetic
    from inpaintnet_amd.measure_vae import MeasureVAE
    from inpaintnet_amd.vae_trainer import VAETrainer
    ds = synthetic.SyntheticFolkDataset(num_notes=48)
    model = MeasureVAE(ds)
    model.load_state_dict({k: torch.from_numpy(synthetic.det_param(k, tuple(v.shape))) for k, v in model.state_dict().items()})
    trainer = VAETrainer(ds, model, lr=1e-4, max_grad_norm=max_grad_norm)
    model.train()
    tok = torch.from_numpy(synthetic.det_tokens("clip", (32, 24), 48)).cuda()
    return model, trainer, tok


def _backward(trainer, tok):
    trainer.zero_grad()
    loss, acc = trainer.loss_and_acc_for_batch(tok, 0, train=True)
    loss.backward()
    ops.side_join()


def _one_step(trainer, tok):
    _backward(trainer, tok)
    trainer.step()


def test_trainer_without_max_grad_norm_launches_what_it_launched():
    from tests.test_gpu_decode_plans import labels_of
    model, trainer, tok = _vae(None)
    _one_step(trainer, tok)
    _, labels = labels_of(lambda: _one_step(trainer, tok))
    trainer.finish()
    assert "adam" in labels and "grad_sqnorm" not in labels and "adam_clip" not in labels
    assert trainer._reports.shape == (trainer._NREP, 8)
    assert trainer.last_grad_norm is None and trainer.clipped_steps == 0 and trainer.nonfinite_steps == 0


def test_trainer_clips_every_step_and_reports_the_norm():
    from tests.test_gpu_decode_plans import labels_of
    model, trainer, tok = _vae(math.inf)
    _one_step(trainer, tok)
    trainer.finish()
    first = trainer.last_grad_norm
    assert math.isfinite(first) and first > 0.0 and trainer.clipped_steps == 0
    steps = 3
    model, trainer, tok = _vae(0.01 * first)
    for s in range(steps):
        _backward(trainer, tok)
        if s == steps - 1:
            torch.cuda.synchronize()
            g = model.grad.clone()
            before = [t.clone() for t in (model.flat, trainer.adam_m, trainer.adam_v)]
            _, labels = labels_of(trainer.step)
        else:
            trainer.step()
    trainer.finish()
    assert "grad_sqnorm" in labels and "adam_clip" in labels and "adam" not in labels
    assert labels.index("grad_sqnorm") < labels.index("adam_clip")
    assert trainer.clipped_steps == steps and trainer.nonfinite_steps == 0 and trainer.adam_t == steps
    norm64 = float(g.double().pow(2).sum().sqrt())
    assert abs(trainer.last_grad_norm - norm64) <= 1e-6 * norm64, (trainer.last_grad_norm, norm64)
    p_ref, m_ref, v_ref, rep_ref, _ = CR.adam_clip_ref(before[0], g, before[1], before[2], trainer.lr, steps, trainer.max_grad_norm)
    assert rep_ref == [1, 0, 0, 0, 1, 0]
    assert P.relmax(trainer.adam_m, m_ref) < 1e-6 and P.relmax(trainer.adam_v, v_ref) < 1e-6
    worst = float(((model.flat.cpu().double() - p_ref).abs() / (2.0 ** -23 * p_ref.abs() + 1e-6 * trainer.lr)).max())
    assert worst <= 1.0, worst


def test_trainer_survives_a_nonfinite_gradient_that_ends_an_unclipped_run(capsys):
    model, trainer, tok = _vae(math.inf)
    for s in range(4):
        _backward(trainer, tok)
        if s == 1:
            model.grad[12345] = INF
            torch.cuda.synchronize()
            before = model.flat.clone()
        trainer.step()
        if s == 1:
            torch.cuda.synchronize()
            assert same_bits(model.flat, before)                         # the weights are unchanged across that step
    trainer.finish()
    assert trainer.nonfinite_steps == 1 and trainer.adam_t == 3 and trainer.chain_fallbacks == 0 and trainer.clipped_steps == 0
    assert not torch.equal(model.flat, before) and bool(torch.isfinite(model.flat).all())
    assert "optimizer step 1 was dropped" in capsys.readouterr().out
    # the same injection without max_grad_norm: the inf reaches the weights and the run ends in the ValueError of check_steps
    model, trainer, tok = _vae(None)
    _one_step(trainer, tok)
    _backward(trainer, tok)
    model.grad[12345] = INF
    trainer.step()
    with pytest.raises(ValueError, match="has become nan"):
        trainer.finish()
