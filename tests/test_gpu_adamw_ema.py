"""Decoupled weight decay and EMA shadow weights inside the optimizer step: adamw_kernel alone through
ops.adamw_step / inet_adam_step_w, then through Trainer(weight_decay=, ema_decay=).  The reference is the float64 restatement of the
rule, tests/adamw_ref.py; without decay and EMA the step must EQUAL ops.adam_step / ops.adam_step_clip bit for bit -- three entry points
of one kernel: what holds the arithmetic itself in place is tests/test_gpu_adam_bits.py, against recorded bits.

Sizes: tail only (1, 3, 4, 5), around a mask word's edge (31 .. 65), the 16-byte body plus a tail of 0..3, and one size past a full
pass of the grid (its grid-stride loop runs twice, with a ragged end and a tail)."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import adamw_ref as AR
from tests import clip_ref as CR
from tests import pointwise_ref as R

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from inpaintnet_amd import _lib, ops
    import tests.test_gpu_pointwise as P            # adam_state / flag / relmax: the optimizer tests' own helpers and bounds

DEV = "cuda:0"
INF, NAN = float("inf"), float("nan")
TAIL_N = [1, 3, 4, 5]
EDGE_N = [31, 32, 33, 63, 65]
BODY_N = [4 * 10007 + k for k in range(4)]
GRID_N = 4 * 4096 * 256 + 4 * 1000 + 3
SMALL_N = TAIL_N + EDGE_N + BODY_N
ALL_N = SMALL_N + [GRID_N]
LR = 1e-3
RANGES = [(0, 5), (37, 70), (4 * 5003 + 2, 4 * 5003 + 9)]


def report8():
    return torch.zeros(8, dtype=torch.int32).pin_memory()


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


@functools.lru_cache(maxsize=None)
def state(n, step, gscale=1.0, key=0, regime="big"):
    """P.adam_state (host tensors, never written to) plus an EMA arena that is not the parameters."""
    p, gr, m, v = P.adam_state(n, step, gscale, regime, 100 + key)
    e = torch.randn(n, generator=torch.Generator().manual_seed(n % 9973 + key)) * 0.5
    return p, gr, m, v, e


def dev(*ts):
    return tuple(t.to(DEV) for t in ts)


def clipped_ranges(n):
    return [(min(a, n), min(b, n)) for a, b in RANGES]


def p_bound(p_ref, lr=LR):
    """Bound 3: p is rounded twice now, after the multiply and after the subtraction; the step's own error is the optimizer tests'."""
    return 2.0 * 2.0 ** -23 * p_ref.abs() + 1e-6 * lr


def e_bound(d, e0, p_ref, lr=LR):
    """Bound 5: the product's rounding and the fma's, plus p's own error through omd."""
    df, omd = AR.f32(d), AR.one_minus(d)
    return 2.0 ** -23 * ((df * e0.double()).abs() + (omd * p_ref).abs()) + omd * p_bound(p_ref, lr)


def assert_within(got, ref, bound, what):
    worst = float(((got.cpu().double() - ref).abs() / bound).max())
    print(f"{what}: {worst:.3f} of its bound")
    assert worst <= 1.0, (what, worst)


# =============================================================================== 1. no decay, no EMA, no partials: adam_step
# (sections 1 and 2 are entry-point checks: both calls reach one kernel, so they hold the argument plumbing and the reports; that the
# arithmetic is what it was is tests/test_gpu_adam_bits.py's to prove, against the recorded fixture)
@pytest.mark.parametrize("gscale", [1.0, 0.125])
def test_plain_form_is_bit_identical_to_adam_step(gscale):
    for n in ALL_N:
        p, gr, m, v, _ = state(n, 3, gscale)
        pa, ma, va, gd = dev(p, m, v, gr)
        ops.adam_step(pa, gd, ma, va, LR, 3, gscale=gscale, step_flag=P.flag(), report=P.report_words())
        pb, mb, vb = dev(p, m, v)
        rep = report8()
        ops.adamw_step(pb, gd, mb, vb, LR, 3, gscale=gscale, step_flag=P.flag(), report=rep)
        torch.cuda.synchronize()
        assert rep.tolist() == [1, 0, 0, 0, 0, 0, 0, 0], (n, rep)
        assert same_bits(pa, pb) and same_bits(ma, mb) and same_bits(va, vb), n
        assert not torch.equal(pb.cpu(), p)


# =============================================================================== 2. the same with partials: adam_step_clip
@pytest.mark.parametrize("how", ["ten_times", "inf", "half"])
def test_plain_form_with_partials_is_bit_identical_to_adam_step_clip(how):
    for n in ALL_N:
        p, gr, m, v, _ = state(n, 3)
        norm = CR.norm_ref(gr)
        max_norm = {"ten_times": 10.0 * norm, "inf": INF, "half": norm / 2.0}[how]
        pa, ma, va, gd = dev(p, m, v, gr)
        part = ops.grad_sqnorm(gd)
        ra, rb = report8(), report8()
        ops.adam_step_clip(pa, gd, ma, va, LR, 3, max_norm, part, step_flag=P.flag(), report=ra)
        pb, mb, vb = dev(p, m, v)
        ops.adamw_step(pb, gd, mb, vb, LR, 3, max_norm=max_norm, partials=part, step_flag=P.flag(), report=rb)
        torch.cuda.synchronize()
        assert ra.tolist() == rb.tolist() and rb.tolist()[:6] == [1, 0, 0, 0, int(how == "half"), 0] and rb.tolist()[7] == 0, (n, ra, rb)
        assert rb.tolist()[6] != 0
        assert same_bits(pa, pb) and same_bits(ma, mb) and same_bits(va, vb), (n, how)


# =============================================================================== 3. every element decays: against the restatement
@pytest.mark.parametrize("regime", ["zero", "tiny", "big"])
@pytest.mark.parametrize("step", [1, 1000])
@pytest.mark.parametrize("wd", [0.01, 0.5])
def test_decay_matches_the_restatement(wd, step, regime):
    """m, v as tests/test_gpu_pointwise.py holds them (1e-6 of the tensor's maximum); |p - p_ref| <= 2 * 2^-23 |p_ref| + 1e-6 lr."""
    # GRID_N (a float64 reference over 4.2 M elements) once per decay: regime and step change the kernel's scalar arguments and data,
    # not the path of its grid-stride loop, whose second pass the big regime at step 1 runs
    for n in (ALL_N if (regime == "big" and step == 1) else SMALL_N):
        p, gr, m, v, _ = state(n, step, 1.0, 1, regime)
        p_ref, m_ref, v_ref, _, rep_ref, _ = AR.adamw_ref(p, gr, m, v, LR, step, wd)
        pd, md, vd, gd = dev(p, m, v, gr)
        rep = report8()
        ops.adamw_step(pd, gd, md, vd, LR, step, weight_decay=wd, step_flag=P.flag(), report=rep)
        torch.cuda.synchronize()
        assert rep.tolist() == rep_ref == [1, 0, 0, 0, 0, 0, 0, 0], (n, rep)
        assert P.relmax(md, m_ref) < 1e-6 and P.relmax(vd, v_ref) < 1e-6, n
        assert_within(pd, p_ref, p_bound(p_ref), f"n {n} wd {wd} step {step} {regime}: p")
        if regime == "zero":                                                    # no update: p * decay, ONE rounding, exactly
            want = (p.double() * AR.decay_factor(LR, wd)).float()
            assert same_bits(pd, want), n


# =============================================================================== 4. the mask
@pytest.mark.parametrize("with_ema", [False, True])
def test_mask_selects_element_by_element(with_ema):
    """Masked-out elements EQUAL the step without decay, masked-in elements the step with every element decaying: the effect is
    element-wise, so bit equality holds (for the EMA as well)."""
    for n in ALL_N:
        p, gr, m, v, e = state(n, 2, 1.0, 2)
        gd, = dev(gr)
        mask = AR.mask_from_ranges(n, RANGES)
        words = ops.pack_decay_mask(n, clipped_ranges(n))
        runs = {}
        for name, kw in (("none", dict(weight_decay=0.0)), ("all", dict(weight_decay=0.5)),
                         ("masked", dict(weight_decay=0.5, decay_mask=words))):
            pd, md, vd, ed = dev(p, m, v, e)
            rep = report8()
            ops.adamw_step(pd, gd, md, vd, LR, 2, ema=ed if with_ema else None, ema_decay=0.9, step_flag=P.flag(), report=rep, **kw)
            torch.cuda.synchronize()
            assert rep.tolist() == [1, 0, 0, 0, 0, 0, 0, 0]
            runs[name] = [bits(t) for t in (pd, md, vd, ed)]
        if not with_ema:
            pa, ma, va = dev(p, m, v)
            ops.adam_step(pa, gd, ma, va, LR, 2, step_flag=P.flag(), report=P.report_words())
            assert torch.equal(bits(pa), runs["none"][0])
        for k in range(4 if with_ema else 3):
            assert torch.equal(runs["masked"][k][~mask], runs["none"][k][~mask]), (n, k)
            assert torch.equal(runs["masked"][k][mask], runs["all"][k][mask]), (n, k)
        assert not torch.equal(runs["all"][0][mask], runs["none"][0][mask])      # (decay 0.9995 is there to be seen)
        if not with_ema:
            assert torch.equal(runs["masked"][3], bits(e))                       # an EMA arena that was not passed is not written


# =============================================================================== 5. the EMA
@pytest.mark.parametrize("d", [0.999, 0.9])
def test_ema_matches_the_restatement(d):
    for n in ALL_N:
        p, gr, m, v, e = state(n, 2, 1.0, 3)
        p_ref, m_ref, v_ref, e_ref, _, _ = AR.adamw_ref(p, gr, m, v, LR, 2, 0.01, ema=e, ema_decay=d)
        pd, md, vd, ed, gd = dev(p, m, v, e, gr)
        rep = report8()
        ops.adamw_step(pd, gd, md, vd, LR, 2, weight_decay=0.01, ema=ed, ema_decay=d, step_flag=P.flag(), report=rep)
        # ... and p, m, v with ema given EQUAL the same call without it
        pq, mq, vq = dev(p, m, v)
        ops.adamw_step(pq, gd, mq, vq, LR, 2, weight_decay=0.01, step_flag=P.flag())
        torch.cuda.synchronize()
        assert rep.tolist() == [1, 0, 0, 0, 0, 0, 0, 0]
        assert same_bits(pd, pq) and same_bits(md, mq) and same_bits(vd, vq), n
        assert_within(pd, p_ref, p_bound(p_ref), f"n {n} d {d}: p")
        assert_within(ed, e_ref, e_bound(d, e, p_ref), f"n {n} d {d}: ema")
        assert not same_bits(ed, e)


def test_ema_decay_zero_copies_the_new_parameters_and_a_second_call_changes_ema_only():
    for n in ALL_N:
        p, gr, m, v, e = state(n, 2, 1.0, 4)
        pd, md, vd, ed, gd = dev(p, m, v, e, gr)
        ops.adamw_step(pd, gd, md, vd, LR, 2, weight_decay=0.01, ema=ed, ema_decay=0.0, step_flag=P.flag())
        torch.cuda.synchronize()
        assert same_bits(ed, pd), n                                              # e_new == p_new bit for bit
        # the same step from the same state with ema prefilled differently: p, m, v as before, ema different
        pq, mq, vq = dev(p, m, v)
        e2 = torch.full((n,), 7.0, device=DEV)
        ops.adamw_step(pq, gd, mq, vq, LR, 2, weight_decay=0.01, ema=e2, ema_decay=0.9, step_flag=P.flag())
        torch.cuda.synchronize()
        assert same_bits(pq, pd) and same_bits(mq, md) and same_bits(vq, vd), n
        want = AR.f32(0.9) * 7.0 + AR.one_minus(0.9) * pd.cpu().double()
        assert bool(((e2.cpu().double() - want).abs() <= 2.0 ** -23 * (6.3 + want.abs())).all()), n


# =============================================================================== 6. untouched state
@pytest.mark.parametrize("partials", [False, True])
def test_step_flag_leaves_all_four_arenas_alone(partials):
    for n in (5, 33, 4 * 10007 + 3, GRID_N):                                     # (GRID_N: the early return holds in every workgroup)
        p, gr, m, v, e = state(n, 2, 1.0, 5)
        gd, = dev(gr)
        for words, want in (((1.0, 0.0), [1, 1, 0, 0, 0, 0, 0]), ((2.0, 1.0), [1, 1, 0, 1, 0, 0, 0])):
            pd, md, vd, ed = dev(p, m, v, e)
            rep = report8()
            kw = dict(max_norm=1.0, partials=ops.grad_sqnorm(gd)) if partials else {}
            ops.adamw_step(pd, gd, md, vd, LR, 2, weight_decay=0.1, ema=ed, ema_decay=0.9, step_flag=P.flag(*words), report=rep, **kw)
            torch.cuda.synchronize()
            rep = rep.tolist()
            assert rep[:6] == want[:6] and rep[7] == 0 and (partials or rep[6] == 0), (n, words, rep)
            assert same_bits(pd, p) and same_bits(md, m) and same_bits(vd, v) and same_bits(ed, e), (n, words)


@pytest.mark.parametrize("bad", [INF, NAN])
@pytest.mark.parametrize("where", ["body", "tail", "second_pass"])
def test_nonfinite_gradient_with_partials_drops_the_step_ema_included(where, bad):
    n = GRID_N if where == "second_pass" else 4 * 10007 + 3
    k = {"body": 4 * 5003 + 2, "tail": n - 1, "second_pass": 4 * 4096 * 256 + 4 * 501 + 1}[where]
    assert k < n and (where != "tail" or k >= (n // 4) * 4)
    p, gr, m, v, e = state(n, 2, 1.0, 6)
    clean, = dev(gr)
    dirty = clean.clone()
    dirty[k] = bad
    pd, md, vd, ed = dev(p, m, v, e)
    words = ops.pack_decay_mask(n, clipped_ranges(n))
    for max_norm in (INF, 1.0):
        rep = report8()
        ops.adamw_step(pd, dirty, md, vd, LR, 2, weight_decay=0.1, decay_mask=words, ema=ed, ema_decay=0.9, max_norm=max_norm,
                       partials=ops.grad_sqnorm(dirty), step_flag=P.flag(), report=rep)
        torch.cuda.synchronize()
        rep = rep.tolist()
        assert rep[:6] == [1, 0, 0, 0, 0, 1] and rep[7] == 0, (where, bad, rep)
        assert same_bits(pd, p) and same_bits(md, m) and same_bits(vd, v) and same_bits(ed, e)
    rep = report8()
    ops.adamw_step(pd, clean, md, vd, LR, 2, weight_decay=0.1, decay_mask=words, ema=ed, ema_decay=0.9, max_norm=INF,
                   partials=ops.grad_sqnorm(clean), step_flag=P.flag(), report=rep)
    torch.cuda.synchronize()
    assert rep.tolist()[:6] == [1, 0, 0, 0, 0, 0]
    p_ref, m_ref, v_ref, e_ref, _, _ = AR.adamw_ref(p, gr, m, v, LR, 2, 0.1, AR.mask_from_ranges(n, RANGES), e, 0.9, max_norm=INF)
    assert P.relmax(md, m_ref) < 1e-6 and P.relmax(vd, v_ref) < 1e-6
    assert_within(pd, p_ref, p_bound(p_ref), f"{where}: p behind the drop")
    assert_within(ed, e_ref, e_bound(0.9, e, p_ref), f"{where}: ema behind the drop")


@pytest.mark.parametrize("at", ["body", "tail"])
def test_inf_gradient_without_partials_behaves_as_adam_step(at):
    n = 4 * 10007 + 1
    p, gr, m, v, e = state(n, 1, 1.0, 7)
    k = 4 * 5003 + 2 if at == "body" else n - 1
    gd, = dev(gr)
    gd[k] = INF
    pa, ma, va = dev(p, m, v)
    ra = P.report_words()
    ops.adam_step(pa, gd, ma, va, LR, 1, step_flag=P.flag(), report=ra)
    pd, md, vd, ed = dev(p, m, v, e)
    rep = report8()
    ops.adamw_step(pd, gd, md, vd, LR, 1, ema=ed, ema_decay=0.9, step_flag=P.flag(), report=rep)
    torch.cuda.synchronize()
    assert ra.tolist() == [1, 0, 1, 0] and rep.tolist() == [1, 0, 1, 0, 0, 0, 0, 0], (ra, rep)
    bad = ~torch.isfinite(pd.cpu())
    assert int(bad.sum()) == 1 and bool(bad[k]) and torch.equal(bad, ~torch.isfinite(pa.cpu()))
    assert torch.equal(bits(pd)[~bad], bits(pa)[~bad]) and same_bits(md, ma) and same_bits(vd, va)
    assert torch.equal(~torch.isfinite(ed.cpu()), bad)


# =============================================================================== 7. clipping, decay and EMA together
def test_clipping_decay_and_ema_together():
    for n in ALL_N:
        gr = state(n, 2, 1.0, 8)[1]
        norm = CR.norm_ref(gr)
        max_norm = float(np.float32(norm / 1000.0))
        _, nonfinite, clipped, scale = CR.clip_decision(gr, max_norm)
        assert clipped and not nonfinite
        p, gr2, m, v, e = state(n, 2, float(np.float32(scale)), 8)                # the moments the CLIPPED gradient leaves behind
        assert torch.equal(gr, gr2)
        mask = AR.mask_from_ranges(n, RANGES)
        p_ref, m_ref, v_ref, e_ref, rep_ref, _ = AR.adamw_ref(p, gr, m, v, LR, 2, 0.1, mask, e, 0.99, max_norm=max_norm)
        pd, md, vd, ed, gd = dev(p, m, v, e, gr)
        rep = report8()
        ops.adamw_step(pd, gd, md, vd, LR, 2, weight_decay=0.1, decay_mask=ops.pack_decay_mask(n, clipped_ranges(n)), ema=ed,
                       ema_decay=0.99, max_norm=max_norm, partials=ops.grad_sqnorm(gd), step_flag=P.flag(), report=rep)
        torch.cuda.synchronize()
        rep = rep.tolist()
        assert rep[:6] == rep_ref[:6] == [1, 0, 0, 0, 1, 0] and rep[7] == 0, (n, rep)
        assert abs(int(rep[6]) - int(np.float32(norm).view(np.int32))) <= 1
        assert P.relmax(md, m_ref) < 1e-6 and P.relmax(vd, v_ref) < 1e-6, n
        assert_within(pd, p_ref, p_bound(p_ref), f"n {n}: p")
        assert_within(ed, e_ref, e_bound(0.99, e, p_ref), f"n {n}: ema")


def test_every_workgroup_applies_the_same_scale():
    """g = 1, p = 1, ema = 2 everywhere, m = v = 0, step 1: m, v, p and ema are the same float32 in every element iff every
    workgroup derived the same scale, to the last bit (a scale that is no power of two: its rounding is in play)."""
    n = GRID_N
    g, p, e = torch.ones(n, device=DEV), torch.ones(n, device=DEV), torch.full((n,), 2.0, device=DEV)
    m, v = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    max_norm = 3.0
    scale = float(np.float32(max_norm / (math.sqrt(n) + 1e-6)))
    assert scale < 1.0 and math.frexp(scale)[0] != 0.5
    rep = report8()
    ops.adamw_step(p, g, m, v, LR, 1, weight_decay=0.1, ema=e, ema_decay=0.99, max_norm=max_norm, partials=ops.grad_sqnorm(g),
                   step_flag=P.flag(), report=rep)
    torch.cuda.synchronize()
    assert rep.tolist()[:6] == [1, 0, 0, 0, 1, 0]
    for t in (m, v, p, e):
        assert bool((bits(t) == bits(t)[0]).all())
    b1 = np.float32(0.9)
    assert abs(float(m[0]) - float((np.float32(1) - b1) * np.float32(scale))) <= 2.0 ** -23 * float(m[0])
    assert float(p[0]) < 1.0 and 1.0 < float(e[0]) < 2.0


# =============================================================================== 8. argument errors at the ABI
def test_entry_point_refuses_bad_arguments():
    p, g, m, v, e = (torch.zeros(8, device=DEV) for _ in range(5))
    part = ops.grad_sqnorm(g)
    L = _lib.lib()
    s = ops.stream_ptr()

    def call(p=p, g=g, m=m, v=v, n=8, step=1, max_norm=1.0, partials=None, wd=0.0, ema_decay=0.0):
        return L.inet_adam_step_w(ops.ptr(p), ops.ptr(g), ops.ptr(m), ops.ptr(v), n, LR, 0.9, 0.999, 1e-8, step, 1.0, max_norm,
                                  ops.ptr(partials), wd, None, ops.ptr(e), ema_decay, None, None, s)
    for kw in (dict(p=None), dict(g=None), dict(m=None), dict(v=None), dict(n=0), dict(n=-4), dict(step=0),
               dict(wd=-1.0), dict(wd=NAN), dict(wd=INF), dict(ema_decay=-0.5), dict(ema_decay=1.0), dict(ema_decay=2.0),
               dict(ema_decay=NAN), dict(partials=part, max_norm=0.0), dict(partials=part, max_norm=-1.0),
               dict(partials=part, max_norm=NAN)):
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert float(p.abs().max()) == 0.0 and float(e.abs().max()) == 0.0
    assert call(max_norm=NAN) == 0 and call(max_norm=-1.0) == 0                  # without partials max_norm is ignored
    assert call(partials=part, max_norm=INF) == 0
    with pytest.raises(ValueError):
        ops.adamw_step(p, g, m, v, LR, 1, weight_decay=-1.0)
    torch.cuda.synchronize()


# =============================================================================== 9. Trainer(weight_decay=, ema_decay=)
CFG = dict(V=20, E=6, H=256, Z=24)                   # the small MeasureVAE of tests/test_gpu_dp.py
B, STEPS = 32, 3


def _vae(**kw):
    from inpaintnet_amd import synthetic
    from inpaintnet_amd.measure_vae import MeasureVAE
    from inpaintnet_amd.vae_trainer import VAETrainer
    ds = synthetic.SyntheticFolkDataset(num_notes=CFG["V"])
    model = MeasureVAE(ds, note_embedding_dim=CFG["E"], encoder_hidden_size=CFG["H"], latent_space_dim=CFG["Z"],
                       decoder_hidden_size=CFG["H"], encoder_dropout_prob=0.0, decoder_dropout_prob=0.0)
    model.load_state_dict({k: torch.from_numpy(synthetic.det_param(k, tuple(v.shape))) for k, v in model.state_dict().items()})
    trainer = VAETrainer(ds, model, lr=1e-3, **kw)
    model.train()
    tok = torch.from_numpy(synthetic.det_tokens("adamw", (B, 24), CFG["V"])).cuda()
    return model, trainer, tok


def _backward(trainer, tok):
    trainer.zero_grad()
    loss, acc = trainer.loss_and_acc_for_batch(tok, 0, train=True)
    loss.backward()
    ops.side_join()


@functools.lru_cache(maxsize=None)
def trained(max_grad_norm=None):
    """Three steps of Trainer(weight_decay=0.01, ema_decay=0.9): the gradient of every step read back, the launch labels of the
    last one, and the state in front of the first.  Shared by the trainer tests; nothing in it is written to afterwards."""
    from tests.test_gpu_decode_plans import labels_of
    model, trainer, tok = _vae(weight_decay=0.01, ema_decay=0.9, max_grad_norm=max_grad_norm)
    start = model.flat.cpu().clone()
    assert same_bits(trainer.ema, model.flat) and trainer.ema.data_ptr() != model.flat.data_ptr()
    grads, labels = [], None
    for s in range(STEPS):
        _backward(trainer, tok)
        torch.cuda.synchronize()
        grads.append(model.grad.cpu().clone())
        if s == STEPS - 1:
            _, labels = labels_of(trainer.step)
        else:
            trainer.step()
    trainer.finish()
    return model, trainer, tok, start, grads, labels


def test_trainer_follows_the_restatement_over_three_steps():
    """model.flat and trainer.ema against three steps of the restatement fed with the gradients read back from the device, the mask
    derived from state_dict() names and shapes.  Bounds 3 and 5 compounded: a step passes p's error on times decay < 1 and adds its
    own, so three steps stay below the sum of the three per-step bounds; the EMA passes its error on times d and adds bound 5 with
    p's compounded bound in the place of the single step's."""
    model, trainer, tok, start, grads, labels = trained()
    n = start.numel()
    mask = torch.zeros(n, dtype=torch.bool)
    where = {}
    for name, t in model.state_dict().items():                                  # (where the model keeps the tensor: the arena has gaps)
        off = (model.param(name).data_ptr() - model.flat.data_ptr()) // 4
        assert 0 <= off and off + t.numel() <= n, name
        where[name] = (off, off + t.numel())
        if "weight" in name and t.dim() == 2:
            mask[off:off + t.numel()] = True
    assert 0 < int(mask.sum()) < n
    p, m, v, e = start.double(), torch.zeros(n).double(), torch.zeros(n).double(), start.double()
    pb, eb = torch.zeros(n).double(), torch.zeros(n).double()
    df, omd = AR.f32(0.9), AR.one_minus(0.9)
    for s in range(STEPS):
        e_prev = e
        p, m, v, e, rep, _ = AR.adamw_ref(p, grads[s], m, v, trainer.lr, s + 1, 0.01, mask, e, 0.9)
        pb = pb + p_bound(p, trainer.lr)
        eb = df * eb + 2.0 ** -23 * ((df * e_prev).abs() + (omd * p).abs()) + omd * pb
    assert trainer.adam_t == STEPS and trainer._reports.shape == (trainer._NREP, 8)
    assert P.relmax(trainer.adam_m, m) < 1e-6 and P.relmax(trainer.adam_v, v) < 1e-6
    assert_within(model.flat, p, pb, "trainer: p")
    assert_within(trainer.ema, e, eb, "trainer: ema")
    assert labels.count("adamw") == 1 and "adam" not in labels and "grad_sqnorm" not in labels and "adamw_clip" not in labels
    assert trainer.last_grad_norm is None and trainer.clipped_steps == 0        # (a report without partials carries no norm)
    sd = trainer.ema_state_dict()
    assert list(sd) == list(model.state_dict()) and all(sd[k].shape == t.shape for k, t in model.state_dict().items())
    assert all(same_bits(sd[k].reshape(-1), trainer.ema[a:b]) for k, (a, b) in where.items())


def test_trainer_biases_do_not_decay_and_the_default_trainer_launches_what_it_launched():
    """The same three gradients through a trainer built with the defaults: its biases (and b_0 / x_0) EQUAL the decaying run's bit
    for bit, its weight matrices do not; its launches carry today's labels (its records have eight words like everybody's)."""
    from tests.test_gpu_decode_plans import labels_of
    model_w, trainer_w, tok, start, grads, _ = trained()
    model, trainer, _ = _vae()
    assert trainer.ema is None and trainer._decay_mask is None
    for s in range(STEPS):
        trainer.zero_grad()
        model.grad.copy_(grads[s])
        if s == STEPS - 1:
            _, labels = labels_of(trainer.step)
        else:
            trainer.step()
    trainer.finish()
    assert labels.count("adam") == 1 and "adamw" not in labels and "grad_sqnorm" not in labels
    assert trainer._reports.shape == (trainer._NREP, 8)
    decayed = 0
    for name, t in model.state_dict().items():
        same = same_bits(t, model_w.state_dict()[name])
        if "weight" in name and t.dim() == 2:
            assert not same, name
            decayed += 1
        else:
            assert same, name
    assert decayed > 0
    assert same_bits(trainer.adam_m, trainer_w.adam_m) and same_bits(trainer.adam_v, trainer_w.adam_v)


def test_trainer_with_max_grad_norm_measures_in_front():
    model, trainer, tok, start, grads, labels = trained(math.inf)
    assert "grad_sqnorm" in labels and "adamw_clip" in labels and "adam_clip" not in labels and "adamw" not in labels
    assert labels.index("grad_sqnorm") < labels.index("adamw_clip")
    norm64 = float(grads[-1].double().pow(2).sum().sqrt())
    assert abs(trainer.last_grad_norm - norm64) <= 1e-6 * norm64
    assert trainer.clipped_steps == 0 and trainer.nonfinite_steps == 0 and trainer.adam_t == STEPS


# =============================================================================== 10. ema_weights()
VAL_B = 4                                            # the validation batch of the ema_weights() test: see its docstring


def _validate(trainer, tok):
    """The validation pass of one batch: the loss as the trainer computes it on the device, and what it is a function of -- the logits
    and the encoder's mu / log sigma -- from a second, identical forward pass."""
    torch.manual_seed(5)                                                        # (the encoder's eps comes from torch's device generator)
    with torch.no_grad():
        loss, _ = trainer.loss_and_acc_for_batch(tok, 0, train=False)
        torch.manual_seed(5)
        out = trainer.model(measure_score_tensor=tok, train=False)
    return loss.clone(), out[0].clone(), out[2].loc.clone(), out[2].log_scale.clone()


def _loss64(w, mu, ls, tok):
    """The validation loss (mean cross-entropy + 1e-3 * mean_b KL) in float64 on the host, in one fixed order."""
    ce = torch.nn.functional.cross_entropy(w.double().cpu().reshape(-1, w.shape[-1]), tok.cpu().reshape(-1).long())
    mu, ls = mu.double().cpu(), ls.double().cpu()
    kl = (0.5 * ((2.0 * ls).exp() + mu * mu - 1.0) - ls).sum(1).mean()
    return float(ce + 1e-3 * kl)


def test_ema_weights_swaps_restores_and_refuses_a_step():
    """... and the validation loss of one batch under the context EQUALS that of a fresh model that loaded ema_state_dict().

    The batch is VAL_B = 4 measures, a size at which the library's forward pass reproduces itself (as at 8): at 1, 2, 16 and 32
    two IDENTICAL calls on one model return different logits, because products with a split of K accumulate with f32
    atomics in an order that changes from launch to launch and the free-running decoder feeds every flipped
    argmax back.  That is asserted first -- two identical calls inside the context return the same bits -- so a planner change that
    takes it away shows here as what it is.  Then, against the fresh model, bit for bit: every logit, the encoder's mu and log sigma,
    and with them the loss computed from them in float64 in one fixed order.
    The loss as the DEVICE sums it is a function of those values AND of the order in which ce_kernel's float atomics retire: at this
    batch the kernel adds 24 workgroups' shares and the KL term into one float, and eight identical calls on one model returned two
    different loss bit patterns from eight times the same logits.  No assertion about its bits can hold even between a model and
    itself, so it is held to what the order can do: 25 additions of non-negative terms, each rounding by at most 2^-24 of a partial
    sum <= loss, in two orders: 50 * 2^-24 * loss.
    The own weights' logits -- what a value that survived the swap would produce -- must differ."""
    from inpaintnet_amd import synthetic
    from inpaintnet_amd.measure_vae import MeasureVAE
    model, trainer, tok, *_ = trained()
    own = model.flat.clone()
    val = tok[:VAL_B].contiguous()
    assert not same_bits(own, trainer.ema)
    model.eval()
    try:
        with trainer.ema_weights():
            assert same_bits(model.flat, trainer.ema)
            with pytest.raises(RuntimeError, match="ema_weights"):
                trainer.step()
            loss_in, w_in, mu_in, ls_in = _validate(trainer, val)
            again = _validate(trainer, val)
            assert all(same_bits(a, b) for a, b in zip((w_in, mu_in, ls_in), again[1:])), "the forward pass does not reproduce itself"
        assert same_bits(model.flat, own)
        with pytest.raises(KeyError):
            with trainer.ema_weights():
                raise KeyError("inside")
        assert same_bits(model.flat, own) and trainer._ema_swapped is None
        # a fresh model that loaded the EMA (nothing derived from the old weights may have survived the swap)
        fresh = MeasureVAE(synthetic.SyntheticFolkDataset(num_notes=CFG["V"]), note_embedding_dim=CFG["E"],
                           encoder_hidden_size=CFG["H"], latent_space_dim=CFG["Z"], decoder_hidden_size=CFG["H"],
                           encoder_dropout_prob=0.0, decoder_dropout_prob=0.0)
        fresh.load_state_dict(trainer.ema_state_dict())
        fresh.eval()
        assert same_bits(fresh.flat, trainer.ema)
        from inpaintnet_amd.vae_trainer import VAETrainer
        other = VAETrainer(trainer.dataset, fresh, lr=1e-3)
        loss_f, w_f, mu_f, ls_f = _validate(other, val)
        loss_own, w_own, mu_own, ls_own = _validate(trainer, val)
        l_in, l_f, l_own = _loss64(w_in, mu_in, ls_in, val), _loss64(w_f, mu_f, ls_f, val), _loss64(w_own, mu_own, ls_own, val)
        print(f"loss under ema_weights() {l_in!r}, of the fresh model {l_f!r}, of the own weights {l_own!r}; as the device sums it "
              f"{float(loss_in)!r}, {float(loss_f)!r}, {float(loss_own)!r}; logits vs the own weights {float((w_in - w_own).abs().max()):.2e}")
        assert same_bits(w_in, w_f) and same_bits(mu_in, mu_f) and same_bits(ls_in, ls_f)
        assert l_in == l_f
        assert abs(float(loss_in) - float(loss_f)) <= 50 * 2.0 ** -24 * l_f
        assert abs(float(loss_f) - l_f) <= 1e-5 * l_f                          # (and the device's float32 loss is that loss)
        assert not same_bits(w_in, w_own) and l_in != l_own                     # (the EMA is not the weights: a stale value would show)
    finally:
        model.train()


# =============================================================================== 11. training state
def test_training_state_round_trip(capsys):
    model, trainer, tok, *_ = trained()
    st = trainer.training_state(2)
    assert st["weight_decay"] == 0.01 and st["decay_all"] is False and st["ema_decay"] == 0.9 and st["ema_warmup"] is False
    assert not st["ema"].is_cuda and same_bits(st["ema"], trainer.ema)
    model2, trainer2, _ = _vae()
    _backward(trainer2, tok)                                                    # a record is in flight when the state arrives:
    trainer2.step()                                                             # loading drains it before it touches adam_t
    assert trainer2._reports.shape[1] == 8 and len(trainer2._inflight) == 1
    trainer2.load_training_state(st)
    assert not trainer2._inflight and trainer2._reports.shape[1] == 8
    assert (trainer2.weight_decay, trainer2.decay_all, trainer2.ema_decay, trainer2.ema_warmup) == (0.01, False, 0.9, False)
    assert same_bits(trainer2.ema, trainer.ema) and same_bits(trainer2._decay_mask, trainer._decay_mask)
    assert trainer2.adam_t == STEPS and same_bits(trainer2.adam_m, trainer.adam_m)
    _backward(trainer2, tok)                                                    # ... and it steps with them (eight-word records)
    trainer2.step()
    trainer2.finish()
    assert trainer2._reports.shape[1] == 8
    old = {k: v for k, v in st.items() if k not in ("weight_decay", "decay_all", "ema_decay", "ema_warmup", "ema")}
    model3, trainer3, _ = _vae(ema_decay=0.5)
    model3.flat.mul_(2.0)
    trainer3.load_training_state(old)
    assert same_bits(trainer3.ema, model3.flat) and trainer3.ema_decay == 0.5 and trainer3.weight_decay == 0.0
    assert "seeded" in capsys.readouterr().out
