"""Host-side checks of AnticipationRNN's per-tick token constraints (no GPU): the count of FREE draws (ticks with more than one allowed
token) within 2e-5 of a step -- of the kept CDF or of the nucleus boundary -- along the float64 oracle's own masked trajectory for the
very seeds and masks tests/test_gpu_arnn_constraint.py runs, held to half that file's cap; the argument errors in front of any library
call; the new entry's signature in the header and in the package's binding; the mask AnticipationRNNTester builds."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

from inpaintnet_amd import _lib, ops
from tests import arnn_constraint_ref as ACR
from tests import arnn_trunc_ref as AR
from tests import decoder_constraint_ref as CR
from tests import decoder_trunc_ref as TR


def margin_count(V, R, E, Hc, H, U):
    W = AR.net(V, E, Hc, H, U)
    allow = CR.plan_mask(V, R, AR.L)
    free = CR.free(allow)
    out = []
    for si, (temp, k, p) in enumerate(AR.SETTINGS):
        oc, hc, u = AR.case(V, R, si, E, Hc, H, U)
        w, tok, n, cm, bm = ACR.constrained_trajectory(W, oc, hc, temp, u, k, p, allow)
        near = int((~TR.firm(cm, bm) & free).sum())
        print(f"V {V} H {H} R {R} setting {(temp, k, p)}: {near} of {int(free.sum())} free draws within the margin, kept mean {n.mean():.1f}")
        assert np.take_along_axis(allow, tok[..., None], -1).all()                  # the oracle returns no banned token
        assert np.array_equal(tok[~free], np.argmax(allow, -1)[~free])              # ... and every fixed tick's token
        assert n.min() >= 1
        out.append((near, int(free.sum())))
    return tuple(sum(x) for x in zip(*out))                  # a case: (V, R) under the three settings


@pytest.mark.parametrize("R", AR.ROWS)
@pytest.mark.parametrize("V", AR.FULL_V)
def test_margin_counts_of_the_token_pass_cases(V, R):
    """Per case of test_gpu_arnn_constraint.test_the_rule_on_the_calls_own_logits -- (V, R) under the three settings -- at most half its
    cap of 5 % of the free draws."""
    near, draws = margin_count(V, R, **AR.FULL)
    assert 0 < draws < 3 * R * AR.L and near <= 0.5 * AR.NEAR_CAP * draws, (V, R, near, draws)


@pytest.mark.parametrize("R", AR.ROWS)
def test_margin_counts_of_the_per_tick_cases(R):
    c = dict(AR.SMALL)
    V = c.pop("V")
    near, draws = margin_count(V, R, **c)
    assert 0 < draws < 3 * R * AR.L and near <= 0.5 * AR.NEAR_CAP * draws, (R, near, draws)


def test_the_plan_mask_fixes_every_fourth_tick_and_bans_a_fifth_elsewhere():
    for V in AR.FULL_V + (AR.SMALL["V"],):
        a = CR.plan_mask(V, 11, AR.L)
        r, t = np.meshgrid(np.arange(11), np.arange(AR.L), indexing="ij")
        fixed = (r + t) % 4 == 0
        assert (a.sum(-1)[fixed] == 1).all() and np.array_equal(CR.free(a), ~fixed)
        banned = (~a).sum(-1)[~fixed]
        assert banned.min() >= V // 5 and banned.max() <= V // 5 + 1
        assert not np.array_equal(a[8], a[0]) and not np.array_equal(a[10], a[2])   # rows of a second launch differ from the first's


def test_a_fixed_token_moves_the_oracles_next_logits():
    """What the GPU feedback test relies on: teacher-forced over tokens that differ at ONE tick t, the oracle's logits are equal up to t
    and move at t + 1 by far more than 1e-3 of max |logit|."""
    W = AR.net(48, **AR.FULL)
    oc, hc, u = AR.case(48, 1, 1, **AR.FULL)
    w, tok, _, _, _ = AR.truncated_trajectory(W, oc, hc, 1.5, u, 0, 1.0)
    t = 9
    other = tok.copy()
    other[0, t] = (tok[0, t] + 17) % 48
    w2, _ = AR.trajectory(W, oc, hc, tokens=other)
    assert np.array_equal(w2[:, :t + 1], w[:, :t + 1])
    assert np.abs(w2[0, t + 1] - w[0, t + 1]).max() > 1e-3 * np.abs(w).max()


def test_argument_errors_come_before_any_library_call(monkeypatch):
    from inpaintnet_amd.arnn import ConstraintModelGaussianReg
    from inpaintnet_amd.arnn_tester import AnticipationRNNTester
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("a library call in front of the argument check"))
    V, L = 12, 48
    # ops.arnn_sample: the words' shape, dtype and place
    oc = torch.zeros(3, L, 16)
    net = [None] * 10 + [torch.zeros(V, 16), None]                       # (..., W2, b2)
    for bad in (torch.ones(3, L, 2, dtype=torch.int64), torch.ones(3, L, dtype=torch.int64), torch.ones(2, L, 1, dtype=torch.int64),
                torch.ones(3, L + 1, 1, dtype=torch.int64), torch.ones(3, L, 1, dtype=torch.int32), torch.ones(3, L, 1, dtype=torch.bool),
                torch.ones(3, L, 1, dtype=torch.int64), np.ones((3, L, 1), dtype=np.int64)):      # (the last two: not on the device)
        with pytest.raises(ValueError):
            ops.arnn_sample(None, oc, *net, 1.0, None, allowed=bad)
    # generate: bool (L, V) for the one row, (B, L, V) for a batch; no empty tick
    me = types.SimpleNamespace(num_notes_per_voice=[V])
    one, batch = torch.zeros(1, L, dtype=torch.int64), torch.zeros(3, 1, L, dtype=torch.int64)
    ok = torch.ones(L, V, dtype=torch.bool)
    for score, bad in ((one, torch.ones(L, V + 1, dtype=torch.bool)), (one, torch.ones(L + 1, V, dtype=torch.bool)),
                       (one, torch.ones(1, L, V, dtype=torch.bool)), (one, torch.ones(L, V, dtype=torch.int64)),
                       (batch, ok), (batch, torch.ones(2, L, V, dtype=torch.bool)), (batch, torch.ones(3, 1, L, V, dtype=torch.bool))):
        with pytest.raises(ValueError):
            ConstraintModelGaussianReg.generate(me, score, None, None, allowed=bad)
    empty = ok.clone()
    empty[7] = False
    with pytest.raises(ValueError, match="nothing is allowed"):
        ConstraintModelGaussianReg.generate(me, one, None, None, allowed=empty)
    with pytest.raises(ValueError, match="nothing is allowed"):
        ConstraintModelGaussianReg.generate(me, batch, None, None, allowed=empty.expand(3, L, V))
    # the tester: out-of-range fixed / banned / score tokens, shapes
    ds = types.SimpleNamespace(subdivision=6, num_beats_per_bar=4)
    te = types.SimpleNamespace(dataset=ds, measure_seq_len=24, model=types.SimpleNamespace(num_notes_per_voice=[V]))
    te._allowed = types.MethodType(AnticipationRNNTester._allowed, te)
    score = torch.arange(96).remainder(V)[None]
    free = torch.full((2, 24), -1)

    def window(**kw):
        return AnticipationRNNTester._generate_window(te, score, None, 2, 2, **kw)
    for banned in ([V], [-1], [2.5], list(range(V))):
        with pytest.raises(ValueError):
            window(banned_tokens=banned)
    for fixed in (free.clone().fill_(V), free.clone().fill_(-2), free.float(), free == -1, torch.full((24,), -1), torch.full((3, 24), -1),
                  torch.full((4, 12), -1)):
        with pytest.raises(ValueError):
            window(fixed_tokens=fixed)
    outside = score.clone()
    outside[0, 3] = V                                                        # the model's no-constraint symbol is no token of the head
    with pytest.raises(ValueError):
        AnticipationRNNTester._generate_window(te, outside, None, 2, 2, clamp_context=True)
    below = score.clone()
    below[0, 90] = -1
    with pytest.raises(ValueError):
        AnticipationRNNTester._generate_window(te, below, None, 2, 2, clamp_context=True)


def test_the_testers_mask():
    """banned_tokens act on the window alone; a fixed tick wins over a ban; clamp_context fixes exactly the ticks outside the window;
    fixed_tokens may be flat; without the three there is no mask."""
    from inpaintnet_amd.arnn_tester import AnticipationRNNTester
    V, L, a, b = 12, 96, 24, 72
    te = types.SimpleNamespace(measure_seq_len=24, model=types.SimpleNamespace(num_notes_per_voice=[V]))
    score = (torch.arange(L) * 5).remainder(V)[None]
    mask = lambda **kw: AnticipationRNNTester._allowed(te, score, a, b, 24, kw.get("banned"), kw.get("fixed"), kw.get("clamp", False))
    assert mask() is None
    m = mask(banned=[0, 3])
    assert m.dtype == torch.bool and tuple(m.shape) == (L, V)
    assert bool(m[:a].all()) and bool(m[b:].all())
    assert not bool(m[a:b, [0, 3]].any()) and bool(m[a:b, [1, 2] + list(range(4, V))].all())
    fixed = torch.full((2, 24), -1)
    fixed[0, 5], fixed[1, 23] = 3, 7                                       # 3 is banned: the fixed tick wins
    m = mask(banned=[0, 3], fixed=fixed)
    assert m[a + 5].nonzero().flatten().tolist() == [3] and m[a + 47].nonzero().flatten().tolist() == [7]
    rest = torch.ones(L, dtype=torch.bool)
    rest[[a + 5, a + 47]] = False
    assert torch.equal(m[rest], mask(banned=[0, 3])[rest])
    assert torch.equal(mask(banned=[0, 3], fixed=fixed.reshape(-1)), m)
    c = mask(clamp=True)
    assert bool(c[a:b].all())
    out = torch.cat((torch.arange(a), torch.arange(b, L)))
    assert bool((c[out].sum(-1) == 1).all()) and torch.equal(c[out].float().argmax(-1), score[0, out])
    both = mask(banned=[0, 3], fixed=fixed, clamp=True)
    assert torch.equal(both[a:b], m[a:b]) and torch.equal(both[out], c[out])
    words = ops.pack_allowed(both)
    assert np.array_equal(words.numpy().view(np.uint64), CR.words(both.numpy()))


def test_header_and_binding_agree_on_the_new_entry():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "inpaintnet_hip.h")).read()
    protos = {}
    for name in ("inet_arnn_sample_ex", "inet_arnn_sample_cx"):
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", hdr)
        assert m, name
        protos[name] = [" ".join(a.split()) for a in m.group(1).split(",")]
    old, new = protos["inet_arnn_sample_ex"], protos["inet_arnn_sample_cx"]
    assert new[:len(old) - 1] == old[:-1] and old[-1] == "void* stream"
    assert new[len(old) - 1:] == ["const uint64_t* allow", "void* stream"]
    res, args = _lib._SIGNATURES["inet_arnn_sample_cx"]
    res0, args0 = _lib._SIGNATURES["inet_arnn_sample_ex"]
    assert res is C.c_int and args[:len(args0) - 1] == args0[:-1]
    assert args[len(args0) - 1:] == [C.c_void_p, C.c_void_p]
    assert "inet_arnn_sample_cx" in _lib.EXPORTS


def test_the_entry_refuses_what_inet_arnn_sample_ex_refuses():
    _lib.build(verbose=False)
    Lb = _lib.lib()
    X, NULL, big = C.c_void_p(16), None, 1 << 40      # X: a pointer that is never followed (tests/test_pointwise_host.py)
    net = [X] * 12

    def cx(R=1, Ln=4, emb=X, oc=X, u=X, tokens=X, ws=X, nws=big, temp=1.0, k=0, p=1.0, H=256):
        return Lb.inet_arnn_sample_cx(R, Ln, 10, 256, H, 256, 48, emb, oc, 256, 256 * Ln, *net, temp, u, NULL, tokens, ws, nws, k, p, NULL,
                                      NULL, X, NULL)
    nan, inf = float("nan"), float("inf")
    calls = {"R": cx(R=0), "L": cx(Ln=0), "emb": cx(emb=NULL), "oc": cx(oc=NULL), "uniforms": cx(u=NULL), "tokens": cx(tokens=NULL),
             "ws": cx(ws=NULL), "ws_floats": cx(nws=16), "temperature inf": cx(temp=inf), "temperature nan": cx(temp=nan), "H": cx(H=250),
             "top_p 0": cx(p=0.0), "top_p > 1": cx(p=1.0000001), "top_p nan": cx(p=nan)}
    assert {k: v for k, v in calls.items() if v != -1} == {}
