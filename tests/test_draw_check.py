"""Draw.check (inpaintnet_amd/draw.py): every ValueError that HierarchicalDecoder.forward, LatentRNN.forward and ConstraintModel.generate
raise for their sampling arguments, once per surface's `who`, with the surface's own text -- and np.random / random untouched behind a
rejected call.  No GPU: check() draws nothing and launches nothing."""
import math
import random

import numpy as np
import pytest
import torch

from inpaintnet_amd.draw import DECODER, GENERATE, LATENT, Draw

V = 20
SHAPE = {DECODER: (2, 24), LATENT: (2, 3, 24), GENERATE: (2, 30)}


def ok_allowed(who):
    return torch.ones(SHAPE[who] + (V,), dtype=torch.bool)


def ok_forced(who):
    return torch.full(SHAPE[who], -1, dtype=torch.int64)


def empty_tick(who):
    a = ok_allowed(who)
    a[(1,) * len(SHAPE[who])] = False
    return a


def cases(who):
    """[(Draw arguments, train, a piece of the surface's text)]"""
    pre = "generate: " if who == GENERATE else ""
    bad_value = ok_forced(who)
    bad_value[(0,) * len(SHAPE[who])] = V
    out = [
        (dict(temperature=1.0, top_p=0.0), False, pre + r"top_p 0.0 outside \(0, 1\]"),
        (dict(temperature=1.0, top_p=1.5), False, pre + "top_p 1.5 outside"),
        (dict(temperature=1.0, top_p=math.nan), False, pre + "top_p nan outside"),
        (dict(temperature=1.0, top_k=2.5), False, "top_k 2.5 is not an integer"),
        (dict(temperature=1.0, forced=ok_forced(who).float()), False, pre + "forced must be an int tensor of shape"),
        (dict(temperature=1.0, forced=ok_forced(who)[..., :-1]), False, pre + "forced must be an int tensor of shape"),
        (dict(temperature=1.0, forced=ok_forced(who) == 0), False, pre + "forced must be an int tensor of shape"),
        (dict(temperature=1.0, forced=bad_value), False,
         r"generate: forced holds a value outside \[-1, 20\)" if who == GENERATE else r"forced: token indices in \[0, 20\), or -1 for a free tick"),
        (dict(temperature=1.0, forced=ok_forced(who) - 2), False, "forced"),
        (dict(temperature=1.0, allowed=ok_allowed(who).long()), False, pre + "allowed must be bool of shape"),
        (dict(temperature=1.0, allowed=ok_allowed(who)[1:]), False, pre + "allowed must be bool of shape"),
        (dict(temperature=1.0, allowed=empty_tick(who)), False, "a tick with nothing allowed" if who == LATENT else "nothing is allowed at"),
    ]
    if who == GENERATE:
        out += [(dict(temperature=1.0, uniforms=np.zeros(SHAPE[who], dtype=np.float32)), False, "generate: uniforms must be float64 of shape"),
                (dict(temperature=1.0, uniforms=np.zeros((2, 29))), False, "generate: uniforms must be float64 of shape")]
    else:                                                            # generate has no train flag and always a temperature
        out += [
            (dict(top_k=3), False, "top_k / top_p without a temperature"),
            (dict(top_p=0.5), False, "top_k / top_p without a temperature"),
            (dict(temperature=1.0, forced=ok_forced(who)), True, r"forced tokens are an inference call \(train=False\)"),
            (dict(forced=ok_forced(who)), False, "forced tokens need a temperature"),
            (dict(allowed=ok_allowed(who)), True, r"token constraints are an inference call \(train=False\)"),
            (dict(uniforms=np.zeros(SHAPE[who])), False, "uniforms without a temperature"),
            (dict(temperature=1.0), True, r"temperature sampling is an inference call \(train=False\)"),
            (dict(temperature=math.inf), False, "temperature inf is not finite"),
            (dict(temperature=math.nan), False, "temperature nan is not finite"),
            (dict(temperature=1.0, uniforms=np.zeros(SHAPE[who][:-1] + (23,))), False, "uniforms of shape"),
        ]
    return out


@pytest.mark.parametrize("who", (DECODER, LATENT, GENERATE))
def test_every_refusal_and_no_stream_touched(who):
    for kw, train, text in cases(who):
        np.random.seed(5)
        random.seed(5)
        torch.manual_seed(5)
        before = (np.random.get_state()[1].copy(), np.random.get_state()[2], random.getstate(), torch.get_rng_state().clone())
        with pytest.raises(ValueError, match=text):
            Draw(**kw).check(SHAPE[who], V, train, who)
        assert np.array_equal(np.random.get_state()[1], before[0]) and np.random.get_state()[2] == before[1], (who, kw)
        assert random.getstate() == before[2] and torch.equal(torch.get_rng_state(), before[3]), (who, kw)


@pytest.mark.parametrize("who", (DECODER, LATENT, GENERATE))
def test_one_order_for_two_invalid_arguments(who):
    """top_k / top_p are refused first on every surface, then forced, then allowed, then uniforms"""
    bad_f, bad_a = ok_forced(who).float(), ok_allowed(who).long()
    with pytest.raises(ValueError, match="top_p"):
        Draw(1.0, None, None, 0.0, bad_a, bad_f).check(SHAPE[who], V, False, who)
    with pytest.raises(ValueError, match="forced must be"):
        Draw(1.0, np.zeros((1,)), None, None, bad_a, bad_f).check(SHAPE[who], V, False, who)
    with pytest.raises(ValueError, match="allowed must be"):
        Draw(1.0, np.zeros((1,)), None, None, bad_a, None).check(SHAPE[who], V, False, who)


@pytest.mark.parametrize("who", (DECODER, LATENT, GENERATE))
def test_an_accepted_call_and_its_forms(who):
    u = np.full(SHAPE[who], 0.25)
    d = Draw(1.5, u, 3, 0.7, ok_allowed(who).numpy(), ok_forced(who).numpy()).check(SHAPE[who], V, False, who)
    assert isinstance(d.allowed, torch.Tensor) and isinstance(d.forced, torch.Tensor) and d.scored()
    assert (d.words is None) == (who == LATENT)
    assert d.uniforms.dtype == (np.float64 if who == GENERATE else torch.float64)
    assert not Draw(1.5, u).check(SHAPE[who], V, False, who).scored()
    assert Draw().check(SHAPE[who], V, True, who).temperature is None            # the training call: nothing asked, nothing refused
    if who == GENERATE:
        Draw(math.nan).check(lambda: SHAPE[who], lambda: V, False, who)          # (left to the library, which refuses it)
        one = Draw(1.0, np.zeros((1, 30)), forced=ok_forced(who)[0], allowed=ok_allowed(who)[0]).check((30,), V, False, who)
        assert tuple(one.words.shape) == (30, 1)
    if who == LATENT:
        m, f = d.measure(1), d.flat()
        assert tuple(m.uniforms.shape) == (2, 24) and tuple(m.allowed.shape) == (2, 24, V) and tuple(m.forced.shape) == (2, 24)
        assert tuple(f.uniforms.shape) == (6, 24) and tuple(f.allowed.shape) == (6, 24, V) and tuple(f.forced.shape) == (6, 24)
        assert (m.temperature, m.top_k, m.top_p) == (1.5, 3, 0.7)
