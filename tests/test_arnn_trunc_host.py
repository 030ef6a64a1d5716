"""Host-side checks of AnticipationRNN's truncated sampling (no GPU): the count of draws within 2e-5 of a step -- of the kept CDF or of
the nucleus boundary -- along the float64 oracle's own trajectory for the very seeds tests/test_gpu_arnn_trunc.py runs, held to half
that file's cap; the argument errors in front of any library call; the model-independent restatement of the rule
(tests/decoder_trunc_ref.py) against the restated generate() of tests/test_arnn_generate_host.py, step by step; the new entry's
signature in the header and in the package's binding."""
import ctypes as C
import re
import os
import types

import numpy as np
import pytest
import torch

from inpaintnet_amd import _lib, ops
from oracle import torch_ref as O
from tests import arnn_trunc_ref as AR
from tests import decoder_trunc_ref as TR
from tests import golden_util as G
from tests import test_arnn_generate_host as GH

X = C.c_void_p(16)              # a pointer that is never followed (tests/test_pointwise_host.py)
NULL = None


def margin_count(V, R, E, Hc, H, U):
    W = AR.net(V, E, Hc, H, U)
    out = []
    for si, (temp, k, p) in enumerate(AR.SETTINGS):
        oc, hc, u = AR.case(V, R, si, E, Hc, H, U)
        w, tok, n, cm, bm = AR.truncated_trajectory(W, oc, hc, temp, u, k, p)
        near = int((~TR.firm(cm, bm)).sum())
        print(f"V {V} H {H} R {R} setting {(temp, k, p)}: {near} of {cm.size} draws within the margin, kept mean {n.mean():.1f} of {V}")
        assert n.max() <= (k if k else V) and n.min() >= 1
        assert tok.min() >= 0 and tok.max() < V
        out.append((near, cm.size))
    return tuple(sum(x) for x in zip(*out))                  # a case: (V, R) under the three settings


@pytest.mark.parametrize("R", AR.ROWS)
@pytest.mark.parametrize("V", AR.FULL_V)
def test_margin_counts_of_the_token_pass_cases(V, R):
    """Per case of test_gpu_arnn_trunc.test_the_rule_on_the_calls_own_logits -- (V, R) under the three settings, 90 R draws -- at most
    half its cap of 5 %."""
    near, draws = margin_count(V, R, **AR.FULL)
    assert draws == 3 * R * AR.L and near <= 0.5 * AR.NEAR_CAP * draws, (V, R, near, draws)


@pytest.mark.parametrize("R", AR.ROWS)
def test_margin_counts_of_the_per_tick_cases(R):
    c = dict(AR.SMALL)
    V = c.pop("V")
    near, draws = margin_count(V, R, **c)
    assert draws == 3 * R * AR.L and near <= 0.5 * AR.NEAR_CAP * draws, (R, near, draws)


def test_the_settings_truncate_on_these_networks():
    """(6, 0, 0.9) and (6, 8, 0.7) keep fewer tokens than top-k alone would; (1, 5, 1) keeps exactly five"""
    W = AR.net(48, **AR.FULL)
    kept = []
    for si, (temp, k, p) in enumerate(AR.SETTINGS):
        oc, hc, u = AR.case(48, 5, si, **AR.FULL)
        kept.append(AR.truncated_trajectory(W, oc, hc, temp, u, k, p)[2])
    assert (kept[0] == 5).all() and kept[1].max() < 48 and kept[2].max() <= 8 and kept[2].min() < 8


def test_the_teacher_forced_trajectory_is_the_free_running_one():
    """Fed its own tokens, the oracle's trajectory returns its own logits bit for bit (what the GPU test feeds it are the GPU's tokens)."""
    c = dict(AR.SMALL)
    V = c.pop("V")
    W = AR.net(V, **c)
    oc, hc, u = AR.case(V, 5, 1, **c)
    w, tok, _, _, _ = AR.truncated_trajectory(W, oc, hc, 6.0, u, 0, 0.9)
    w2, tok2 = AR.trajectory(W, oc, hc, tokens=tok)
    assert np.array_equal(w, w2) and np.array_equal(tok, tok2)
    w3, _ = AR.trajectory(W, oc, hc, tokens=(tok + 1) % V)
    assert np.abs(w3 - w).max() > 1e-3 * np.abs(w).max()        # ... and other tokens move them


def test_argument_errors_come_before_any_library_call(monkeypatch):
    from inpaintnet_amd.arnn import ConstraintModelGaussianReg
    from inpaintnet_amd.arnn_tester import AnticipationRNNTester
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("a library call in front of the argument check"))
    nan, inf = float("nan"), float("inf")
    none = [None] * 14
    for bad in (0.0, -0.5, 1.0000001, 1.5, nan, inf):
        with pytest.raises(ValueError):
            ops.arnn_sample(*none, 1.0, None, top_p=bad)
        with pytest.raises(ValueError):
            ConstraintModelGaussianReg.generate(types.SimpleNamespace(), None, None, None, top_p=bad)
    for bad in (2.5, nan, inf, True):
        with pytest.raises(ValueError):
            ops.arnn_sample(*none, 1.0, None, top_k=bad)
        with pytest.raises(ValueError):
            ConstraintModelGaussianReg.generate(types.SimpleNamespace(), None, None, None, top_k=bad)
    me = types.SimpleNamespace()
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError):
            AnticipationRNNTester.generation(me, None, 4, 2, num_variations=bad)
        with pytest.raises(ValueError):
            AnticipationRNNTester._generate_window(me, None, None, 4, 2, num_variations=bad)


def test_the_restated_generate_is_the_rule_with_truncation_off(monkeypatch):
    """One fixture row of the reference's generate (tests/golden/arnn_generate.npz): at every one of its 384 steps the token the
    restated generate() takes by searchsorted is decoder_trunc_ref.pick's with truncation off, on the step's own logits."""
    fx = G.load("arnn_generate")
    P = G.arnn_params("small")
    score = torch.from_numpy(fx["small/score"].astype(np.int64))
    md = torch.from_numpy(fx["small/metadata"].astype(np.int64))
    loc = torch.from_numpy(fx["small/constraints_loc"].astype(np.int64))
    key, temp = "small/t1/0", float(fx["temperatures"][1])
    u = fx[key + "/uniforms"]
    seen, head = [], O._arnn_head

    def recording_head(P_, h):
        w = head(P_, h)
        seen.append(w[0].numpy().copy())
        return w
    monkeypatch.setattr(O, "_arnn_head", recording_head)
    with torch.no_grad():
        toks = GH._restated_generate(P, score[0], md[0], loc[0], temp, u)
    assert len(seen) == GH.L and np.array_equal(toks, fx[key + "/tokens"].astype(np.int64))
    V = seen[0].size
    for t in range(GH.L):
        tok, lp, n, cm, bm = TR.pick(seen[t], temp, u[t], 0, 1.0)
        assert n == V and bm == np.inf and cm >= TR.MARGIN, t            # (the fixture's uniforms keep 2e-5 from every step)
        assert tok == toks[t], t
        p = np.exp(np.float64(temp) * seen[t].astype(np.float64))
        assert abs(float(lp) - np.log(p[tok] / p.sum())) < 1e-5 * max(1.0, abs(float(lp))), t


def test_header_and_binding_agree_on_the_new_entry():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "inpaintnet_hip.h")).read()
    protos = {}
    for name in ("inet_arnn_sample", "inet_arnn_sample_ex"):
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", hdr)
        assert m, name
        protos[name] = [" ".join(a.split()) for a in m.group(1).split(",")]
    old, new = protos["inet_arnn_sample"], protos["inet_arnn_sample_ex"]
    assert new[:len(old) - 1] == old[:-1] and old[-1] == "void* stream"
    assert new[len(old) - 1:] == ["int top_k", "double top_p", "float* logp", "float* logits", "void* stream"]
    res, args = _lib._SIGNATURES["inet_arnn_sample_ex"]
    res0, args0 = _lib._SIGNATURES["inet_arnn_sample"]
    assert res is C.c_int and args[:len(args0) - 1] == args0[:-1]
    assert args[len(args0) - 1:] == [C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]
    assert "inet_arnn_sample_ex" in _lib.EXPORTS


def test_the_entry_refuses_what_inet_arnn_sample_refuses_and_a_bad_top_p():
    _lib.build(verbose=False)
    Lb = _lib.lib()
    big = 1 << 40
    net = [X] * 12

    def ex(R=1, Ln=4, emb=X, oc=X, u=X, tokens=X, ws=X, nws=big, temp=1.0, k=0, p=1.0, H=256):
        return Lb.inet_arnn_sample_ex(R, Ln, 10, 256, H, 256, 48, emb, oc, 256, 256 * Ln, *net, temp, u, NULL, tokens, ws, nws, k, p, NULL,
                                      NULL, NULL)
    nan, inf = float("nan"), float("inf")
    calls = {"R": ex(R=0), "L": ex(Ln=0), "emb": ex(emb=NULL), "oc": ex(oc=NULL), "uniforms": ex(u=NULL), "tokens": ex(tokens=NULL),
             "ws": ex(ws=NULL), "ws_floats": ex(nws=16), "temperature inf": ex(temp=inf), "temperature nan": ex(temp=nan), "H": ex(H=250),
             "top_p 0": ex(p=0.0), "top_p < 0": ex(p=-0.5), "top_p > 1": ex(p=1.0000001), "top_p nan": ex(p=nan), "top_p inf": ex(p=inf)}
    assert {k: v for k, v in calls.items() if v != -1} == {}
