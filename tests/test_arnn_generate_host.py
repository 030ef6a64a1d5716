"""Host-side checks of AnticipationRNN's temperature-sampled generation and of its tester (no GPU).

tests/golden/arnn_generate.npz holds calls of the reference's ConstraintModelGaussianReg.generate
(AnticipationRNN/anticipation_rnn_gauss_reg_model.py:570-679) under np.random.seed(seed): the L uniforms np.random.choice drew and
the tokens.  A CPU restatement -- 23 warm-up ticks on the start symbol with oc[1..23], then L ticks with oc[t], token t = the first v
whose prefix of softmax(temperature * logits) exceeds u_t -- reproduces every stored sequence: this pins the reading of the reference
that the GPU kernels (csrc/arnn_gen.hip, csrc/sample.h) implement."""
import types

import numpy as np
import pytest
import torch

from oracle import torch_ref as O
from tests import golden_util as G

L = 384
WARM = 23


def _fx():
    return G.load("arnn_generate")


def _restated_generate(P, score, md, loc, temperature, u):
    """score (1,L), md (1,L,M), loc (1,L) of one row; u [L] float64 -> tokens [L]"""
    _, m = O.arnn_embed(P, score[None], md[None], loc[None])
    Hc = P["lstm_constraint.0.weight_hh_l0"].shape[1]
    z = torch.zeros(1, Hc)
    oc = m
    for l in range(2):
        oc, _ = O.lstm_layer(oc, z, z, P, f"lstm_constraint.{l}", reverse=True)
    oc = oc[0]                                                               # [L, Hc]
    E = P["note_embeddings.0.weight"]
    H = P["lstm_generation.0.weight_hh_l0"].shape[1]
    h = [torch.zeros(1, H) for _ in range(2)]
    c = [torch.zeros(1, H) for _ in range(2)]

    def tick(tok, o):
        inp = torch.cat((E[tok].view(1, -1), o.view(1, -1)), 1)
        for l in range(2):
            pf = f"lstm_generation.{l}"
            gi = inp @ P[f"{pf}.weight_ih_l0"].t() + P[f"{pf}.bias_ih_l0"]
            h[l], c[l] = O.lstm_cell(gi, h[l], c[l], P[f"{pf}.weight_hh_l0"], P[f"{pf}.bias_hh_l0"])
            inp = h[l]
        return inp

    for t in range(WARM):                                                    # the start symbol of an empty score: token 0
        tick(0, oc[t + 1])
    toks, prev = [], 0
    for t in range(L):
        w = O._arnn_head(P, tick(prev, oc[t]))[0] * temperature
        p = torch.softmax(w, 0).double().numpy()
        cdf = np.cumsum(p)
        cdf /= cdf[-1]
        prev = int(np.searchsorted(cdf, u[t], side="right"))
        toks.append(prev)
    return np.array(toks)


@pytest.mark.parametrize("name", ["small", "full"])
def test_restated_generate_reproduces_the_reference_tokens(name):
    fx = _fx()
    P = G.arnn_params(name)                                                  # (regenerated: the fixture stores keys and shapes)
    score = torch.from_numpy(fx[f"{name}/score"].astype(np.int64))
    md = torch.from_numpy(fx[f"{name}/metadata"].astype(np.int64))
    loc = torch.from_numpy(fx[f"{name}/constraints_loc"].astype(np.int64))
    assert list(fx[f"{name}/param_keys"]) == list(P)
    for k, shp in zip(fx[f"{name}/param_keys"], fx[f"{name}/param_shapes"]):
        assert tuple(int(d) for d in str(shp).split(",")) == tuple(P[str(k)].shape), k
    with torch.no_grad():
        for ti, temp in enumerate(fx["temperatures"]):
            for i in range(score.shape[0]):
                key = f"{name}/t{ti}/{i}"
                seed = int(fx[key + "/seed"])
                u = fx[key + "/uniforms"]
                assert np.array_equal(u, np.random.RandomState(seed).random_sample(L))
                assert float(fx[key + "/margin"].min()) >= float(fx["min_margin"])
                got = _restated_generate(P, score[i], md[i], loc[i], float(temp), u)
                ref = fx[key + "/tokens"].astype(np.int64)
                assert np.array_equal(got, ref), (key, int(np.argmax(got != ref)))


def test_tester_constraints_location_matches_the_reference():
    from inpaintnet_amd.arnn_tester import AnticipationRNNTester
    fx = _fx()
    ds = types.SimpleNamespace(subdivision=6, num_beats_per_bar=4, n_bars=16)
    me = types.SimpleNamespace(dataset=ds)
    score = torch.zeros(3, 1, L, dtype=torch.int64)
    loc, a, b = AnticipationRNNTester.get_constraints_location(me, score, is_stochastic=False)
    assert np.array_equal(loc.numpy(), fx["tester/default_loc"]) and [a, b] == list(fx["tester/default_ticks"])
    loc, a, b = AnticipationRNNTester.get_constraints_location(me, score, is_stochastic=False, start_measure=3, num_measures=4)
    assert np.array_equal(loc.numpy(), fx["tester/given_loc"]) and [a, b] == list(fx["tester/given_ticks"])
    torch.manual_seed(int(fx["tester/stochastic_seed"]))
    for k, ticks in enumerate(fx["tester/stochastic_ticks"]):
        loc, a, b = AnticipationRNNTester.get_constraints_location(me, score, is_stochastic=True)
        assert [a, b] == list(ticks), k
        assert np.array_equal(loc.numpy(), fx[f"tester/stochastic_loc{k}"]), k
