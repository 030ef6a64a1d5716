"""GPU: AnticipationRNN's temperature-sampled generation (ConstraintModelGaussianReg.generate, ops.arnn_sample: the sampling build
of the token pass and head_b1_kernel<NI, 1> of the per-tick launches, both in csrc/arnn_gen.hip) and AnticipationRNNTester, against
tests/golden/arnn_generate.npz (the reference's generate under np.random.seed, its tester on the arnn_inpaint_small model).
Every comparison of tokens is exact over all L ticks: the fixture's uniforms sit at least 2e-5 from every CDF step."""
import types

import numpy as np
import pytest
import torch

from tests import golden_util as G

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from inpaintnet_amd import ops, synthetic
    from inpaintnet_amd.arnn import AnticipationRNNBaseline, ConstraintModelGaussianReg
    from inpaintnet_amd.arnn_tester import AnticipationRNNTester

L = 384


class _Dataset(object):
    """What generate and the tester read: the reference's test dataset (oracle/gen_golden.py FakeDataset) -- start symbol 0."""

    def __init__(self, V):
        ds = synthetic.SyntheticFolkDataset(num_notes=V)
        self.__dict__.update(ds.__dict__)
        self.metadatas = [types.SimpleNamespace(num_values=6), types.SimpleNamespace(num_values=6)]

    def empty_score_tensor(self, length):
        return torch.zeros(self.num_voices, length, dtype=torch.long)

    def __repr__(self):
        return "Fake"


def _model(name, cls=None):
    c = G.ARNN_CFGS[name]
    ds = _Dataset(c["V"])
    model = (cls or ConstraintModelGaussianReg)(ds, note_embedding_dim=c["E"], metadata_embedding_dim=c["Em"],
                                                num_lstm_constraints_units=c["H"], num_lstm_generation_units=c["H"],
                                                linear_hidden_size=c["LH"], num_layers=2, dropout_input_prob=0.0,
                                                dropout_prob=0.0, unary_constraint=True, teacher_forcing=True)
    model.load_state_dict(G.arnn_params(name))
    return ds, model


def _inputs(fx, name):
    s = torch.from_numpy(fx[f"{name}/score"].astype(np.int64)).cuda()
    m = torch.from_numpy(fx[f"{name}/metadata"].astype(np.int64)).cuda()
    c = torch.from_numpy(fx[f"{name}/constraints_loc"].astype(np.int64)).cuda()
    return s, m, c


def _first_diff(a, b):
    d = np.nonzero(np.asarray(a) != np.asarray(b))[0]
    return int(d[0]) if d.size else None


@pytest.mark.parametrize("name", ["small", "full"])
def test_generate_reproduces_the_reference_tokens_under_np_random_seed(name):
    fx = G.load("arnn_generate")
    _, model = _model(name)
    s, m, c = _inputs(fx, name)
    for ti, temp in enumerate(fx["temperatures"]):
        for i in range(s.shape[0]):
            key = f"{name}/t{ti}/{i}"
            seed = int(fx[key + "/seed"])
            mi = m[i]
            np.random.seed(seed)
            score, gen, md = model.generate(s[i], mi, c[i], temperature=float(temp))
            nxt = np.random.random_sample()
            assert score is None and md is mi and not model.training
            assert gen.shape == (1, L) and gen.dtype == torch.int64 and gen.is_cuda
            ref = fx[key + "/tokens"].astype(np.int64)
            got = gen[0].cpu().numpy()
            assert _first_diff(got, ref) is None, (key, _first_diff(got, ref))
            assert nxt == np.random.RandomState(seed).random_sample(L + 1)[L]      # exactly L draws taken, as by the reference
    assert ops.chain_status() == 0


def test_generate_is_the_same_under_every_token_pass_mode():
    fx = G.load("arnn_generate")
    _, model = _model("full")
    s, m, c = _inputs(fx, "full")
    key = "full/t1/0"
    ref = fx[key + "/tokens"].astype(np.int64)
    try:
        for mode in (0, 1, 2, 3, 4):
            ops.set_option(14, mode)
            np.random.seed(int(fx[key + "/seed"]))
            _, gen, _ = model.generate(s[0], m[0], c[0], temperature=float(fx["temperatures"][1]))
            assert ops.chain_status() == 0, mode
            assert _first_diff(gen[0].cpu().numpy(), ref) is None, (mode, _first_diff(gen[0].cpu().numpy(), ref))
    finally:
        ops.set_option(14, 3)


def _batch(V, B, seed):
    s = torch.from_numpy(synthetic.folk_score(B, V, seed=seed)).long().cuda()
    md = torch.from_numpy(synthetic.folk_metadata(B)).long()
    md[..., 0] = torch.from_numpy(synthetic.det_tokens("test_gpu_arnn_generate/md0", (B, 1, L), 6))
    g = torch.Generator().manual_seed(seed)
    loc = torch.zeros(B, 1, L, dtype=torch.int64)
    for b in range(B):
        a = int(torch.randint(0, 12, (1,), generator=g)) * 24
        loc[b, :, :a] = 1
        loc[b, :, a + 96:] = 1
    return s, md.cuda(), loc.cuda()


@pytest.mark.parametrize("name,B", [("full", 5), ("full", 11), ("small", 5)])
def test_batched_generate_equals_the_single_row_calls(name, B, monkeypatch):
    """B = 5: one launch of 5 teams; B = 11: 8 teams, then 3 (persistent kernel); small: the per-tick launches, row after row."""
    _, model = _model(name)
    s, md, loc = _batch(G.ARNN_CFGS[name]["V"], B, seed=B)
    np.random.seed(77)
    _, gen, _ = model.generate(s, md, loc, temperature=1.5)
    assert gen.shape == (B, 1, L)
    u = np.random.RandomState(77).random_sample((B, L))
    rows = []
    for b in range(B):
        monkeypatch.setattr(np.random, "random_sample", lambda shape, _u=u[b:b + 1]: _u.copy())
        rows.append(model.generate(s[b], md[b], loc[b], temperature=1.5)[1])
    monkeypatch.undo()
    single = torch.cat(rows, 0).view(B, 1, L)
    assert torch.equal(gen, single)
    assert len({tuple(r[0].tolist()) for r in gen.cpu()}) == B                # (independent rows: all different)
    assert ops.chain_status() == 0


@pytest.mark.parametrize("name", ["small", "full"])
def test_generate_with_nan_weights_stays_inside_the_vocabulary(name):
    fx = G.load("arnn_generate")
    _, model = _model(name)
    V = G.ARNN_CFGS[name]["V"]
    s, m, c = _inputs(fx, name)
    model.param("linear_ouput_notes.0.weight")[:] = float("nan")
    np.random.seed(3)
    _, gen, _ = model.generate(s[0], m[0], c[0], temperature=1.5)
    assert int(gen.min()) == 0 and int(gen.max()) == 0                        # the argmax rule: the lowest NaN
    _, model = _model(name)
    model.param("lstm_generation.1.weight_hh_l0")[5, 7] = float("nan")       # NaN from the second tick on
    _, gen, _ = model.generate(s[1], m[1], c[1], temperature=1.0)
    assert 0 <= int(gen.min()) and int(gen.max()) < V
    assert ops.chain_status() == 0


def test_tester_loss_accuracy_and_generation():
    fx = G.load("arnn_generate")
    ds, model = _model("small", AnticipationRNNBaseline)
    tester = AnticipationRNNTester(ds, model)
    w = [torch.from_numpy(fx["tester/w"]).cuda()]
    t = torch.from_numpy(fx["tester/t"]).cuda()
    ce, acc = fx["tester/ce_acc"]
    np.testing.assert_allclose(float(AnticipationRNNTester.mean_crossentropy_loss(w, t)), ce, rtol=1e-5)
    np.testing.assert_allclose(float(AnticipationRNNTester.mean_accuracy(w, t)), acc, rtol=1e-5)
    batches = [(torch.from_numpy(fx[f"tester/batch{k}_score"].astype(np.int64)),
                torch.from_numpy(fx[f"tester/batch{k}_metadata"].astype(np.int64))) for k in range(2)]
    lo, ac = tester.loss_and_acc_test(batches)
    np.testing.assert_allclose([lo, ac], fx["tester/loss_acc"], rtol=1e-5)
    # generation: past | generated | future, the generated window = generate()'s tokens for the same seed
    score, md = batches[0][0][:1, 0].cuda(), batches[0][1][:1, 0].cuda()
    np.random.seed(11)
    gen_score, gen_tensor, orig_score = tester.generation(score, start_measure=4, num_measures_gen=3, tensor_metadata=md)
    assert gen_score is None and orig_score is None and gen_tensor.shape == (1, L)
    a, b = 3 * 24, 6 * 24
    assert torch.equal(gen_tensor[:, :a], score[:, :a]) and torch.equal(gen_tensor[:, b:], score[:, b:])
    loc = torch.ones_like(score)
    loc[:, a:b] = 0
    np.random.seed(11)
    _, gen, _ = model.generate(score, md, loc, temperature=1.5)
    assert torch.equal(gen_tensor[:, a:b], gen[:, a:b])
    with pytest.raises(ValueError):
        tester.generation(score, start_measure=4, num_measures_gen=3)      # no metadata and no music21 conversion
    assert ops.chain_status() == 0


def test_arnn_sample_rejects_bad_arguments():
    _, model = _model("full")
    pr = model.param
    args = [pr(k) for k in ("note_embeddings.0.weight", "lstm_generation.0.weight_ih_l0", "lstm_generation.0.bias_ih_l0",
                            "lstm_generation.0.weight_hh_l0", "lstm_generation.0.bias_hh_l0", "lstm_generation.1.weight_ih_l0",
                            "lstm_generation.1.bias_ih_l0", "lstm_generation.1.weight_hh_l0", "lstm_generation.1.bias_hh_l0",
                            "linear_1.weight", "linear_1.bias", "linear_ouput_notes.0.weight", "linear_ouput_notes.0.bias")]
    oc = torch.zeros(2, 30, 256, device="cuda")
    u = np.full((2, 30), 0.5)
    t = ops.arnn_sample(args[0], oc, *args[1:], 1.0, u)
    assert t.shape == (2, 30) and int(t.min()) >= 0 and int(t.max()) < 48
    with pytest.raises(ValueError):
        ops.arnn_sample(args[0], oc, *args[1:], float("inf"), u)
    with pytest.raises(ValueError):
        ops.arnn_sample(args[0], oc, *args[1:], 1.0, u[:1])
    with pytest.raises(ValueError):
        model.generate(torch.zeros(1, 20, dtype=torch.int64, device="cuda"), torch.zeros(1, 20, 3, dtype=torch.int64, device="cuda"),
                       torch.zeros(1, 20, dtype=torch.int64, device="cuda"))      # L < 24: the warm-up reads oc[23]
