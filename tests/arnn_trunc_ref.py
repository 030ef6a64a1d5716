"""What is AnticipationRNN-specific about its truncated sampling (inet_arnn_sample_ex): the float64 trajectory of the generation network
-- [embedding of the previous token | constraint output of the tick] -> LSTM 0 -> LSTM 1 -> ReLU(linear_1) -> note head, the cells from
oracle.torch_ref -- teacher-forced over given tokens or choosing its own tick by tick, and the inputs of the GPU test's cases.  The
rule itself is model-independent: tests/decoder_trunc_ref.py (pick_rows, kept_rows, firm, logp_tol)."""
import numpy as np
import torch

from inpaintnet_amd import synthetic
from oracle import torch_ref as O
from tests import decoder_trunc_ref as TR

SETTINGS = TR.SETTINGS                                       # (temperature, top_k, top_p): (1, 5, 1), (6, 0, 0.9), (6, 8, 0.7)
L = 30
FULL = dict(E=10, Hc=256, H=256, U=256)                      # the persistent token pass's configuration (V <= 128)
SMALL = dict(E=4, Hc=16, H=16, U=16, V=12)                   # the per-tick launches
FULL_V = (48, 64, 65, 128)                                   # one logit chunk per lane, its edge, the first and the full two-chunk shape
ROWS = (1, 5, 11)                                            # one team, five, and 8 teams then 3
NEAR_CAP = 0.05                                              # draws within a margin, of a case's draws -- (V, R), its three settings

KEYS = ("note_embeddings.0.weight", "lstm_generation.0.weight_ih_l0", "lstm_generation.0.bias_ih_l0", "lstm_generation.0.weight_hh_l0",
        "lstm_generation.0.bias_hh_l0", "lstm_generation.1.weight_ih_l0", "lstm_generation.1.bias_ih_l0",
        "lstm_generation.1.weight_hh_l0", "lstm_generation.1.bias_hh_l0", "linear_1.weight", "linear_1.bias",
        "linear_ouput_notes.0.weight", "linear_ouput_notes.0.bias")


def net(V, E, Hc, H, U):
    """The generation network's weights in ops.arnn_sample's order (KEYS), float32 numpy, synthetic.det_param values"""
    shapes = ((V + 1, E), (4 * H, E + Hc), (4 * H,), (4 * H, H), (4 * H,), (4 * H, H), (4 * H,), (4 * H, H), (4 * H,), (U, H), (U,),
              (V, U), (V,))
    return [synthetic.det_param(f"arnn_trunc/{V}/{H}/{k}", s) for k, s in zip(KEYS, shapes)]


def case(V, R, si, E, Hc, H, U, length=L):
    """-> (oc [R,L,Hc] f32, hc_init [R,2,2,H] f32, u [R,L] f64) of the case (V, R) under SETTINGS[si]"""
    oc = synthetic.det_normal(f"arnn_trunc/oc/{V}/{H}/{R}", (R, length, Hc), 0.5)
    hc = synthetic.det_normal(f"arnn_trunc/hc/{V}/{H}/{R}", (R, 2, 2, H), 0.3)
    u = synthetic.det_uniform(f"arnn_trunc/u/{V}/{H}/{R}/{si}", (R, length), 0.0, 1.0).astype(np.float64)
    return oc, hc, u


def trajectory(W, oc, hc, tokens=None, choose=None):
    """The float64 generation network over R rows: tick 0 feeds token 0, tick t the token of t - 1 -- tokens[:, t - 1] (teacher-forced
    over given tokens [R,L]) or choose(t, logits [R,V] as f32 numpy) -> tokens [R].  -> (logits [R,L,V] float64 numpy, tokens [R,L])"""
    emb, wi0, bi0, wh0, bh0, wi1, bi1, wh1, bh1, w1, b1, w2, b2 = (torch.from_numpy(np.asarray(w)).double() for w in W)
    oc, hc = torch.from_numpy(np.asarray(oc)).double(), torch.from_numpy(np.asarray(hc)).double()
    R, length, _ = oc.shape
    h0, c0, h1, c1 = hc[:, 0, 0], hc[:, 0, 1], hc[:, 1, 0], hc[:, 1, 1]
    prev = np.zeros(R, dtype=np.int64)
    ws, toks = [], []
    with torch.no_grad():
        for t in range(length):
            x = torch.cat((emb[torch.from_numpy(prev)], oc[:, t]), 1)
            h0, c0 = O.lstm_cell(x @ wi0.t() + bi0, h0, c0, wh0, bh0)
            h1, c1 = O.lstm_cell(h0 @ wi1.t() + bi1, h1, c1, wh1, bh1)
            w_t = torch.relu(h1 @ w1.t() + b1) @ w2.t() + b2
            prev = np.asarray(tokens[:, t] if tokens is not None else choose(t, w_t.numpy().astype(np.float32)), dtype=np.int64)
            ws.append(w_t)
            toks.append(prev)
    return torch.stack(ws, 1).numpy(), np.stack(toks, 1)


def truncated_trajectory(W, oc, hc, temperature, u, top_k, top_p):
    """The oracle choosing its own tokens by the truncated rule -> (logits [R,L,V], tokens, kept counts, CDF margins, nucleus margins)"""
    R, length = u.shape
    n, cm, bm = np.empty((R, length), dtype=np.int64), np.empty((R, length)), np.empty((R, length))

    def choose(t, w):
        tok, _, n[:, t], cm[:, t], bm[:, t], _ = TR.pick_rows(w, temperature, u[:, t], top_k, top_p)
        return tok
    w, tok = trajectory(W, oc, hc, choose=choose)
    return w, tok, n, cm, bm
