"""What is AnticipationRNN-specific about its constrained sampling (inet_arnn_sample_cx): the float64 trajectory of the generation
network (tests/arnn_trunc_ref.py) choosing its own tokens by the constrained rule.  The rule itself is model-independent:
tests/decoder_constraint_ref.py (pick_rows, kept_rows, free, plan_mask, words); the network, the cases and the settings are
tests/arnn_trunc_ref.py's (net, case, trajectory, SETTINGS, FULL, SMALL, L = 30)."""
import numpy as np

from tests import arnn_trunc_ref as AR
from tests import decoder_constraint_ref as CR


def constrained_trajectory(W, oc, hc, temperature, u, top_k, top_p, allow):
    """The oracle choosing its own tokens by the constrained rule; allow bool [R,L,V] -> (logits [R,L,V], tokens, kept counts, CDF
    margins, nucleus margins), [R,L] each"""
    R, length = u.shape
    n, cm, bm = np.empty((R, length), dtype=np.int64), np.empty((R, length)), np.empty((R, length))

    def choose(t, w):
        tok, _, n[:, t], cm[:, t], bm[:, t], _ = CR.pick_rows(w, temperature, u[:, t], top_k, top_p, allow[:, t])
        return tok
    w, tok = AR.trajectory(W, oc, hc, choose=choose)
    return w, tok, n, cm, bm
