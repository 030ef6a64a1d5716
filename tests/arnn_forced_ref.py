"""What is AnticipationRNN-specific about its forced tokens (inet_arnn_sample_fx): the float64 trajectory of the generation network
(tests/arnn_trunc_ref.py) taking the forced token where a tick has one and choosing its own by the constrained rule elsewhere.  The rule
itself is model-independent: tests/decoder_forced_ref.py (pick_rows, plan_forced, FORCED_SETTINGS); the masks are
tests/decoder_constraint_ref.py's (plan_mask); the network, the cases and their uniforms are tests/arnn_trunc_ref.py's (net, case,
trajectory, FULL, SMALL, L = 30).  arnn_trunc_ref.SETTINGS is NOT used with forced tokens: its first setting (top_k = 5 at temperature 1)
truncates away nearly every pattern token, and almost no finite forced logp would be compared."""
import numpy as np

from tests import arnn_trunc_ref as AR
from tests import decoder_forced_ref as FR


def forced_trajectory(W, oc, hc, temperature, u, top_k, top_p, allow, forced):
    """The oracle under the forced rule; allow bool [R,L,V] or None, forced int [R,L] or None -> (logits [R,L,V], tokens, logp f32, kept
    counts, CDF margins, nucleus margins, s_tok - m), [R,L] each"""
    R, length = u.shape
    lp = np.empty((R, length), dtype=np.float32)
    n, cm, bm, d = np.empty((R, length), dtype=np.int64), np.empty((R, length)), np.empty((R, length)), np.empty((R, length))

    def choose(t, w):
        tok, lp[:, t], n[:, t], cm[:, t], bm[:, t], d[:, t] = FR.pick_rows(w, temperature, u[:, t], top_k, top_p,
                                                                         None if allow is None else allow[:, t],
                                                                         None if forced is None else forced[:, t])
        return tok
    w, tok = AR.trajectory(W, oc, hc, choose=choose)
    return w, tok, lp, n, cm, bm, d
