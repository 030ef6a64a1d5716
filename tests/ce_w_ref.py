"""Float64 restatement of the class-weighted, label-smoothed cross-entropy with an ignore index, which is
torch.nn.functional.cross_entropy(x, t, weight=w, label_smoothing=e, ignore_index=i, reduction='mean'):

  valid_r = t_r != i (and 0 <= t_r < V: a target outside the vocabulary is treated as ignored and counted in n_bad)
  p = softmax(x_r);  W = sum_c w_c;  denom = sum_valid w[t_r]
  loss = [(1 - e) sum_valid w[t_r] (lse_r - x_r[t_r]) + (e / V) sum_valid sum_c w_c (lse_r - x_r[c])] / denom
  dloss / dx_r[c] = valid_r [(1 - e) w[t_r] (p_c - 1{c = t_r}) + (e / V) (W p_c - w_c)] / denom

tests/test_ce_w_host.py holds it equal to torch in float64, value and autograd gradient.  With denom == 0 the loss is NaN (as torch's)
and the gradient ALL ZEROS (the project's rule; torch gives zeros when every row is ignored and NaN when every present target has
weight 0).  The integer side -- counts, per-class statistics, the confusion matrix -- follows argmax_first of tests/pointwise_ref.py
(np.argmax: a NaN is the maximum, the lowest index wins among equals) over the valid rows."""
import numpy as np


def _valid(t, V, ignore_index):
    t = np.asarray(t, dtype=np.int64)
    inside = (t >= 0) & (t < V)
    ignored = np.zeros(t.shape, bool) if ignore_index is None else t == ignore_index
    return inside & ~ignored, ~inside & ~ignored


def counts(t, V, weight=None, ignore_index=None):
    """-> dict(counts (V,) int64, n_valid, n_bad, denom = sum_c w_c counts_c added in class order)."""
    t = np.asarray(t, dtype=np.int64).reshape(-1)
    valid, bad = _valid(t, V, ignore_index)
    c = np.bincount(t[valid], minlength=V).astype(np.int64)
    w = np.ones(V) if weight is None else np.asarray(weight, dtype=np.float64)
    denom = 0.0
    for k in range(V):
        denom += w[k] * float(c[k])
    return dict(counts=c, n_valid=int(valid.sum()), n_bad=int(bad.sum()), denom=denom)


def evaluate(x, t, weight=None, label_smoothing=0.0, ignore_index=None):
    """x [rows, V] (any float dtype), t [rows] -> dict(loss, grad [rows, V], denom, n_valid, n_bad, counts, accuracy, stats (V, 3)
    int64 = {target count, hits, predicted}, confusion (V, V) int64 indexed [target, argmax]), floats in float64."""
    x = np.asarray(x, dtype=np.float64)
    t = np.asarray(t, dtype=np.int64).reshape(-1)
    rows, V = x.shape
    e = float(label_smoothing)
    w = np.ones(V) if weight is None else np.asarray(weight, dtype=np.float64)
    cnt = counts(t, V, weight, ignore_index)
    valid, _ = _valid(t, V, ignore_index)
    ts = np.where(valid, t, 0)
    m = x.max(axis=1, keepdims=True)
    ex = np.exp(x - m)
    se = ex.sum(axis=1, keepdims=True)
    lse = (m + np.log(se))[:, 0]
    p = ex / se
    wt = w[ts]
    nll = wt * (lse - x[np.arange(rows), ts])
    smooth = (w[None, :] * (lse[:, None] - x)).sum(axis=1)
    denom = float(wt[valid].sum())
    onehot = np.zeros((rows, V))
    onehot[np.arange(rows), ts] = 1.0
    if denom == 0.0:
        loss, grad = float("nan"), np.zeros((rows, V))
    else:
        loss = ((1.0 - e) * nll[valid].sum() + (e / V) * smooth[valid].sum()) / denom
        grad = ((1.0 - e) * wt[:, None] * (p - onehot) + (e / V) * (w.sum() * p - w[None, :])) / denom
        grad[~valid] = 0.0
    am = np.argmax(x, axis=1)                   # argmax_first
    stats = np.zeros((V, 3), np.int64)
    conf = np.zeros((V, V), np.int64)
    for r in np.nonzero(valid)[0]:
        stats[t[r], 0] += 1
        stats[t[r], 1] += am[r] == t[r]
        stats[am[r], 2] += 1
        conf[t[r], am[r]] += 1
    n_valid = int(valid.sum())
    return dict(loss=loss, grad=grad, denom=denom, n_valid=n_valid, n_bad=cnt["n_bad"], counts=cnt["counts"],
                accuracy=float(stats[:, 1].sum()) / n_valid if n_valid else float("nan"), stats=stats, confusion=conf)


def report(stats, confusion):
    """The testers' per-class report from the integers, restated: recall, precision, f1 (NaN where undefined), accuracy, balanced
    accuracy = the mean recall over the classes present."""
    stats = np.asarray(stats, dtype=np.int64)
    c, h, p = (stats[:, k].astype(np.float64) for k in range(3))
    with np.errstate(divide="ignore", invalid="ignore"):
        recall, precision, f1 = h / c, h / p, 2.0 * h / (c + p)
    for a, d in ((recall, c), (precision, p), (f1, c + p)):
        a[d == 0] = np.nan
    return dict(counts=stats[:, 0], hits=stats[:, 1], predicted=stats[:, 2], recall=recall, precision=precision, f1=f1,
                accuracy=h.sum() / c.sum() if c.sum() else float("nan"),
                balanced_accuracy=float(np.mean(recall[c > 0])) if (c > 0).any() else float("nan"),
                confusion=np.asarray(confusion, dtype=np.int64))


def class_weights(n, scheme="inverse", beta=0.999, normalize=True):
    """Trainer.class_weights restated in float64."""
    n = np.asarray(n, dtype=np.float64)
    present = n > 0
    safe = np.where(present, n, 1.0)
    w = {"inverse": lambda: 1.0 / safe, "inverse_sqrt": lambda: 1.0 / np.sqrt(safe),
         "effective": lambda: (1.0 - beta) / (1.0 - beta ** safe)}[scheme]()
    w = np.where(present, w, w[present].max())
    return w * (n.sum() / (w * n).sum()) if normalize else w
