"""CPU references of the channel-selection tests - TEST INFRASTRUCTURE (no reference-project code).

``scipy_loop`` is the yardstick: ``scipy.stats.f_oneway`` once per channel, the way the selectors of the original project
call it.  ``closed_form`` restates the same test in NumPy float64 from group sums taken after subtracting the column mean,
with ``scipy.special.fdtrc`` for p.  The distance between the two is the yardstick's own floor (summation order only: both
use the same p-value routine).  ``reference_selection`` is the selection logic on a p-value array."""
import warnings

import numpy as np
from scipy import special, stats


def _groups(x, labels):
    if labels is None:
        return [np.asarray(g, dtype=np.float64) for g in x]
    x = np.asarray(x, dtype=np.float64)
    return [x[labels == v] for v in np.unique(labels)]


def scipy_loop(x, labels=None):
    """(F, p), each (C, T): f_oneway per channel of groups (n_g, C, T)."""
    groups = _groups(x, labels)
    C, T = groups[0].shape[1:]
    F, p = np.empty((C, T)), np.empty((C, T))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for c in range(C):
            res = stats.f_oneway(*[g[:, c, :] for g in groups])
            F[c], p[c] = res.statistic, res.pvalue
    return F, p


def closed_form(x, labels=None):
    groups = _groups(x, labels)
    k, N = len(groups), sum(g.shape[0] for g in groups)
    mean = sum(g.sum(axis=0) for g in groups) / N
    ssb, ssw = 0.0, 0.0
    with np.errstate(all="ignore"):
        for g in groups:
            d = g - mean
            s = d.sum(axis=0)
            ssb = ssb + s * s / g.shape[0]
            ssw = ssw + (d * d).sum(axis=0) - s * s / g.shape[0]
        F = (ssb / (k - 1)) / (ssw / (N - k))
        return F, special.fdtrc(k - 1, N - k, F)


def rel_floor(a, b, mask):
    """max |a - b| / |b| over mask."""
    with np.errstate(all="ignore"):
        r = np.abs(a - b) / np.abs(b)
    r = np.where(a == b, 0.0, r)
    return float(np.max(r[mask])) if mask.any() else 0.0


def max_length(indices):
    """Longest run of consecutive integers, by counting (independent of the package's get_max_length)."""
    best = run = 1
    for a, b in zip(indices[:-1], indices[1:]):
        run = run + 1 if b == a + 1 else 1
        best = max(best, run)
    return best


def reference_selection(p, threshold, length_threshold):
    """(selected channels, longest run per channel (0 if none), points within 1e-9 relative of the threshold)."""
    selected, runs = [], []
    for c in range(p.shape[0]):
        below = np.where(p[c] < threshold)[0]
        run = max_length(below) if len(below) else 0
        runs.append(run)
        if len(below) and run > length_threshold:
            selected.append(c)
    near = int(np.sum(np.abs(p - threshold) <= 1e-9 * threshold))
    return selected, runs, near
