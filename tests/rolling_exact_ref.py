"""The rolling z-score in exact rational arithmetic - TEST INFRASTRUCTURE ONLY.

Per channel: prefix sums of the valid values v, of v^2 and of the valid count, kept exactly.  Every float64 is a rational
with a power-of-two denominator, so the channel's values are brought to one common denominator once and the prefix sums
are plain Python integers (the same numbers as ``fractions.Fraction`` prefix sums, without a gcd per addition).  For a
window holding v_1..v_n:

    n q = n sum(v^2) - sum(v)^2        n d = n x_t - sum(v)        z^2 = (n d)^2 (n - 1) / (n (n q))

z^2 is an exact ``Fraction``; ``float()`` rounds it correctly, one square root follows, the sign is that of n d: the result
is within an ulp and a half of the true z.  NaN where x_t is NaN, where n < 2, or where n q = 0 (all values equal: pandas'
rule).  O(T) per channel."""
import math
from fractions import Fraction

import numpy as np


def exact_rolling_zscore(x: np.ndarray, window: int, preserve_nans: bool = True) -> np.ndarray:
    x = np.asarray(x)
    assert x.ndim == 2 and x.dtype in (np.float32, np.float64)
    x = x.astype(np.float64)                                    # exact for float32
    C, T = x.shape
    W = min(int(window), T)
    out = np.full((C, T), np.nan)
    for c in range(C):
        row = x[c].tolist()
        valid = [v == v for v in row]
        ratios = [v.as_integer_ratio() if ok else (0, 1) for v, ok in zip(row, valid)]
        den = max(d for _, d in ratios)                         # powers of two: the largest is the common denominator
        ints = [p * (den // d) for p, d in ratios]
        p1, p2, pn = [0] * (T + 1), [0] * (T + 1), [0] * (T + 1)
        for t in range(T):
            v = ints[t]
            p1[t + 1] = p1[t] + v
            p2[t + 1] = p2[t] + v * v
            pn[t + 1] = pn[t] + (1 if valid[t] else 0)
        o = out[c]
        for t in range(T):
            if not valid[t]:
                continue
            a = max(0, t - W + 1)
            n = pn[t + 1] - pn[a]
            if n < 2:
                continue
            s1 = p1[t + 1] - p1[a]
            nq = n * (p2[t + 1] - p2[a]) - s1 * s1              # scaled by den^2, like (n d)^2
            if nq == 0:
                continue
            nd = n * ints[t] - s1
            z = math.sqrt(float(Fraction(nd * nd * (n - 1), n * nq)))
            o[t] = -z if nd < 0 else z
    if not preserve_nans:
        out[np.isnan(out)] = 0.0
    return out
