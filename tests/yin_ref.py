"""Host restatement of the YIN steps of ``tl_yin_f0`` / ``utils.audio.yin_f0`` as a plain loop over frames and lags, in
``np.float64`` or ``np.longdouble``, for tests/test_gpu_f0.py and tests/test_f0_host.py; the test clips; and the rule that
says on which frames the pick can be compared (every comparison it makes has a margin).
"""
import functools
from typing import NamedTuple

import numpy as np

U = 2.0 ** -53

# (sr, frame_length, win_length, hop, fmin, fmax, S)
GEOMETRIES = {
    "A": (8000, 256, 128, 64, 100, 1000, 700),            # one pass of lags; S no multiple of the hop
    "B": (8000, 512, 256, 128, 60, 500, 3001),            # 135 lags
    "C": (24414, 2048, 1024, 512, 30, 600, 6000),         # 815 lags: several passes of a 256-thread block, the largest default frame
    "D": (8000, 256, 96, 50, 100, 1000, 700),             # win_length != frame_length / 2, a hop that divides nothing, padding > W
}
THRESHOLD = 0.1
#: margin below which a comparison of the pick is left out (>= 2 eps_c for every geometry above)
MARGIN = 1e-11


def periods(sr, frame_length, win_length, fmin, fmax):
    return max(int(np.floor(sr / fmax)), 1), min(int(np.ceil(sr / fmin)), frame_length - win_length - 1)


def eps_c(win_length, pmax):
    """Relative error bound of a CMND value: d is a sum of W non-negative terms, each a rounded difference squared
    (gamma_{W+2}); the running sum adds up to pmax non-negative terms of that kind (gamma_{pmax}) and d itself carries its
    error again in the numerator; two divisions, the DBL_MIN add and slack make the rest."""
    return (2 * win_length + pmax + 8) * U


def clips(sr, S, seed=0):
    """Five clips (5, S) float64: level 220 Hz, rising 120 -> 260, falling 300 -> 140, dipping 180 - 60 sin(pi t / T) - each
    sum_h sin(h phi) / h, h = 1..5, plus 0.01 N(0, 1), behind a noise-only lead of S // 6 samples at 0.02, the rising clip
    ending in S // 8 exact zeros - and white noise."""
    rng = np.random.default_rng(seed)
    lead = S // 6
    n = S - lead
    t = np.arange(n) / max(n - 1, 1)
    contours = [np.full(n, 220.0), 120.0 + 140.0 * t, 300.0 - 160.0 * t, 180.0 - 60.0 * np.sin(np.pi * t)]
    out = np.empty((5, S))
    for k, f in enumerate(contours):
        phi = 2.0 * np.pi * np.cumsum(f) / sr
        tone = sum(np.sin(h * phi) / h for h in range(1, 6)) + 0.01 * rng.standard_normal(n)
        out[k, :lead] = 0.02 * rng.standard_normal(lead)
        out[k, lead:] = tone
    out[1, S - S // 8:] = 0.0
    out[4] = rng.standard_normal(S)
    return out


class Ref(NamedTuple):
    f0: np.ndarray
    aperiodicity: np.ndarray
    period_index: np.ndarray
    rms: np.ndarray
    cmnd: np.ndarray
    shift: np.ndarray
    a: np.ndarray
    decidable: np.ndarray


def frames_of(y, frame_length, hop, center, dtype):
    y = np.asarray(y).astype(dtype)
    S = y.shape[0]
    n_frames = 1 + S // hop if center else 1 + (S - frame_length) // hop
    if center:
        y = np.concatenate([np.zeros(frame_length // 2, dtype), y, np.zeros(frame_length // 2, dtype)])
    need = (n_frames - 1) * hop + frame_length
    if y.shape[0] < need:
        y = np.concatenate([y, np.zeros(need - y.shape[0], dtype)])
    return [y[f * hop:f * hop + frame_length] for f in range(n_frames)]


def _decided(x, y):
    """Is the comparison of x and y safe from rounding?  Two exact zeros are."""
    if x == 0 and y == 0:
        return True
    return abs(x - y) > MARGIN * max(1.0, abs(x), abs(y))


def pick(c, threshold):
    """(index, decidable) by steps 4 and 5."""
    nc = len(c)
    first = -1
    for i in range(nc - 1):
        trough = c[0] < c[1] if i == 0 else (c[i] < c[i - 1] and c[i] <= c[i + 1])
        if trough and c[i] < threshold:
            first = i
            break
    if first >= 0:
        i = first
        ok = all(_decided(c[k], threshold) for k in range(min(i + 2, nc)))
        ok = ok and all(_decided(c[k], c[k + 1]) for k in range(min(i + 2, nc - 1)))
        return i, ok
    i = int(np.argmin(c))
    order = np.sort(c)
    ok = _decided(order[0], order[1]) and all(_decided(v, threshold) for v in c)
    return i, ok


def yin_ref(y, sr, frame_length, win_length, hop, fmin, fmax, threshold=THRESHOLD, center=True, dtype=np.float64):
    W = win_length
    pmin, pmax = periods(sr, frame_length, W, fmin, fmax)
    nc = pmax - pmin + 1
    tiny = dtype(np.finfo(np.float64).tiny)
    frames = frames_of(y, frame_length, hop, center, dtype)
    nf = len(frames)
    out = Ref(np.empty(nf, dtype), np.empty(nf, dtype), np.empty(nf, np.int32), np.empty(nf, dtype), np.empty((nf, nc), dtype),
              np.zeros(nf, dtype), np.zeros(nf, dtype), np.zeros(nf, bool))
    taus = np.arange(1, pmax + 1).astype(dtype)
    for f, x in enumerate(frames):
        d = np.empty(pmax + 1, dtype)
        for tau in range(pmax + 1):
            df = x[:W] - x[tau:tau + W]
            d[tau] = np.sum(df * df)
        cm = np.cumsum(d[1:]) / taus
        c = d[pmin:] / (cm[pmin - 1:] + tiny)
        i, ok = pick(c, dtype(threshold))
        shift = dtype(0)
        if 0 < i < nc - 1:
            a = c[i + 1] + c[i - 1] - 2 * c[i]
            b = (c[i + 1] - c[i - 1]) / 2
            out.a[f] = a
            if abs(b) < abs(a):
                shift = -b / a
        out.f0[f] = dtype(sr) / (pmin + i + shift)
        out.aperiodicity[f], out.period_index[f], out.cmnd[f] = c[i], i, c
        out.rms[f] = np.sqrt(np.mean(x[:W] ** 2))
        out.shift[f], out.decidable[f] = shift, ok
    return out


@functools.lru_cache(maxsize=None)
def reference(name, in_dtype, dtype):
    """The reference of geometry ``name`` on its five clips stored as ``in_dtype`` ('float32' / 'float64'), evaluated in
    ``dtype`` ('float64' / 'longdouble'); computed once per session, never modified.  Fields are stacked (5, n_frames, ...)."""
    sr, fl, W, hop, fmin, fmax, S = GEOMETRIES[name]
    x = clips(sr, S).astype(in_dtype)
    per = [yin_ref(row, sr, fl, W, hop, fmin, fmax, dtype=getattr(np, dtype)) for row in x]
    ref = Ref(*(np.stack([getattr(p, k) for p in per]) for k in Ref._fields))
    for v in ref:
        v.setflags(write=False)
    return ref
