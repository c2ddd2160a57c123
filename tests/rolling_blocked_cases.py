"""The recordings the blocked rolling z-score is tested on, with their references - TEST INFRASTRUCTURE ONLY.

Shared by tests/test_rolling_blocked_host.py and tests/test_gpu_rolling_blocked.py: every case's exact reference
(tests/rolling_exact_ref.py) and NumPy restatement (tests/rolling_blocked_ref.py) are computed once per process and never
modified.  The shapes are the smallest at which the kernels can go wrong: head lengths 0 .. 510, no / one / many whole
tiles, a last tile that is full or holds one sample, a window as long as and longer than the recording, more than 256 table
rows per window, float32 input, and a DC level of 1e4."""
from functools import lru_cache

import numpy as np

from tests.rolling_blocked_ref import blocked_rolling_zscore
from tests.rolling_exact_ref import exact_rolling_zscore
from tests.signal_refs import rolling_cases

FLOOR = 1e-25                        # for outputs that are exactly 0


def _dc(W):
    rng = np.random.default_rng(1000 + W)
    x = rng.standard_normal((3, 3001)) + 1e4
    x[0, 700:700 + W // 2] = np.nan                              # a NaN run shorter than the window
    x[1, 1200:1200 + W + 50] = 1e4 + 0.1                         # a flat stretch longer than it
    x[2, 2000:2000 + W + 9] = np.nan                             # and a NaN run longer than it
    return x


def _build():
    cases = {}
    for W in (256, 257, 511, 512, 513, 1024):
        cases[f"C8 T3001 W{W}"] = (lambda W=W: rolling_cases(np.random.default_rng(100 + W), 8, 3001, W), W)
    cases["C3 T3072 W256"] = (lambda: rolling_cases(np.random.default_rng(21), 3, 3072, 256), 256)
    for W in (256, 257):
        cases[f"C2 T257 W{W}"] = (lambda W=W: rolling_cases(np.random.default_rng(30 + W), 2, 257, W), W)
    cases["C3 T10007 W4000"] = (lambda: rolling_cases(np.random.default_rng(41), 3, 10007, 4000), 4000)
    wide = lambda: rolling_cases(np.random.default_rng(42), 3, 10007, 10007)   # noqa: E731 - one recording, two windows
    cases["C3 T10007 W10007"] = (wide, 10007)
    cases["C3 T10007 W25000"] = (wide, 25000)
    cases["C2 T70001 W66000"] = (lambda: rolling_cases(np.random.default_rng(51), 2, 70001, 66000), 66000)
    # 66 000 = 257.8 tiles: 256 whole tiles inside every window, one table row per lane.  66 100 makes them 257, so that lane 0
    # takes a second row (tiles 257 .. 273 of the 274)
    cases["C2 T70001 W66100"] = (lambda: rolling_cases(np.random.default_rng(52), 2, 70001, 66100), 66100)
    cases["C4 T2999 W300 f32"] = (lambda: rolling_cases(np.random.default_rng(61), 4, 2999, 300).astype(np.float32), 300)
    for W in (256, 600):
        cases[f"DC1e4 C3 T3001 W{W}"] = (lambda W=W: _dc(W), W)
    return cases


_CASES = _build()
NAMES = tuple(_CASES)
RANDOM_NAMES = tuple(n for n in NAMES if n.startswith("C8 ") or n.endswith("f32"))   # where the two-pass statement runs
DC_NAMES = tuple(n for n in NAMES if n.startswith("DC"))


def _frozen(a):
    a.setflags(write=False)
    return a


@lru_cache(maxsize=None)
def case(name):
    """(x, W) of a case; x is read-only."""
    make, W = _CASES[name]
    return _frozen(make()), W


@lru_cache(maxsize=None)
def exact(name):
    x, W = case(name)
    return _frozen(exact_rolling_zscore(x, W))


@lru_cache(maxsize=None)
def restated(name):
    x, W = case(name)
    return _frozen(blocked_rolling_zscore(x, W))


def rel_distance(out, ref):
    """Largest elementwise |out - ref| / |ref| over the outputs where ref is a non-zero number."""
    m = ~np.isnan(ref) & (ref != 0)
    return float(np.max(np.abs(out[m] - ref[m]) / np.abs(ref[m]))) if m.any() else 0.0


def within(out, ref, bound):
    """|out - ref| <= bound |ref| + FLOOR on every output that is a number in ref (the NaN patterns are compared apart)."""
    m = ~np.isnan(ref)
    return bool(np.all(np.abs(out[m] - ref[m]) <= bound * np.abs(ref[m]) + FLOOR))
