"""CPU: the yardsticks of the blocked rolling z-score and the host side of its entry point.

The exact rational reference (tests/rolling_exact_ref.py) is pinned to the float64 two-pass statement and to pandas' NaN
pattern; the NumPy restatement of the kernels' tiling and pair arithmetic (tests/rolling_blocked_ref.py) is held to the
exact reference on every case of tests/rolling_blocked_cases.py; ``tl_rolling_zscore_blocked`` is exported, typed, and
refuses bad arguments before anything is launched; ``rolling_zscore.run`` refuses an unknown ``method``."""
import os
import re
from argparse import Namespace

import numpy as np
import pytest

from tests import rolling_blocked_cases as rc
from tests.rolling_blocked_ref import blocked_rolling_zscore
from tests.rolling_exact_ref import exact_rolling_zscore
from tests.signal_refs import pandas_rolling_zscore, rolling_cases, two_pass_rolling_zscore

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "tl_rolling_zscore_blocked"
INT32_MAX = 2 ** 31 - 1


def _rel(a, b):
    return float(np.max(np.abs(np.nan_to_num(a) - np.nan_to_num(b))) / np.max(np.abs(np.nan_to_num(b))))


@pytest.mark.parametrize("name", rc.RANDOM_NAMES)
def test_exact_reference_agrees_with_the_two_pass_statement(name):
    """Observed: at most 9.4e-16 of the largest z (the two-pass statement's own rounding)."""
    x, W = rc.case(name)
    ref = rc.exact(name)
    two = two_pass_rolling_zscore(x, W)
    assert np.array_equal(np.isnan(ref), np.isnan(two))
    assert np.array_equal(np.isnan(ref), np.isnan(pandas_rolling_zscore(x, W)))
    d = _rel(ref, two)
    print(f"{name}: exact vs two-pass {d:.3g}")
    assert d < 1e-12, (name, d)


def test_exact_reference_on_small_windows_and_zeroed_nans():
    rng = np.random.default_rng(7)
    for W in (2, 3, 255):
        x = rolling_cases(rng, 4, 1201, W)
        ref = exact_rolling_zscore(x, W)
        two = two_pass_rolling_zscore(x, W)
        assert np.array_equal(np.isnan(ref), np.isnan(two)) and np.array_equal(np.isnan(ref), np.isnan(pandas_rolling_zscore(x, W)))
        assert _rel(ref, two) < 1e-12, W
        zeroed = exact_rolling_zscore(x, W, preserve_nans=False)
        assert not np.isnan(zeroed).any() and np.array_equal(zeroed, np.nan_to_num(ref))


@pytest.mark.parametrize("name", rc.NAMES)
def test_exact_reference_has_pandas_nan_pattern(name):
    x, W = rc.case(name)
    assert np.array_equal(np.isnan(rc.exact(name)), np.isnan(pandas_rolling_zscore(np.asarray(x, dtype=np.float64), W))), name


@pytest.mark.parametrize("name", rc.NAMES)
def test_restatement_agrees_with_the_exact_reference(name):
    """|out - ref| <= 1.8e-15 |ref| + 1e-25: four times the 4.5e-16 (2 ulp) observed for the pair form, which leaves room for
    another summation order; the floor is for outputs that are exactly 0."""
    ref, out = rc.exact(name), rc.restated(name)
    assert out.dtype == np.float64 and out.shape == ref.shape
    assert np.array_equal(np.isnan(out), np.isnan(ref)), name
    print(f"{name}: restatement vs exact {rc.rel_distance(out, ref):.3g}")
    assert rc.within(out, ref, 1.8e-15), (name, rc.rel_distance(out, ref))


def test_restatement_window_past_the_recording_and_zeroed_nans():
    a, b = rc.restated("C3 T10007 W10007"), rc.restated("C3 T10007 W25000")
    assert np.array_equal(a, b, equal_nan=True)
    x, W = rc.case("C8 T3001 W513")
    zeroed = blocked_rolling_zscore(x, W, preserve_nans=False)
    assert not np.isnan(zeroed).any() and np.array_equal(zeroed, np.nan_to_num(rc.restated("C8 T3001 W513")))


def test_entry_is_exported_declared_and_typed_with_matching_arity():
    from decode_tonal_langauge_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "tonal_hip.h")).read()
    m = re.search(r"\bint\s+" + ENTRY + r"\s*\(([^)]*)\)\s*;", header)
    assert m, f"{ENTRY} is not declared in include/tonal_hip.h"
    assert ENTRY in _lib.SIGNATURES and hasattr(lib, ENTRY)
    assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[ENTRY][1]) == 10


# 16 stands for a non-null device pointer, never followed
def _call(lib, **over):
    a = dict(x=16, is_f64=1, y=16, work=16, work_elems=8 * 3 * 12, C=3, T=3001, window=300, zero_nans=0, stream=None)
    a.update(over)
    return lib.tl_rolling_zscore_blocked(*a.values())


def test_entry_refuses_bad_arguments_without_gpu():
    from decode_tonal_langauge_amd import _lib
    lib = _lib.load()
    for ptr_name in ("x", "y", "work"):
        assert _call(lib, **{ptr_name: None}) == -1 and b"null" in lib.tl_last_error(), ptr_name
    for C in (0, -1, 65536):
        assert _call(lib, C=C, work_elems=1 << 40) == -1 and b"65535" in lib.tl_last_error(), C
    for window in (1, 0, -5):
        assert _call(lib, window=window) == -1 and b"greater than 1" in lib.tl_last_error(), window
    assert _call(lib, T=INT32_MAX - 255, work_elems=1 << 40) == -1 and b"too long" in lib.tl_last_error()
    for T, window in ((3001, 255), (255, 4000), (100, 2)):
        assert _call(lib, T=T, window=window) == -1, (T, window)
        msg = lib.tl_last_error()
        assert b"window kernel" in msg and b"tl_rolling_zscore" in msg and b"256" in msg, msg
    assert _call(lib, work_elems=8 * 3 * 12 - 1) == -1 and b"workspace" in lib.tl_last_error()
    assert _call(lib, T=3073, work_elems=8 * 3 * 12) == -1 and b"workspace" in lib.tl_last_error()     # 13 tiles


def test_run_refuses_an_unknown_method():
    from decode_tonal_langauge_amd.preprocess.signal import rolling_zscore
    for method in ("blocks", "", None, "Window"):
        with pytest.raises(ValueError, match="'window' or 'blocked'"):
            rolling_zscore.run(np.zeros((2, 600)), Namespace(window_length=300, signal_freq=1, method=method))
