"""GPU: the blocked rolling z-score (``method: blocked``, tl_rolling_zscore_blocked) against the exact rational reference.

Cases, references and the NumPy restatement come from tests/rolling_blocked_cases.py.  The bound of every case is
|out - ref| <= B |ref| + 1e-25 with B = 8 x the restatement's own largest elementwise distance from the exact reference
on that case (4.5e-16 at most, tests/test_rolling_blocked_host.py): the restatement does the kernels' arithmetic, the 8 x
covers another summation order and the device's division and square root.  B never comes from the kernel's output.
Observed deviations go to ``parity_observed.json``, sections ``rolling_blocked_*``."""
from argparse import Namespace

import numpy as np
import pytest
import torch

from tests import rolling_blocked_cases as rc
from tests.parity_record import record
from tests.signal_refs import pandas_rolling_zscore, rolling_cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch.device("cuda:0")


def _run(x, W, keep=True, method="blocked"):
    from decode_tonal_langauge_amd.preprocess.signal import rolling_zscore
    assert method in rolling_zscore.METHODS                      # the step knows the parameter, it does not ignore it
    x = x if isinstance(x, torch.Tensor) else np.array(x)       # the cases are read-only; the step gets a copy of its own
    return rolling_zscore.run(x, Namespace(window_length=W, signal_freq=1, preserve_nans=keep, method=method))


def _check(name, obs):
    x, W = rc.case(name)
    ref = rc.exact(name)
    out = _run(x, W)
    assert out.dtype == np.float64 and out.shape == x.shape
    assert np.array_equal(np.isnan(out), np.isnan(ref)), name
    assert np.array_equal(np.isnan(out), np.isnan(pandas_rolling_zscore(np.asarray(x, dtype=np.float64), W))), name
    bound = 8.0 * rc.rel_distance(rc.restated(name), ref)
    d = rc.rel_distance(out, ref)
    obs[f"{name} exact"] = d
    obs[f"{name} bound"] = bound
    obs[f"{name} restatement bits"] = float(np.array_equal(out, rc.restated(name), equal_nan=True))
    print(f"{name}: blocked vs exact {d:.3g} (bound {bound:.3g}), equals the restatement: {obs[f'{name} restatement bits']}")
    assert 0.0 < bound < 1e-14, (name, bound)
    assert rc.within(out, ref, bound), (name, d, bound)
    return out


@pytest.mark.parametrize("W", (256, 257, 511, 512, 513, 1024))
def test_blocked_head_lengths_and_both_nan_settings(dev, W):
    """8 x 3 001: head lengths 0 .. 510, no whole tile and one whole tile, T not a multiple of 256."""
    name, obs = f"C8 T3001 W{W}", {}
    out = _check(name, obs)
    x, _ = rc.case(name)
    zeroed = _run(x, W, keep=False)
    assert not np.isnan(zeroed).any()
    assert np.array_equal(zeroed, np.nan_to_num(out))
    # a flat stretch gives NaN on every sample whose window lies inside it (pandas: std = 0)
    assert np.isnan(out[0, W - 1:W + 37]).all() and np.isnan(out[1, 3001 // 3 + W - 1:3001 // 3 + W + 37]).all()
    record(f"rolling_blocked_heads.W{W}", obs)


def test_blocked_last_tile_full_and_of_one_sample(dev):
    obs = {}
    for name in ("C3 T3072 W256", "C2 T257 W256", "C2 T257 W257"):
        _check(name, obs)
    record("rolling_blocked_last_tile", obs)


def test_blocked_wide_windows_and_windows_past_the_recording(dev):
    obs = {}
    _check("C3 T10007 W4000", obs)
    a = _check("C3 T10007 W10007", obs)
    b = _check("C3 T10007 W25000", obs)
    assert np.array_equal(a, b, equal_nan=True)                 # a window wider than the recording runs as W = T
    record("rolling_blocked_wide", obs)


def test_blocked_256_and_more_table_rows_per_window(dev):
    """W = 66 000: a table row for every lane; W = 66 100: 257 rows, lane 0 adds a second one."""
    obs = {}
    _check("C2 T70001 W66000", obs)
    _check("C2 T70001 W66100", obs)
    record("rolling_blocked_table", obs)


def test_blocked_float32_input(dev):
    obs = {}
    _check("C4 T2999 W300 f32", obs)
    record("rolling_blocked_f32", obs)


@pytest.mark.parametrize("name", rc.DC_NAMES)
def test_blocked_on_a_dc_level(dev, name):
    """N(0, 1) on a level of 1e4.  The default route's distance from the exact reference is recorded, not asserted."""
    obs = {}
    _check(name, obs)
    x, W = rc.case(name)
    ref = rc.exact(name)
    default = _run(x, W, method="window")
    assert np.array_equal(np.isnan(default), np.isnan(ref))
    obs[f"{name} window route exact"] = rc.rel_distance(default, ref)
    obs[f"{name} window route of largest z"] = float(np.nanmax(np.abs(default - ref)) / np.nanmax(np.abs(ref)))
    print(f"{name}: window route vs exact {obs[f'{name} window route exact']:.3g}")
    record(f"rolling_blocked_dc.W{W}", obs)


def test_small_windows_keep_the_default_routes_bits(dev):
    rng = np.random.default_rng(5)
    for W in (2, 255):
        x = rolling_cases(rng, 5, 1501, W)
        for keep in (True, False):
            assert np.array_equal(_run(x, W, keep), _run(x, W, keep, method="window"), equal_nan=True), (W, keep)
    x = rolling_cases(rng, 5, 1501, 256)                         # the first window the blocked route takes
    assert not np.array_equal(_run(x, 256), _run(x, 256, method="window"), equal_nan=True)
    x = rolling_cases(rng, 2, 200, 150)                       # a wide window on a recording shorter than a tile
    assert np.array_equal(_run(x, 4000), _run(x, 4000, method="window"), equal_nan=True)


def test_two_runs_give_the_same_bits(dev):
    for name in ("C8 T3001 W513", "C2 T70001 W66000"):
        x, W = rc.case(name)
        assert np.array_equal(_run(x, W), _run(x, W), equal_nan=True), name


def test_cuda_tensor_in_gives_cuda_tensor_out(dev):
    x, W = rc.case("C8 T3001 W512")
    for dtype in (torch.float64, torch.float32):
        xt = torch.from_numpy(np.array(x)).to(dev, dtype)
        out = _run(xt, W)
        assert isinstance(out, torch.Tensor) and out.device == xt.device and out.dtype == torch.float64
        assert np.array_equal(out.cpu().numpy(), _run(xt.cpu().numpy(), W), equal_nan=True)


def test_direct_call_leaves_canaries_behind_output_and_workspace(dev):
    from decode_tonal_langauge_amd import _lib
    from decode_tonal_langauge_amd._lib import check, ptr
    lib = _lib.load()
    for name in ("C8 T3001 W257", "C3 T3072 W256", "C2 T257 W257"):
        x, W = rc.case(name)
        C, T = x.shape
        n_y, n_work, pad = C * T, 8 * C * (-(-T // 256)), 4096
        xt = torch.from_numpy(np.array(x)).to(dev)
        y = torch.full((n_y + pad,), -7.25, dtype=torch.float64, device=dev)
        work = torch.full((n_work + pad,), -7.25, dtype=torch.float64, device=dev)
        check(lib.tl_rolling_zscore_blocked(ptr(xt), 1, ptr(y), ptr(work), n_work, C, T, W, 0,
                                            torch.cuda.current_stream().cuda_stream), "tl_rolling_zscore_blocked")
        torch.cuda.synchronize()
        assert bool((y[n_y:] == -7.25).all()) and bool((work[n_work:] == -7.25).all()), name
        assert not bool((work[:n_work] == -7.25).any())          # every table row was written
        assert np.array_equal(y[:n_y].view(C, T).cpu().numpy(), _run(x, W), equal_nan=True)


def test_through_preprocess_signal(dev):
    from decode_tonal_langauge_amd.preprocess.preprocessor import preprocess_signal
    x, W = rc.case("C8 T3001 W512")
    steps = [{"module": "preprocess.signal.rolling_zscore",
              "params": {"window_length": W, "preserve_nans": False, "method": "blocked"}}]
    out, freq = preprocess_signal(np.array(x), steps, Namespace(signal_freq=1))
    assert freq == 1
    direct = _run(x, W, keep=False)
    assert np.array_equal(out, direct)
    assert not np.array_equal(direct, _run(x, W, keep=False, method="window"))   # the step did take the blocked route
