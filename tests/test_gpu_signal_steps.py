"""GPU: the preprocess/signal step kernels against plain float64 references on the CPU, at recording sizes and at the
edges where they can go wrong - scipy where the reference calls scipy (``resample``, ``filtfilt``, ``sosfilt``), pandas for
the rolling z-score (plus the exact two-pass statement of it, tests/signal_refs.py), numpy for the row statistics and CAR.

Each case records its worst observed deviation with ``tests.parity_record`` under a section of its own."""
import os
from argparse import Namespace
from copy import deepcopy

import numpy as np
import pytest
import torch
from scipy import signal as sps

from oracle import signal_oracle as sg
from tests.parity_record import record
from tests.signal_refs import pandas_rolling_zscore, rolling_cases, two_pass_rolling_zscore

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

RAW_FS = 3051.7578125                    # a TDT recording rate; 120 s of it is 366 210 samples
RESAMPLE_GRID = [(900, 1200), (901, 1200), (900, 1201), (1000, 1000), (1001, 1001), (1200, 900), (1201, 900), (2, 5),
                 (7, 1)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch.device("cuda:0")


def rel(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(float(np.max(np.abs(b))), 1e-30))


def ulps32(got, ref64, floor=1e-3):
    """Largest |got - round32(ref64)| in units of the float32 spacing at the rounded reference (at least at ``floor``, so
    that a value near 0 is not held to a spacing far below the float64 rounding of its inputs)."""
    r = ref64.astype(np.float32)
    sp = np.spacing(np.maximum(np.abs(r), np.float32(floor))).astype(np.float64)
    return float(np.max(np.abs(got.astype(np.float64) - r.astype(np.float64)) / sp))


def same_nonfinite(a, b):
    return (np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isposinf(a), np.isposinf(b))
            and np.array_equal(np.isneginf(a), np.isneginf(b)))


# ---------------------------------------------------------------------------------------------------------------------
# resampling (tl_fft_resample: Bluestein over power-of-two Stockham passes)
# ---------------------------------------------------------------------------------------------------------------------

def test_resample_parity_grid_against_scipy(dev):
    """Up, down and equal lengths, odd and even N = min(nx, num): the even-N Nyquist bin is doubled when downsampling and
    halved when upsampling (900 -> 1200), kept at equal lengths (1000 -> 1000)."""
    from decode_tonal_langauge_amd.preprocess.signal import downsample
    rng = np.random.default_rng(21)
    obs = {}
    for nx, num in RESAMPLE_GRID:
        for C in (3, 37):
            x = rng.standard_normal((C, nx)) * 2.0 + 0.5
            ref = sps.resample(x, num, axis=1)
            out = downsample.resample(x, num)
            assert out.dtype == np.float64 and out.shape == (C, num)
            d = rel(out, ref)
            obs[f"{nx}->{num} C{C}"] = d
            assert d < 1e-13, (nx, num, C, d)
    record("signal_steps.resample_grid", obs)


def test_resample_raw_recording_through_run(dev):
    """120 s of 16 channels at a non-integer raw rate to 400 Hz: nx = 366 210, a 2^20-point Bluestein transform, and
    num = int(366 210 * 400 / 3051.7578125) = 47 999 - odd, as the reference's truncation makes it."""
    from decode_tonal_langauge_amd.preprocess.signal import downsample
    T = int(RAW_FS * 120)
    assert T == 366210
    x = np.random.default_rng(3).standard_normal((16, T)) * 30.0 + 5.0
    prm = Namespace(signal_freq=RAW_FS, downsample_freq=400)
    out = downsample.run(x, prm)
    assert prm.signal_freq == 400 and out.shape == (16, 47999)
    d = rel(out, sps.resample(x, 47999, axis=1))
    record("signal_steps.resample_raw", {"366210->47999 C16": d})
    assert d < 1e-13


def test_resample_float32_and_device_input(dev):
    from decode_tonal_langauge_amd.preprocess.signal import downsample
    rng = np.random.default_rng(4)
    obs = {}
    for C, nx, num in ((3, 1001, 700), (37, 900, 1200)):
        x = (rng.standard_normal((C, nx)) * 2.0 + 0.5).astype(np.float32)
        out = downsample.resample(x, num)
        assert out.dtype == np.float32 and out.shape == (C, num)
        # scipy.fft keeps float32 input in single precision; the kernel transforms in float64 and rounds once
        obs[f"f32 {nx}->{num} vs scipy"] = d32 = rel(out, sps.resample(x, num, axis=1))
        # against scipy in float64: the float32 rounding of the output and no more
        obs[f"f32 {nx}->{num} vs f64"] = d64 = rel(out, sps.resample(x.astype(np.float64), num, axis=1))
        assert d32 < 1e-6 and d64 < 1e-7, (nx, num, d32, d64)
    x = rng.standard_normal((37, 4001)) * 2.0
    t = torch.from_numpy(x).to(dev)
    out = downsample.resample(t, 3000)
    assert isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float64
    obs["device 4001->3000"] = d = rel(out.cpu().numpy(), sps.resample(x, 3000, axis=1))
    assert d < 1e-13
    record("signal_steps.resample_f32_device", obs)


# ---------------------------------------------------------------------------------------------------------------------
# channel_zscore / zscore_rereference (tl_row_zscore) and car_rereference (tl_car) against numpy float64
# ---------------------------------------------------------------------------------------------------------------------

def _np_zscore(x, t0, t1):
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (x - x[:, t0:t1].mean(axis=1, keepdims=True)) / x[:, t0:t1].std(axis=1, keepdims=True)


def test_row_zscore_against_numpy(dev):
    from decode_tonal_langauge_amd.preprocess.signal import channel_zscore, zscore_rereference
    rng = np.random.default_rng(8)
    obs = {}
    for C, T in ((256, 24000), (3, 1200007)):
        x64 = rng.standard_normal((C, T)) * 40.0 + 7.0
        for dt in (np.float64, np.float32):
            x = x64.astype(dt)
            tag = f"{C}x{T} {np.dtype(dt).name}"
            for name, (t0, t1) in (("whole", (0, T)), ("[0,25s]", (0, 10000)), ("to T", (T - 5003, T)),
                                   ("mid", (T // 3, T // 3 + 777))):
                if name == "whole":
                    out = channel_zscore.run(x, Namespace())
                else:
                    out = zscore_rereference.rereference(x, (t0, t1))
                assert out.dtype == dt and out.shape == (C, T)
                ref = _np_zscore(x, t0, t1)
                if dt == np.float64:
                    obs[f"{tag} {name}"] = d = rel(out, ref)
                    assert d < 1e-14, (tag, name, d)
                else:
                    # the float64 statistics of the float32 data, rounded once; numpy's float32 accumulation at 1e-5
                    obs[f"{tag} {name} ulps"] = u = ulps32(out, ref)
                    assert u <= 1.0, (tag, name, u)
                    with np.errstate(invalid="ignore", divide="ignore"):
                        r32 = (x - x[:, t0:t1].mean(axis=1, keepdims=True)) / x[:, t0:t1].std(axis=1, keepdims=True)
                    assert rel(out, r32) < 1e-5
    # a statistics interval of one sample: std is exactly 0, so +-inf, and NaN where x equals the mean - as numpy gives them
    x = rng.standard_normal((5, 3001))
    x[:, 1500] = x[:, 17]                                   # another sample equal to the mean: 0 / 0
    for dt in (np.float64, np.float32):
        for t0 in (0, 17, 3000):
            out = zscore_rereference.rereference(x.astype(dt), (t0, t0 + 1))
            ref = _np_zscore(x.astype(dt), t0, t0 + 1)
            assert same_nonfinite(out, ref), (dt, t0)
            assert np.isnan(out[:, t0]).all() and np.isinf(out[:, t0 + 1 if t0 < 3000 else 0]).all()
    # a channel holding a NaN: all NaN with preserve_nans, all 0 without; the other channels untouched
    x = rng.standard_normal((4, 5003))
    x[2, 4000] = np.nan
    for dt in (np.float64, np.float32):
        out = channel_zscore.run(x.astype(dt), Namespace())
        assert np.isnan(out[2]).all() and not np.isnan(out[[0, 1, 3]]).any()
        zero = channel_zscore.run(x.astype(dt), Namespace(preserve_nans=False))
        assert (zero[2] == 0).all() and np.array_equal(zero[[0, 1, 3]], out[[0, 1, 3]])
        assert same_nonfinite(out, _np_zscore(x.astype(dt), 0, 5003))
    record("signal_steps.row_zscore", obs)


def test_car_against_numpy(dev):
    from decode_tonal_langauge_amd.preprocess.signal import car_rereference
    rng = np.random.default_rng(9)
    obs = {}
    for C, T, excl in ((256, 24001, sorted(set(rng.integers(0, 256, 40).tolist()))), (2, 10007, [1])):
        x64 = rng.standard_normal((C, T)) * 25.0 + 3.0
        mask = np.ones(C, bool)
        mask[excl] = False
        ref = x64 - x64[mask].mean(axis=0, keepdims=True)
        for dt in (np.float64, np.float32):
            x = x64.astype(dt)
            out = car_rereference.run(x, Namespace(exclude_channels=list(excl)))
            assert out.dtype == dt
            if dt == np.float64:
                obs[f"{C}x{T} f64"] = d = rel(out, ref)
                assert d < 1e-14
            else:
                r = x.astype(np.float64) - x.astype(np.float64)[mask].mean(axis=0, keepdims=True)
                obs[f"{C}x{T} f32 ulps"] = u = ulps32(out, r)
                assert u <= 1.0
    # a NaN in an included channel poisons that sample of every channel; in an excluded one, only its own
    x = rng.standard_normal((6, 3001))
    x[1, 100] = np.nan
    x[4, 200] = np.nan
    out = car_rereference.run(x, Namespace(exclude_channels=[4]))
    ref = x - x[[0, 1, 2, 3, 5]].mean(axis=0, keepdims=True)
    assert np.array_equal(np.isnan(out), np.isnan(ref))
    assert np.isnan(out[:, 100]).all() and np.isnan(out[:, 200]).sum() == 1 and np.isnan(out[4, 200])
    assert rel(np.nan_to_num(out), np.nan_to_num(ref)) < 1e-12
    record("signal_steps.car", obs)


# ---------------------------------------------------------------------------------------------------------------------
# rolling z-score (tl_rolling_zscore) against pandas, as the reference calls it
# ---------------------------------------------------------------------------------------------------------------------

def _rolling(x, W, keep=True):
    from decode_tonal_langauge_amd.preprocess.signal import rolling_zscore
    return rolling_zscore.run(x, Namespace(window_length=W, signal_freq=1, preserve_nans=keep))


def _check_rolling(x, W, obs, tag, keep=True):
    out = _rolling(x, W, keep)
    assert out.dtype == np.float64 and out.shape == x.shape
    pd_ref = pandas_rolling_zscore(x, W, keep)
    assert np.array_equal(np.isnan(out), np.isnan(pd_ref)), (tag, W)          # pandas' NaN pattern, exactly
    exact = two_pass_rolling_zscore(x, W, keep)
    assert np.array_equal(np.isnan(out), np.isnan(exact))
    d = rel(np.nan_to_num(out), np.nan_to_num(exact))
    dp = rel(np.nan_to_num(out), np.nan_to_num(pd_ref))
    obs[f"{tag} exact"] = max(d, obs.get(f"{tag} exact", 0.0))
    obs[f"{tag} pandas"] = max(dp, obs.get(f"{tag} pandas", 0.0))
    assert d < 1e-12, (tag, W, d)
    # pandas moves its window sums sample by sample and takes the variance as a difference of them: on a window whose
    # spread is small against the recording's level that difference loses digits (observed: 7e-4 of the largest z at
    # W = 2, on pairs of samples ~1e-6 apart; 7e-11 at W = 4000).  The accuracy check is the exact statement above.
    assert dp < 1e-3, (tag, W, dp)
    return out


def test_rolling_zscore_small_windows_many_channels(dev):
    """W around one 256-sample tile, T not a multiple of 256, 65 channels holding flat stretches of 0.1 and 1/3 (from t = 0
    and mid-recording), exact zeros, and NaN stretches shorter and longer than W; both preserve_nans settings."""
    rng = np.random.default_rng(12)
    obs = {}
    for W in (2, 3, 255, 256, 257):
        x = rolling_cases(rng, 65, 3001, W)
        for keep in (True, False):
            out = _check_rolling(x, W, obs, f"C65 T3001 W{W}", keep)
            if keep:
                # a flat stretch gives NaN on every sample whose window lies inside it (pandas: std = 0)
                assert np.isnan(out[0, W - 1:W + 37]).all() and np.isnan(out[1, 3001 // 3 + W - 1:3001 // 3 + W + 37]).all()
            else:
                assert not np.isnan(out).any()
    record("signal_steps.rolling_small", obs)


def test_rolling_zscore_wide_windows(dev):
    """Windows up to and past the LDS tile (7 937 samples fit one; 7 938 and 10 000 stream through it) and past T."""
    rng = np.random.default_rng(13)
    obs = {}
    T = 10007
    for W in (4000, 7937, 7938, 10000, 25000):
        x = rolling_cases(rng, 3, T, W)
        _check_rolling(x, W, obs, f"C3 T{T} W{W}")
    x = rolling_cases(rng, 3, T, 9000)
    _check_rolling(x, 9000, obs, f"C3 T{T} W9000", keep=False)
    # float32 input: the references read the same float32 values
    x32 = rolling_cases(rng, 3, T, 8500).astype(np.float32)
    _check_rolling(x32, 8500, obs, f"C3 T{T} W8500 f32")
    x32 = rolling_cases(rng, 4, 2999, 300).astype(np.float32)
    _check_rolling(x32, 300, obs, "C4 T2999 W300 f32")
    record("signal_steps.rolling_wide", obs)


def test_rolling_zscore_the_reported_flat_stretch(dev):
    """40 N(0,1) samples, then 0.1: pandas gives NaN on the flat stretch; the plain sum gave +-sqrt((n-1)/n) there."""
    x = np.concatenate([np.random.default_rng(0).standard_normal(40), np.full(60, 0.1)])[None]
    for W in (10, 50):
        out = _rolling(x, W)
        assert np.isnan(out[0, 40 + W - 1:]).all()
        assert np.array_equal(np.isnan(out), np.isnan(pandas_rolling_zscore(x, W)))
        assert (_rolling(x, W, keep=False)[0, 40 + W - 1:] == 0).all()


def test_rolling_zscore_is_bit_identical_to_the_single_tile_kernel(dev):
    """Windows that fit one LDS tile keep the per-output summation order of the kernel before windows could stream:
    the outputs recorded from it (tests/golden/rolling_single_tile.npz) are reproduced bit for bit."""
    g = np.load(os.path.join(GOLD, "rolling_single_tile.npz"))
    for key in ("a", "b"):
        x, W = g[f"{key}.x"], int(g[f"{key}.W"])
        out = _rolling(x, W, keep=bool(g[f"{key}.keep"]))
        assert np.array_equal(out, g[f"{key}.out"], equal_nan=True), key


# ---------------------------------------------------------------------------------------------------------------------
# Butterworth: zero-phase (tl_filtfilt_f64) against scipy.signal.filtfilt, causal (tl_sosfilt_f64) against sosfilt
# ---------------------------------------------------------------------------------------------------------------------

FS = 400.0
# (btype, order, freqs) -> taps: band-pass order n has 2n + 1, low-pass n + 1.  <= 9 taps run on filtfilt_iir8_kernel,
# 10 - 17 on filtfilt_iir_kernel<17>.  The band keeps the transfer-function form well conditioned at order 8 (a 2 Hz
# lower edge puts a pole of butter(8)'s (b, a) outside the unit circle, and scipy's own output then depends on 1e-15
# perturbations at O(1))
FILTFILT_DESIGNS = [("bandpass", 2, [30.0, 150.0]), ("bandpass", 4, [30.0, 150.0]), ("lowpass", 8, 60.0),
                    ("bandpass", 5, [30.0, 150.0]), ("bandpass", 8, [30.0, 150.0])]


def _ba(btype, order, freqs):
    return sps.butter(order, np.asarray(freqs, dtype=float) / (0.5 * FS), btype=btype)


def test_filtfilt_against_scipy(dev):
    from decode_tonal_langauge_amd.preprocess.signal import frequency_filter as ff
    rng = np.random.default_rng(14)
    x_big = (rng.standard_normal((256, 24000)) * 20.0 + 3.0).astype(np.float32)
    x_long = rng.standard_normal((1, 300007)) * 20.0 + 3.0
    obs = {}
    for btype, order, freqs in FILTFILT_DESIGNS:
        b, a = _ba(btype, order, freqs)
        ntaps = max(len(a), len(b))
        tag = f"{btype}{order} ({ntaps} taps)"
        short = rng.standard_normal((3, 3 * ntaps + 1))
        for name, x in (("256x24000 f32", x_big), ("1x300007 f64", x_long), (f"3x{3 * ntaps + 1}", short)):
            out = ff.butter_filter(x, freqs, FS, order=order, filter_type=btype)
            assert out.dtype == np.float64 and out.shape == x.shape
            obs[f"{tag} {name}"] = d = rel(out, sps.filtfilt(b, a, x, axis=-1))
            assert d < 1e-13, (tag, name, d)                 # observed: 0 (the recurrence rounds as scipy's loop)
        # T = padlen: the same ValueError as scipy
        edge = rng.standard_normal((3, 3 * ntaps))
        with pytest.raises(ValueError) as want:
            sps.filtfilt(b, a, edge, axis=-1)
        with pytest.raises(ValueError) as got:
            ff.butter_filter(edge, freqs, FS, order=order, filter_type=btype)
        assert str(got.value) == str(want.value)
    # band-pass order 9 (19 taps) is past the kernel's state registers: refused, naming the limit
    with pytest.raises(RuntimeError, match=r"2\.\.17"):
        ff.butter_filter(x_long, [30.0, 150.0], FS, order=9)
    record("signal_steps.filtfilt", obs)


def test_sosfilt_against_scipy(dev):
    from decode_tonal_langauge_amd.preprocess.signal import frequency_filter as ff
    rng = np.random.default_rng(15)
    x = (rng.standard_normal((65, 100003)) * 20.0 + 3.0).astype(np.float32)
    obs = {}
    designs = [("lowpass", n, 60.0) for n in range(2, 17)] + [("bandpass", n, [2.0, 60.0]) for n in range(1, 9)]
    seen = set()
    for btype, order, freqs in designs:
        sos = sps.butter(order, np.asarray(freqs, dtype=float) / (0.5 * FS), btype=btype, output="sos")
        seen.add(sos.shape[0])
        out = ff.butter_filter(x, freqs, FS, order=order, causal=True, filter_type=btype)
        assert out.dtype == np.float64 and out.shape == x.shape
        obs[f"{btype}{order} ({sos.shape[0]} sections)"] = d = rel(out, sps.sosfilt(sos, x, axis=-1))
        assert d < 1e-13, (btype, order, d)                  # observed: 0
    assert seen == set(range(1, 9))
    with pytest.raises(RuntimeError, match=r"1\.\.8"):
        ff.butter_filter(x[:2], 60.0, FS, order=17, causal=True, filter_type="lowpass")
    with pytest.raises(RuntimeError, match=r"1\.\.8"):
        ff.butter_filter(x[:2], [2.0, 60.0], FS, order=9, causal=True)
    record("signal_steps.sosfilt", obs)


# ---------------------------------------------------------------------------------------------------------------------
# the example_config.yaml chain at the raw rate
# ---------------------------------------------------------------------------------------------------------------------

CONFIG_STEPS = [
    {"module": "preprocess.downsample", "params": {"downsample_freq": 400}},
    {"module": "preprocess.frequency_filter", "params": {"bands": [
        # (floats: the reference's gaussian_bank reads a list of two ints as two ranges and fails, and so does this package)
        {"method": "hilbert", "params": {"freq_ranges": [70., 150.], "envelope": True}},
        {"method": "butter", "params": {"freqs": [0.3, 100], "filter_type": "bandpass"}}]}},
    {"module": "preprocess.zscore_rereference", "params": {"rereference_interval": [0., 25.]}},
]


def _chain_ref(ds):
    hil = sg.hilbert_filter(ds, 400, [70., 150.], envelope=True)
    b, a = sps.butter(4, np.array([0.3, 100.0]) / 200.0, btype="bandpass")
    bands = np.concatenate([hil, sps.filtfilt(b, a, ds, axis=-1)], axis=0)
    return _np_zscore(bands, 0, 10000)


def test_example_config_chain_at_the_raw_rate(dev):
    from decode_tonal_langauge_amd.preprocess import preprocessor
    from decode_tonal_langauge_amd.preprocess.signal import downsample
    T = int(RAW_FS * 120)
    x = np.random.default_rng(16).standard_normal((16, T)) * 30.0 + 5.0
    prm = Namespace(signal_freq=RAW_FS)
    out, freq = preprocessor.preprocess_signal(x.copy(), deepcopy(CONFIG_STEPS), prm)
    n = int(T * 400 / RAW_FS)
    assert freq == 400 and out.shape == (32, n) == (32, 47999)
    # the Butterworth rows against the oracle chain on the GPU's own resampled signal: a filter error shows here
    ds_gpu = downsample.resample(x, n)
    own = _chain_ref(ds_gpu)
    d_own = rel(out[16:], own[16:])
    d_own_h = rel(out[:16], own[:16])
    # end to end: the order-4 0.3 Hz band-pass (poles near |z| = 1) amplifies the resampling's 1e-15 differences
    full = _chain_ref(sps.resample(x, n, axis=1))
    d_end = rel(out, full)
    record("signal_steps.example_chain", {"butter rows on own resample": d_own, "hilbert rows on own resample": d_own_h,
                                          "end to end": d_end})
    assert d_own < 1e-11 and d_own_h < 1e-11
    assert d_end < 2e-7
