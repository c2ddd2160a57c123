"""Plain CPU references of the preprocess/signal steps for the tests - TEST INFRASTRUCTURE ONLY.

``pandas_rolling_zscore`` is the reference's own call (preprocess/signal/rolling_zscore.py:36-49): pandas
updates its window sums as the window moves, so on long windows it carries a rounding drift of its own.
``two_pass_rolling_zscore`` is the exact float64 statement of the same quantity - mean, then the sum of squared
deviations from it, over each trailing window - with pandas' rule for a window whose non-NaN values are all
equal (mean = that value, std = 0).

Band filters (tests/test_gpu_band_filters.py): ``hilbert_filter_longdouble`` and ``fir_bank_longdouble`` are the
extended-precision statements that tests/test_oracle_golden.py pins the float64 references to - the Hilbert oracle and
``scipy_fir_bank``, the reference's ``lfilter`` call; ``band_cases`` builds the recordings."""
import numpy as np
import pandas as pd
from numpy.lib.stride_tricks import sliding_window_view


def pandas_rolling_zscore(x: np.ndarray, window: int, preserve_nans: bool = True) -> np.ndarray:
    df = pd.DataFrame(np.asarray(x).T)
    rolling = df.rolling(window=window, min_periods=1, center=False)
    z = (df - rolling.mean()) / rolling.std()
    if not preserve_nans:
        z = z.fillna(0)
    return z.T.to_numpy()


def two_pass_rolling_zscore(x: np.ndarray, window: int, preserve_nans: bool = True,
                            max_elems: int = 1 << 24) -> np.ndarray:
    x = np.asarray(x, dtype=np.float64)
    C, T = x.shape
    W = min(window, T)
    pad = np.concatenate([np.full((C, W - 1), np.nan), x], axis=1)
    view = sliding_window_view(pad, W, axis=1)                  # (C, T, W): window of output t
    out = np.empty((C, T))
    step = max(1, max_elems // (C * W))
    with np.errstate(invalid="ignore", divide="ignore"):
        for a in range(0, T, step):
            w = view[:, a:a + step]
            n = np.sum(~np.isnan(w), axis=2)
            mean = np.nansum(w, axis=2) / n
            var = np.nansum((w - mean[..., None]) ** 2, axis=2) / (n - 1)
            flat = np.fmin.reduce(w, axis=2) == np.fmax.reduce(w, axis=2)
            z = (x[:, a:a + step] - mean) / np.sqrt(var)
            out[:, a:a + step] = np.where((n >= 2) & ~flat, z, np.nan)
    if not preserve_nans:
        out[np.isnan(out)] = 0
    return out


def hilbert_filter_longdouble(data: np.ndarray, sampling_rate: float, freq_ranges, envelope: bool = True,
                              **bank) -> np.ndarray:
    """The reference's ``hilbert_filter`` (preprocess/signal/frequency_filter.py:155-184) with its transforms, products,
    magnitudes and band mean in ``np.longdouble`` (``scipy.fft`` transforms in the precision of its input): whole-recording
    FFT, per band the Gaussian times the one-sided multiplier with ``H[0] = 0``, inverse FFT, ``|.|`` or the real part,
    mean over bands.  The multiplier itself is the float64 array the reference builds - it is part of the filter's
    definition, not of its arithmetic - widened exactly.  (C, T) longdouble."""
    import scipy.fft as sfft
    from oracle.signal_oracle import gaussian_bank
    x = np.asarray(data).astype(np.longdouble)
    C, T = x.shape
    cfs, sds = gaussian_bank(freq_ranges, sampling_rate, **bank)
    freqs = np.fft.fftfreq(T, d=1.0 / sampling_rate)
    mult = np.zeros(T)
    mult[0] = 1
    mult[1:(T + 1) // 2] = 2
    if T % 2 == 0:
        mult[T // 2] = 1
    X = sfft.fft(x, axis=1)
    assert X.dtype == np.clongdouble
    acc = np.zeros((C, T), dtype=np.longdouble)
    for fc, sf in zip(cfs, sds):
        H = np.exp(-0.5 * ((freqs - fc) / sf) ** 2)
        H[0] = 0
        sig = sfft.ifft(X * (H * mult).astype(np.longdouble)[None, :], axis=1)
        acc += np.abs(sig) if envelope else sig.real
    return acc / np.longdouble(len(cfs))


def fir_bank_longdouble(data: np.ndarray, taps: np.ndarray) -> np.ndarray:
    """Causal FIR bank with zero initial state, mean over bands, as one ``np.convolve`` per band and channel in
    ``np.longdouble``.  taps: (n_bands, n_taps) float64."""
    x = np.asarray(data).astype(np.longdouble)
    C, T = x.shape
    acc = np.zeros((C, T), dtype=np.longdouble)
    for h in np.asarray(taps).astype(np.longdouble):
        for c in range(C):
            acc[c] += np.convolve(x[c], h)[:T]
    return acc / np.longdouble(len(taps))


def scipy_fir_bank(data: np.ndarray, taps: np.ndarray) -> np.ndarray:
    """``scipy.signal.lfilter(h, 1, x)`` per band in float64, mean over bands (the reference's own call, :270-272)."""
    from scipy.signal import lfilter
    x = np.asarray(data, dtype=np.float64)
    acc = np.zeros_like(x)
    for h in taps:
        acc += lfilter(h, 1.0, x, axis=1)
    return acc / len(taps)


def band_cases(rng: np.random.Generator, C: int, T: int, offset: float = 0.0, scale: float = 1.0) -> np.ndarray:
    """(C, T) float64 recording for the band filters: noise of standard deviation ``scale`` on a DC level of ``offset``
    standard deviations; with C >= 3 the last channel is silent (exactly 0) and the one before it holds a constant
    non-zero level over its first third."""
    x = (rng.standard_normal((C, T)) + offset) * scale
    if C >= 3:
        x[-1] = 0.0
        x[-2, :T // 3] = (offset + 0.75) * scale
    return x


def rolling_cases(rng: np.random.Generator, C: int, T: int, W: int) -> np.ndarray:
    """(C, T) float64: noise with a DC offset, NaN stretches shorter and longer than W (windows holding 0 and 1
    valid values), constant stretches of 0.1 and 1/3 longer than W - one of them from t = 0 - and an exact zero run."""
    x = rng.standard_normal((C, T)) * 2.0 + 1.5
    L = W + 37
    for c in range(C):
        k = c % 4
        if k == 0:
            x[c, :L] = 0.1                                      # flat from the first sample
            x[c, T // 2:T // 2 + max(1, W // 3)] = np.nan       # shorter than the window
        elif k == 1:
            x[c, T // 3:T // 3 + L] = 1.0 / 3.0                 # flat mid-recording
            x[c, T // 2 + L:T // 2 + L + W + 5] = np.nan        # longer: empty windows, then single-valued ones
        elif k == 2:
            x[c, T // 4:T // 4 + L] = 0.1
            x[c, T // 4 + L + 3:T // 4 + L + 4] = np.nan
            x[c, -min(T // 5, L):] = 0.0
    return x
