"""Host restatements of the recording diagnostics (utils/diagnostics.py), for the tests of ``tl_welch_psd`` and
``tl_segment_moments``.

``welch_f64``     Welch's method in plain NumPy float64: segment, optional mean removal, window, ``rfft``, mean of ``|X|^2``,
                  scaling, one-sided doubling.  The host tests pin it to ``scipy.signal.welch`` and ``matplotlib.mlab.psd``.
``welch_ld``      the same quantity by a direct DFT in ``np.longdouble``: the twiddle angle is reduced exactly
                  (``k n mod n_fft``) and pi is a double plus its residual, so the table is good to the last bit of the long
                  double; sums run in long double.  This is what the kernels are measured against.
``moments_f64`` / ``moments_ld``   the same pair for the per-segment mean and population standard deviation.
``rel_err``       the error measure of the tests: per row, as a fraction of the row's largest reference value."""
import functools

import numpy as np

LD = np.longdouble
PI_LD = LD(np.pi) + LD(1.2246467991473532e-16)                # pi = the double nearest to it + the residual


def segments(T: int, nperseg: int, noverlap: int) -> int:
    return (T - noverlap) // (nperseg - noverlap)


def scale_of(window, fs, scaling: str, dtype=np.float64):
    w = np.asarray(window, dtype=dtype)
    return 1 / (dtype(fs) * (w * w).sum()) if scaling == "density" else 1 / w.sum() ** 2


def welch_f64(x, fs, window, noverlap: int, nfft: int, detrend: bool, scaling: str = "density"):
    """``psd (C, nfft / 2 + 1)`` float64; ``window`` holds the ``nperseg`` coefficients."""
    x = np.asarray(x, dtype=np.float64)
    w = np.asarray(window, dtype=np.float64)
    nperseg, step = w.shape[0], w.shape[0] - noverlap
    n_seg = segments(x.shape[1], nperseg, noverlap)
    seg = np.stack([x[:, s * step:s * step + nperseg] for s in range(n_seg)], axis=1)          # (C, n_seg, nperseg)
    if detrend:
        seg = seg - seg.mean(axis=-1, keepdims=True)
    X = np.fft.rfft(seg * w, n=nfft, axis=-1)
    p = (X.real ** 2 + X.imag ** 2) * scale_of(w, fs, scaling)
    p[..., 1:-1] *= 2.0
    return p.mean(axis=1)


@functools.lru_cache(maxsize=4)
def _dft_tables(nfft: int, nperseg: int):
    """cos, sin (nfft / 2 + 1, nperseg) long double of 2 pi k n / nfft, the product k n reduced mod nfft exactly."""
    t = (LD(2) * PI_LD / LD(nfft)) * np.arange(nfft, dtype=LD)
    c, s = np.cos(t), np.sin(t)
    idx = (np.arange(nfft // 2 + 1, dtype=np.int64)[:, None] * np.arange(nperseg, dtype=np.int64)[None, :]) % nfft
    return c[idx], s[idx]


def welch_ld(x, fs, window, noverlap: int, nfft: int, detrend: bool, scaling: str = "density"):
    """The same in long double by direct evaluation; float32 input is widened (exactly) first."""
    x = np.asarray(x).astype(LD)
    w = np.asarray(window, dtype=np.float64).astype(LD)
    nperseg, step = w.shape[0], w.shape[0] - noverlap
    n_seg = segments(x.shape[1], nperseg, noverlap)
    cos, sin = _dft_tables(nfft, nperseg)
    total = np.zeros((x.shape[0], nfft // 2 + 1), dtype=LD)
    for s in range(n_seg):
        seg = x[:, s * step:s * step + nperseg]
        if detrend:
            seg = seg - seg.sum(axis=1, keepdims=True) / LD(nperseg)
        seg = seg * w
        re, im = seg @ cos.T, seg @ sin.T
        total += re * re + im * im
    p = total / LD(n_seg) * scale_of(w, fs, scaling, dtype=LD)
    p[:, 1:-1] *= LD(2)
    return p


def moments_f64(x, s0: int, L: int, n_seg: int):
    seg = np.asarray(x, dtype=np.float64)[:, s0:s0 + n_seg * L].reshape(x.shape[0], n_seg, L)
    return seg.mean(axis=2), seg.std(axis=2)


def moments_ld(x, s0: int, L: int, n_seg: int):
    seg = np.asarray(x).astype(LD)[:, s0:s0 + n_seg * L].reshape(x.shape[0], n_seg, L)
    mean = seg.sum(axis=2) / LD(L)
    dev = seg - mean[:, :, None]
    return mean, np.sqrt((dev * dev).sum(axis=2) / LD(L))


def rel_err(got, ref_ld) -> float:
    """max over rows of max_k |got - ref| / max_k |ref|."""
    ref_ld = np.asarray(ref_ld, dtype=LD)
    err = np.abs(np.asarray(got).astype(LD) - ref_ld).max(axis=-1) / np.abs(ref_ld).max(axis=-1)
    return float(err.max())


def moments_err(mean, std, mean_ld, std_ld) -> float:
    """max over (channel, segment) of the error of the mean and of the std, as fractions of |mean| + std."""
    size = np.abs(mean_ld) + std_ld
    e1 = np.abs(np.asarray(mean).astype(LD) - mean_ld) / size
    e2 = np.abs(np.asarray(std).astype(LD) - std_ld) / size
    return float(max(e1.max(), e2.max()))
