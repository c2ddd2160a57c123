"""Recording diagnostics on the GPU: the arithmetic behind the reference's ``plot_psd`` (a Welch spectrum per channel, drawn
by ``plt.psd`` in a Python loop, utils/visualise.py:137) and ``plot_channel_mean_std`` (mean and standard deviation of every
channel per one-second segment, :176) - how one checks that a band-pass did what it should, where the line noise sits and
that no channel is dead or drifting, without downloading the recording.

``welch_psd``          ``scipy.signal.welch(axis=1, return_onesided=True, average='mean')`` of a (C, T) recording: two
                       launches of ``tl_welch_psd`` (csrc/tonal_mel.hip) on the LDS-resident fp64 transform of the mel front end.
``segment_mean_std``   mean and population std per channel and segment: ``tl_segment_moments`` (csrc/tonal_steps.hip), two-pass.
``summarise``          both, at their defaults, as the dict the preprocess stage writes per step (``diagnostics_dir``).

NumPy in (uploaded once) -> NumPy out; CUDA tensor in (read in place, a row-strided view included) -> CUDA tensors out on the
input's device - the rule of ``_lib.to_gpu``.  There is no CPU fallback."""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np

from .audio import MEL_BATCH_N_FFT, _hann, _stft_twiddles

#: the transform sizes ``tl_welch_psd`` is instantiated for: those of the mel front end
WELCH_N_FFT = MEL_BATCH_N_FFT

_SUPPORTED = ("supported: average='mean'; detrend='constant' or False; window 'hann', 'boxcar' or an array of nperseg "
              f"coefficients; scaling 'density' or 'spectrum'; even nfft in {WELCH_N_FFT}; one-sided output of real input")


def frames_per_workgroup(n_fft: int) -> int:
    """F: the segments a workgroup transforms side by side (1024 complex points of n_fft / 2 each)."""
    return 1024 // (n_fft // 2)


def plan_slabs(n_seg: int, n_fft: int, n_channels: int, n_cu: int = 256, slabs: Optional[int] = None) -> Tuple[int, int]:
    """``(n_slabs, trips)``: a channel's segments are cut into ``n_slabs`` runs of ``trips * F`` consecutive segments, one
    workgroup each (the last run may be short).  About four workgroups per compute unit over all channels, never more slabs
    than ``ceil(n_seg / F)`` and none without a segment; ``slabs`` overrides the count before that clamp."""
    if n_seg < 1 or n_channels < 1:
        raise ValueError("plan_slabs: n_seg and n_channels must be at least 1")
    F = frames_per_workgroup(n_fft)
    all_trips = -(-n_seg // F)
    want = -(-4 * n_cu // n_channels) if slabs is None else int(slabs)
    if want < 1:
        raise ValueError(f"the slab count must be at least 1 (got {want})")
    trips = -(-all_trips // min(want, all_trips))
    return -(-all_trips // trips), trips


def window_coefficients(window, nperseg: int) -> np.ndarray:
    """The ``nperseg`` float64 coefficients of a window given by name (``'hann'``: periodic, as scipy builds it for spectral
    analysis; ``'boxcar'``) or as an array of that length (``np.hanning(256)`` is matplotlib's)."""
    if isinstance(window, str):
        if window == "hann":
            return _hann(nperseg)
        if window == "boxcar":
            return np.ones(nperseg)
        raise ValueError(f"welch_psd: window '{window}' is not supported ({_SUPPORTED})")
    w = np.asarray(window, dtype=np.float64)
    if w.ndim != 1 or w.shape[0] != nperseg:
        raise ValueError(f"welch_psd: a window array must hold nperseg = {nperseg} coefficients (got shape {w.shape})")
    return w


def _on_device(data, what: str):
    """(C, T) float32 / float64 CUDA tensor with unit column stride and row stride >= T (kept as it is when it already is
    one), and whether the input was NumPy."""
    import torch
    from .. import _lib
    if not isinstance(data, torch.Tensor):
        data = np.asarray(data)
    if data.ndim != 2:
        raise ValueError(f"{what}: expected data of shape (n_channels, n_timepoints)")
    if np.iscomplexobj(data) if isinstance(data, np.ndarray) else data.is_complex():
        raise ValueError(f"{what}: complex input is not supported ({_SUPPORTED})")
    return _lib.to_gpu(data, what, rows="strided")


def _row_stride(x) -> int:
    return x.stride(0) if x.shape[0] > 1 else x.shape[1]


def welch_psd(data, fs: float = 1.0, window="hann", nperseg: int = 256, noverlap: Optional[int] = None,
              nfft: Optional[int] = None, detrend="constant", scaling: str = "density", *, return_onesided: bool = True,
              average: str = "mean", _slabs: Optional[int] = None):
    """``(freqs, psd)`` with the meaning of ``scipy.signal.welch(data, fs, window, nperseg, noverlap, nfft, detrend,
    return_onesided=True, scaling, axis=1, average='mean')``: ``freqs (nfft / 2 + 1)``, ``psd (C, nfft / 2 + 1)`` float64.
    float32 input is widened in registers and transformed in fp64 (scipy would transform it in float32).

    ``noverlap=None`` is ``nperseg // 2``; ``nfft=None`` is the smallest supported size >= ``nperseg``.  ``nperseg > T``
    raises (scipy shrinks the segment with a warning).  Median averaging, linear detrend, odd ``nfft``, two-sided output and
    complex input are refused by name.  ``_slabs`` overrides the number of slabs a channel's segments are cut into."""
    import torch
    from .. import _lib
    if average != "mean":
        raise ValueError(f"welch_psd: average='{average}' is not supported ({_SUPPORTED})")
    if not return_onesided:
        raise ValueError(f"welch_psd: two-sided output (return_onesided=False) is not supported ({_SUPPORTED})")
    if detrend in (False, None):
        detrend_code = 0
    elif detrend == "constant":
        detrend_code = 1
    else:
        raise ValueError(f"welch_psd: detrend={detrend!r} is not supported ({_SUPPORTED})")
    if scaling not in ("density", "spectrum"):
        raise ValueError(f"welch_psd: scaling='{scaling}' is not supported ({_SUPPORTED})")
    nperseg = int(nperseg)
    if nperseg < 2:
        raise ValueError(f"welch_psd: nperseg = {nperseg} must be at least 2")
    if nfft is None:
        fits = [n for n in WELCH_N_FFT if n >= nperseg]
        if not fits:
            raise ValueError(f"welch_psd: nperseg = {nperseg} exceeds the largest supported nfft ({_SUPPORTED})")
        nfft = fits[0]
    if nfft not in WELCH_N_FFT:
        kind = "odd nfft" if int(nfft) % 2 else "nfft"
        raise ValueError(f"welch_psd: {kind} = {nfft} is not supported ({_SUPPORTED})")
    nfft = int(nfft)
    if nperseg > nfft:
        raise ValueError(f"welch_psd: nfft = {nfft} must be at least nperseg = {nperseg}")
    noverlap = nperseg // 2 if noverlap is None else int(noverlap)
    if not 0 <= noverlap < nperseg:
        raise ValueError(f"welch_psd: noverlap = {noverlap} must lie in [0, nperseg = {nperseg})")
    w = window_coefficients(window, nperseg)
    shape = data.shape if hasattr(data, "shape") else np.asarray(data).shape
    if len(shape) == 2 and nperseg > shape[1]:
        raise ValueError(f"welch_psd: nperseg = {nperseg} is greater than the recording's {shape[1]} samples (not shrunk)")
    fs = float(fs)
    scale = 1.0 / (fs * float((w * w).sum())) if scaling == "density" else 1.0 / float(w.sum()) ** 2

    x, was_np = _on_device(data, "welch_psd")
    C, T = int(x.shape[0]), int(x.shape[1])
    if C < 1:
        raise ValueError("welch_psd: the recording holds no channel")
    dev = x.device
    n_seg = (T - noverlap) // (nperseg - noverlap)
    n_cu = torch.cuda.get_device_properties(dev).multi_processor_count
    n_slabs, _trips = plan_slabs(n_seg, nfft, C, n_cu=n_cu, slabs=_slabs)
    nb = nfft // 2 + 1
    win = np.zeros(nfft)
    win[:nperseg] = w
    win_d = torch.from_numpy(win).to(dev)
    tw = _stft_twiddles(str(dev), nfft)
    work = torch.empty(C, n_slabs, nb, dtype=torch.float64, device=dev)
    psd = torch.empty(C, nb, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().tl_welch_psd(x.data_ptr(), int(x.dtype == torch.float64), _row_stride(x), win_d.data_ptr(),
                                            tw.data_ptr(), work.data_ptr(), work.numel(), psd.data_ptr(), C, T, nfft, nperseg,
                                            noverlap, detrend_code, scale, n_seg, n_slabs, _lib.stream_ptr()), "tl_welch_psd")
    freqs = np.arange(nb) * (fs / nfft)
    if was_np:
        return freqs, psd.cpu().numpy()
    return torch.from_numpy(freqs).to(dev), psd


def _segment_moments(x, s0: int, L: int, n_seg: int):
    import torch
    from .. import _lib
    C, T = int(x.shape[0]), int(x.shape[1])
    mean = torch.empty(C, n_seg, dtype=torch.float64, device=x.device)
    std = torch.empty(C, n_seg, dtype=torch.float64, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().tl_segment_moments(x.data_ptr(), int(x.dtype == torch.float64), _row_stride(x), mean.data_ptr(),
                                                  std.data_ptr(), C, T, s0, L, n_seg, _lib.stream_ptr()), "tl_segment_moments")
    return mean, std


def segment_range(n_timepoints: int, sampling_rate, start: float, end: float) -> Tuple[int, int, int]:
    """``(first sample, L, n_segments)`` of ``segment_mean_std``; ``ValueError`` for a range that leaves the recording."""
    L, n_seg, s0 = int(sampling_rate), int(end - start), int(start * sampling_rate)
    if L < 1:
        raise ValueError(f"segment_mean_std: sampling_rate = {sampling_rate} gives segments of no sample")
    if n_seg < 1:
        raise ValueError(f"segment_mean_std: [start, end) = [{start}, {end}) holds no whole second")
    if s0 < 0 or s0 + n_seg * L > n_timepoints:
        raise ValueError(f"segment_mean_std: samples [{s0}, {s0 + n_seg * L}) of the range [{start}, {end}) s run past the "
                         f"recording's {n_timepoints} samples")
    return s0, L, n_seg


def segment_mean_std(data, sampling_rate, start: float = 0.0, end: float = 30.0):
    """``(means, stds)``, each ``(C, n_segments)`` float64: mean and population standard deviation (``np.std``) of every
    channel over one-second segments.  ``L = int(sampling_rate)`` samples a segment, ``n_segments = int(end - start)``, and
    segment ``i`` covers the samples ``[int(start * sampling_rate) + i L, ... + L)``.

    The reference's own loop (utils/visualise.py:212-215) indexes with ``start + i * segment_length``: a float under the
    default ``start=0.0``, and seconds mixed with samples, so it raises as written; the definition above is what its
    docstring and axis labels describe.  A range that runs past the recording raises ``ValueError``."""
    shape = data.shape if hasattr(data, "shape") else np.asarray(data).shape
    if len(shape) != 2:
        raise ValueError("segment_mean_std: expected data of shape (n_channels, n_timepoints)")
    s0, L, n_seg = segment_range(int(shape[1]), sampling_rate, start, end)
    x, was_np = _on_device(data, "segment_mean_std")
    mean, std = _segment_moments(x, s0, L, n_seg)
    return (mean.cpu().numpy(), std.cpu().numpy()) if was_np else (mean, std)


def summarise(data, signal_freq) -> dict:
    """What the preprocess stage writes per step: ``freqs``, ``psd`` (``welch_psd`` at its defaults, ``fs = signal_freq``),
    ``seg_mean``, ``seg_std`` (all whole seconds of the recording) and ``signal_freq``, as NumPy arrays - only these small
    arrays leave the device.  A recording shorter than 256 samples has no ``freqs`` / ``psd``, one shorter than a second no
    ``seg_mean`` / ``seg_std``."""
    out = {"signal_freq": np.asarray(signal_freq)}
    x, _was_np = _on_device(data, "diagnostics")
    T = int(x.shape[1])
    if x.shape[0] >= 1 and T >= 256:
        freqs, psd = welch_psd(x, fs=float(signal_freq))
        out["freqs"], out["psd"] = freqs.cpu().numpy(), psd.cpu().numpy()
    L = int(signal_freq)
    if x.shape[0] >= 1 and L >= 1 and T // L >= 1:
        mean, std = _segment_moments(x, 0, L, T // L)
        out["seg_mean"], out["seg_std"] = mean.cpu().numpy(), std.cpu().numpy()
    return out
