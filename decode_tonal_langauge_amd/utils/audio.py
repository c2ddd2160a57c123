"""Audio <-> mel-spectrogram helpers (mirror of reference utils/audio.py:7-87), without librosa.

The reference delegates to ``librosa.feature.melspectrogram`` + ``librosa.power_to_db`` (``audio_to_mel``, :36-43) and to
``librosa.db_to_power`` + ``librosa.feature.inverse.mel_to_audio`` (``mel_to_audio``, :76-87).  librosa is a third-party
dependency that is neither vendored in the reference nor installable in this image, so this module RESTATES the published
algorithms of librosa 0.10 with NumPy / SciPy:

* STFT: ``n_fft`` 2048, ``hop_length`` n_fft / 4 = 512 by default, periodic Hann window, ``center=True`` with zero
  ("constant") padding, power spectrogram ``|S|^2``;
* mel filter bank: Slaney scale (linear below 1 kHz, logarithmic above; ``htk=False``), triangular filters with area
  normalisation (``norm='slaney'``), ``fmin`` 0, ``fmax`` sr / 2, 128 bands by default;
* ``power_to_db(S, ref=np.max)``: ``10 log10(max(S, 1e-10)) - 10 log10(max(ref, 1e-10))`` clipped at ``top_db`` = 80 below the peak;
* inverse: ``db_to_power`` (``ref * 10^(dB / 10)``), mel -> linear magnitude by non-negative least squares against the
  filter bank, Griffin-Lim with momentum 0.99 and 32 iterations from random phases.

**Parity unpinned**: the reference holds no golden vector for these calls and librosa cannot be imported here to make one;
the tests check the published properties (filter-bank partition / normalisation, dB reference and floor, a tone landing in
its band, spectral convergence of the inversion).  This is CPU host code beside the hot path: the
synthesis trainer consumes its output (mel targets), nothing here runs per train step.
"""
from __future__ import annotations

import functools
from typing import NamedTuple, Optional

import numpy as np


# ------------------------------------------------------------------------------------------ mel scale (Slaney)
def _hz_to_mel(f):
    f = np.asarray(f, dtype=np.float64)
    f_sp = 200.0 / 3
    mels = f / f_sp
    min_log_hz, logstep = 1000.0, np.log(6.4) / 27.0
    min_log_mel = min_log_hz / f_sp
    return np.where(f >= min_log_hz, min_log_mel + np.log(np.maximum(f, 1e-300) / min_log_hz) / logstep, mels)


def _mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    f_sp = 200.0 / 3
    min_log_hz, logstep = 1000.0, np.log(6.4) / 27.0
    min_log_mel = min_log_hz / f_sp
    return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)


def mel_filterbank(sr: float, n_fft: int, n_mels: int = 128, fmin: float = 0.0, fmax: Optional[float] = None) -> np.ndarray:
    """(n_mels, 1 + n_fft // 2) triangular filters on the Slaney mel scale, each normalised to unit area in Hz."""
    fmax = sr / 2.0 if fmax is None else fmax
    fft_f = np.linspace(0.0, sr / 2.0, 1 + n_fft // 2)
    mel_f = _mel_to_hz(np.linspace(_hz_to_mel(fmin), _hz_to_mel(fmax), n_mels + 2))
    fdiff = np.diff(mel_f)
    ramps = mel_f[:, None] - fft_f[None, :]
    lower = -ramps[:-2] / fdiff[:-1, None]
    upper = ramps[2:] / fdiff[1:, None]
    w = np.maximum(0.0, np.minimum(lower, upper))
    w *= (2.0 / (mel_f[2:n_mels + 2] - mel_f[:n_mels]))[:, None]
    return w.astype(np.float32)


# ------------------------------------------------------------------------------------------ STFT
def _hann(n: int) -> np.ndarray:
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n) / n)          # periodic ("fftbins=True")


def _padded_window(n_fft: int, win_length: int) -> np.ndarray:
    """The Hann window of ``win_length`` samples centred in ``n_fft``, zeros around it."""
    win = np.zeros(n_fft)
    off = (n_fft - win_length) // 2
    win[off:off + win_length] = _hann(win_length)
    return win


def stft(y: np.ndarray, n_fft: int = 2048, hop_length: Optional[int] = None, win_length: Optional[int] = None,
         center: bool = True) -> np.ndarray:
    hop = n_fft // 4 if hop_length is None else int(hop_length)
    win = _padded_window(n_fft, n_fft if win_length is None else int(win_length))
    y = np.asarray(y, dtype=np.float64)
    if center:
        y = np.pad(y, n_fft // 2, mode="constant")
    if y.shape[0] < n_fft:
        raise ValueError(f"audio of {y.shape[0]} samples is shorter than n_fft = {n_fft}")
    n_frames = 1 + (y.shape[0] - n_fft) // hop
    idx = np.arange(n_fft)[:, None] + hop * np.arange(n_frames)[None, :]
    return np.fft.rfft(y[idx] * win[:, None], axis=0)                    # (1 + n_fft // 2, n_frames)


def istft(S: np.ndarray, hop_length: Optional[int] = None, win_length: Optional[int] = None, center: bool = True,
          length: Optional[int] = None) -> np.ndarray:
    n_fft = 2 * (S.shape[0] - 1)
    hop = n_fft // 4 if hop_length is None else int(hop_length)
    win = _padded_window(n_fft, n_fft if win_length is None else int(win_length))
    frames = np.fft.irfft(S, n=n_fft, axis=0) * win[:, None]
    n_frames = S.shape[1]
    out = np.zeros(n_fft + hop * (n_frames - 1))
    wsum = np.zeros_like(out)
    for t in range(n_frames):
        out[t * hop:t * hop + n_fft] += frames[:, t]
        wsum[t * hop:t * hop + n_fft] += win ** 2
    nz = wsum > np.finfo(np.float32).tiny
    out[nz] /= wsum[nz]
    if center:
        out = out[n_fft // 2:len(out) - n_fft // 2] if length is None else out[n_fft // 2:n_fft // 2 + length]
    elif length is not None:
        out = out[:length]
    return out


# ------------------------------------------------------------------------------------------ dB
def power_to_db(S: np.ndarray, ref=1.0, amin: float = 1e-10, top_db: Optional[float] = 80.0) -> np.ndarray:
    S = np.asarray(S)
    ref_value = ref(S) if callable(ref) else np.abs(ref)
    log_spec = 10.0 * np.log10(np.maximum(amin, S)) - 10.0 * np.log10(np.maximum(amin, ref_value))
    if top_db is not None:
        log_spec = np.maximum(log_spec, log_spec.max() - top_db)
    return log_spec


def db_to_power(S_db: np.ndarray, ref: float = 1.0) -> np.ndarray:
    return ref * np.power(10.0, 0.1 * np.asarray(S_db))


# ------------------------------------------------------------------------------------------ the reference's two functions
def _split_kwargs(kw: Optional[dict]):
    kw = dict(kw or {})
    stft_kw = {k: kw.pop(k) for k in ("n_fft", "hop_length", "win_length", "center") if k in kw}
    power = kw.pop("power", 2.0)
    mel_kw = {k: kw.pop(k) for k in ("n_mels", "fmin", "fmax") if k in kw}
    if kw:
        raise TypeError(f"unsupported mel keyword(s) {sorted(kw)} (supported: n_fft, hop_length, win_length, center, "
                        "power, n_mels, fmin, fmax)")
    return stft_kw, power, mel_kw


def audio_to_mel(audio: np.ndarray, audio_sampling_rate: int, mel_in_db: bool = True,
                 mel_kwargs: Optional[dict] = None) -> np.ndarray:
    """Mel spectrogram of a 1-D signal, flattened to (n_mels * n_frames,) - reference utils/audio.py:7-43."""
    audio = np.asarray(audio)
    if audio.ndim > 1:
        raise ValueError("Audio input must be a 1D array.")
    stft_kw, power, mel_kw = _split_kwargs(mel_kwargs)
    n_fft = stft_kw.get("n_fft", 2048)
    S = np.abs(stft(audio, **{"n_fft": n_fft, **{k: v for k, v in stft_kw.items() if k != "n_fft"}})) ** power
    mel = mel_filterbank(audio_sampling_rate, n_fft, **mel_kw).astype(np.float64) @ S
    if mel_in_db:
        mel = power_to_db(mel, ref=np.max)
    return mel.astype(np.float32).reshape(-1)


# ------------------------------------------------------------------------------------------ the same, a batch on the GPU
MEL_BATCH_N_FFT = (256, 512, 1024, 2048)


def pack_mel_filterbank(fb: np.ndarray):
    """A dense (n_mels, n_bins) bank as per-band runs: ``bands`` (n_mels, 3) int32 = first bin, one past the last non-zero
    bin, offset of the run in ``weights`` (float64, the float32 values widened).  A triangle touches a short run of bins."""
    bands = np.zeros((fb.shape[0], 3), dtype=np.int32)
    runs, off = [], 0
    for m, row in enumerate(fb):
        nz = np.flatnonzero(row)
        first, last = (int(nz[0]), int(nz[-1]) + 1) if nz.size else (0, 0)
        bands[m] = (first, last, off)
        runs.append(row[first:last].astype(np.float64))
        off += last - first
    return bands, (np.concatenate(runs) if off else np.zeros(0))


def _upload(a: np.ndarray, device):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


@functools.lru_cache(maxsize=8)
def _stft_twiddles(device: str, n_fft: int):
    """Device copy of the full-circle twiddles (cos, -sin)(2 pi i / n_fft) every kernel of csrc/tonal_mel.hip reads."""
    ang = 2.0 * np.pi * np.arange(n_fft) / n_fft
    return _upload(np.stack([np.cos(ang), -np.sin(ang)], axis=1), device)


@functools.lru_cache(maxsize=8)
def _stft_batch_tables(device: str, n_fft: int, win_length: int):
    """Device copies of the window (as ``stft`` builds it) and the twiddles."""
    return _upload(_padded_window(n_fft, win_length), device), _stft_twiddles(device, n_fft)


@functools.lru_cache(maxsize=8)
def _mel_batch_tables(device: str, sr: float, n_fft: int, win_length: int, n_mels: int, fmin: float, fmax: Optional[float]):
    """Device copies of the per-call tables of ``tl_mel_power``: window (as ``stft`` builds it), twiddles, packed bank."""
    win, tw = _stft_batch_tables(device, n_fft, win_length)
    bands, weights = pack_mel_filterbank(mel_filterbank(sr, n_fft, n_mels=n_mels, fmin=fmin, fmax=fmax))
    up = lambda a: _upload(a, device)
    # an empty tensor has no device pointer: keep one weight so the entry point always gets an address
    return win, tw, up(bands), up(weights if weights.size else np.zeros(1)), int(weights.size)


def audio_to_mel_batch(audio, audio_sampling_rate: int, mel_in_db: bool = True, mel_kwargs: Optional[dict] = None,
                       device=None):
    """``audio_to_mel`` of every row of an (N, S) batch in two kernel launches (``tl_mel_power``, ``tl_mel_finish``): row n of
    the (N, n_mels * n_frames) float32 result is ``audio_to_mel(audio[n], ...)`` up to float32 rounding, the dB reference
    being each trial's own maximum.  NumPy in (float32 / float64 kept, anything else becomes float64) -> NumPy out; CUDA
    tensor in -> CUDA tensor out on its device.  ``n_fft`` must be one of ``MEL_BATCH_N_FFT``.  No CPU fallback."""
    import torch
    from .. import _lib
    is_tensor = isinstance(audio, torch.Tensor)
    if not is_tensor:
        audio = np.asarray(audio)
    if audio.ndim != 2:
        raise ValueError("Audio input must be a 2D array (trials, samples).")
    stft_kw, power, mel_kw = _split_kwargs(mel_kwargs)
    n_fft, hop, wl = _check_stft_args(stft_kw.get("n_fft", 2048), stft_kw.get("hop_length"), stft_kw.get("win_length"))
    center = bool(stft_kw.get("center", True))
    n_mels = int(mel_kw.get("n_mels", 128))
    if power not in (1, 2):
        raise ValueError(f"power = {power} is not supported on the GPU (supported: 1, 2)")
    if n_mels < 1:
        raise ValueError(f"n_mels = {n_mels} must be at least 1")
    N, S = int(audio.shape[0]), int(audio.shape[1])
    if N < 1:
        raise ValueError("Audio input holds no trial.")
    padded = S + n_fft if center else S
    if padded < n_fft or S < 1:
        raise ValueError(f"audio of {padded} samples is shorter than n_fft = {n_fft}")
    n_frames = 1 + (padded - n_fft) // hop

    x, _ = _lib.to_gpu(audio, "audio_to_mel_batch", device=device, rows="strided")
    dev = x.device
    fmax = mel_kw.get("fmax")
    win, tw, bands, weights, n_weights = _mel_batch_tables(
        str(dev), float(audio_sampling_rate), n_fft, wl, n_mels, float(mel_kw.get("fmin", 0.0)),
        None if fmax is None else float(fmax))
    work = torch.empty(N, n_mels, n_frames, dtype=torch.float64, device=dev)
    rowmax = torch.empty(N, dtype=torch.float64, device=dev)
    out = torch.empty(N, n_mels * n_frames, dtype=torch.float32, device=dev)
    lib = _lib.load()
    with torch.cuda.device(dev):
        _lib.check(lib.tl_mel_power(x.data_ptr(), int(x.dtype == torch.float64), x.stride(0) if N > 1 else S, win.data_ptr(),
                                    tw.data_ptr(), bands.data_ptr(), weights.data_ptr(), n_weights, work.data_ptr(),
                                    rowmax.data_ptr(), N, S, n_fft, wl, hop, int(center), int(power), n_mels, n_frames,
                                    _lib.stream_ptr()), "tl_mel_power")
        _lib.check(lib.tl_mel_finish(work.data_ptr(), rowmax.data_ptr(), out.data_ptr(), N, n_mels, n_frames,
                                     int(bool(mel_in_db)), _lib.stream_ptr()), "tl_mel_finish")
    return out if is_tensor else out.cpu().numpy()


# ------------------------------------------------------------------------------------------ mel -> linear spectrum
#: FISTA iterations of ``mel_to_linear`` / ``tl_mel_invert``: the smallest count of the CPU sweep in profiles/mel_inverse.md
#: whose per-frame relative residual exceeds ``scipy.optimize.nnls``'s by at most 1e-5 on every input of that sweep
NNLS_ITER_DEFAULT = 1000


def _bank_lipschitz(fb: np.ndarray) -> float:
    """Largest eigenvalue of ``fb^T fb``: the Lipschitz constant of the gradient of ``||fb x - p||^2 / 2``."""
    return float(np.linalg.svd(np.asarray(fb, dtype=np.float64), compute_uv=False)[0]) ** 2


def fista_momentum(nnls_iter: int) -> np.ndarray:
    """``beta_k = (t_k - 1) / t_{k+1}`` of the standard sequence ``t_1 = 1``, ``t_{k+1} = (1 + sqrt(1 + 4 t_k^2)) / 2``."""
    beta, t = np.empty(int(nnls_iter)), 1.0
    for k in range(int(nnls_iter)):
        t_new = 0.5 * (1.0 + np.sqrt(1.0 + 4.0 * t * t))
        beta[k] = (t - 1.0) / t_new
        t = t_new
    return beta


def bank_operators(fb: np.ndarray):
    """``apply(z)`` = ``fb @ z`` and ``transposed(r)`` = ``fb.T @ r`` of a triangular bank with the order of operations written
    out, every product and every sum rounded on its own: a band's sum runs over its bins ``[first, last)`` as four interleaved
    partial sums (bins ``first + s, first + s + 4, ...``, each in rising order) combined as ``(s0 + s1) + (s2 + s3)``; a bin's
    gradient is ``w0 r[b0] + w1 r[b1]`` over the at most two bands that cover it.  ``tl_mel_invert`` computes exactly this."""
    fb = np.asarray(fb, dtype=np.float64)
    bands, weights = pack_mel_filterbank(fb)
    bin_bands, bin_weights = bin_pair_table(fb)
    first, last, off = bands[:, 0], bands[:, 1], bands[:, 2]
    steps = int(-(-max(int((last - first).max()), 1) // 4))
    k = first[None, None, :] + np.arange(4)[None, :, None] + 4 * np.arange(steps)[:, None, None]       # (steps, 4, n_mels)
    live = k < last[None, None, :]
    idx = np.where(live, k, 0)
    wt = np.where(live, np.append(weights, 0.0)[np.where(live, off[None, None, :] + k - first[None, None, :], weights.size)], 0.0)
    b = np.maximum(bin_bands, 0)
    w0, w1 = bin_weights[:, 0, None], bin_weights[:, 1, None]

    def apply(z):
        acc = np.zeros((4, fb.shape[0], z.shape[1]))
        for j in range(steps):
            acc = acc + wt[j][:, :, None] * z[idx[j]]
        return (acc[0] + acc[1]) + (acc[2] + acc[3])

    def transposed(r):
        return w0 * r[b[:, 0]] + w1 * r[b[:, 1]]

    return apply, transposed


def mel_to_linear(mel_power: np.ndarray, fb: np.ndarray, nnls_iter: int = NNLS_ITER_DEFAULT, _perturb=None) -> np.ndarray:
    """``min_{x >= 0} ||fb x - p_t||^2`` for every column ``p_t`` of ``mel_power`` (n_mels, T) by accelerated projected
    gradient (FISTA) from ``x = 0``: step ``1 / L`` with ``L`` the squared largest singular value of ``fb``, the standard
    ``t_k`` momentum sequence, ``nnls_iter`` iterations, float64.  Returns (n_bins, T).  ``fb`` must be a triangular bank (at
    most two bands per bin).  This NumPy form states the method of ``tl_mel_invert`` down to the order of its sums
    (``bank_operators``), so the kernel reproduces it bit for bit: the projection and, downstream, the square root make the
    solve sensitive to rounding at the 1e-7 level of the final waveform, and an oracle that rounds differently could not be
    compared there.  It is the oracle of the tests; ``mel_to_audio_batch`` never calls it.  ``_perturb(grad)`` is for the
    sensitivity measurements of scripts/mel_inverse_sweep.py."""
    fb = np.asarray(fb, dtype=np.float64)
    p = np.asarray(mel_power, dtype=np.float64)
    if p.ndim != 2 or p.shape[0] != fb.shape[0]:
        raise ValueError(f"mel_power must be (n_mels = {fb.shape[0]}, T), got {p.shape}")
    if nnls_iter < 1:
        raise ValueError(f"nnls_iter = {nnls_iter} must be at least 1")
    step = 1.0 / _bank_lipschitz(fb)
    apply, transposed = bank_operators(fb)
    x = np.zeros((fb.shape[1], p.shape[1]))
    z = x
    for beta in fista_momentum(nnls_iter):
        grad = transposed(apply(z) - p)
        if _perturb is not None:
            grad = _perturb(grad)
        x_new = np.maximum(z - step * grad, 0.0)
        z = x_new + beta * (x_new - x)
        x = x_new
    return x


def griffinlim(mag: np.ndarray, n_iter: int = 32, hop_length: Optional[int] = None, win_length: Optional[int] = None,
               momentum: float = 0.99, seed: int = 0, length: Optional[int] = None) -> np.ndarray:
    """Fast Griffin-Lim (Perraudin et al. 2013) from random initial phases."""
    rng = np.random.default_rng(seed)
    angles = np.exp(2j * np.pi * rng.random(mag.shape))
    n_fft = 2 * (mag.shape[0] - 1)
    rebuilt = tprev = None
    for _ in range(n_iter):
        inverse = istft(mag * angles, hop_length=hop_length, win_length=win_length, length=length)
        rebuilt = stft(inverse, n_fft=n_fft, hop_length=hop_length, win_length=win_length)
        rebuilt = rebuilt[:, :mag.shape[1]] if rebuilt.shape[1] >= mag.shape[1] else \
            np.pad(rebuilt, ((0, 0), (0, mag.shape[1] - rebuilt.shape[1])))
        angles = rebuilt - (momentum / (1 + momentum)) * tprev if tprev is not None else rebuilt.copy()
        angles /= np.abs(angles) + 1e-16
        tprev = rebuilt
    return istft(mag * angles, hop_length=hop_length, win_length=win_length, length=length)


def _inverse_kwargs(kwargs: dict, **extra) -> dict:
    """The keywords of ``mel_to_audio`` (and ``extra``: name = default) with their defaults; any other is a ``TypeError``."""
    defaults = dict(n_fft=2048, hop_length=None, win_length=None, power=2.0, n_iter=32, length=None, seed=0, fmin=0.0,
                    fmax=None, **extra)
    kw = {k: kwargs.pop(k, d) for k, d in defaults.items()}
    if kwargs:
        raise TypeError(f"unsupported keyword(s) {sorted(kwargs)}")
    return kw


def mel_to_audio(mel: np.ndarray, n_mels: int, audio_sampling_rate: int = 24414, mel_in_db: bool = True, **kwargs) -> np.ndarray:
    """Waveform from a flattened mel spectrogram by NNLS mel inversion + Griffin-Lim - reference utils/audio.py:46-87."""
    mel = np.asarray(mel, dtype=np.float64).reshape(n_mels, -1)
    if mel_in_db:
        mel = db_to_power(mel, ref=0.0001)
    from scipy.optimize import nnls                  # here, its one use: importing this module (utils/diagnostics.py does) stays light
    kw = _inverse_kwargs(kwargs)
    fb = mel_filterbank(audio_sampling_rate, kw["n_fft"], n_mels=n_mels, fmin=kw["fmin"], fmax=kw["fmax"]).astype(np.float64)
    lin = np.stack([nnls(fb, mel[:, t])[0] for t in range(mel.shape[1])], axis=1)      # power (or magnitude^power) spectrum
    mag = np.power(np.maximum(lin, 0.0), 1.0 / kw["power"])
    return griffinlim(mag, n_iter=kw["n_iter"], hop_length=kw["hop_length"], win_length=kw["win_length"], seed=kw["seed"],
                      length=kw["length"]).astype(np.float32)


# ------------------------------------------------------------------------------------------ the way back, a batch on the GPU
#: Griffin-Lim workspace (frames, angles, tprev, the frame-major magnitudes) of one chunk of trials stays under this
GL_WORKSPACE_BYTES = 1 << 30
MEL_INVERT_MAX_MELS = 256


def bin_pair_table(fb: np.ndarray):
    """A dense (n_mels, n_bins) bank by bin: ``bin_bands`` (n_bins, 2) int32 = the at most two bands whose triangles cover
    the bin (-1 = none), ``bin_weights`` (n_bins, 2) float64 their weights - what ``fb.T @ r`` needs per bin."""
    fb = np.asarray(fb)
    bin_bands = np.full((fb.shape[1], 2), -1, dtype=np.int32)
    bin_weights = np.zeros((fb.shape[1], 2))
    for k in range(fb.shape[1]):
        nz = np.flatnonzero(fb[:, k])
        if nz.size > 2:
            raise ValueError(f"bin {k} lies in {nz.size} bands; a triangular mel bank covers a bin with at most two")
        bin_bands[k, :nz.size] = nz
        bin_weights[k, :nz.size] = fb[nz, k]
    return bin_bands, bin_weights


@functools.lru_cache(maxsize=8)
def _mel_inverse_tables(device: str, sr: float, n_fft: int, n_mels: int, fmin: float, fmax: Optional[float]):
    """What ``tl_mel_invert`` needs beside the packed bank of ``_mel_batch_tables``: the bank by bin and the step 1 / L."""
    fb = mel_filterbank(sr, n_fft, n_mels=n_mels, fmin=fmin, fmax=fmax)
    bin_bands, bin_weights = bin_pair_table(fb)
    return _upload(bin_bands, device), _upload(bin_weights, device), 1.0 / _bank_lipschitz(fb)


@functools.lru_cache(maxsize=4)
def _fista_momentum_table(device: str, nnls_iter: int):
    return _upload(fista_momentum(nnls_iter), device)


def _batch_on_gpu(a, device, what: str):
    """``a`` (NumPy array or tensor) as a contiguous float64 CUDA tensor, by the container rules of ``audio_to_mel_batch``."""
    import torch
    from .. import _lib
    if not isinstance(a, torch.Tensor):
        a = np.asarray(a, dtype=np.float64)
    return _lib.to_gpu(a, what, device=device)[0].double()


def _check_stft_args(n_fft, hop_length, win_length, inverse: bool = False):
    """(n_fft, hop, win_length) as ints, or the refusal every batch entry gives; ``inverse`` also refuses a hop that leaves
    gaps between the windows."""
    if n_fft not in MEL_BATCH_N_FFT:
        raise ValueError(f"n_fft = {n_fft} is not supported on the GPU (supported: {', '.join(map(str, MEL_BATCH_N_FFT))})")
    n_fft = int(n_fft)
    hop = n_fft // 4 if hop_length is None else int(hop_length)
    wl = n_fft if win_length is None else int(win_length)
    if not 1 <= wl <= n_fft:
        raise ValueError(f"win_length = {wl} must lie in [1, n_fft = {n_fft}]")
    if hop < 1:
        raise ValueError(f"hop_length = {hop} must be at least 1")
    if inverse and hop > wl:
        raise ValueError(f"hop_length = {hop} > win_length = {wl} leaves gaps in the window-square sum of the inverse STFT")
    return n_fft, hop, wl


def griffinlim_batch(mag, n_iter: int = 32, hop_length: Optional[int] = None, win_length: Optional[int] = None,
                     momentum: float = 0.99, seed: int = 0, length: Optional[int] = None, device=None):
    """``griffinlim`` of every trial of an (N, n_bins, T) batch on the GPU: row n of the (N, samples) float64 result is
    ``griffinlim(mag[n], ..., seed=seed)`` up to fp64 rounding.  All trials start from the one (n_bins, T) phase table the
    host function draws from ``default_rng(seed)``.  Per iteration one ``tl_gl_synth`` and one ``tl_gl_analyse`` launch, then
    ``tl_gl_synth`` + ``tl_gl_overlap_add``; trials go in chunks whose workspace stays under 1 GiB.  NumPy in -> NumPy out,
    CUDA tensor in -> CUDA tensor out.  ``n_fft = 2 (n_bins - 1)`` must be one of ``MEL_BATCH_N_FFT`` and
    ``hop_length <= win_length``.  No CPU fallback."""
    import torch
    from .. import _lib
    is_tensor = isinstance(mag, torch.Tensor)
    if not is_tensor:
        mag = np.asarray(mag)
    if mag.ndim != 3:
        raise ValueError("Magnitude input must be a 3D array (trials, bins, frames).")
    N, n_bins, T = (int(v) for v in mag.shape)
    n_fft, hop, wl = _check_stft_args(2 * (n_bins - 1), hop_length, win_length, inverse=True)
    if N < 1 or T < 1:
        raise ValueError("Magnitude input holds no trial or no frame.")
    if n_iter < 0:
        raise ValueError(f"n_iter = {n_iter} must not be negative")
    if length is not None and length < 0:
        raise ValueError(f"length = {length} must not be negative")
    # what istft keeps after the centre trim: hop (T - 1) samples, or the first `length` of the n_fft / 2 + hop (T - 1) it has
    L = hop * (T - 1) if length is None else min(int(length), n_fft // 2 + hop * (T - 1))
    x = _batch_on_gpu(mag, device, "griffinlim_batch")
    dev = x.device
    out = torch.empty(N, L, dtype=torch.float64, device=dev)
    if L > 0:
        win, tw = _stft_batch_tables(str(dev), n_fft, wl)
        phases = np.exp(2j * np.pi * np.random.default_rng(seed).random((n_bins, T)))      # as griffinlim draws them
        phase0 = _upload(np.ascontiguousarray(phases.T).view(np.float64).reshape(T, n_bins, 2), dev)
        w2 = _padded_window(n_fft, wl) ** 2
        wsum_host = np.zeros(n_fft + hop * (T - 1))
        for t in range(T):                                                                 # the additions of istft, in its order
            wsum_host[t * hop:t * hop + n_fft] += w2
        wsum = _upload(wsum_host, dev)
        per_trial = T * (8 * n_fft + 8 * n_bins + 2 * 16 * n_bins)
        chunk = max(1, min(N, 65535, GL_WORKSPACE_BYTES // per_trial))
        frames = torch.empty(chunk, T, n_fft, dtype=torch.float64, device=dev)
        angles = torch.empty(chunk, T, n_bins, 2, dtype=torch.float64, device=dev)
        tprev = torch.empty_like(angles)
        lib = _lib.load()
        with torch.cuda.device(dev):
            for c0 in range(0, N, chunk):
                c = min(chunk, N - c0)
                mag_t = x[c0:c0 + c].transpose(1, 2).contiguous()                          # frame-major, as the kernels read it
                src, shared = phase0, 1
                for it in range(int(n_iter) + 1):
                    _lib.check(lib.tl_gl_synth(mag_t.data_ptr(), src.data_ptr(), shared, win.data_ptr(), tw.data_ptr(),
                                               frames.data_ptr(), c, n_fft, T, _lib.stream_ptr()), "tl_gl_synth")
                    if it == n_iter:
                        break
                    _lib.check(lib.tl_gl_analyse(frames.data_ptr(), wsum.data_ptr(), win.data_ptr(), tw.data_ptr(),
                                                 angles.data_ptr(), tprev.data_ptr(), c, n_fft, wl, hop, T, L, float(momentum),
                                                 int(it == 0), _lib.stream_ptr()), "tl_gl_analyse")
                    src, shared = angles, 0
                _lib.check(lib.tl_gl_overlap_add(frames.data_ptr(), wsum.data_ptr(), out[c0:c0 + c].data_ptr(), c, n_fft, wl,
                                                 hop, T, L, _lib.stream_ptr()), "tl_gl_overlap_add")
    return out if is_tensor else out.cpu().numpy()


def mel_invert_batch(mel_power, audio_sampling_rate: float, n_fft: int, n_mels: int, fmin: float = 0.0,
                     fmax: Optional[float] = None, nnls_iter: int = NNLS_ITER_DEFAULT, power: int = 2):
    """``tl_mel_invert`` on a contiguous float64 CUDA tensor (N, n_mels, T) of mel power: (N, n_bins, T) =
    ``mel_to_linear(mel_power[n], fb, nnls_iter) ** (1 / power)`` for the bank of these arguments."""
    import torch
    from .. import _lib
    _lib.require_gpu(mel_power, "mel_invert_batch")
    N, _, T = mel_power.shape
    dev = mel_power.device
    fmax = None if fmax is None else float(fmax)
    sr = float(audio_sampling_rate)
    _, _, bands, weights, n_weights = _mel_batch_tables(str(dev), sr, n_fft, n_fft, n_mels, float(fmin), fmax)
    bin_bands, bin_weights, step = _mel_inverse_tables(str(dev), sr, n_fft, n_mels, float(fmin), fmax)
    momentum = _fista_momentum_table(str(dev), int(nnls_iter))
    p = mel_power.double().contiguous()
    mag = torch.empty(N, n_fft // 2 + 1, T, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().tl_mel_invert(p.data_ptr(), bands.data_ptr(), weights.data_ptr(), n_weights, bin_bands.data_ptr(),
                                             bin_weights.data_ptr(), momentum.data_ptr(), mag.data_ptr(), N, n_fft, n_mels, T, int(nnls_iter),
                                             step,
                                             int(power), _lib.stream_ptr()), "tl_mel_invert")
    return mag


def mel_to_audio_batch(mels, n_mels: int, audio_sampling_rate: int = 24414, mel_in_db: bool = True, device=None, **kwargs):
    """Waveforms of an (N, n_mels * T) batch of flattened mel spectrograms on the GPU: ``db_to_power(., ref=1e-4)`` ->
    ``tl_mel_invert`` (the FISTA solve ``mel_to_linear`` states, ``nnls_iter`` iterations) -> ``griffinlim_batch``; returns
    (N, samples) float32.  Keywords are those of ``mel_to_audio`` (n_fft, hop_length, win_length, power, n_iter, length, seed,
    fmin, fmax) plus ``nnls_iter``.  NumPy in -> NumPy out, CUDA tensor in -> CUDA tensor out.  No CPU fallback.

    Row n is NOT ``mel_to_audio(mels[n], ...)`` sample for sample: the mel bank is under-determined, so the active-set solver
    of the host function and the projected-gradient solver here pick different minimisers of the same objective.  The
    contract is: row n equals ``griffinlim(mel_to_linear(p_n, fb, nnls_iter) ** (1 / power), ...)`` cast to float32 within
    2e-7 of the row's peak, and the per-frame residual of the inversion exceeds ``scipy.optimize.nnls``'s by at most 1e-4
    relative (tests/test_gpu_mel_inverse.py, profiles/mel_inverse.md)."""
    import torch
    is_tensor = isinstance(mels, torch.Tensor)
    if not is_tensor:
        mels = np.asarray(mels)
    if mels.ndim != 2:
        raise ValueError("Mel input must be a 2D array (trials, n_mels * frames).")
    kw = _inverse_kwargs(kwargs, nnls_iter=NNLS_ITER_DEFAULT)
    power, nnls_iter = kw["power"], kw["nnls_iter"]
    n_fft, hop, wl = _check_stft_args(kw["n_fft"], kw["hop_length"], kw["win_length"], inverse=True)
    if power not in (1, 2):
        raise ValueError(f"power = {power} is not supported on the GPU (supported: 1, 2)")
    n_mels = int(n_mels)
    if n_mels < 1:
        raise ValueError(f"n_mels = {n_mels} must be at least 1")
    if n_mels > MEL_INVERT_MAX_MELS:
        raise ValueError(f"n_mels = {n_mels} is not supported by the GPU mel inversion (at most {MEL_INVERT_MAX_MELS})")
    if nnls_iter < 1:
        raise ValueError(f"nnls_iter = {nnls_iter} must be at least 1")
    N, width = int(mels.shape[0]), int(mels.shape[1])
    if N < 1:
        raise ValueError("Mel input holds no trial.")
    if width < n_mels or width % n_mels:
        raise ValueError(f"mel rows of {width} values are not n_mels = {n_mels} bands times a whole number of frames")
    T = width // n_mels
    x = _batch_on_gpu(mels, device, "mel_to_audio_batch")
    p = x.reshape(N, n_mels, T)
    if mel_in_db:
        p = 0.0001 * torch.pow(10.0, 0.1 * p)                                              # db_to_power(., ref=1e-4)
    mag = mel_invert_batch(p, audio_sampling_rate, n_fft, n_mels, fmin=kw["fmin"], fmax=kw["fmax"], nnls_iter=nnls_iter,
                           power=int(power))
    wave = griffinlim_batch(mag, n_iter=kw["n_iter"], hop_length=hop, win_length=wl, seed=kw["seed"], length=kw["length"]).float()
    return wave if is_tensor else wave.cpu().numpy()


# ------------------------------------------------------------------------------------------ F0 tracking (YIN)
# librosa 0.10's ``yin`` restated, like the mel functions above: de Cheveigne & Kawahara's difference function, its
# cumulative-mean normalisation, the first trough below a threshold (else the global minimum) and a parabolic refinement.
# The difference function is the direct sum of squared differences - not librosa's E(0) + E(tau) - 2 r(tau) from an FFT
# autocorrelation, which cancels exactly at the period of a voiced frame - so the host path and ``tl_yin_f0`` state the same
# arithmetic and every term of every sum is non-negative.
#: the longest frame ``tl_yin_f0`` keeps in LDS (YIN_MAX_FRAME of csrc/tonal_pitch.hip)
YIN_MAX_FRAME = 4096


class F0Track(NamedTuple):
    """Per frame: ``f0`` in Hz, ``aperiodicity`` (the CMND value at the pick; small = periodic), ``period_index`` (the pick,
    counted from ``min_period``) and ``rms`` of the frame's first ``win_length`` samples."""
    f0: object
    aperiodicity: object
    period_index: object
    rms: object


class F0TrackCmnd(NamedTuple):
    """``F0Track`` plus ``cmnd`` (..., n_frames, max_period - min_period + 1): the whole normalised difference curve."""
    f0: object
    aperiodicity: object
    period_index: object
    rms: object
    cmnd: object


def yin_geometry(sr: float, fmin: float, fmax: float, frame_length: int = 2048, win_length: Optional[int] = None,
                 hop_length: Optional[int] = None):
    """(frame_length, win_length, hop, min_period, max_period) as ``yin_f0`` and ``yin_f0_batch`` derive them."""
    frame_length = int(frame_length)
    wl = frame_length // 2 if win_length is None else int(win_length)
    hop = frame_length // 4 if hop_length is None else int(hop_length)
    if not sr > 0:
        raise ValueError(f"sr = {sr} must be positive")
    if not 0 < fmin < fmax:
        raise ValueError(f"0 < fmin < fmax is required (got fmin = {fmin}, fmax = {fmax})")
    if not 1 <= wl < frame_length:
        raise ValueError(f"win_length = {wl} must lie in [1, frame_length = {frame_length})")
    if hop < 1:
        raise ValueError(f"hop_length = {hop} must be at least 1")
    min_period = max(int(np.floor(sr / fmax)), 1)
    max_period = min(int(np.ceil(sr / fmin)), frame_length - wl - 1)
    if max_period < min_period + 1:
        raise ValueError(f"fmin = {fmin}, fmax = {fmax} at sr = {sr} give the periods [{min_period}, {max_period}] for "
                         f"frame_length = {frame_length}, win_length = {wl}: at least two lags are needed")
    return frame_length, wl, hop, min_period, max_period


def yin_n_frames(S: int, frame_length: int, hop: int, center: bool) -> int:
    if center:
        return 1 + S // hop
    if S < frame_length:
        raise ValueError(f"audio of {S} samples is shorter than frame_length = {frame_length}")
    return 1 + (S - frame_length) // hop


def yin_f0(y, sr: float, fmin: float, fmax: float, frame_length: int = 2048, win_length: Optional[int] = None,
           hop_length: Optional[int] = None, trough_threshold: float = 0.1, center: bool = True, return_cmnd: bool = False):
    """F0 track of one clip on the host, NumPy float64: the meaning of ``librosa.yin(y, fmin=, fmax=, sr=, frame_length=,
    win_length=, hop_length=, trough_threshold=, center=, pad_mode='constant')`` with the difference function as a direct sum.
    Returns ``F0Track`` of (n_frames,) arrays (``F0TrackCmnd`` with ``return_cmnd``).  ``yin_f0_batch`` is the same on the GPU."""
    y = np.asarray(y, dtype=np.float64)
    if y.ndim != 1:
        raise ValueError("Audio input must be a 1D array.")
    if y.shape[0] < 1:
        raise ValueError("Audio input holds no sample.")
    frame_length, W, hop, pmin, pmax = yin_geometry(sr, fmin, fmax, frame_length, win_length, hop_length)
    if not trough_threshold > 0:
        raise ValueError(f"trough_threshold = {trough_threshold} must be positive")
    n_frames = yin_n_frames(y.shape[0], frame_length, hop, center)
    if center:
        y = np.pad(y, frame_length // 2, mode="constant")
    if y.shape[0] < (n_frames - 1) * hop + frame_length:              # a short clip: the frames past its padding read zeros
        y = np.pad(y, (0, (n_frames - 1) * hop + frame_length - y.shape[0]), mode="constant")
    nc = pmax - pmin + 1
    f0, aper, rms = np.empty(n_frames), np.empty(n_frames), np.empty(n_frames)
    pidx = np.empty(n_frames, dtype=np.int32)
    cmnd = np.empty((n_frames, nc))
    tiny = np.finfo(np.float64).tiny
    taus = np.arange(1, pmax + 1, dtype=np.float64)
    for f in range(n_frames):
        x = y[f * hop:f * hop + frame_length]
        df = x[None, :W] - np.lib.stride_tricks.sliding_window_view(x[:W + pmax], W)          # (pmax + 1, W): row tau
        d = np.sum(df * df, axis=1)
        cm = np.cumsum(d[1:]) / taus
        c = d[pmin:] / (cm[pmin - 1:] + tiny)
        trough = np.zeros(nc, dtype=bool)
        trough[0] = c[0] < c[1]
        trough[1:-1] = (c[1:-1] < c[:-2]) & (c[1:-1] <= c[2:])
        below = np.flatnonzero(trough & (c < trough_threshold))
        i = int(below[0]) if below.size else int(np.argmin(c))
        shift = 0.0
        if 0 < i < nc - 1:
            a = c[i + 1] + c[i - 1] - 2.0 * c[i]
            b = (c[i + 1] - c[i - 1]) / 2.0
            if abs(b) < abs(a):
                shift = -b / a
        f0[f] = sr / (pmin + i + shift)
        aper[f], pidx[f], cmnd[f] = c[i], i, c
        rms[f] = np.sqrt(np.mean(x[:W] ** 2))
    return F0TrackCmnd(f0, aper, pidx, rms, cmnd) if return_cmnd else F0Track(f0, aper, pidx, rms)


def yin_f0_batch(audio, sr: float, fmin: float, fmax: float, frame_length: int = 2048, win_length: Optional[int] = None,
                 hop_length: Optional[int] = None, trough_threshold: float = 0.1, center: bool = True, device=None,
                 return_cmnd: bool = False):
    """``yin_f0`` of every row of an (N, S) batch in one kernel launch (``tl_yin_f0``, one workgroup per frame): row n of each
    (N, n_frames) result is ``yin_f0(audio[n], ...)`` up to fp64 rounding of the sums.  float32 and float64 input is read as it
    is (float32 widened in registers), anything else becomes float64; a CUDA tensor is read in place, also a view whose rows
    are strided (unit stride along the samples).  NumPy in -> NumPy out; CUDA tensor in -> CUDA tensors out on its device.
    ``f0``, ``aperiodicity``, ``rms`` (and ``cmnd`` with ``return_cmnd``) are float64, ``period_index`` int32.
    ``frame_length`` at most ``YIN_MAX_FRAME``.  No CPU fallback: on the host call ``yin_f0`` per clip."""
    import torch
    from .. import _lib
    is_tensor = isinstance(audio, torch.Tensor)
    if not is_tensor:
        audio = np.asarray(audio)
    if audio.ndim != 2:
        raise ValueError("Audio input must be a 2D array (clips, samples).")
    frame_length, W, hop, pmin, pmax = yin_geometry(sr, fmin, fmax, frame_length, win_length, hop_length)
    if frame_length > YIN_MAX_FRAME:
        raise ValueError(f"frame_length = {frame_length} is not supported on the GPU (at most {YIN_MAX_FRAME})")
    if not trough_threshold > 0:
        raise ValueError(f"trough_threshold = {trough_threshold} must be positive")
    N, S = int(audio.shape[0]), int(audio.shape[1])
    if N < 1 or S < 1:
        raise ValueError("Audio input holds no clip or no sample.")
    n_frames = yin_n_frames(S, frame_length, hop, bool(center))
    x, _ = _lib.to_gpu(audio, "yin_f0_batch", device=device, rows="strided")
    dev = x.device
    f0 = torch.empty(N, n_frames, dtype=torch.float64, device=dev)
    aper, rms = torch.empty_like(f0), torch.empty_like(f0)
    pidx = torch.empty(N, n_frames, dtype=torch.int32, device=dev)
    cmnd = torch.empty(N, n_frames, pmax - pmin + 1, dtype=torch.float64, device=dev) if return_cmnd else None
    with torch.cuda.device(dev):
        _lib.check(_lib.load().tl_yin_f0(x.data_ptr(), int(x.dtype == torch.float64), x.stride(0) if N > 1 else S,
                                         f0.data_ptr(), aper.data_ptr(), pidx.data_ptr(), rms.data_ptr(), _lib.ptr(cmnd), N, S,
                                         frame_length, W, hop, int(bool(center)), pmin, pmax, float(trough_threshold),
                                         float(sr), n_frames, _lib.stream_ptr()), "tl_yin_f0")
    out = (f0, aper, pidx, rms) + ((cmnd,) if return_cmnd else ())
    if not is_tensor:
        out = tuple(t.cpu().numpy() for t in out)
    return F0TrackCmnd(*out) if return_cmnd else F0Track(*out)
