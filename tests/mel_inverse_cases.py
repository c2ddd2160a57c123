"""Inputs shared by the mel-inverse tests (host and GPU) and ``scripts/mel_inverse_sweep.py`` - TEST INFRASTRUCTURE.

Signals follow ``test_gpu_mel_frontend.py``: per trial a 220 Hz tone that stops at 60 % of the length plus 1e-3 Gaussian
noise at 24 414 Hz, amplitude ``0.1 * 4**-n``.  A case is (N, S, mel keywords, Griffin-Lim ``length`` is S unless the case
says None)."""
import functools

import numpy as np

SR = 24414
#: name -> (N, S, mel keywords of audio_to_mel, keep the length S in the inversion)
CASES = {
    "nfft512": (3, 3000, dict(n_mels=40, n_fft=512, hop_length=128), True),
    "nfft256": (2, 1500, dict(n_mels=20, n_fft=256, hop_length=64), True),
    "nfft2048": (2, 6000, dict(n_mels=80, n_fft=2048), True),
    "win400_in_512": (2, 3000, dict(n_mels=40, n_fft=512, hop_length=100, win_length=400, fmin=50, fmax=8000), True),
    "magnitude": (2, 3000, dict(n_mels=40, n_fft=512, hop_length=128, power=1.0), True),
    "no_length": (2, 1500, dict(n_mels=20, n_fft=256, hop_length=64), False),
    "two_frames": (2, 100, dict(n_mels=20, n_fft=256, hop_length=64), True),
}
#: 1 000 x the largest spread of ``mel_to_linear`` under a 1e-15 relative perturbation of every iteration's gradient, as a
#: fraction of the trial's largest value (profiles/mel_inverse.md, "Perturbation measurements")
INVERT_BOUND = 1.02e-9
#: Griffin-Lim against the host, as a fraction of the row's peak (the same section)
GL_BOUND = 1e-9
#: what the residual of the projected-gradient solve may exceed scipy's active-set solve by, per frame
RESIDUAL_EXCESS = 1e-4


@functools.lru_cache(maxsize=None)
def signals(N: int, S: int, seed: int = 0) -> np.ndarray:
    rng = np.random.default_rng(seed)
    t = np.arange(S) / SR
    tone = np.sin(2.0 * np.pi * 220.0 * t) * (np.arange(S) < int(0.6 * S))
    x = np.stack([0.1 * 4.0 ** -n * tone + 1e-3 * rng.standard_normal(S) for n in range(N)]).astype(np.float32)
    x.setflags(write=False)
    return x


def bank(kw: dict) -> np.ndarray:
    from decode_tonal_langauge_amd.utils.audio import mel_filterbank
    return mel_filterbank(SR, kw.get("n_fft", 2048), n_mels=kw["n_mels"], fmin=kw.get("fmin", 0.0),
                          fmax=kw.get("fmax")).astype(np.float64)


@functools.lru_cache(maxsize=None)
def mel_power(name: str, noisy: bool = False) -> np.ndarray:
    """(N, n_mels, T) float64 mel power (or magnitude) of the case's signals; ``noisy`` multiplies by 3 dB Gaussian noise."""
    from decode_tonal_langauge_amd.utils.audio import audio_to_mel
    N, S, kw, _ = CASES[name]
    mel = np.stack([audio_to_mel(row, SR, mel_in_db=False, mel_kwargs=kw).reshape(kw["n_mels"], -1)
                    for row in signals(N, S)]).astype(np.float64)
    if noisy:
        mel = mel * np.power(10.0, 0.3 * np.random.default_rng(1).standard_normal(mel.shape))
    mel.setflags(write=False)
    return mel


@functools.lru_cache(maxsize=None)
def host_linear(name: str, noisy: bool = False) -> np.ndarray:
    """(N, n_bins, T): ``mel_to_linear`` of every trial at the default iteration count."""
    from decode_tonal_langauge_amd.utils.audio import mel_to_linear
    fb = bank(CASES[name][2])
    lin = np.stack([mel_to_linear(p, fb) for p in mel_power(name, noisy)])
    lin.setflags(write=False)
    return lin


def relative_residual(fb: np.ndarray, x: np.ndarray, p: np.ndarray) -> np.ndarray:
    """Per frame ``||fb x - p|| / ||p||`` of (n_bins, T) against (n_mels, T)."""
    return np.linalg.norm(fb @ x - p, axis=0) / np.linalg.norm(p, axis=0)


@functools.lru_cache(maxsize=None)
def scipy_residual(name: str, noisy: bool = False):
    """Frames ``0, 4, 8, ...`` of every trial through ``scipy.optimize.nnls``: (frame indices, (N, len) residuals)."""
    from scipy.optimize import nnls
    fb = bank(CASES[name][2])
    mel = mel_power(name, noisy)
    frames = np.arange(0, mel.shape[2], 4)
    res = np.array([[np.linalg.norm(fb @ nnls(fb, p[:, t])[0] - p[:, t]) / np.linalg.norm(p[:, t]) for t in frames]
                    for p in mel])
    return frames, res
