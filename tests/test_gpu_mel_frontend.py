"""GPU: ``utils.audio.audio_to_mel_batch`` (tl_mel_power + tl_mel_finish) against the float64 host function
``utils.audio.audio_to_mel`` called once per trial.

Bounds.  The kernels compute in fp64 and round once, to the float32 output, as the host does; so a correct result differs
from the host's by float32 output rounding only.
  dB output:      |gpu - host| <= 2e-5.  One float32 ulp in [64, 128) dB is 7.6e-6: under three ulps.  The 80 dB clip keeps
                  every compared value above 1e-8 of the trial's peak, where the fp64 transform's own error is < 1e-7 dB.
  linear output:  |gpu - host| <= 2e-7 |host| + 2e-7 max(host row).
Signals: per trial a 220 Hz tone that stops at 60 % of the length plus 1e-3 Gaussian noise, 24 414 Hz, and a different
amplitude per trial (0.1 * 4**-n) - a batch-wide dB reference instead of the per-trial one misses the bound by many dB."""
import functools
from argparse import Namespace

import numpy as np
import pytest
import torch

from tests import parity_record

pytestmark = pytest.mark.gpu
SR = 24414
DB_BOUND = 2e-5
CASES = {
    "short_700": (3, 700, dict(n_mels=80)),
    "default_5000": (4, 5000, dict(n_mels=80)),
    "win400_in_512": (5, 3000, dict(n_mels=40, n_fft=512, hop_length=100, win_length=400, fmin=50, fmax=8000)),
    "nfft_256": (2, 1000, dict(n_mels=20, n_fft=256, hop_length=64)),
    "nfft_1024_uncentred": (2, 1500, dict(n_mels=32, n_fft=1024, center=False)),
    "nfft_512_magnitude": (2, 3000, dict(n_mels=40, n_fft=512, power=1.0)),
}


@functools.lru_cache(maxsize=None)
def _signals(N: int, S: int, seed: int = 0) -> np.ndarray:
    rng = np.random.default_rng(seed)
    t = np.arange(S) / SR
    tone = np.sin(2.0 * np.pi * 220.0 * t) * (np.arange(S) < int(0.6 * S))
    x = np.stack([0.1 * 4.0 ** -n * tone + 1e-3 * rng.standard_normal(S) for n in range(N)]).astype(np.float32)
    x.setflags(write=False)
    return x


def _host(x: np.ndarray, in_db: bool, kw: dict) -> np.ndarray:
    from decode_tonal_langauge_amd.utils.audio import audio_to_mel
    return np.stack([audio_to_mel(row, SR, mel_in_db=in_db, mel_kwargs=kw) for row in x])


@functools.lru_cache(maxsize=None)
def _case_reference(name: str, in_db: bool) -> np.ndarray:
    N, S, kw = CASES[name]
    ref = _host(_signals(N, S), in_db, kw)
    ref.setflags(write=False)
    return ref


def _check(got: np.ndarray, ref: np.ndarray, in_db: bool, tag: str) -> float:
    """Prints and records the worst deviation over its bound, then asserts the bound."""
    assert got.shape == ref.shape and got.dtype == np.float32
    assert np.isfinite(got).all()
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    if in_db:
        bound = np.full_like(err, DB_BOUND)
    else:
        bound = 2e-7 * np.abs(ref.astype(np.float64)) + 2e-7 * ref.astype(np.float64).max(axis=1, keepdims=True)
    worst = float((err / bound).max())
    print(f"[{tag}] max |gpu - host| {float(err.max()):.3e}   worst deviation / bound {worst:.3f}")
    parity_record.record(f"mel_frontend_{tag}", {"max_abs_err": float(err.max()), "worst_over_bound": worst,
                                                 "values": int(err.size)})
    assert (err <= bound).all(), (tag, float(err.max()), worst)
    return worst


# ---------------------------------------------------------------------------------------------- numbers
@pytest.mark.parametrize("in_db", [True, False], ids=["db", "linear"])
@pytest.mark.parametrize("name", list(CASES))
def test_batch_matches_the_host_function_per_trial(name, in_db):
    from decode_tonal_langauge_amd.utils.audio import audio_to_mel_batch
    N, S, kw = CASES[name]
    got = audio_to_mel_batch(_signals(N, S), SR, mel_in_db=in_db, mel_kwargs=kw)
    assert isinstance(got, np.ndarray)
    ref = _case_reference(name, in_db)
    _check(got, ref, in_db, f"{name}_{'db' if in_db else 'linear'}")
    if in_db:
        # every trial has its own reference: its own maximum is 0 dB and nothing lies more than 80 dB below it
        assert np.array_equal(got.max(axis=1), np.zeros(N, dtype=np.float32)) and got.min() >= -80.0


def test_float64_audio_and_cuda_tensor_input():
    from decode_tonal_langauge_amd.utils.audio import audio_to_mel_batch
    N, S, kw = CASES["default_5000"]
    x32 = _signals(N, S)
    base = audio_to_mel_batch(x32, SR, mel_kwargs=kw)
    got64 = audio_to_mel_batch(x32.astype(np.float64), SR, mel_kwargs=kw)
    _check(got64, _case_reference("default_5000", True), True, "default_5000_float64_audio")
    assert np.array_equal(got64, base)                    # float32 samples widened on either side of the upload
    xt = torch.from_numpy(np.array(x32)).cuda()
    out = audio_to_mel_batch(xt, SR, mel_kwargs=kw)
    assert isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float32 and out.device == xt.device
    assert np.array_equal(out.cpu().numpy(), base)
    lin = audio_to_mel_batch(xt, SR, mel_in_db=False, mel_kwargs=kw)
    assert np.array_equal(lin.cpu().numpy(), audio_to_mel_batch(x32, SR, mel_in_db=False, mel_kwargs=kw))


def test_integer_audio_is_converted_to_float64():
    from decode_tonal_langauge_amd.utils.audio import audio_to_mel_batch
    N, S, kw = CASES["nfft_256"]
    xi = np.round(_signals(N, S) * 32767.0).astype(np.int16)
    got = audio_to_mel_batch(xi, SR, mel_kwargs=kw)
    _check(got, _host(xi, True, kw), True, "nfft_256_int16_audio")


def test_all_zero_trial_between_two_normal_ones():
    from decode_tonal_langauge_amd.utils.audio import audio_to_mel_batch
    kw = dict(n_mels=80)
    x = np.array(_signals(3, 3000))
    x[1] = 0.0
    got = audio_to_mel_batch(x, SR, mel_kwargs=kw)
    assert np.array_equal(got[1], np.zeros_like(got[1]))  # both terms sit on the 1e-10 floor: 0 dB everywhere
    _check(got, _host(x, True, kw), True, "zero_trial_db")
    alone = audio_to_mel_batch(x[[0, 2]], SR, mel_kwargs=kw)
    assert np.array_equal(alone, got[[0, 2]])             # the neighbours do not see it
    lin = audio_to_mel_batch(x, SR, mel_in_db=False, mel_kwargs=kw)
    assert np.array_equal(lin[1], np.zeros_like(lin[1])) and lin[0].max() > 0 and lin[2].max() > 0


def test_row_strided_view_equals_its_contiguous_copy():
    from decode_tonal_langauge_amd.utils.audio import audio_to_mel_batch
    N, S, kw = CASES["win400_in_512"]
    big = torch.full((N, S + 37), 7.0, dtype=torch.float32, device="cuda")       # what lies past S must not be read as signal
    big[:, :S] = torch.from_numpy(np.array(_signals(N, S))).cuda()
    view = big[:, :S]
    assert not view.is_contiguous()
    for in_db in (True, False):
        a = audio_to_mel_batch(view, SR, mel_in_db=in_db, mel_kwargs=kw)
        b = audio_to_mel_batch(view.contiguous(), SR, mel_in_db=in_db, mel_kwargs=kw)
        assert torch.equal(a, b)
        _check(a.cpu().numpy(), _case_reference("win400_in_512", in_db), in_db, f"strided_{'db' if in_db else 'linear'}")


# ---------------------------------------------------------------------------------------------- errors
def test_error_paths_follow_the_host_function():
    from decode_tonal_langauge_amd.utils.audio import audio_to_mel, audio_to_mel_batch
    x = _signals(2, 3000)
    with pytest.raises(TypeError) as batch_err:
        audio_to_mel_batch(x, SR, mel_kwargs={"n_mels": 80, "htk": True})
    with pytest.raises(TypeError) as host_err:
        audio_to_mel(x[0], SR, mel_kwargs={"n_mels": 80, "htk": True})
    assert str(batch_err.value) == str(host_err.value)
    with pytest.raises(ValueError, match="256, 512, 1024, 2048"):
        audio_to_mel_batch(x, SR, mel_kwargs={"n_fft": 300})
    with pytest.raises(ValueError):
        audio_to_mel_batch(x[0], SR)
    with pytest.raises(ValueError):
        audio_to_mel_batch(torch.zeros(3000, device="cuda"), SR)
    with pytest.raises(ValueError) as batch_err:
        audio_to_mel_batch(x[:, :1000], SR, mel_kwargs={"n_fft": 1024, "center": False})
    with pytest.raises(ValueError) as host_err:
        audio_to_mel(x[0, :1000], SR, mel_kwargs={"n_fft": 1024, "center": False})
    assert str(batch_err.value) == str(host_err.value)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        audio_to_mel_batch(torch.zeros(2, 3000), SR)


# ---------------------------------------------------------------------------------------------- wiring
def test_synthesiser_entry_point_takes_the_batch_path_on_cuda():
    from decode_tonal_langauge_amd.train_synthesizer import _mels_from_dataset
    from decode_tonal_langauge_amd.utils.audio import audio_to_mel_batch
    N, S, kw = CASES["default_5000"]
    x = np.array(_signals(N, S))
    got = _mels_from_dataset({"audio": x}, Namespace(device="cuda:0", audio_sampling_rate=SR), kw)
    assert isinstance(got, np.ndarray) and got.dtype == np.float32
    assert np.array_equal(got, audio_to_mel_batch(x, SR, mel_kwargs=kw))
    host = _mels_from_dataset({"audio": x}, Namespace(device="cpu", audio_sampling_rate=SR), kw)
    assert np.array_equal(host, _case_reference("default_5000", True))
    _check(got, host, True, "wiring_db")
    ready = np.arange(12, dtype=np.float64).reshape(3, 4)
    kept = _mels_from_dataset({"audio": x, "mel": ready}, Namespace(device="cuda:0", audio_sampling_rate=SR), kw)
    assert kept.dtype == np.float32 and np.array_equal(kept, ready.astype(np.float32))
