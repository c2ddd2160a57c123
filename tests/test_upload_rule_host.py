"""CPU: the package's one input rule (``_lib.to_gpu`` and its tensor half ``_lib.normalise``) - which dtypes and layouts are kept,
and the refusals of every public entry that goes through it, word for word and in each site's order."""
import warnings
from argparse import Namespace

import numpy as np
import pytest
import torch

from decode_tonal_langauge_amd import _lib

NO_GPU = "{} (MI355X build): no GPU visible; this package has no CPU fallback"


# ---- the tensor half, on CPU tensors
@pytest.mark.parametrize("rows", ["contiguous", "strided"])
def test_float32_and_float64_are_kept_and_other_dtypes_become_float64(rows):
    for dtype in (torch.float32, torch.float64):
        t = torch.arange(12, dtype=dtype).reshape(3, 4)
        out = _lib.normalise(t, rows=rows)
        assert out is t or (out.dtype == dtype and out.data_ptr() == t.data_ptr())
    for dtype in (torch.int16, torch.float16):
        t = torch.arange(12).reshape(3, 4).to(dtype)
        out = _lib.normalise(t, rows=rows)
        assert out.dtype == torch.float64 and torch.equal(out, t.double())


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int16, torch.float16, torch.int32, torch.int64, torch.float32])
def test_floats_false_keeps_the_dtype(dtype):
    t = torch.arange(12).reshape(3, 4).to(dtype)
    out = _lib.normalise(t, floats=False, rows="strided")
    assert out.dtype == dtype and out.data_ptr() == t.data_ptr()


def test_a_row_strided_view_is_kept_only_under_strided():
    base = torch.arange(30, dtype=torch.float64).reshape(3, 10)
    view = base[:, :7]
    assert view.stride() == (10, 1) and not view.is_contiguous()
    kept = _lib.normalise(view, rows="strided")
    assert kept.data_ptr() == view.data_ptr() and kept.stride() == (10, 1)
    packed = _lib.normalise(view, rows="contiguous")
    assert packed.is_contiguous() and packed.stride() == (7, 1) and torch.equal(packed, view)


@pytest.mark.parametrize("rows", ["contiguous", "strided"])
def test_transposed_and_column_strided_views_are_made_contiguous(rows):
    base = torch.arange(30, dtype=torch.float32).reshape(3, 10)
    for view in (base.t(), base[:, ::2]):
        out = _lib.normalise(view, rows=rows)
        assert out.is_contiguous() and torch.equal(out, view) and out.dtype == torch.float32


def test_one_row_is_kept_whatever_its_row_stride():
    base = torch.arange(30, dtype=torch.float64).reshape(3, 10)
    for view in (base[1:2, :7], torch.as_strided(base, (1, 7), (3, 1)), torch.as_strided(base, (1, 7), (0, 1))):
        out = _lib.normalise(view, rows="strided")
        assert out.data_ptr() == view.data_ptr() and out.stride() == view.stride()


def test_an_unknown_rows_option_is_refused():
    with pytest.raises(ValueError, match="rows must be"):
        _lib.normalise(torch.zeros(2, 2), rows="any")


# ---- the refusals of the helper
def test_without_a_gpu_an_array_is_refused_in_the_callers_name(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    for what in ("car_rereference", "some step"):
        with pytest.raises(RuntimeError) as e:
            _lib.to_gpu(np.zeros((2, 3)), what)
        assert str(e.value) == NO_GPU.format(what)


def test_a_cpu_tensor_draws_the_message_of_require_gpu():
    t = torch.zeros(2, 3)
    with pytest.raises(RuntimeError) as e:
        _lib.to_gpu(t, "welch_psd")
    with pytest.raises(RuntimeError) as want:
        _lib.require_gpu(t, "welch_psd")
    assert str(e.value) == str(want.value) and str(e.value).startswith("welch_psd: tensor is on 'cpu'.")


def test_a_device_that_is_not_cuda_is_refused(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    with pytest.raises(RuntimeError) as e:
        _lib.to_gpu(np.zeros((2, 3)), "yin_f0_batch", device="cpu")
    assert str(e.value) == "yin_f0_batch: device 'cpu' is not a CUDA device; this package has no CPU fallback"


# ---- every public caller, without a GPU
def _public_callers():
    from decode_tonal_langauge_amd.channel_selection.utils import anova_oneway
    from decode_tonal_langauge_amd.data_loading.epoching import extract_windows
    from decode_tonal_langauge_amd.preprocess.signal import car_rereference, frequency_filter
    from decode_tonal_langauge_amd.utils import audio, diagnostics
    rec = np.random.default_rng(0).standard_normal((2, 600))
    return {
        "car_rereference": lambda: car_rereference.run(rec, Namespace()),
        "frequency_filter": lambda: frequency_filter.hilbert_filter(rec, 400, [(70.0, 150.0)]),
        "welch_psd": lambda: diagnostics.welch_psd(rec),
        "segment_mean_std": lambda: diagnostics.segment_mean_std(rec, 100, 0.0, 3.0),
        "audio_to_mel_batch": lambda: audio.audio_to_mel_batch(rec, 16000, mel_kwargs={"n_fft": 256, "n_mels": 20}),
        "yin_f0_batch": lambda: audio.yin_f0_batch(rec, 16000, 100.0, 400.0, frame_length=512),
        "griffinlim_batch": lambda: audio.griffinlim_batch(np.ones((1, 129, 5))),
        "mel_to_audio_batch": lambda: audio.mel_to_audio_batch(np.zeros((1, 20 * 5)), 20, n_fft=256),
        "extract_windows": lambda: extract_windows(rec, [0, 10], 50),
        "anova_oneway": lambda: anova_oneway(rec.reshape(6, 2, 100), np.arange(6) % 2),
    }


@pytest.mark.parametrize("what", ["car_rereference", "frequency_filter", "welch_psd", "segment_mean_std", "audio_to_mel_batch",
                                  "yin_f0_batch", "griffinlim_batch", "mel_to_audio_batch", "extract_windows", "anova_oneway"])
def test_every_public_caller_refuses_an_array_without_a_gpu_in_its_own_name(monkeypatch, what):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError) as e:
        _public_callers()[what]()
    assert str(e.value) == NO_GPU.format(what)


def test_the_audio_entries_refuse_a_device_that_is_not_cuda(monkeypatch):
    from decode_tonal_langauge_amd.utils import audio
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    rec = np.zeros((2, 600))
    calls = {"audio_to_mel_batch": lambda: audio.audio_to_mel_batch(rec, 16000, mel_kwargs={"n_fft": 256}, device="cpu"),
             "yin_f0_batch": lambda: audio.yin_f0_batch(rec, 16000, 100.0, 400.0, frame_length=512, device="cpu"),
             "griffinlim_batch": lambda: audio.griffinlim_batch(np.ones((1, 129, 5)), device="cpu"),
             "mel_to_audio_batch": lambda: audio.mel_to_audio_batch(np.zeros((1, 100)), 20, n_fft=256, device="cpu")}
    for what, call in calls.items():
        with pytest.raises(RuntimeError) as e:
            call()
        assert str(e.value) == f"{what}: device 'cpu' is not a CUDA device; this package has no CPU fallback"


# ---- the order of the refusals per site
def test_diagnostics_refuse_rank_and_complex_input_before_they_look_for_a_gpu(monkeypatch):
    from decode_tonal_langauge_amd.utils import diagnostics
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    for bad in (np.zeros(600), np.zeros((2, 3, 600)), torch.zeros(600)):
        with pytest.raises(ValueError) as e:
            diagnostics.welch_psd(bad)
        assert str(e.value) == "welch_psd: expected data of shape (n_channels, n_timepoints)"
        with pytest.raises(ValueError) as e:
            diagnostics.summarise(bad, 100)
        assert str(e.value) == "diagnostics: expected data of shape (n_channels, n_timepoints)"
    for bad in (np.zeros((2, 600), dtype=np.complex128), torch.zeros(2, 600, dtype=torch.complex64)):
        with pytest.raises(ValueError, match=r"^welch_psd: complex input is not supported \(supported: "):
            diagnostics.welch_psd(bad)
        with pytest.raises(ValueError, match=r"^segment_mean_std: complex input is not supported \(supported: "):
            diagnostics.segment_mean_std(bad, 100, 0.0, 3.0)


def test_the_signal_steps_look_for_a_gpu_before_they_check_the_rank(monkeypatch):
    from decode_tonal_langauge_amd.preprocess.signal import _common, channel_zscore, frequency_filter
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    flat = np.zeros((2, 3, 50))
    for what, call in (("channel_zscore", lambda: channel_zscore.run(flat, Namespace())),
                       ("frequency_filter", lambda: frequency_filter.hilbert_filter(flat, 400, [(70.0, 150.0)])),
                       ("downsample", lambda: _common.to_device(flat, "downsample"))):
        with pytest.raises(RuntimeError) as e:
            call()
        assert str(e.value) == NO_GPU.format(what)


def test_extract_windows_keeps_its_own_refusals_after_the_gpu_check(monkeypatch):
    from decode_tonal_langauge_amd.data_loading.epoching import to_recording
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError) as e:
        to_recording(np.zeros(5, dtype=np.int16))                       # the rank refusal needs a GPU
    assert str(e.value) == NO_GPU.format("extract_windows")
    with pytest.raises(RuntimeError, match="^extract_windows: tensor is on 'cpu'"):
        to_recording(torch.zeros(5))


def test_the_host_copy_is_made_only_for_an_array_that_is_not_c_contiguous_and_writable(monkeypatch):
    """What ``to_gpu`` hands ``torch.from_numpy``: the caller's own buffer for a C-contiguous writable array of a kept dtype,
    a fresh C-contiguous writable one otherwise - so a read-only array draws no warning."""
    seen = []
    real = torch.from_numpy

    class Stop(Exception):
        pass

    def spy(arr):
        seen.append(arr)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            real(arr)
        raise Stop

    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    monkeypatch.setattr(torch, "from_numpy", spy)
    plain = np.zeros((3, 8))
    frozen = np.zeros((3, 8), dtype=np.float32)
    frozen.setflags(write=False)
    for arr, shared in ((plain, True), (frozen, False), (np.asfortranarray(plain), False), (plain[:, ::2], False),
                        (np.zeros((3, 8), dtype=np.int16), False)):
        with pytest.raises(Stop):
            _lib.to_gpu(arr, "probe")
        got = seen[-1]
        assert got.flags.c_contiguous and got.flags.writeable and np.array_equal(got, arr)
        assert np.shares_memory(got, arr) == shared
        assert got.dtype == (np.float64 if arr.dtype == np.int16 else arr.dtype)
    with pytest.raises(Stop):
        _lib.to_gpu(np.zeros((3, 8), dtype=np.int16), "probe", floats=False)
    assert seen[-1].dtype == np.int16
