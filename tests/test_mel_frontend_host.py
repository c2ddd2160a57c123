"""CPU: the two mel front-end entries (tl_mel_power, tl_mel_finish) are declared and typed alike, refuse bad arguments before
anything is launched, and the packed mel bank the host uploads is the dense ``mel_filterbank`` run by run."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mel_entries_are_declared_and_typed_with_matching_arity():
    from decode_tonal_langauge_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "tonal_hip.h")).read()
    for name in ("tl_mel_power", "tl_mel_finish"):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert m, f"{name} is not declared in include/tonal_hip.h"
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name


def _power(lib, **over):
    # tl_mel_power(audio, is_f64, row_stride, window, tw, bands, weights, n_weights, mel, rowmax, N, S, n_fft, win_length,
    #              hop, center, power, n_mels, n_frames, stream); 16 stands for a non-null device pointer, never followed
    a = dict(audio=16, is_f64=0, row_stride=5000, window=16, tw=16, bands=16, weights=16, n_weights=100, mel=16, rowmax=16,
             N=4, S=5000, n_fft=2048, win_length=2048, hop=512, center=1, power=2, n_mels=80, n_frames=10, stream=None)
    a.update(over)
    return lib.tl_mel_power(*a.values())


def test_mel_power_refuses_bad_arguments_without_gpu():
    from decode_tonal_langauge_amd import _lib
    lib = _lib.load()
    for ptr_name in ("audio", "window", "tw", "bands", "weights", "mel", "rowmax"):
        assert _power(lib, **{ptr_name: None}) == -1 and b"null" in lib.tl_last_error(), ptr_name
    for n_fft in (300, 128, 4096, 0):
        assert _power(lib, n_fft=n_fft) == -1 and b"n_fft" in lib.tl_last_error() and b"256, 512, 1024, 2048" in lib.tl_last_error()
    assert _power(lib, win_length=2049) == -1 and b"win_length" in lib.tl_last_error()
    assert _power(lib, win_length=0) == -1 and b"win_length" in lib.tl_last_error()
    assert _power(lib, hop=0) == -1 and b"hop" in lib.tl_last_error()
    for power in (0, 3):
        assert _power(lib, power=power) == -1 and b"power" in lib.tl_last_error()
    assert _power(lib, n_mels=0) == -1 and b"n_mels" in lib.tl_last_error()
    assert _power(lib, N=0) == -1 and b"N and S" in lib.tl_last_error()
    assert _power(lib, row_stride=4999) == -1 and b"row_stride" in lib.tl_last_error()
    # the frame count must be the one S, n_fft, hop and center give: 1 + 5000 // 512 = 10 centred, 1 + 2952 // 512 = 6 not
    for n_frames in (9, 11, 0):
        assert _power(lib, n_frames=n_frames) == -1 and b"n_frames" in lib.tl_last_error()
    assert _power(lib, center=0, n_frames=10) == -1 and b"n_frames" in lib.tl_last_error()
    assert _power(lib, center=0, S=2047, row_stride=2047, n_frames=1) == -1 and b"shorter than n_fft" in lib.tl_last_error()


def test_mel_finish_refuses_bad_arguments_without_gpu():
    from decode_tonal_langauge_amd import _lib
    lib = _lib.load()
    # tl_mel_finish(mel, rowmax, out, N, n_mels, n_frames, in_db, stream)
    assert lib.tl_mel_finish(None, 16, 16, 4, 80, 10, 1, None) == -1 and b"null" in lib.tl_last_error()
    assert lib.tl_mel_finish(16, None, 16, 4, 80, 10, 1, None) == -1 and b"null" in lib.tl_last_error()
    assert lib.tl_mel_finish(16, 16, None, 4, 80, 10, 1, None) == -1 and b"null" in lib.tl_last_error()
    assert lib.tl_mel_finish(16, 16, 16, 0, 80, 10, 1, None) == -1 and b"N must" in lib.tl_last_error()
    assert lib.tl_mel_finish(16, 16, 16, 4, 0, 10, 1, None) == -1 and b"n_mels" in lib.tl_last_error()
    assert lib.tl_mel_finish(16, 16, 16, 4, 80, 0, 1, None) == -1 and b"n_frames" in lib.tl_last_error()
    assert lib.tl_mel_finish(16, 16, 16, 4, 80, 10, 2, None) == -1 and b"in_db" in lib.tl_last_error()


@pytest.mark.parametrize("kw", [dict(sr=24414, n_fft=2048, n_mels=128),
                                dict(sr=24414, n_fft=2048, n_mels=80),
                                dict(sr=24414, n_fft=512, n_mels=40, fmin=50, fmax=8000)])
def test_packed_bank_expands_to_the_dense_bank_exactly(kw):
    from decode_tonal_langauge_amd.utils.audio import mel_filterbank, pack_mel_filterbank
    dense = mel_filterbank(**kw)
    bands, weights = pack_mel_filterbank(dense)
    assert bands.dtype == np.int32 and bands.shape == (kw["n_mels"], 3) and weights.dtype == np.float64
    again = np.zeros(dense.shape, dtype=np.float64)
    for m, (first, last, off) in enumerate(bands):
        assert 0 <= first <= last <= dense.shape[1] and off + last - first <= weights.size
        again[m, first:last] = weights[off:off + last - first]
    assert np.array_equal(again, dense.astype(np.float64))
    assert np.array_equal(again.astype(np.float32), dense)
    assert int(bands[-1, 2] + bands[-1, 1] - bands[-1, 0]) == weights.size          # the runs tile the weight array
    assert weights.size < 0.1 * dense.size                                            # and are short: that is the point


def test_batch_function_checks_its_arguments_before_it_needs_a_gpu():
    import torch
    from decode_tonal_langauge_amd.utils.audio import audio_to_mel, audio_to_mel_batch
    x = np.zeros((2, 3000), dtype=np.float32)
    with pytest.raises(TypeError) as batch_err:
        audio_to_mel_batch(x, 24414, mel_kwargs={"n_mels": 80, "htk": True})
    with pytest.raises(TypeError) as host_err:
        audio_to_mel(x[0], 24414, mel_kwargs={"n_mels": 80, "htk": True})
    assert str(batch_err.value) == str(host_err.value)
    with pytest.raises(ValueError, match="256, 512, 1024, 2048"):
        audio_to_mel_batch(x, 24414, mel_kwargs={"n_fft": 300})
    with pytest.raises(ValueError, match="2D"):
        audio_to_mel_batch(x[0], 24414)
    with pytest.raises(ValueError) as batch_err:
        audio_to_mel_batch(x[:, :1000], 24414, mel_kwargs={"n_fft": 1024, "center": False})
    with pytest.raises(ValueError) as host_err:
        audio_to_mel(x[0, :1000], 24414, mel_kwargs={"n_fft": 1024, "center": False})
    assert str(batch_err.value) == str(host_err.value)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            audio_to_mel_batch(x, 24414, mel_kwargs={"n_mels": 80})
