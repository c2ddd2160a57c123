"""CPU: the four entries of the mel inverse (tl_mel_invert, tl_gl_synth, tl_gl_analyse, tl_gl_overlap_add) are declared and
typed alike and refuse bad arguments before anything is launched; the host statement ``mel_to_linear`` of the inversion
reaches the residual of ``scipy.optimize.nnls``; ``mel_to_audio_batch`` checks its arguments before it needs a GPU."""
import os
import re

import numpy as np
import pytest

from tests import mel_inverse_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("tl_mel_invert", "tl_gl_synth", "tl_gl_analyse", "tl_gl_overlap_add")


def test_inverse_entries_are_declared_and_typed_with_matching_arity():
    from decode_tonal_langauge_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "tonal_hip.h")).read()
    for name in ENTRIES:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert m, f"{name} is not declared in include/tonal_hip.h"
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name


# 16 stands for a non-null device pointer, never followed
def _invert(lib, **over):
    a = dict(mel_power=16, bands=16, weights=16, n_weights=300, bin_bands=16, bin_weights=16, momentum=16, out=16, N=2, n_fft=512,
             n_mels=40, n_frames=10, nnls_iter=100, step=0.5, power=2, stream=None)
    a.update(over)
    return lib.tl_mel_invert(*a.values())


def _synth(lib, **over):
    a = dict(mag=16, angles=16, angles_shared=0, window=16, tw=16, frames=16, N=2, n_fft=512, n_frames=10, stream=None)
    a.update(over)
    return lib.tl_gl_synth(*a.values())


def _analyse(lib, **over):
    a = dict(frames=16, wsum=16, window=16, tw=16, angles=16, tprev=16, N=2, n_fft=512, win_length=512, hop=128, n_frames=10,
             length=1152, momentum=0.99, first=0, stream=None)
    a.update(over)
    return lib.tl_gl_analyse(*a.values())


def _overlap_add(lib, **over):
    a = dict(frames=16, wsum=16, out=16, N=2, n_fft=512, win_length=512, hop=128, n_frames=10, length=1152, stream=None)
    a.update(over)
    return lib.tl_gl_overlap_add(*a.values())


def test_mel_invert_refuses_bad_arguments_without_gpu():
    from decode_tonal_langauge_amd import _lib
    lib = _lib.load()
    for ptr_name in ("mel_power", "bands", "weights", "bin_bands", "bin_weights", "momentum", "out"):
        assert _invert(lib, **{ptr_name: None}) == -1 and b"null" in lib.tl_last_error(), ptr_name
    for n_fft in (300, 128, 4096, 0):
        assert _invert(lib, n_fft=n_fft) == -1 and b"256, 512, 1024, 2048" in lib.tl_last_error()
    for n_mels in (0, 257):
        assert _invert(lib, n_mels=n_mels) == -1 and b"n_mels" in lib.tl_last_error()
    assert _invert(lib, N=0) == -1 and b"N and n_frames" in lib.tl_last_error()
    assert _invert(lib, n_frames=0) == -1 and b"N and n_frames" in lib.tl_last_error()
    for power in (0, 3):
        assert _invert(lib, power=power) == -1 and b"power" in lib.tl_last_error()
    for nnls_iter in (0, -5):
        assert _invert(lib, nnls_iter=nnls_iter) == -1 and b"nnls_iter" in lib.tl_last_error()
    for step in (0.0, -1.0, float("inf"), float("nan")):
        assert _invert(lib, step=step) == -1 and b"step" in lib.tl_last_error()
    for n_weights in (-1, 515):                                  # more than two bands per bin cannot be a triangular bank
        assert _invert(lib, n_weights=n_weights) == -1 and b"n_weights" in lib.tl_last_error()


def test_griffin_lim_entries_refuse_bad_arguments_without_gpu():
    from decode_tonal_langauge_amd import _lib
    lib = _lib.load()
    for ptr_name in ("mag", "angles", "window", "tw", "frames"):
        assert _synth(lib, **{ptr_name: None}) == -1 and b"null" in lib.tl_last_error(), ptr_name
    for ptr_name in ("frames", "wsum", "window", "tw", "angles", "tprev"):
        assert _analyse(lib, **{ptr_name: None}) == -1 and b"null" in lib.tl_last_error(), ptr_name
    for ptr_name in ("frames", "wsum", "out"):
        assert _overlap_add(lib, **{ptr_name: None}) == -1 and b"null" in lib.tl_last_error(), ptr_name
    assert _synth(lib, angles_shared=2) == -1 and b"angles_shared" in lib.tl_last_error()
    for call in (_synth, _analyse, _overlap_add):
        for n_fft in (300, 128, 4096, 0):
            assert call(lib, n_fft=n_fft) == -1 and b"256, 512, 1024, 2048" in lib.tl_last_error()
        assert call(lib, N=0) == -1 and b"N and n_frames" in lib.tl_last_error()
        assert call(lib, n_frames=0) == -1 and b"N and n_frames" in lib.tl_last_error()
    for call in (_analyse, _overlap_add):
        for win_length in (0, 513):
            assert call(lib, win_length=win_length) == -1 and b"win_length" in lib.tl_last_error()
        assert call(lib, hop=0) == -1 and b"hop must" in lib.tl_last_error()
        assert call(lib, hop=401, win_length=400) == -1 and b"gaps" in lib.tl_last_error()
        # ten frames of 512 at hop 128 hold 256 + 9 * 128 = 1408 samples after the centre trim
        for length in (0, -1, 1409):
            assert call(lib, length=length) == -1 and b"disagrees with n_frames" in lib.tl_last_error()
        assert call(lib, n_frames=2, length=385) == -1 and b"disagrees with n_frames" in lib.tl_last_error()
    assert _analyse(lib, momentum=-0.1) == -1 and b"momentum" in lib.tl_last_error()
    assert _analyse(lib, first=2) == -1 and b"first" in lib.tl_last_error()
    assert _overlap_add(lib, N=65536) == -1 and b"65535" in lib.tl_last_error()


@pytest.mark.parametrize("kw", [dict(sr=24414, n_fft=2048, n_mels=128),
                                dict(sr=24414, n_fft=1024, n_mels=80),
                                dict(sr=24414, n_fft=512, n_mels=40, fmin=50, fmax=8000)])
def test_bin_pair_table_expands_to_the_dense_bank_exactly(kw):
    from decode_tonal_langauge_amd.utils.audio import bin_pair_table, mel_filterbank, pack_mel_filterbank
    dense = mel_filterbank(**kw)
    bin_bands, bin_weights = bin_pair_table(dense)
    assert bin_bands.dtype == np.int32 and bin_bands.shape == (dense.shape[1], 2) and bin_weights.dtype == np.float64
    again = np.zeros(dense.shape)
    for k in range(dense.shape[1]):
        for b, w in zip(bin_bands[k], bin_weights[k]):
            if b >= 0:
                again[b, k] = w
            else:
                assert w == 0.0
    assert np.array_equal(again, dense.astype(np.float64))
    assert pack_mel_filterbank(dense)[1].size <= kw["n_fft"] + 2        # the bound tl_mel_invert sizes its LDS copy by
    with pytest.raises(ValueError, match="at most two"):
        bin_pair_table(np.ones((3, 4)))


@pytest.mark.parametrize("noisy", [False, True], ids=["true", "noise_3dB"])
@pytest.mark.parametrize("name", list(mc.CASES))
def test_mel_to_linear_reaches_the_residual_of_scipy_nnls(name, noisy):
    fb = mc.bank(mc.CASES[name][2])
    lin, mel = mc.host_linear(name, noisy), mc.mel_power(name, noisy)
    assert lin.shape == (mel.shape[0], fb.shape[1], mel.shape[2]) and np.isfinite(lin).all()
    assert (lin >= 0.0).all()
    frames, ref = mc.scipy_residual(name, noisy)
    for n in range(lin.shape[0]):
        res = mc.relative_residual(fb, lin[n], mel[n])[frames]
        print(f"[{name} trial {n}] worst residual {res.max():.3e}, scipy {ref[n].max():.3e}, excess {(res - ref[n]).max():.3e}")
        assert (res <= ref[n] + mc.RESIDUAL_EXCESS).all(), (name, n, float((res - ref[n]).max()))


def test_mel_to_linear_arguments_and_determinism():
    from decode_tonal_langauge_amd.utils.audio import NNLS_ITER_DEFAULT, mel_to_linear
    fb = mc.bank(mc.CASES["nfft256"][2])
    p = mc.mel_power("nfft256")[0]
    assert NNLS_ITER_DEFAULT >= 1
    assert np.array_equal(mel_to_linear(p, fb, nnls_iter=50), mel_to_linear(p.astype(np.float64), fb, 50))
    one = mel_to_linear(p, fb, nnls_iter=1)                      # one projected gradient step from zero
    L = np.linalg.svd(fb, compute_uv=False)[0] ** 2
    assert np.allclose(one, np.maximum(fb.T @ p / L, 0.0), rtol=1e-13, atol=0.0)
    with pytest.raises(ValueError, match="nnls_iter"):
        mel_to_linear(p, fb, nnls_iter=0)
    with pytest.raises(ValueError, match="n_mels"):
        mel_to_linear(p[:-1], fb)


def test_batch_functions_check_their_arguments_before_they_need_a_gpu():
    import torch
    from decode_tonal_langauge_amd.utils.audio import griffinlim_batch, mel_to_audio, mel_to_audio_batch
    mels = np.full((2, 40 * 6), -30.0, dtype=np.float32)
    with pytest.raises(TypeError) as batch_err:
        mel_to_audio_batch(mels, 40, n_fft=512, htk=True)
    with pytest.raises(TypeError) as host_err:
        mel_to_audio(mels[0], 40, n_fft=512, htk=True)
    assert str(batch_err.value) == str(host_err.value)
    with pytest.raises(ValueError, match="256, 512, 1024, 2048"):
        mel_to_audio_batch(mels, 40, n_fft=300)
    with pytest.raises(ValueError, match="2D"):
        mel_to_audio_batch(mels[0], 40, n_fft=512)
    with pytest.raises(ValueError, match="win_length"):
        mel_to_audio_batch(mels, 40, n_fft=512, win_length=513)
    with pytest.raises(ValueError, match="hop_length"):
        mel_to_audio_batch(mels, 40, n_fft=512, hop_length=0)
    with pytest.raises(ValueError, match="gaps"):
        mel_to_audio_batch(mels, 40, n_fft=512, hop_length=401, win_length=400)
    with pytest.raises(ValueError, match="power"):
        mel_to_audio_batch(mels, 40, n_fft=512, power=3)
    with pytest.raises(ValueError, match="n_mels"):
        mel_to_audio_batch(mels, 0, n_fft=512)
    with pytest.raises(ValueError, match="n_mels"):
        mel_to_audio_batch(np.zeros((2, 300 * 2)), 300, n_fft=512)
    with pytest.raises(ValueError, match="whole number of frames"):
        mel_to_audio_batch(mels, 37, n_fft=512)
    with pytest.raises(ValueError, match="nnls_iter"):
        mel_to_audio_batch(mels, 40, n_fft=512, nnls_iter=0)
    with pytest.raises(ValueError, match="no trial"):
        mel_to_audio_batch(mels[:0], 40, n_fft=512)
    with pytest.raises(ValueError, match="3D"):
        griffinlim_batch(np.zeros((257, 6)))
    with pytest.raises(ValueError, match="256, 512, 1024, 2048"):
        griffinlim_batch(np.zeros((2, 151, 6)))
    with pytest.raises(ValueError, match="gaps"):
        griffinlim_batch(np.zeros((2, 257, 6)), hop_length=300, win_length=256)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            mel_to_audio_batch(mels, 40, n_fft=512)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            griffinlim_batch(np.zeros((2, 257, 6)))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mel_to_audio_batch(torch.from_numpy(mels), 40, n_fft=512)
