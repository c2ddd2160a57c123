"""GPU: the way back from mel spectrograms - ``tl_mel_invert`` (FISTA mel inversion), ``griffinlim_batch`` (tl_gl_synth,
tl_gl_analyse, tl_gl_overlap_add) and ``mel_to_audio_batch`` - against ``scipy.optimize.nnls`` and the float64 host functions
``mel_to_linear`` / ``griffinlim`` of ``utils.audio``.  Inputs and bounds: ``tests/mel_inverse_cases.py``.

Bounds.
  inversion vs scipy:  x >= 0 exactly and per frame ||fb x - p|| / ||p|| <= scipy's + 1e-4: ten times the worst excess of the
                       CPU iteration sweep at the default count (profiles/mel_inverse.md).
  inversion vs host:   |gpu - host| <= 1.02e-9 max(host trial) = 1 000 x the spread of the host statement when every gradient
                       is perturbed by 1e-15 relative.  The kernel follows the order of operations the host statement
                       writes out (utils.audio.bank_operators), so the observed deviation is expected to be zero.
  Griffin-Lim vs host: |gpu - host| <= 1e-9 max|host row|.  A 1e-15 relative perturbation of every resynthesised signal moves
                       the 32-iteration host output by 7e-15 .. 2.3e-11 of its peak on these inputs; 1e-9 leaves the room
                       for the transform's own rounding.
  end to end:          |gpu - host| <= 2e-7 max|host row| against griffinlim(mel_to_linear(.) ** (1 / power)) cast to
                       float32: float32 output rounding on top of the two bounds above."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import mel_inverse_cases as mc
from tests import parity_record

pytestmark = pytest.mark.gpu
ALL = list(mc.CASES)


def _gl_kwargs(name):
    N, S, kw, keep = mc.CASES[name]
    gl = {k: kw[k] for k in ("hop_length", "win_length") if k in kw}
    gl["length"] = S if keep else None
    return gl


def _host_mag(name):
    return np.power(mc.host_linear(name), 1.0 / mc.CASES[name][2].get("power", 2.0))


@functools.lru_cache(maxsize=None)
def _host_griffinlim(name: str, n_iter: int) -> np.ndarray:
    from decode_tonal_langauge_amd.utils.audio import griffinlim
    ref = np.stack([griffinlim(m, n_iter=n_iter, **_gl_kwargs(name)) for m in _host_mag(name)])
    ref.setflags(write=False)
    return ref


def _gpu_linear(name, noisy=False, power=1):
    from decode_tonal_langauge_amd.utils.audio import mel_invert_batch
    kw = mc.CASES[name][2]
    p = torch.from_numpy(np.array(mc.mel_power(name, noisy))).cuda()
    out = mel_invert_batch(p, mc.SR, kw.get("n_fft", 2048), kw["n_mels"], fmin=kw.get("fmin", 0.0), fmax=kw.get("fmax"),
                           power=power)
    return out.cpu().numpy()


# ---------------------------------------------------------------------------------------------- mel inversion
@pytest.mark.parametrize("noisy", [False, True], ids=["true", "noise_3dB"])
@pytest.mark.parametrize("name", ALL)
def test_invert_kernel_reaches_the_residual_of_scipy_nnls(name, noisy):
    fb, mel = mc.bank(mc.CASES[name][2]), mc.mel_power(name, noisy)
    lin = _gpu_linear(name, noisy)
    assert lin.shape == (mel.shape[0], fb.shape[1], mel.shape[2]) and lin.dtype == np.float64 and np.isfinite(lin).all()
    assert (lin >= 0.0).all()
    frames, ref = mc.scipy_residual(name, noisy)
    excess = max(float((mc.relative_residual(fb, lin[n], mel[n])[frames] - ref[n]).max()) for n in range(lin.shape[0]))
    tag = f"{name}_{'noisy' if noisy else 'true'}"
    print(f"[{tag}] worst excess of the relative residual over scipy {excess:.3e}")
    parity_record.record(f"mel_inverse_residual_{tag}", {"worst_excess_over_scipy": excess, "bound": mc.RESIDUAL_EXCESS})
    assert excess <= mc.RESIDUAL_EXCESS, (tag, excess)


@pytest.mark.parametrize("noisy", [False, True], ids=["true", "noise_3dB"])
@pytest.mark.parametrize("name", ALL)
def test_invert_kernel_matches_the_host_statement(name, noisy):
    lin, host = _gpu_linear(name, noisy), mc.host_linear(name, noisy)
    dev = np.abs(lin - host).max(axis=(1, 2)) / host.max(axis=(1, 2))
    tag = f"{name}_{'noisy' if noisy else 'true'}"
    print(f"[{tag}] max |gpu - mel_to_linear| / max(trial) {float(dev.max()):.3e}   over bound {float(dev.max()) / mc.INVERT_BOUND:.3f}")
    differing = int((lin != host).sum())                         # the kernel follows bank_operators' order: expected 0
    print(f"[{tag}] values that differ from mel_to_linear in any bit: {differing} of {lin.size}")
    parity_record.record(f"mel_inverse_invert_{tag}", {"max_abs_err_over_trial_max": float(dev.max()),
                                                       "values_differing": differing, "values": int(lin.size),
                                                       "max_abs_err": float(np.abs(lin - host).max()),
                                                       "worst_over_bound": float(dev.max()) / mc.INVERT_BOUND})
    assert (dev <= mc.INVERT_BOUND).all(), (tag, dev.tolist())


def test_invert_kernel_power_two_output_is_the_square_root():
    x, mag = _gpu_linear("nfft512", power=1), _gpu_linear("nfft512", power=2)
    assert np.allclose(mag, np.sqrt(x), rtol=4e-16, atol=0.0)
    again = _gpu_linear("nfft512", power=2)
    assert np.array_equal(mag, again)                            # a fixed iteration count and no atomics: the same bits


def test_invert_kernel_iteration_count_is_honoured():
    from decode_tonal_langauge_amd.utils.audio import mel_invert_batch, mel_to_linear
    kw = mc.CASES["nfft256"][2]
    p = mc.mel_power("nfft256")
    got = mel_invert_batch(torch.from_numpy(np.array(p)).cuda(), mc.SR, 256, 20, nnls_iter=7, power=1).cpu().numpy()
    host = np.stack([mel_to_linear(q, mc.bank(kw), nnls_iter=7) for q in p])
    assert np.allclose(got, host, rtol=1e-12, atol=1e-12 * host.max())


# ---------------------------------------------------------------------------------------------- Griffin-Lim
@pytest.mark.parametrize("n_iter", [4, 32])
@pytest.mark.parametrize("name", ALL)
def test_griffinlim_batch_matches_the_host_row_by_row(name, n_iter):
    from decode_tonal_langauge_amd.utils.audio import griffinlim_batch
    ref = _host_griffinlim(name, n_iter)
    got = griffinlim_batch(_host_mag(name), n_iter=n_iter, **_gl_kwargs(name))
    assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == ref.shape and np.isfinite(got).all()
    dev = np.abs(got - ref).max(axis=1) / np.abs(ref).max(axis=1)
    print(f"[{name} n_iter {n_iter}] max |gpu - host| / peak {float(dev.max()):.3e}   over bound {float(dev.max()) / mc.GL_BOUND:.3f}")
    parity_record.record(f"mel_inverse_griffinlim_{name}_iter{n_iter}", {"max_abs_err_over_peak": float(dev.max()),
                                                                        "worst_over_bound": float(dev.max()) / mc.GL_BOUND})
    assert (dev <= mc.GL_BOUND).all(), (name, n_iter, dev.tolist())


def test_griffinlim_batch_containers_chunks_and_empty_output(monkeypatch):
    from decode_tonal_langauge_amd.utils import audio as au
    mag, gl = _host_mag("nfft512"), _gl_kwargs("nfft512")
    base = au.griffinlim_batch(mag, n_iter=4, **gl)
    out = au.griffinlim_batch(torch.from_numpy(np.array(mag)).cuda(), n_iter=4, **gl)
    assert isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float64
    assert np.array_equal(out.cpu().numpy(), base)
    monkeypatch.setattr(au, "GL_WORKSPACE_BYTES", 1)             # one trial per chunk
    assert np.array_equal(au.griffinlim_batch(mag, n_iter=4, **gl), base)
    monkeypatch.undo()
    assert np.array_equal(au.griffinlim_batch(mag[1:], n_iter=4, **gl), base[1:])      # a trial does not see its neighbours
    other = au.griffinlim_batch(mag, n_iter=4, seed=1, **gl)
    assert not np.array_equal(other, base)
    # one frame and no length: a centred istft keeps hop * (T - 1) = 0 samples
    empty = au.griffinlim_batch(mag[:, :, :1], n_iter=4, hop_length=gl["hop_length"])
    assert empty.shape == (mag.shape[0], 0) and empty.dtype == np.float64
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        au.griffinlim_batch(torch.from_numpy(np.array(mag)))


# ---------------------------------------------------------------------------------------------- end to end
def _db_mels(name):
    """(N, n_mels * T) float32 dB mels with the convention of mel_to_audio (ref = 1e-4)."""
    from decode_tonal_langauge_amd.utils.audio import power_to_db
    mel = mc.mel_power(name)
    return power_to_db(mel, ref=1e-4, top_db=None).astype(np.float32).reshape(mel.shape[0], -1)


@pytest.mark.parametrize("name", ALL)
def test_mel_to_audio_batch_end_to_end(name):
    """The inversion returns the host statement's bits, so what is compared here is Griffin-Lim's deviation (1e-12) under the
    float32 rounding of both outputs.  Against a host statement that summed in another order this case missed the bound at
    n_fft 2048: profiles/mel_inverse.md, "End to end"."""
    from decode_tonal_langauge_amd.utils.audio import db_to_power, griffinlim, mel_to_audio_batch, mel_to_linear
    N, S, kw, keep = mc.CASES[name]
    power, fb, gl = kw.get("power", 2.0), mc.bank(kw), _gl_kwargs(name)
    extra = {k: kw[k] for k in ("n_fft", "fmin", "fmax", "power") if k in kw}
    db = _db_mels(name)
    got = mel_to_audio_batch(db, kw["n_mels"], mc.SR, **extra, **gl)
    T = db.shape[1] // kw["n_mels"]
    hop = kw.get("hop_length", kw.get("n_fft", 2048) // 4)
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == (N, S if keep else hop * (T - 1))
    assert np.isfinite(got).all() and np.abs(got).max() > 0
    out = mel_to_audio_batch(torch.from_numpy(db).cuda(), kw["n_mels"], mc.SR, **extra, **gl)
    assert isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float32
    assert np.array_equal(out.cpu().numpy(), got)
    worst = 0.0
    for n in range(N):
        lin = mel_to_linear(db_to_power(db[n].astype(np.float64).reshape(kw["n_mels"], -1), ref=0.0001), fb)
        ref = griffinlim(np.power(lin, 1.0 / power), **gl).astype(np.float32)
        dev = float(np.abs(got[n].astype(np.float64) - ref.astype(np.float64)).max() / np.abs(ref).max())
        worst = max(worst, dev)
    print(f"[{name}] max |gpu - host| / peak {worst:.3e}   over bound {worst / 2e-7:.3f}")
    parity_record.record(f"mel_inverse_end_to_end_{name}", {"max_abs_err_over_peak": worst, "worst_over_bound": worst / 2e-7})
    assert worst <= 2e-7, (name, worst)


def test_mel_to_audio_batch_linear_input_single_frame_and_errors():
    from decode_tonal_langauge_amd.utils.audio import mel_to_audio_batch
    N, S, kw, _ = mc.CASES["nfft256"]
    mel = mc.mel_power("nfft256")
    lin_in = mel_to_audio_batch(mel.reshape(N, -1), 20, mc.SR, mel_in_db=False, n_fft=256, hop_length=64, length=S)
    db_in = mel_to_audio_batch(_db_mels("nfft256"), 20, mc.SR, n_fft=256, hop_length=64, length=S)
    assert lin_in.shape == db_in.shape == (N, S) and lin_in.dtype == db_in.dtype == np.float32
    assert np.isfinite(lin_in).all() and np.isfinite(db_in).all() and np.abs(lin_in).max() > 0 and np.abs(db_in).max() > 0
    one = mel_to_audio_batch(np.full((3, 20), -30.0), 20, mc.SR, n_fft=256, hop_length=64)
    assert one.shape == (3, 0) and one.dtype == np.float32
    with pytest.raises(TypeError, match="unsupported keyword"):
        mel_to_audio_batch(_db_mels("nfft256"), 20, mc.SR, n_fft=256, htk=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mel_to_audio_batch(torch.zeros(2, 40), 20, n_fft=256)


def test_two_partial_tone_comes_back_with_the_spectral_convergence_of_the_host_test():
    from decode_tonal_langauge_amd.utils import audio as au
    sr = 8000
    t = np.arange(2 * sr) / sr
    y = 0.3 * np.sin(2 * np.pi * 440.0 * t) + 0.2 * np.sin(2 * np.pi * 1320.0 * t)
    kw = {"n_fft": 512, "hop_length": 128, "n_mels": 64}
    mel = au.audio_to_mel(y, sr, mel_in_db=False, mel_kwargs=kw)
    wave = au.mel_to_audio_batch(mel[None, :], 64, audio_sampling_rate=sr, mel_in_db=False, n_fft=512, hop_length=128,
                                 length=len(y))[0]
    assert wave.shape == y.shape and wave.dtype == np.float32 and np.isfinite(wave).all()
    mel2 = au.audio_to_mel(wave, sr, mel_in_db=False, mel_kwargs=kw)
    err = float(np.linalg.norm(np.sqrt(mel2) - np.sqrt(mel)) / np.linalg.norm(np.sqrt(mel)))
    print(f"[two_partial_tone] spectral convergence {err:.4f}")
    parity_record.record("mel_inverse_two_partial_tone", {"spectral_convergence": err, "bound": 0.35})
    assert err < 0.35


# ---------------------------------------------------------------------------------------------- wiring
def test_synthesiser_entry_point_writes_audio_through_the_batch_call(tmp_path, monkeypatch):
    import json
    import yaml
    from scipy.io.wavfile import read as read_wave
    from decode_tonal_langauge_amd.main import run_pipeline
    from decode_tonal_langauge_amd.utils import audio as au
    tmp, n_mels, frames = str(tmp_path), 80, 4
    rng = np.random.default_rng(0)
    N, C, T = 48, 24, 200
    np.savez(os.path.join(tmp, "subject_1.npz"), ecog=rng.standard_normal((N, C, T)).astype(np.float32), ecog_sf=200,
             mel=(-40.0 + 10 * rng.standard_normal((N, n_mels * frames))).astype(np.float32),
             tone=rng.integers(0, 4, N), syllable=rng.integers(0, 2, N))
    json.dump({"active_channels": list(range(C)), "tone_discriminative": [0, 1, 2, 3], "syllable_discriminative": [4, 5, 6, 7]},
              open(os.path.join(tmp, "channels.json"), "w"))
    json.dump({"mel_kwargs": {"n_mels": n_mels, "n_fft": 512, "hop_length": 128}, "n_syllables": 2, "n_tones": 4,
               "tone_dynamic_mapping": {"0": [3, 3, 3, 3, 3], "1": [1, 2, 3, 4, 5], "2": [3, 2, 1, 2, 4], "3": [5, 4, 3, 2, 1]}},
              open(os.path.join(tmp, "config.json"), "w"))
    params = dict(sample_path=os.path.join(tmp, "subject_1.npz"), subject_id="1",
                  result_file=os.path.join(tmp, "out", "results.csv"), audio_dir=os.path.join(tmp, "audio"),
                  channel_file=os.path.join(tmp, "channels.json"), config_file=os.path.join(tmp, "config.json"),
                  model_name="lite-test", synthesis_model_name="SynthesisLite", syllable_model_name="logistic",
                  tone_model_name="logistic", device="cuda:0", batch_size=8, epochs=2, repeat=1, verbose=0)
    ypath = os.path.join(tmp, "cfg.yaml")
    yaml.safe_dump({"training": {"module": "decode_tonal_langauge_amd.train_synthesizer", "params": params}}, open(ypath, "w"))
    calls = []
    batch = au.mel_to_audio_batch
    monkeypatch.setattr(au, "mel_to_audio_batch", lambda m, *a, **k: calls.append(np.asarray(m).shape) or batch(m, *a, **k))
    monkeypatch.setattr(au, "mel_to_audio", lambda *a, **k: pytest.fail("the host loop ran on a CUDA device"))
    run_pipeline(ypath)
    n_test = len(np.load(os.path.join(tmp, "audio", "mels.npz"))["origin"])
    assert 1 <= n_test <= 10 and calls == [(2 * n_test, n_mels * frames)]        # one call for originals and reconstructions
    for tag in ("origin", "recon"):
        for i in range(n_test):
            rate, wave = read_wave(os.path.join(tmp, "audio", f"{tag}_audio_{i}.wav"))
            assert rate == 24414 and wave.dtype == np.float32 and wave.shape == (128 * (frames - 1),)
            assert np.isfinite(wave).all() and np.abs(wave).max() > 0
    assert not os.path.exists(os.path.join(tmp, "audio", f"origin_audio_{n_test}.wav"))
