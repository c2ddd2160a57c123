"""GPU: ``tl_yin_f0`` through ``utils.audio.yin_f0_batch`` against the long-double restatement of tests/yin_ref.py, and the
``--f0_metrics`` switch of ``train_synthesizer``.

Bounds (u = 2^-53; derived, not measured - the observed figures are in profiles/f0_tracking.md):
 * CMND: relative error <= eps_c = (2 W + pmax + 8) u.  d[tau] is a sum of W non-negative terms, each a rounded difference
   squared, so the gamma_n bound holds in any order; the running sum over the lags is again a sum of non-negative terms; two
   divisions and the DBL_MIN add make the rest.  An exact zero of the reference is an exact zero of the kernel.
 * period_index: equal wherever every comparison of the pick has a margin above 1e-11 max(1, |c|) (>= 2 eps_c here); two
   exact zeros count as decided.  At most 2 % of a geometry's frames may be left out.
 * f0 from the kernel's own CMND values by the float64 formula: within 2 ulp; aperiodicity == cmnd[i].
 * f0 against long double on agreeing frames: eps_c cmax3 (1 + 4 |shift|) / (|a| p) + 4 u, from shift = -b / a.
 * rms: (W + 4) u relative.
"""
import json
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

from decode_tonal_langauge_amd.utils import audio
from tests import golden_inputs as gi
from tests import yin_ref as yr

pytestmark = pytest.mark.gpu

U = yr.U
DTYPES = ("float32", "float64")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch.device("cuda:0")


_GOT = {}


def _run(name, dt, dev):
    """The kernel's outputs for geometry ``name`` on its five clips, as NumPy arrays; one launch per (geometry, dtype)."""
    if (name, dt) not in _GOT:
        sr, fl, W, hop, fmin, fmax, S = yr.GEOMETRIES[name]
        x = torch.from_numpy(yr.clips(sr, S).astype(dt)).to(dev)
        got = audio.yin_f0_batch(x, sr, fmin, fmax, fl, W, hop, yr.THRESHOLD, return_cmnd=True)
        _GOT[name, dt] = audio.F0TrackCmnd(*(t.cpu().numpy() for t in got))
    return _GOT[name, dt]


def _rel(got, ref):
    """Largest relative error over the non-zero entries of the long-double ``ref``; zeros must be met exactly."""
    got, zero = np.asarray(got).astype(np.longdouble), ref == 0
    assert (got[zero] == 0).all(), "an exact zero of the reference is not an exact zero of the kernel"
    if zero.all():
        return 0.0
    return float((np.abs(got - ref)[~zero] / np.abs(ref[~zero])).max())


def _check(got, ref, sr, W, pmin, pmax, what):
    """Checks 1 - 5 of one call against the long-double reference ``ref`` (fields stacked like the outputs)."""
    eps = yr.eps_c(W, pmax)
    nc = pmax - pmin + 1
    assert got.cmnd.shape == ref.cmnd.shape and got.f0.shape == ref.f0.shape
    # 1. the curve
    err = _rel(got.cmnd, ref.cmnd)
    print(f"{what}: CMND rel err {err:.2e} (bound {eps:.2e})")
    assert err <= eps, (what, err, eps)
    # 2. the pick
    left_out = int((~ref.decidable).sum())
    print(f"{what}: {left_out} of {ref.decidable.size} frames left out of the index comparison")
    assert left_out <= 0.02 * ref.decidable.size, (what, left_out)
    agree = got.period_index == ref.period_index
    assert agree[ref.decidable].all(), (what, np.argwhere(~agree & ref.decidable).tolist())
    # 3. f0 and aperiodicity from the kernel's own curve
    i = got.period_index.astype(np.int64)
    assert i.min() >= 0 and i.max() < nc
    take = lambda k: np.take_along_axis(got.cmnd, np.clip(k, 0, nc - 1)[..., None], axis=-1)[..., 0]
    c0, cm, cp = take(i), take(i - 1), take(i + 1)
    assert np.array_equal(got.aperiodicity, c0), what
    interior = (i > 0) & (i < nc - 1)
    a = cp + cm - 2.0 * c0
    b = (cp - cm) / 2.0
    with np.errstate(divide="ignore", invalid="ignore"):
        shift = np.where(interior & (np.abs(b) < np.abs(a)), -b / a, 0.0)
    own = sr / (pmin + i + shift)
    ulps = np.abs(got.f0 - own) / np.spacing(np.abs(own))
    print(f"{what}: f0 against the float64 formula on its own CMND: {ulps.max():.1f} ulp")
    assert ulps.max() <= 2, (what, ulps.max())
    # 4. f0 against long double where the index agrees
    ref_i = ref.period_index.astype(np.int64)
    r_take = lambda k: np.take_along_axis(ref.cmnd, np.clip(k, 0, nc - 1)[..., None], axis=-1)[..., 0]
    cmax3 = np.maximum(np.maximum(np.abs(r_take(ref_i)), np.abs(r_take(ref_i - 1))), np.abs(r_take(ref_i + 1)))
    p = pmin + ref_i + ref.shift
    ref_interior = (ref_i > 0) & (ref_i < nc - 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        moved = np.where(ref_interior, eps * cmax3 * (1 + 4 * np.abs(ref.shift)) / (np.abs(ref.a) * p), 0.0)
    bound = np.where(np.isnan(moved), np.inf, moved) + 4 * U
    df = np.abs(got.f0.astype(np.longdouble) - ref.f0) / ref.f0
    print(f"{what}: f0 rel err on agreeing frames {float(df[agree].max()):.2e}")
    assert (df[agree] <= bound[agree]).all(), (what, float((df / bound)[agree].max()))
    # 5. rms
    err = _rel(got.rms, ref.rms)
    print(f"{what}: rms rel err {err:.2e} (bound {(W + 4) * U:.2e})")
    assert err <= (W + 4) * U, (what, err)


def _stack(refs):
    return yr.Ref(*(np.stack([getattr(r, k) for r in refs]) for k in yr.Ref._fields))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name", list(yr.GEOMETRIES))
def test_against_long_double(dev, name, dt):
    sr, fl, W, hop, fmin, fmax, S = yr.GEOMETRIES[name]
    pmin, pmax = yr.periods(sr, fl, W, fmin, fmax)
    ref = yr.reference(name, dt, "longdouble")
    if name == "D":
        # the centre padding (128) exceeds W (96): the window of frame 0 is all zeros and the curve starts with a run of exact
        # zeros, whose ties the zero rule settles
        assert ((ref.cmnd[:, 0] == 0).sum(axis=-1) == 25).all() and (ref.period_index[:, 0] == 0).all()
    _check(_run(name, dt, dev), ref, sr, W, pmin, pmax, f"{name}/{dt}")


@pytest.mark.parametrize("name", list(yr.GEOMETRIES))
def test_end_to_end_truth(dev, name):
    """The level clip reads 220 Hz behind its lead, the noise clip is nowhere periodic."""
    sr, fl, W, hop, fmin, fmax, S = yr.GEOMETRIES[name]
    got = _run(name, "float64", dev)
    first = -(-(S // 6 + fl // 2) // hop)                        # the first frame that starts behind the lead
    assert first < got.f0.shape[1] - 1
    assert (np.abs(sr / got.f0[0, first:] - sr / 220.0) <= 0.5).all(), sr / got.f0[0, first:]
    # a frame whose window x[0:W] lies wholly in the centre padding holds none of the clip (rms 0; frame 0 of D): it is a
    # frame of silence, not of noise
    of_the_clip = got.rms[4] > 0
    assert of_the_clip.sum() >= got.rms.shape[1] - 1
    assert (got.aperiodicity[4][of_the_clip] >= 0.1).all()


def test_single_clip_strided_rows_and_repeat(dev):
    sr, fl, W, hop, fmin, fmax, S = yr.GEOMETRIES["A"]
    x = yr.clips(sr, S)
    base = _run("A", "float64", dev)
    xd = torch.from_numpy(x).to(dev)
    one = audio.yin_f0_batch(xd[2:3], sr, fmin, fmax, fl, W, hop, yr.THRESHOLD, return_cmnd=True)
    for got, want in zip(one, base):
        assert np.array_equal(got.cpu().numpy(), want[2:3])
    # every second row of a tensor that is wider than the clips: read in place through its row stride
    wide = torch.full((10, S + 37), float("nan"), dtype=torch.float64, device=dev)
    wide[::2, :S] = xd
    view = wide[::2, :S]
    assert view.stride() == (2 * (S + 37), 1)
    strided = audio.yin_f0_batch(view, sr, fmin, fmax, fl, W, hop, yr.THRESHOLD, return_cmnd=True)
    again = audio.yin_f0_batch(view, sr, fmin, fmax, fl, W, hop, yr.THRESHOLD, return_cmnd=True)
    for got, twice, want in zip(strided, again, base):
        assert np.array_equal(got.cpu().numpy(), want)
        assert torch.equal(got, twice)                                       # two runs: the same bits


def test_clip_shorter_than_a_frame(dev):
    sr, fl, W, hop, fmin, fmax, _ = yr.GEOMETRIES["A"]
    pmin, pmax = yr.periods(sr, fl, W, fmin, fmax)
    x = yr.clips(sr, 700)[:, 300:400]                                        # S = 100: padding at both ends of every frame
    for dt in DTYPES:
        xs = np.ascontiguousarray(x.astype(dt))
        got = audio.yin_f0_batch(xs, sr, fmin, fmax, fl, W, hop, yr.THRESHOLD, device=dev, return_cmnd=True)
        assert got.f0.shape == (5, 2)
        ref = _stack([yr.yin_ref(row, sr, fl, W, hop, fmin, fmax, dtype=np.longdouble) for row in xs])
        _check(got, ref, sr, W, pmin, pmax, f"short/{dt}")


def test_all_zero_clip_is_bit_equal(dev):
    for name in ("A", "D"):
        sr, fl, W, hop, fmin, fmax, S = yr.GEOMETRIES[name]
        pmin, pmax = yr.periods(sr, fl, W, fmin, fmax)
        x = np.zeros((2, S), dtype=np.float32)
        got = audio.yin_f0_batch(x, sr, fmin, fmax, fl, W, hop, yr.THRESHOLD, device=dev, return_cmnd=True)
        ref = yr.yin_ref(x[0], sr, fl, W, hop, fmin, fmax)
        assert (ref.period_index == 0).all() and (ref.f0 == sr / pmin).all()          # the lowest index the rule gives
        for k in audio.F0TrackCmnd._fields:
            assert np.array_equal(getattr(got, k)[0], getattr(ref, k)) and np.array_equal(getattr(got, k)[1], getattr(ref, k)), k


def test_longest_frame_and_lag_range(dev):
    """frame_length 4096 with a short window: 4079 lags (16 passes of the block, 16 lags per lane in the scan) and more than
    64 KB of LDS, the size at which the entry point raises the kernel's dynamic LDS limit."""
    sr, fl, W, hop, fmin, fmax, S = 8000, 4096, 16, 2048, 1.0, 1000.0, 5000
    pmin, pmax = yr.periods(sr, fl, W, fmin, fmax)
    assert (pmin, pmax) == (8, 4079) and (fl + pmax + 1) * 8 + 256 > 65536
    x = yr.clips(sr, S)[:2]
    got = audio.yin_f0_batch(x, sr, fmin, fmax, fl, W, hop, yr.THRESHOLD, device=dev, return_cmnd=True)
    ref = _stack([yr.yin_ref(row, sr, fl, W, hop, fmin, fmax, dtype=np.longdouble) for row in x])
    _check(got, ref, sr, W, pmin, pmax, "4096")


def test_plumbing(dev):
    sr, fl, W, hop, fmin, fmax, S = yr.GEOMETRIES["A"]
    pmin, pmax = yr.periods(sr, fl, W, fmin, fmax)
    x = yr.clips(sr, S).astype(np.float32)
    n_frames = 1 + S // hop
    on_dev = audio.yin_f0_batch(torch.from_numpy(x).to(dev), sr, fmin, fmax, fl, W, hop)
    assert isinstance(on_dev, audio.F0Track) and len(on_dev) == 4
    assert all(isinstance(t, torch.Tensor) and t.is_cuda and t.shape == (5, n_frames) for t in on_dev)
    assert on_dev.period_index.dtype == torch.int32 and on_dev.f0.dtype == torch.float64
    host = audio.yin_f0_batch(x, sr, fmin, fmax, fl, W, hop, device=dev, return_cmnd=True)
    assert isinstance(host, audio.F0TrackCmnd) and all(isinstance(t, np.ndarray) for t in host)
    assert host.cmnd.shape == (5, n_frames, pmax - pmin + 1) and host.cmnd.dtype == np.float64
    for a, b in zip(on_dev, host):
        assert np.array_equal(a.cpu().numpy(), b)
    # the derived defaults: win_length = frame_length // 2, hop = frame_length // 4
    dflt = audio.yin_f0_batch(x, sr, fmin, fmax, fl, device=dev)
    assert np.array_equal(dflt.f0, host.f0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        audio.yin_f0_batch(torch.from_numpy(x), sr, fmin, fmax, fl)


# ---------------------------------------------------------------------------------------------- train_synthesizer --f0_metrics
N_TRIALS, N_CH, N_T, N_MEL, N_FRAMES, N_FFT, HOP, SR = 23, 12, 64, 16, 12, 256, 64, 8000


def _params(root, tag, f0_metrics):
    out = root / tag
    return Namespace(sample_path=str(root / "samples.npz"), subject_id="1", result_file=str(out / "results.csv"), figure_dir=None,
                     audio_dir=str(out / "audio"), channel_file=str(root / "channels.json"), config_file=str(root / "config.json"),
                     model_name="lite", syllable_model_path=str(root / "syl.pt"), tone_model_path=str(root / "tone.pt"),
                     synthesis_model_name="SynthesisLite", syllable_model_name="logistic", tone_model_name="logistic",
                     audio_sampling_rate=SR, seed=42, repeat=1, verbose=0, train_ratio=0.8, device="cuda:0", batch_size=4,
                     epochs=2, lr=0.0005, resident=False, ensemble=False, n_audio_samples=3, f0_metrics=f0_metrics)


def test_train_synthesizer_f0_metrics(dev, tmp_path):
    import pandas as pd
    from scipy.io import wavfile
    from decode_tonal_langauge_amd import train_synthesizer as ts
    from decode_tonal_langauge_amd.models.simple_classifiers import LogisticRegressionClassifier
    root = tmp_path
    rng = np.random.default_rng(4)
    np.savez(root / "samples.npz", ecog=rng.standard_normal((N_TRIALS, N_CH, N_T)).astype(np.float32),
             mel=(-40 + 10 * rng.standard_normal((N_TRIALS, N_MEL * N_FRAMES))).astype(np.float32))
    chans = {"active_channels": list(range(N_CH)), "tone_discriminative": [0, 1, 2], "syllable_discriminative": [3, 4]}
    (root / "channels.json").write_text(json.dumps(chans))
    config = {"mel_kwargs": {"n_mels": N_MEL, "n_fft": N_FFT, "hop_length": HOP}, "tone_dynamic_mapping": gi.TONE_MAP,
              "n_syllables": 2, "n_tones": 4}
    (root / "config.json").write_text(json.dumps(config))
    torch.manual_seed(8)
    torch.save(LogisticRegressionClassifier(3 * N_T, 4).state_dict(), root / "tone.pt")
    torch.save(LogisticRegressionClassifier(2 * N_T, 2).state_dict(), root / "syl.pt")
    ts.train(_params(root, "plain", False))
    ts.train(_params(root, "f0", True))
    plain, f0dir = root / "plain" / "audio", root / "f0" / "audio"
    assert not os.path.exists(plain / "f0_metrics.json") and not os.path.exists(plain / "f0_tracks.npz")
    metrics = json.loads((f0dir / "f0_metrics.json").read_text())
    assert set(metrics) == {"f0_rmse_cents", "f0_corr", "gross_pitch_error", "voicing_error", "n_voiced"}
    assert all(isinstance(metrics[k], float) for k in metrics if k != "n_voiced") and isinstance(metrics["n_voiced"], int)
    waves = np.stack([wavfile.read(f0dir / f"{tag}_audio_{i}.wav")[1] for tag in ("origin", "recon") for i in range(3)])
    assert waves.shape == (6, HOP * (N_FRAMES - 1)) and waves.dtype == np.float32
    direct = audio.yin_f0_batch(waves, SR, 60.0, 500.0, frame_length=N_FFT, hop_length=HOP, device=dev)
    tracks = np.load(f0dir / "f0_tracks.npz")
    assert set(tracks.files) == set(audio.F0Track._fields)
    for k in audio.F0Track._fields:
        assert tracks[k].shape == (6, 1 + waves.shape[1] // HOP) and np.array_equal(tracks[k], getattr(direct, k)), k
    a, b = pd.read_csv(root / "plain" / "results.csv"), pd.read_csv(root / "f0" / "results.csv")
    assert list(a.columns) == list(b.columns) and len(b) == 1
