"""GPU: ``tl_welch_psd`` and ``tl_segment_moments`` through ``utils/diagnostics.py`` against the long-double evaluations of
tests/welch_ref.py, the two plot functions, and the preprocess stage's ``diagnostics`` switch.

Tolerance.  For every case two errors are taken against the long-double value, each as a fraction of the row's largest value
(for the moments, of |mean| + std): scipy's / NumPy's own, on the float64-widened input, and the kernel's.  The assertion is
``kernel <= MARGIN * max(reference error, eps)``, eps the float64 machine epsilon.  The rule for MARGIN: twice the largest
ratio kernel / max(reference, eps) of the first run on an MI355X, rounded up - and not above 8, which is what the kernel's FFT
factorisation, fixed-order sums and shuffle mean account for.  That run (profiles/spectral_diagnostics.md): largest ratio 1.80
over all Welch cases but one and 0.93 for the moments; 4.39 for the DC level of 1e4 under constant detrend (kernel 4.0e-13,
scipy 9.2e-14 of the row's largest value: the segment mean is good to a few ulps of the level only).  Twice 4.39 rounds up to
9; the bound is not raised for it: MARGIN = 8.  Every figure is printed before it is asserted (``pytest -s``).

Shapes: a few thousand samples a case.  F, the segments a workgroup transforms side by side, is 8, 4, 2, 1 at n_fft 256, 512,
1024, 2048; the segment counts straddle it."""
import os
from copy import deepcopy

import numpy as np
import pytest
import scipy.signal
import torch

from decode_tonal_langauge_amd import preprocess_main
from decode_tonal_langauge_amd.data_loading import synthetic
from decode_tonal_langauge_amd.utils import diagnostics, visualise
from tests import welch_ref

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float64).eps)
MARGIN = 8
FS = 400.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch.device("cuda:0")


def _length(nperseg, noverlap, n_seg, tail=0):
    return nperseg + (n_seg - 1) * (nperseg - noverlap) + tail


def _signal(seed, C, T, dtype, dc=0.0):
    """Noise on a slow drift and a 50 Hz line, so that the spectrum is not flat and detrending has something to remove."""
    rng = np.random.default_rng(seed)
    t = np.arange(T) / FS
    x = rng.standard_normal((C, T)) + 0.7 * np.sin(2 * np.pi * 50.0 * t) + 0.5 * t + rng.standard_normal((C, 1)) + dc
    return x.astype(dtype)


def _scipy(x, w, noverlap, nfft, detrend, scaling):
    return scipy.signal.welch(np.asarray(x, dtype=np.float64), fs=FS, window=w, nperseg=len(w), noverlap=noverlap, nfft=nfft,
                              detrend="constant" if detrend else False, return_onesided=True, scaling=scaling, axis=1,
                              average="mean")[1]


def _check_welch(label, x, window, nperseg, noverlap, nfft, detrend=True, scaling="density", slabs=(None,), data=None):
    """``welch_psd`` of ``data`` (default: ``x`` itself, a NumPy array) for every slab count against the long-double value
    of ``x``; every run twice, bit-equal.  Returns the last result."""
    w = window if isinstance(window, np.ndarray) else diagnostics.window_coefficients(window, nperseg)
    want = welch_ref.welch_ld(x, FS, w, noverlap, nfft, detrend, scaling)
    ref_err = welch_ref.rel_err(_scipy(x, w, noverlap, nfft, detrend, scaling), want)
    got = None
    for s in slabs:
        run = lambda: diagnostics.welch_psd(x if data is None else data, FS, window=window, nperseg=nperseg, noverlap=noverlap,
                                            nfft=nfft, detrend="constant" if detrend else False, scaling=scaling, _slabs=s)
        freqs, got = run()
        again = run()[1]
        if isinstance(got, torch.Tensor):
            freqs, got, again = freqs.cpu().numpy(), got.cpu().numpy(), again.cpu().numpy()
        assert got.dtype == np.float64 and got.shape == (x.shape[0], nfft // 2 + 1) and got.tobytes() == again.tobytes(), label
        assert np.array_equal(freqs, np.arange(nfft // 2 + 1) * (FS / nfft))
        err = welch_ref.rel_err(got, want)
        print(f"welch {label} slabs={s}: kernel {err:.3e} reference {ref_err:.3e} ratio {err / max(ref_err, EPS):.2f}")
        assert np.isfinite(got).all() and err <= MARGIN * max(ref_err, EPS), (label, s, err, ref_err)
    return got


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("nfft", diagnostics.WELCH_N_FFT)
def test_welch_sizes_segment_counts_and_slabs(dev, nfft, dtype):
    F = diagnostics.frames_per_workgroup(nfft)
    for n_seg in sorted({1, max(F - 1, 1), F, F + 1, 2 * F + 1}):
        x = _signal(nfft + n_seg, 3, _length(nfft, nfft // 2, n_seg), dtype)
        for C in (1, 3):
            _check_welch(f"nfft={nfft} {np.dtype(dtype).name} C={C} n_seg={n_seg}", x[:C], "hann", nfft, nfft // 2, nfft,
                         slabs=sorted({1, 2, n_seg}) + [None])


@pytest.mark.parametrize("noverlap,n_seg,tail", [(0, 3, 255), (128, 10, 127), (255, 41, 0), (255, 1, 0)])
def test_welch_overlaps_and_tails(dev, noverlap, n_seg, tail):
    T = _length(256, noverlap, n_seg, tail)                     # the tail of step - 1 samples fills no segment
    assert welch_ref.segments(T, 256, noverlap) == n_seg and (noverlap < 255 or T <= 256 + 40)
    _check_welch(f"noverlap={noverlap} n_seg={n_seg} tail={tail}", _signal(noverlap, 3, T, np.float64), "hann", 256, noverlap, 256,
                 slabs=(1, 2, None))


@pytest.mark.parametrize("nperseg", [199, 200])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_welch_padding_past_the_end_of_the_allocation(dev, nperseg, dtype):
    """nperseg < n_fft and T ending exactly on the last segment: the padded part of the last segment of the last row lies
    past the tensor; it is never read (the guard is the kernel's; the values say that nothing but zeros went in)."""
    noverlap = nperseg // 2
    x = _signal(nperseg, 3, _length(nperseg, noverlap, 9), dtype)
    on_device = torch.from_numpy(x).to(dev)
    assert on_device.numel() == x.size and on_device.is_contiguous()
    _check_welch(f"nperseg={nperseg} {np.dtype(dtype).name}", x, "hann", nperseg, noverlap, 256, slabs=(1, 2, None), data=on_device)


@pytest.mark.parametrize("scaling", ["density", "spectrum"])
@pytest.mark.parametrize("window", ["hann", "boxcar", "hanning"])
@pytest.mark.parametrize("detrend", [True, False], ids=["constant", "none"])
def test_welch_windows_scalings_and_detrend(dev, window, scaling, detrend):
    x = _signal(17, 3, _length(256, 128, 9, 50), np.float64)
    w = np.hanning(256) if window == "hanning" else window
    _check_welch(f"{window} {scaling} detrend={detrend}", x, w, 256, 128, 256, detrend=detrend, scaling=scaling)


@pytest.mark.parametrize("nfft", [256, 2048])
def test_welch_dc_level_under_constant_detrend(dev, nfft):
    x = _signal(23, 3, _length(nfft, nfft // 2, 5), np.float64, dc=1e4)
    _check_welch(f"dc=1e4 nfft={nfft}", x, "hann", nfft, nfft // 2, nfft, detrend=True, slabs=(1, None))


def test_welch_row_strided_view_and_return_types(dev):
    T = _length(256, 128, 9)
    x = _signal(29, 3, T, np.float32)
    base = torch.full((3, T + 37), float("nan"), dtype=torch.float32, device=dev)
    base[:, :T] = torch.from_numpy(x).to(dev)
    view = base[:, :T]
    assert view.stride(0) == T + 37 and not view.is_contiguous()
    from_view = _check_welch("row-strided view", x, "hann", 256, 128, 256, data=view)
    freqs, psd = diagnostics.welch_psd(x, FS)                                   # NumPy in -> NumPy out, the same bits
    assert isinstance(freqs, np.ndarray) and isinstance(psd, np.ndarray) and psd.tobytes() == from_view.tobytes()
    freqs, psd = diagnostics.welch_psd(view, FS)                                # CUDA in -> CUDA out on the input's device
    assert isinstance(freqs, torch.Tensor) and isinstance(psd, torch.Tensor) and freqs.device == psd.device == view.device
    assert freqs.dtype == psd.dtype == torch.float64
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        diagnostics.welch_psd(torch.zeros(2, 600), FS)


@pytest.mark.parametrize("detrend", [True, False], ids=["constant", "none"])
def test_welch_nan_stays_in_its_channel(dev, detrend):
    x = _signal(31, 3, _length(256, 128, 19), np.float64)
    kw = dict(detrend="constant" if detrend else False, _slabs=2)
    clean = diagnostics.welch_psd(x, FS, **kw)[1]
    x[1, 128 * 17 + 100] = np.nan                                               # in segments 16 and 17: the second slab
    got = diagnostics.welch_psd(x, FS, **kw)[1]
    assert np.isnan(got[1]).all()
    assert got[0].tobytes() == clean[0].tobytes() and got[2].tobytes() == clean[2].tobytes()


# ---------------------------------------------------------------------------------------------- segment moments
# L: the wave kernel up to 512 with its 64-lane edge, the workgroup kernel beyond, samples in registers up to 2048 and read
# a second time beyond
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("L", [1, 63, 64, 65, 512, 513, 1000, 1017, 2048, 2049, 2600])
def test_segment_moments(dev, L, dtype):
    for n_seg in (1, 3):
        for start, extra, dc in ((0.0, 5, 0.0), (2.0, 0, 0.0), (1.0, 0, 1e4)):       # s0 = start L; extra = 0: ends at T
            s0 = int(start * L)
            T = s0 + n_seg * L + extra
            rng = np.random.default_rng([L, n_seg, s0])
            x = (rng.standard_normal((3, T)) * rng.uniform(0.5, 2.0, (3, 1)) + rng.standard_normal((3, 1)) + dc).astype(dtype)
            want = welch_ref.moments_ld(x, s0, L, n_seg)
            ref_err = welch_ref.moments_err(*welch_ref.moments_f64(x, s0, L, n_seg), *want)
            mean, std = diagnostics.segment_mean_std(x, L, start=start, end=start + n_seg)
            again = diagnostics.segment_mean_std(x, L, start=start, end=start + n_seg)
            assert isinstance(mean, np.ndarray) and mean.dtype == std.dtype == np.float64 and mean.shape == std.shape == (3, n_seg)
            assert mean.tobytes() == again[0].tobytes() and std.tobytes() == again[1].tobytes()
            err = welch_ref.moments_err(mean, std, *want)
            print(f"moments L={L} {np.dtype(dtype).name} n_seg={n_seg} s0={s0} dc={dc:g}: kernel {err:.3e} reference "
                  f"{ref_err:.3e} ratio {err / max(ref_err, EPS):.2f}")
            assert np.isfinite(mean).all() and np.isfinite(std).all() and err <= MARGIN * max(ref_err, EPS), (L, n_seg, s0, dc)


@pytest.mark.parametrize("L", [64, 1000, 2600])
def test_segment_moments_nan_and_device_input(dev, L):
    x = _signal(L, 3, 3 * L + 9, np.float64)
    view = torch.from_numpy(np.concatenate([x, np.full((3, 11), np.nan)], axis=1)).to(dev)[:, :3 * L + 9]      # row stride > T
    mean, std = diagnostics.segment_mean_std(view, L, start=0.0, end=3.0)
    assert isinstance(mean, torch.Tensor) and mean.device == std.device == view.device and mean.dtype == torch.float64
    clean = diagnostics.segment_mean_std(x, L, start=0.0, end=3.0)
    assert mean.cpu().numpy().tobytes() == clean[0].tobytes() and std.cpu().numpy().tobytes() == clean[1].tobytes()
    x[1, 2 * L - 1] = np.nan                                                        # the last sample of (channel 1, segment 1)
    got = diagnostics.segment_mean_std(x, L, start=0.0, end=3.0)
    for g, c in zip(got, clean):
        assert np.isnan(g[1, 1]) and np.isnan(g).sum() == 1
        keep = ~np.isnan(g)
        assert g[keep].tobytes() == c[keep].tobytes()


# ---------------------------------------------------------------------------------------------- plots
def test_plots_write_a_png_from_a_cuda_tensor(dev, tmp_path):
    pytest.importorskip("matplotlib")
    x = torch.from_numpy(_signal(41, 4, 3100, np.float32)).to(dev)
    visualise.plot_psd(x, figure_path=str(tmp_path / "psd.png"))
    visualise.plot_channel_mean_std(x, 1000, start=0.0, end=3.0, figure_path=str(tmp_path / "moments.png"))
    for name in ("psd.png", "moments.png"):
        with open(tmp_path / name, "rb") as f:
            assert f.read(8) == b"\x89PNG\r\n\x1a\n" and os.path.getsize(tmp_path / name) > 1000


# ---------------------------------------------------------------------------------------------- the stage hook
CHAIN = [
    {"module": "preprocess.downsample", "params": {"downsample_freq": 400}},
    {"module": "preprocess.frequency_filter", "params": {"bands": [
        {"method": "hilbert", "params": {"freq_ranges": [70., 150.], "envelope": True}}]}},
    {"module": "preprocess.zscore_rereference", "params": {"rereference_interval": [0., 2.]}},
]


def _stage_config(tree, out, **pipeline):
    return {"preprocess": {"module": "preprocess_main", "params": {
        "pipeline": {"module": "preprocess.pipelines.subject_block",
                     "params": {"subject_dirs": tree["subject_dirs"], "subject_ids": tree["subject_ids"], "figures": False,
                                **pipeline}},
        "io": {"module": "preprocess.io.npz_blocks", "params": {"root_dir": tree["root_dir"], "output_dir": out}},
        "preprocessor": {"module": "preprocess.preprocessor"},
        "modalities": {"ecog": {"type": "signal", "preprocessing": {"steps": deepcopy(CHAIN)}}, "audio": {"type": "signal"}}}}}


def test_stage_writes_one_summary_per_step_and_changes_no_block(dev, tmp_path):
    tree = synthetic.write_raw_tree(str(tmp_path / "raw"), {1: {1: 3.0, 2: 4.0}}, n_channels=6, audio_samples=4000, seed=3)
    plain = preprocess_main.run(_stage_config(tree, str(tmp_path / "plain")))
    with_d = preprocess_main.run(_stage_config(tree, str(tmp_path / "diag"), diagnostics=True))
    assert "diagnostics" not in os.listdir(plain) and "diagnostics" in os.listdir(with_d)
    for block, (raw_n, n) in ((1, (3051, 1199)), (2, (4069, 1600))):
        for modality in ("ecog", "audio"):
            with open(os.path.join(plain, "subject_1", f"B{block}_{modality}.npz"), "rb") as a, \
                    open(os.path.join(with_d, "subject_1", f"B{block}_{modality}.npz"), "rb") as b:
                assert a.read() == b.read(), (block, modality)
        where = os.path.join(with_d, "diagnostics", "subject_1", f"block_{block}")
        assert os.listdir(where) == ["ecog"]                                         # the audio has no steps
        names = ["step0_input.npz", "step1_downsample.npz", "step2_frequency_filter.npz", "step3_zscore_rereference.npz"]
        assert sorted(os.listdir(os.path.join(where, "ecog"))) == names
        with np.load(os.path.join(tree["blocks"][(1, block)], "ecog.npz")) as raw:
            first = raw["data"]
        with np.load(os.path.join(with_d, "subject_1", f"B{block}_ecog.npz")) as saved:
            last = saved["data"]
        for name, data, fs, T in ((names[0], first, 1017.25, raw_n), (names[1], None, 400, n), (names[2], None, 400, n),
                                  (names[3], last, 400, n)):
            with np.load(os.path.join(where, "ecog", name)) as d:
                assert sorted(d.files) == ["freqs", "psd", "seg_mean", "seg_std", "signal_freq"]
                assert d["signal_freq"] == fs and d["psd"].shape == (6, 129) and d["psd"].dtype == np.float64
                assert d["seg_mean"].shape == d["seg_std"].shape == (6, T // int(fs))
                assert np.isfinite(d["psd"]).all() and np.isfinite(d["seg_std"]).all()
                if data is not None:                                                  # the stage's own saved array of that step
                    freqs, psd = diagnostics.welch_psd(data, fs)
                    mean, std = diagnostics.segment_mean_std(data, fs, start=0.0, end=float(T // int(fs)))
                    assert d["freqs"].tobytes() == freqs.tobytes() and d["psd"].tobytes() == psd.tobytes()
                    assert d["seg_mean"].tobytes() == mean.tobytes() and d["seg_std"].tobytes() == std.tobytes()
                    assert welch_ref.rel_err(psd, welch_ref.welch_f64(data, fs, diagnostics.window_coefficients("hann", 256), 128,
                                                                      256, True)) < 1e-12


def test_short_recording_writes_the_keys_it_can(dev):
    x = torch.from_numpy(_signal(43, 2, 300, np.float64)).to(dev)
    assert sorted(diagnostics.summarise(x[:, :200], 100.0)) == ["seg_mean", "seg_std", "signal_freq"]       # under 256 samples
    assert sorted(diagnostics.summarise(x, 400.0)) == ["freqs", "psd", "signal_freq"]                       # under a second
    assert sorted(diagnostics.summarise(x[:, :100], 400.0)) == ["signal_freq"]
    assert diagnostics.summarise(x, 100.0)["seg_mean"].shape == (2, 3)
