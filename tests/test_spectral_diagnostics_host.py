"""No GPU: the host side of the recording diagnostics (utils/diagnostics.py) - the float64 restatement of Welch's method the
GPU tests lean on is pinned to scipy and matplotlib, the slab planner, what the two C entries and the Python functions
refuse, and the stage hook's switch."""
import os
from argparse import Namespace

import numpy as np
import pytest
import scipy.signal

from decode_tonal_langauge_amd.data_loading import synthetic
from decode_tonal_langauge_amd.preprocess import preprocessor
from decode_tonal_langauge_amd.preprocess.pipelines import subject_block
from decode_tonal_langauge_amd.utils import diagnostics
from tests import welch_ref

# (nfft, nperseg, noverlap, n_seg, tail, window, detrend, scaling): the shapes of the GPU cases
WELCH_CASES = [
    (256, 256, 128, 9, 0, "hann", True, "density"),
    (256, 256, 0, 3, 255, "boxcar", False, "spectrum"),
    (256, 256, 255, 41, 0, "hann", True, "density"),
    (256, 199, 99, 5, 0, "hann", True, "density"),
    (256, 200, 100, 5, 0, "hanning", False, "spectrum"),
    (512, 512, 256, 5, 17, "hann", False, "density"),
    (1024, 1024, 512, 3, 0, "hann", True, "spectrum"),
    (2048, 2048, 1024, 3, 100, "hanning", True, "density"),
]


def _window(name, nperseg):
    return np.hanning(nperseg) if name == "hanning" else diagnostics.window_coefficients(name, nperseg)


@pytest.mark.parametrize("case", WELCH_CASES, ids=lambda c: "-".join(map(str, c)))
def test_restatement_is_scipy_welch(case):
    nfft, nperseg, noverlap, n_seg, tail, name, detrend, scaling = case
    T = nperseg + (n_seg - 1) * (nperseg - noverlap) + tail
    assert welch_ref.segments(T, nperseg, noverlap) == n_seg
    x = np.random.default_rng(nfft + nperseg).standard_normal((3, T)) * 3.0 + 0.5
    w = _window(name, nperseg)
    ours = welch_ref.welch_f64(x, 400.0, w, noverlap, nfft, detrend, scaling)
    scipy_window = name if name in ("hann", "boxcar") else w
    f, theirs = scipy.signal.welch(x, fs=400.0, window=scipy_window, nperseg=nperseg, noverlap=noverlap, nfft=nfft,
                                   detrend="constant" if detrend else False, return_onesided=True, scaling=scaling, axis=1,
                                   average="mean")
    assert theirs.shape == ours.shape == (3, nfft // 2 + 1)
    assert (np.abs(ours - theirs).max(axis=1) <= 1e-13 * np.abs(theirs).max(axis=1)).all()
    assert np.allclose(f, np.arange(nfft // 2 + 1) * 400.0 / nfft, rtol=1e-15, atol=0)
    # and the long-double evaluation says the same, far inside that bound
    assert welch_ref.rel_err(theirs, welch_ref.welch_ld(x, 400.0, w, noverlap, nfft, detrend, scaling)) <= 1e-13


def test_restatement_is_mlab_psd_at_the_reference_settings():
    mlab = pytest.importorskip("matplotlib.mlab")
    x = np.random.default_rng(5).standard_normal((3, 256 + 7 * 128 + 50)) * 2.0 + 1.0
    ours = welch_ref.welch_f64(x, 1000.0, np.hanning(256), 128, 256, False, "density")
    for c in range(3):
        theirs, f = mlab.psd(x[c], NFFT=256, Fs=1000, noverlap=128)              # what plt.psd computes
        assert np.abs(ours[c] - theirs).max() <= 1e-13 * theirs.max()
        assert np.array_equal(f, np.arange(129) * 1000.0 / 256)


def test_moment_restatements_agree():
    x = np.random.default_rng(6).standard_normal((3, 5000)) + 1e4
    for s0, L, n_seg in ((0, 1, 3), (7, 63, 3), (130, 1017, 3), (0, 1000, 5)):
        m, s = welch_ref.moments_f64(x, s0, L, n_seg)
        ml, sl = welch_ref.moments_ld(x, s0, L, n_seg)
        assert m.shape == s.shape == (3, n_seg) and welch_ref.moments_err(m, s, ml, sl) <= 1e-15
        assert np.array_equal(m[:, 1], x[:, s0 + L:s0 + 2 * L].mean(axis=1))


@pytest.mark.parametrize("n_fft", diagnostics.WELCH_N_FFT)
def test_slab_planner_covers_every_segment_once(n_fft):
    F = diagnostics.frames_per_workgroup(n_fft)
    assert F == {256: 8, 512: 4, 1024: 2, 2048: 1}[n_fft]
    for n_seg in sorted({1, max(F - 1, 1), F, F + 1, 1000}):
        for channels in (1, 6, 256, 5000):
            for slabs in (None, 1, 2, n_seg, 10 ** 6):
                n_slabs, trips = diagnostics.plan_slabs(n_seg, n_fft, channels, n_cu=256, slabs=slabs)
                assert 1 <= n_slabs <= -(-n_seg // F)
                if slabs is not None:
                    assert n_slabs <= slabs
                covered = np.zeros(n_seg, dtype=int)
                for s in range(n_slabs):
                    lo, hi = s * trips * F, min((s + 1) * trips * F, n_seg)
                    assert lo < hi                                                  # no slab without a segment
                    covered[lo:hi] += 1
                assert (covered == 1).all()
    # about four workgroups a compute unit over all channels, where the segments allow it
    assert diagnostics.plan_slabs(1430, 256, 256)[0] == 4 and diagnostics.plan_slabs(1430, 256, 6)[0] == 90
    assert diagnostics.plan_slabs(1430, 256, 1)[0] == 179
    with pytest.raises(ValueError):
        diagnostics.plan_slabs(4, 256, 1, slabs=0)


def test_entries_exist_and_refuse_without_a_gpu():
    from decode_tonal_langauge_amd import _lib
    lib = _lib.load()
    err = lambda: lib.tl_last_error()
    # x, f64, stride, window, tw, work, work_elems, psd, C, T, n_fft, nperseg, noverlap, detrend, scale, n_seg, n_slabs, stream
    good = dict(x=16, f64=1, stride=1000, window=16, tw=16, work=16, work_elems=3 * 2 * 129, psd=16, C=3, T=1000, n_fft=256,
                nperseg=256, noverlap=128, detrend=1, scale=1.0, n_seg=6, n_slabs=2)

    def welch(**change):
        a = {**good, **change}
        return lib.tl_welch_psd(a["x"], a["f64"], a["stride"], a["window"], a["tw"], a["work"], a["work_elems"], a["psd"], a["C"],
                                a["T"], a["n_fft"], a["nperseg"], a["noverlap"], a["detrend"], a["scale"], a["n_seg"], a["n_slabs"],
                                None)

    for name in ("x", "window", "tw", "work", "psd"):
        assert welch(**{name: None}) == -1 and b"null" in err(), name
    for n_fft in (0, 1, 128, 255, 257, 300, 768, 4096):
        assert welch(n_fft=n_fft) == -1 and b"n_fft must be one of 256, 512, 1024, 2048" in err(), n_fft
    for nperseg in (-1, 0, 1, 257):
        assert welch(nperseg=nperseg) == -1 and b"nperseg must lie in [2, n_fft]" in err(), nperseg
    for noverlap in (256, 300, -1):
        assert welch(noverlap=noverlap) == -1 and b"step" in err(), noverlap
    for n_seg in (5, 7, 0):
        assert welch(n_seg=n_seg) == -1 and b"n_seg" in err() and b"disagrees" in err(), n_seg
    assert welch(T=255, n_seg=0) == -1 and b"T = 255" in err()
    assert welch(stride=999) == -1 and b"row_stride" in err()
    assert welch(detrend=2) == -1 and b"detrend" in err()
    assert welch(n_slabs=0) == -1 and b"n_slabs" in err()
    assert welch(work_elems=3 * 2 * 129 - 1) == -1 and b"workspace" in err()
    assert welch(C=0) == -1 and welch(C=65536) == -1

    # x, f64, stride, mean, std, C, T, s0, L, n_seg, stream
    assert lib.tl_segment_moments(None, 1, 100, 16, 16, 2, 100, 0, 10, 10, None) == -1 and b"null" in err()
    assert lib.tl_segment_moments(16, 1, 100, None, 16, 2, 100, 0, 10, 10, None) == -1 and b"null" in err()
    assert lib.tl_segment_moments(16, 1, 100, 16, None, 2, 100, 0, 10, 10, None) == -1 and b"null" in err()
    for s0, L, n_seg in ((1, 10, 10), (0, 10, 11), (0, 101, 1), (100, 1, 1), (101, 1, 1), (0, 2 ** 62, 4)):
        assert lib.tl_segment_moments(16, 1, 100, 16, 16, 2, 100, s0, L, n_seg, None) == -1 and b"runs past T" in err(), (s0, L)
    for s0, L, n_seg in ((-1, 10, 1), (0, 0, 1), (0, 10, 0)):
        assert lib.tl_segment_moments(16, 1, 100, 16, 16, 2, 100, s0, L, n_seg, None) == -1 and b"required" in err()
    assert lib.tl_segment_moments(16, 1, 99, 16, 16, 2, 100, 0, 10, 10, None) == -1 and b"row_stride" in err()


def test_python_refusals_name_what_is_supported():
    x = np.zeros((2, 1000))
    for kwargs, word in (({"average": "median"}, "median"), ({"detrend": "linear"}, "linear"), ({"nfft": 255}, "odd nfft"),
                         ({"nfft": 300}, "nfft = 300"), ({"return_onesided": False}, "two-sided"), ({"scaling": "psd"}, "psd"),
                         ({"window": "blackman"}, "blackman")):
        with pytest.raises(ValueError, match=word) as info:
            diagnostics.welch_psd(x, 400.0, **kwargs)
        assert "supported: average='mean'" in str(info.value)
    with pytest.raises(ValueError, match="complex") as info:
        diagnostics.welch_psd(x.astype(np.complex128), 400.0)
    assert "supported: average='mean'" in str(info.value)
    with pytest.raises(ValueError, match="greater than the recording's 1000 samples"):
        diagnostics.welch_psd(x, 400.0, nperseg=1001, nfft=1024)
    with pytest.raises(ValueError, match="must hold nperseg = 256 coefficients"):
        diagnostics.welch_psd(x, 400.0, window=np.hanning(255))
    with pytest.raises(ValueError, match="noverlap"):
        diagnostics.welch_psd(x, 400.0, noverlap=256)
    with pytest.raises(ValueError, match="at least nperseg"):
        diagnostics.welch_psd(x, 400.0, nperseg=300, nfft=256)
    for start, end in ((0.0, 30.0), (2.0, 12.0), (-1.0, 1.0)):
        with pytest.raises(ValueError, match="run past the recording's 1000 samples"):
            diagnostics.segment_mean_std(x, 100, start=start, end=end)
    with pytest.raises(ValueError, match="no whole second"):
        diagnostics.segment_mean_std(x, 100, start=3.0, end=3.5)
    assert diagnostics.segment_range(1000, 100, 2.0, 10.0) == (200, 100, 8)
    assert diagnostics.segment_range(3051, 1017.25, 0.0, 3.0) == (0, 1017, 3)


class _Io:
    @staticmethod
    def load_block(path):
        with np.load(os.path.join(path, "ecog.npz")) as a:
            return {"ecog": a["data"], "ecog_sf": a["sf"].item()}

    saved = []

    @classmethod
    def save_block(cls, setup_dir, subject_id, block_id, data_dict):
        cls.saved.append((subject_id, block_id))


class _Preprocessor:
    """Takes ``diagnostics_dir`` and notes it; no arithmetic."""
    calls = []

    @classmethod
    def preprocess_modalities(cls, data_dict, modalities_cfg, base_params, figure_dir=None, diagnostics_dir=None):
        cls.calls.append(diagnostics_dir)
        return data_dict


class _OldPreprocessor:
    @staticmethod
    def preprocess_modalities(data_dict, modalities_cfg, base_params, figure_dir=None):
        return data_dict


def test_stage_switch_is_off_by_default_and_refuses_shards(tmp_path):
    tree = synthetic.write_raw_tree(str(tmp_path / "raw"), {1: {1: 0.01, 2: 0.01}})
    io = lambda out: Namespace(root_dir=tree["root_dir"], output_dir=str(tmp_path / out))
    cfg = {"ecog": {"type": "signal"}}
    pipeline = dict(subject_dirs=tree["subject_dirs"], subject_ids=tree["subject_ids"], figures=False)
    _Preprocessor.calls.clear()
    for extra in ({}, {"diagnostics": False}):
        setup = subject_block.run(Namespace(**pipeline, **extra), io("off"), _Io, _Preprocessor, cfg)
        assert "diagnostics" not in os.listdir(setup)
    assert _Preprocessor.calls == [None] * 4
    setup = subject_block.run(Namespace(**pipeline, diagnostics=True), io("on"), _Io, _Preprocessor, cfg)
    assert _Preprocessor.calls[4:] == [os.path.join(setup, "diagnostics", "subject_1", f"block_{b}") for b in (1, 2)]
    with pytest.raises(ValueError, match="shard_channels"):
        subject_block.run(Namespace(**pipeline, diagnostics=True, shard_channels=True), io("sh"), _Io, _Preprocessor, cfg)
    with pytest.raises(ValueError, match="diagnostics_dir"):
        subject_block.run(Namespace(**pipeline, diagnostics=True), io("old"), _Io, _OldPreprocessor, cfg)
    # the preprocessor itself: refused before anything is touched; without the argument nothing is written
    steps = [{"module": "preprocess.signal.car_rereference"}]
    with pytest.raises(ValueError, match="shard_channels"):
        preprocessor.preprocess_signal(np.zeros((2, 10)), steps, Namespace(signal_freq=100.0), shard_channels=True,
                                       diagnostics_dir=str(tmp_path / "d"))
    with pytest.raises(ValueError, match="shard_channels"):
        preprocessor.preprocess_modalities({}, {}, Namespace(), shard_channels=True, diagnostics_dir=str(tmp_path / "d"))
    data = {"audio": np.zeros((1, 10)), "audio_sf": 100.0}
    assert preprocessor.preprocess_modalities(data, {"audio": {"type": "signal"}}, Namespace(),
                                              diagnostics_dir=str(tmp_path / "d")) is data      # no steps: nothing to summarise
    assert not os.path.exists(tmp_path / "d")


def test_compare_confusion_matrices_is_host_only(tmp_path):
    pytest.importorskip("matplotlib")
    from decode_tonal_langauge_amd.utils import visualise
    a, b = np.array([[5, 1], [2, 4]]), np.array([[4, 2], [2, 4]])
    visualise.compare_confusion_matrices(a, b, label_names=["t1", "t2"], figure_path=str(tmp_path / "diff.png"))
    with open(tmp_path / "diff.png", "rb") as f:
        assert f.read(8) == b"\x89PNG\r\n\x1a\n"
    for name in ("plot_psd", "plot_channel_mean_std"):
        with pytest.raises(RuntimeError, match="no CPU fallback"):                    # the numbers come from the GPU or not at all
            getattr(visualise, name)(*((torch_cpu(),) if name == "plot_psd" else (torch_cpu(), 100, 0.0, 3.0)),
                                     figure_path=str(tmp_path / "x.png"))


def torch_cpu():
    import torch
    return torch.zeros(2, 600)
