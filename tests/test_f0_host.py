"""No GPU: the host side of F0 tracking - what ``tl_yin_f0`` refuses before any GPU call, ``utils.audio.yin_f0`` against the
plain-loop restatement of tests/yin_ref.py, ``compute_f0_metrics`` on hand-made tracks, ``estimate_tone_dynamics`` on the
host path, and the ``--f0_metrics`` switch of ``train_synthesizer``."""
import json
import math
from argparse import Namespace

import numpy as np
import pytest

from decode_tonal_langauge_amd import train_synthesizer as ts
from decode_tonal_langauge_amd.data_loading import utils as dl_utils
from decode_tonal_langauge_amd.utils import audio
from decode_tonal_langauge_amd.utils.metrics import compute_f0_metrics, f0_voicing
from tests import yin_ref as yr


def test_entry_refuses_without_a_gpu():
    from decode_tonal_langauge_amd import _lib
    lib = _lib.load()
    assert len(_lib.SIGNATURES["tl_yin_f0"][1]) == 20
    err = lambda: lib.tl_last_error()
    good = dict(audio=16, f64=0, stride=700, f0=16, aper=16, pidx=16, rms=16, cmnd=None, N=5, S=700, fl=256, W=128, hop=64,
                center=1, pmin=8, pmax=80, thr=0.1, sr=8000.0, n_frames=11)

    def yin(**change):
        a = {**good, **change}
        return lib.tl_yin_f0(a["audio"], a["f64"], a["stride"], a["f0"], a["aper"], a["pidx"], a["rms"], a["cmnd"], a["N"], a["S"],
                             a["fl"], a["W"], a["hop"], a["center"], a["pmin"], a["pmax"], a["thr"], a["sr"], a["n_frames"], None)

    for name in ("audio", "f0", "aper", "pidx", "rms"):
        assert yin(**{name: None}) == -1 and b"null" in err(), name
    assert yin(N=0) == -1 and b"N and S" in err()
    assert yin(S=0, n_frames=1) == -1 and b"N and S" in err()
    for W, fl in ((0, 256), (256, 256), (300, 256), (128, 4097), (4096, 8192)):
        assert yin(W=W, fl=fl) == -1 and b"win_length < frame_length <= 4096" in err(), (W, fl)
    assert yin(hop=0) == -1 and b"hop" in err()
    for pmin, pmax in ((0, 80), (8, 8), (80, 8), (8, 128), (8, 4000)):
        assert yin(pmin=pmin, pmax=pmax) == -1 and b"max_period <= frame_length - win_length - 1 = 127" in err(), (pmin, pmax)
    for thr in (0.0, -1.0, float("nan")):
        assert yin(thr=thr) == -1 and b"threshold" in err(), thr
    for sr in (0.0, -8000.0, float("nan")):
        assert yin(sr=sr) == -1 and b"sr must be positive" in err(), sr
    for n_frames in (10, 12, 0):
        assert yin(n_frames=n_frames) == -1 and b"n_frames" in err() and b"give 11" in err(), n_frames
    assert yin(center=0, n_frames=11) == -1 and b"give 7" in err()
    assert yin(center=0, S=255, stride=255, n_frames=1) == -1 and b"shorter than frame_length" in err()
    assert yin(stride=699) == -1 and b"row_stride" in err()


def test_geometry_defaults_and_refusals():
    assert audio.yin_geometry(24414, 60.0, 500.0) == (2048, 1024, 512, 48, 407)
    assert audio.yin_geometry(8000, 100, 1000, 256, 96, 50) == (256, 96, 50, 8, 80)
    assert audio.yin_geometry(8000, 1.0, 20000.0, 256) == (256, 128, 64, 1, 127)          # both ends clamped
    assert audio.yin_n_frames(700, 256, 64, True) == 11 and audio.yin_n_frames(700, 256, 64, False) == 7
    for bad in (dict(fmin=0.0), dict(fmin=600.0), dict(win_length=256), dict(win_length=0), dict(hop_length=0), dict(sr=0)):
        kw = {**dict(sr=8000, fmin=100.0, fmax=500.0, frame_length=256), **bad}
        with pytest.raises(ValueError):
            audio.yin_geometry(**kw)
    with pytest.raises(ValueError, match="two lags"):
        audio.yin_geometry(8000, 8000.0, 9000.0, 256)
    with pytest.raises(ValueError, match="shorter than frame_length"):
        audio.yin_f0(np.zeros(100), 8000, 100, 1000, 256, center=False)
    with pytest.raises(ValueError, match="1D"):
        audio.yin_f0(np.zeros((2, 700)), 8000, 100, 1000, 256)
    with pytest.raises(ValueError, match="2D"):
        audio.yin_f0_batch(np.zeros(700), 8000, 100, 1000, 256)
    with pytest.raises(ValueError, match="at most 4096"):
        audio.yin_f0_batch(np.zeros((1, 700)), 8000, 100, 1000, 8192)


@pytest.mark.parametrize("name", ["A", "D"])
def test_host_path_is_the_restatement(name):
    sr, fl, W, hop, fmin, fmax, S = yr.GEOMETRIES[name]
    ref = yr.reference(name, "float64", "float64")
    for k, row in enumerate(yr.clips(sr, S)):
        got = audio.yin_f0(row, sr, fmin, fmax, fl, W, hop, yr.THRESHOLD, return_cmnd=True)
        assert isinstance(got, audio.F0TrackCmnd)
        for field in got._fields:
            assert np.array_equal(getattr(got, field), getattr(ref, field)[k]), (k, field)
    plain = audio.yin_f0(row, sr, fmin, fmax, fl, W, hop, yr.THRESHOLD)
    assert isinstance(plain, audio.F0Track) and np.array_equal(plain.f0, got.f0)
    # the float64 restatement against long double: far inside the bounds the GPU tests set
    ld = yr.reference(name, "float64", "longdouble")
    nz = ld.cmnd != 0
    assert ((ref.cmnd == 0) == ~nz).all()
    assert (np.abs(ref.cmnd - ld.cmnd)[nz] / ld.cmnd[nz]).max() <= yr.eps_c(W, yr.periods(sr, fl, W, fmin, fmax)[1])
    assert np.array_equal(ref.period_index, ld.period_index) and ld.decidable.all()


def test_margin_covers_twice_the_curve_bound():
    for sr, fl, W, hop, fmin, fmax, S in yr.GEOMETRIES.values():
        assert yr.MARGIN >= 2 * yr.eps_c(W, yr.periods(sr, fl, W, fmin, fmax)[1])


def _track(f0, aper=None, rms=None):
    f0 = np.asarray(f0, dtype=np.float64)
    return audio.F0Track(f0, np.full(f0.shape, 0.01) if aper is None else np.asarray(aper, dtype=np.float64),
                         np.zeros(f0.shape, np.int32), np.ones(f0.shape) if rms is None else np.asarray(rms, dtype=np.float64))


def test_f0_metrics_on_hand_made_tracks():
    f = 200.0 * 2.0 ** (np.arange(10) / 24.0)
    same = compute_f0_metrics(_track(f), _track(f))
    assert same == {"f0_rmse_cents": 0.0, "f0_corr": 1.0, "gross_pitch_error": 0.0, "voicing_error": 0.0, "n_voiced": 10}
    # an octave too high on every second frame
    est = f.copy()
    est[::2] *= 2.0
    m = compute_f0_metrics(_track(f), _track(est))
    assert m["gross_pitch_error"] == 0.5 and m["voicing_error"] == 0.0 and m["n_voiced"] == 10
    assert abs(m["f0_rmse_cents"] - 1200.0 * math.sqrt(0.5)) < 1e-9
    only = compute_f0_metrics(_track(f[::2]), _track(est[::2]))
    assert abs(only["f0_rmse_cents"] - 1200.0) < 1e-9 and only["gross_pitch_error"] == 1.0 and abs(only["f0_corr"] - 1.0) < 1e-12
    # 19 % off is no gross error, 21 % is
    assert compute_f0_metrics(_track(f), _track(1.19 * f))["gross_pitch_error"] == 0.0
    assert compute_f0_metrics(_track(f), _track(1.21 * f))["gross_pitch_error"] == 1.0
    # voicing: an aperiodic frame, and one 46 dB below the clip's loudest, in one track only
    aper = np.full(10, 0.01)
    aper[3] = 0.5
    rms = np.ones(10)
    rms[7] = 0.005
    m = compute_f0_metrics(_track(f), _track(f, aper=aper, rms=rms))
    assert m["voicing_error"] == 0.2 and m["n_voiced"] == 8 and m["f0_rmse_cents"] == 0.0
    assert compute_f0_metrics(_track(f, rms=rms), _track(f, rms=rms), silence_db=60.0)["n_voiced"] == 10
    assert not f0_voicing(_track(f, rms=np.zeros(10))).any()                    # a silent clip has no voiced frame
    # the loudest frame is each clip's own
    two = _track(np.stack([f, f]), rms=np.stack([np.ones(10), np.full(10, 1e-4)]))
    assert f0_voicing(two).all()
    # fewer than two frames voiced in both: NaN, no exception
    aper = np.full(10, 0.5)
    aper[4] = 0.01
    m = compute_f0_metrics(_track(f), _track(f, aper=aper))
    assert m["n_voiced"] == 1 and m["voicing_error"] == 0.9
    assert all(math.isnan(m[k]) for k in ("f0_rmse_cents", "f0_corr", "gross_pitch_error"))
    m = compute_f0_metrics(_track(f, aper=np.ones(10)), _track(f, aper=np.ones(10)))
    assert m["n_voiced"] == 0 and m["voicing_error"] == 0.0 and math.isnan(m["f0_corr"])
    assert math.isnan(compute_f0_metrics(_track(np.full(10, 200.0)), _track(f))["f0_corr"])      # a constant contour
    with pytest.raises(ValueError, match="shape"):
        compute_f0_metrics(_track(f), _track(f[:5]))


def _host_batch(audio_in, sr, fmin, fmax, device=None, **kw):
    tracks = [audio.yin_f0(row, sr, fmin, fmax, **kw) for row in np.asarray(audio_in)]
    return audio.F0Track(*(np.stack(col) for col in zip(*tracks)))


def test_estimate_tone_dynamics_on_the_host_path(monkeypatch):
    from decode_tonal_langauge_amd.models.synthesis_trainer import tone_dynamics_table
    monkeypatch.setattr(dl_utils, "yin_f0_batch", _host_batch)
    sr, fl, W, hop, fmin, fmax, S = yr.GEOMETRIES["B"]
    x = yr.clips(sr, S)
    kw = dict(fmin=fmin, fmax=fmax, frame_length=fl, win_length=W, hop_length=hop)
    got = dl_utils.estimate_tone_dynamics(x[:4], [0, 1, 2, 3], sr, 5, **kw)
    assert list(got) == ["0", "1", "2", "3"] and all(len(v) == 5 and all(isinstance(t, float) for t in v) for v in got.values())
    level, rising, falling, dipping = (np.array(got[k]) for k in "0123")
    print(got)
    assert all(((v >= 1.0) & (v <= 5.0)).all() for v in (level, rising, falling, dipping))
    assert level.max() - level.min() < 1.0
    assert (np.diff(rising) > 0).all() and (np.diff(falling) < 0).all()
    assert 0 < int(np.argmin(dipping)) < 4
    table, L, n_rows = tone_dynamics_table(got)                              # what SynthesisTrainer builds its label table from
    assert (L, n_rows) == (5, 4) and np.allclose(table.numpy(), np.array([got[k] for k in "0123"]), rtol=1e-6)
    # two clips of a tone: the median; labels as an array of another order
    both = dl_utils.estimate_tone_dynamics(x[[1, 2, 1]], np.array([7, 3, 7]), sr, 5, **kw)
    assert list(both) == ["3", "7"] and (np.diff(both["7"]) > 0).all()
    # the noise clip has no voiced frame: its tone cannot be estimated
    with pytest.raises(ValueError, match=r"tone\(s\) \[4\]"):
        dl_utils.estimate_tone_dynamics(x, [0, 1, 2, 3, 4], sr, 5, **kw)
    with pytest.raises(ValueError, match="one tone label per clip"):
        dl_utils.estimate_tone_dynamics(x, [0, 1], sr, 5, **kw)


def test_estimate_tone_dynamics_script(monkeypatch, tmp_path, capsys):
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "estimate_tone_dynamics.py")
    spec = importlib.util.spec_from_file_location("estimate_tone_dynamics_script", path)
    script = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(script)
    monkeypatch.setattr(dl_utils, "yin_f0_batch", _host_batch)
    sr, fl, W, hop, fmin, fmax, S = yr.GEOMETRIES["B"]
    np.savez(tmp_path / "samples.npz", audio=yr.clips(sr, S)[:4], tone=np.arange(4), audio_sf=sr)
    table = {"0": [3, 3, 3], "1": [1, 3, 5], "2": [5, 3, 1], "3": [3, 1, 3]}
    (tmp_path / "config.json").write_text(json.dumps({"tone_dynamic_mapping": table}))
    out = script.main(["--sample_path", str(tmp_path / "samples.npz"), "--config_file", str(tmp_path / "config.json"),
                       "--frame_length", str(fl), "--output", str(tmp_path / "dyn.json")])
    assert json.loads((tmp_path / "dyn.json").read_text()) == out and all(len(v) == 3 for v in out.values())
    said = capsys.readouterr().out
    assert all(f"tone {t}: config {table[str(t)]}" in said for t in range(4))
    assert script.table_distance({"1": [1.0, 2.0]}, {"1": [2, 4], "9": [0, 0]}) == {"1": (1.5, 2.0)}


def test_train_synthesizer_switch(monkeypatch):
    required = ['--sample_path', 's', '--subject_id', '1', '--result_file', 'r', '--model_name', 'm',
                '--synthesis_model_name', 'SynthesisLite', '--syllable_model_name', 'logistic', '--tone_model_name', 'logistic']
    parser = ts.build_parser()
    assert parser.parse_args(required).f0_metrics is False
    assert parser.parse_args(required + ['--f0_metrics']).f0_metrics is True
    seen = []
    monkeypatch.setattr(ts, "train", lambda params: seen.append(params) or {})
    base = dict(sample_path='s', subject_id='1', result_file='out/r.csv', model_name='m', synthesis_model_name='SynthesisLite',
                syllable_model_name='logistic', tone_model_name='logistic')
    ts.run({"training": {"params": {**base, "audio_dir": "a", "f0_metrics": True}}})
    ts.run({"training": {"params": base}})
    assert seen[0].f0_metrics is True and seen[0].audio_dir == "a" and seen[1].f0_metrics is False
    # refused by name, before anything is read
    assert ts.check_f0_metrics(Namespace(f0_metrics=True, audio_dir="a")) and not ts.check_f0_metrics(Namespace(audio_dir=None))
    with pytest.raises(ValueError, match="--f0_metrics needs --audio_dir"):
        ts.check_f0_metrics(Namespace(f0_metrics=True, audio_dir=None))
    monkeypatch.undo()
    with pytest.raises(ValueError, match="--f0_metrics needs --audio_dir"):
        ts.train(Namespace(sample_path=__file__, f0_metrics=True, audio_dir=None))


def test_f0_metrics_writer_on_the_host(tmp_path, capsys):
    """The 'cpu' leg of ``--f0_metrics``: ``yin_f0`` clip by clip, the same files."""
    sr, fl, W, hop, fmin, fmax, S = yr.GEOMETRIES["B"]
    x = yr.clips(sr, S).astype(np.float32)
    waves = np.concatenate([x[:3], x[[0, 2, 1]]])                              # "reconstructions": one right, two swapped
    params = Namespace(audio_sampling_rate=sr, device="cpu", audio_dir=str(tmp_path))
    m = ts.write_f0_metrics(waves, 3, params, {"n_mels": 16, "n_fft": fl, "hop_length": hop})
    assert json.loads((tmp_path / "f0_metrics.json").read_text()) == m and m["n_voiced"] > 20
    assert m["gross_pitch_error"] > 0.3 and m["f0_rmse_cents"] > 100.0
    tracks = np.load(tmp_path / "f0_tracks.npz")
    want = audio.yin_f0(waves[4], sr, 60.0, 500.0, frame_length=fl, hop_length=hop)
    assert all(tracks[k].shape == (6, 1 + S // hop) and np.array_equal(tracks[k][4], getattr(want, k)) for k in want._fields)
    assert "gross pitch error" in capsys.readouterr().out
    assert ts.write_f0_metrics(np.zeros((2, 0), np.float32), 1, params, {}) is None
