"""GPU: the preprocess stage end to end - what it writes against ``preprocess_signal`` applied by hand (bit for bit), residency
(every step sees a CUDA tensor, a modality without steps is never uploaded), the figures switch, the resident hand-over to
sample collection against the file route, and the YAML pipeline preprocess -> sample_collection -> channel_selection.

Shapes: 2 subjects; subject 1 has two blocks of 3 s and 4 s at 1017.25 Hz (3051 and 4069 samples -> 1199 and 1600 at 400 Hz:
two lengths for the resample coefficient cache, and the Hilbert bank on either side of its 1024-sample overlap-save
threshold), 6 channels; audio 1 x 8000 float32 without steps; one stray directory per subject."""
import json
import os
import sys
import warnings
from argparse import Namespace
from copy import deepcopy

import numpy as np
import pytest
import torch
import yaml

from decode_tonal_langauge_amd import extract_samples, preprocess_main
from decode_tonal_langauge_amd.data_loading import synthetic
from decode_tonal_langauge_amd.preprocess import handover, preprocessor
from decode_tonal_langauge_amd.preprocess.pipelines import subject_block
from decode_tonal_langauge_amd.preprocess.signal import downsample

pytestmark = pytest.mark.gpu

ECOG_SF, AUDIO_SF, AUDIO_SAMPLES, CHANNELS = 1017.25, 2000.5, 8000, 6
BLOCKS = {1: {1: 3.0, 2: 4.0}, 2: {1: 3.0}}
LENGTHS = {3.0: (3051, 1199), 4.0: (4069, 1600)}                    # seconds -> samples raw, samples at 400 Hz

# the chain of example_config.yaml (floats in freq_ranges: a list of two ints reads as two ranges, in the reference too),
# the z-score against an interval inside the shortest block
CHAIN = [
    {"module": "preprocess.downsample", "params": {"downsample_freq": 400}},
    {"module": "preprocess.frequency_filter", "params": {"bands": [
        {"method": "hilbert", "params": {"freq_ranges": [70., 150.], "envelope": True}},
        {"method": "butter", "params": {"freqs": [0.3, 100], "filter_type": "bandpass"}}]}},
    {"module": "preprocess.zscore_rereference", "params": {"rereference_interval": [0., 2.]}},
]
SPY = {"module": "stage_spy.between_steps"}
SPY_SOURCE = '''
CHANNEL_LOCAL = True
CALLS = []


def run(data, params):
    CALLS.append((type(data).__name__, bool(getattr(data, "is_cuda", False)), tuple(data.shape), str(data.dtype),
                  params.subject_id, params.block_id, params.signal_freq))
    return data
'''


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch.device("cuda:0")


def _events(seconds):
    return [(0.8 + 0.4 * k, 1.1 + 0.4 * k, 1 + k % 4, "ai"[k % 2]) for k in range(5 if seconds < 4 else 7)]


def _stage_config(tree, out, steps, **pipeline):
    return {"preprocess": {"module": "preprocess_main", "params": {
        "pipeline": {"module": "preprocess.pipelines.subject_block",
                     "params": {"subject_dirs": tree["subject_dirs"], "subject_ids": tree["subject_ids"], **pipeline}},
        "io": {"module": "preprocess.io.npz_blocks", "params": {"root_dir": tree["root_dir"], "output_dir": out}},
        "preprocessor": {"module": "preprocess.preprocessor"},
        "modalities": {"ecog": {"type": "signal", "preprocessing": {"steps": steps}}, "audio": {"type": "signal"}}}}}


def _collection_config(recording_dir, tg_root, out, **settings):
    subject = lambda s: {"textgrid_dir": f"s{s}", "sample_length": 0.25, "rest_period": [0.0, 0.6]}
    io = {"textgrid_root": tg_root, "output_dir": out}
    if recording_dir is not None:
        io["recording_dir"] = recording_dir
    return {"module": "extract_samples", "params": {"io": io, "settings": {"syllable_identifiers": ["a", "i"], "figures": False,
                                                                           **settings},
                                                     "subjects": {1: subject(1), 2: subject(2)}}}


@pytest.fixture(scope="module")
def stage(tmp_path_factory, dev):
    """The raw tree, its TextGrids, and ONE run of the stage over it (spy step between downsample and the band step,
    ``keep_resident``, no figures) with every ``torch.from_numpy`` of the run noted."""
    tmp = tmp_path_factory.mktemp("preprocess_stage")
    (tmp / "plugins" / "stage_spy").mkdir(parents=True)
    (tmp / "plugins" / "stage_spy" / "__init__.py").write_text("")
    (tmp / "plugins" / "stage_spy" / "between_steps.py").write_text(SPY_SOURCE)
    sys.path.insert(0, str(tmp / "plugins"))
    tree = synthetic.write_raw_tree(str(tmp / "raw"), BLOCKS, n_channels=CHANNELS, ecog_sf=ECOG_SF, audio_sf=AUDIO_SF,
                                    audio_samples=AUDIO_SAMPLES, seed=11, stray=("HS0-notes",))
    for subject, lengths in BLOCKS.items():
        for block, seconds in lengths.items():
            synthetic.write_block_annotations(str(tmp / "tg" / f"s{subject}"), block, _events(seconds), seconds=seconds)
    steps = [CHAIN[0], SPY, CHAIN[1], CHAIN[2]]
    cfg = _stage_config(tree, str(tmp / "processed"), steps, keep_resident=True, figures=False)
    handover.release()
    downsample._COEF_CACHE.clear()
    uploads, from_numpy = [], torch.from_numpy

    def noted(array):
        uploads.append(tuple(array.shape))
        return from_numpy(array)

    with pytest.MonkeyPatch.context() as patch:
        patch.setattr(torch, "from_numpy", noted)
        setup_dir = preprocess_main.run(deepcopy(cfg))
    import stage_spy.between_steps as spy
    try:
        yield {"tmp": tmp, "tree": tree, "cfg": cfg, "setup_dir": setup_dir, "uploads": uploads, "spy_calls": list(spy.CALLS),
               "resample_lengths": {key[0] for key in downsample._COEF_CACHE},
               "registry": {s: handover.lookup(os.path.join(setup_dir, f"subject_{s}")) for s in BLOCKS}}
    finally:
        handover.release()
        sys.path.remove(str(tmp / "plugins"))


def _raw(tree, subject, block, modality):
    with np.load(os.path.join(tree["blocks"][(subject, block)], f"{modality}.npz")) as archive:
        return archive["data"], archive["sf"]


def test_written_blocks_equal_the_by_hand_run_bit_for_bit(stage, dev):
    setup_dir, tree = stage["setup_dir"], stage["tree"]
    assert os.path.basename(setup_dir) == subject_block.generate_setup_name(stage["cfg"]["preprocess"]["params"]["modalities"])
    assert os.path.basename(setup_dir).startswith("downsample__between_steps__frequency_filter__zscore_rereference_")
    assert sorted(os.listdir(setup_dir)) == ["config.yaml", "figures", "subject_1", "subject_2"]
    assert sorted(os.listdir(os.path.join(setup_dir, "subject_1"))) == ["B1_audio.npz", "B1_ecog.npz", "B2_audio.npz", "B2_ecog.npz"]
    assert sorted(os.listdir(os.path.join(setup_dir, "subject_2"))) == ["B1_audio.npz", "B1_ecog.npz"]      # the stray one skipped
    for subject, lengths in BLOCKS.items():
        for block, seconds in lengths.items():
            raw, sf = _raw(tree, subject, block, "ecog")
            assert raw.shape == (CHANNELS, LENGTHS[seconds][0]) and raw.dtype == np.float32 and float(sf) == ECOG_SF
            want, freq = preprocessor.preprocess_signal(raw, deepcopy(CHAIN), Namespace(signal_freq=sf.item(), block_id=block,
                                                                                         subject_id=subject))
            assert isinstance(want, np.ndarray) and want.shape == (2 * CHANNELS, LENGTHS[seconds][1]) and freq == 400
            with np.load(os.path.join(setup_dir, f"subject_{subject}", f"B{block}_ecog.npz")) as got:
                assert sorted(got.files) == ["data", "sf"]
                assert got["data"].dtype == want.dtype == np.float64 and got["data"].shape == want.shape
                assert np.isfinite(got["data"]).all()
                assert got["data"].tobytes() == want.tobytes(), (subject, block)
                assert got["sf"] == 400 and got["sf"].shape == () and got["sf"].dtype == np.asarray(freq).dtype
            audio, audio_sf = _raw(tree, subject, block, "audio")
            with np.load(os.path.join(setup_dir, f"subject_{subject}", f"B{block}_audio.npz")) as got:
                assert got["data"].dtype == np.float32 and got["data"].shape == (1, AUDIO_SAMPLES)
                assert got["data"].tobytes() == audio.tobytes()
                assert got["sf"].dtype == audio_sf.dtype and got["sf"].tobytes() == audio_sf.tobytes() and float(got["sf"]) == AUDIO_SF
    with open(os.path.join(setup_dir, "config.yaml")) as f:
        params = stage["cfg"]["preprocess"]["params"]
        assert yaml.safe_load(f) == {"preprocess": {"pipeline": params["pipeline"]["params"], "io": params["io"]["params"],
                                                    "modalities": params["modalities"]}}
    # each block length went through its own resample coefficients
    assert {3051, 1199, 4069, 1600} <= stage["resample_lengths"]


def test_every_step_sees_a_cuda_tensor_and_audio_is_never_uploaded(stage):
    want = [(subject, block, LENGTHS[seconds][1]) for subject, lengths in BLOCKS.items() for block, seconds in lengths.items()]
    assert stage["spy_calls"] == [("Tensor", True, (CHANNELS, n), "torch.float32", subject, block, 400)
                                  for subject, block, n in want]
    # one upload per block: the ECoG, whole; nothing of the audio's shape went to torch at all
    blocks = [(CHANNELS, LENGTHS[seconds][0]) for lengths in BLOCKS.values() for seconds in lengths.values()]
    assert [shape for shape in stage["uploads"] if shape in set(blocks)] == blocks
    between = {(rows, n) for rows in (CHANNELS, 2 * CHANNELS) for _raw_n, n in LENGTHS.values()}
    assert not [shape for shape in stage["uploads"] if shape in between]              # no step's result went up again
    assert not [shape for shape in stage["uploads"] if AUDIO_SAMPLES in shape]
    # what the stage kept: the ECoG where the steps left it, the audio where it was loaded
    for subject, lengths in BLOCKS.items():
        kept = stage["registry"][subject]
        assert sorted(kept) == sorted(lengths)
        for block, seconds in lengths.items():
            assert list(kept[block]) == ["sound", "ecog"]
            ecog, sf = kept[block]["ecog"]
            assert isinstance(ecog, torch.Tensor) and ecog.is_cuda and ecog.shape == (2 * CHANNELS, LENGTHS[seconds][1]) and sf == 400
            audio, audio_sf = kept[block]["sound"]
            assert isinstance(audio, np.ndarray) and audio.dtype == np.float32 and audio_sf == AUDIO_SF


def test_figures_switch(stage, tmp_path):
    setup_dir = stage["setup_dir"]
    assert [f for _b, _d, files in os.walk(os.path.join(setup_dir, "figures")) for f in files] == []       # figures: false
    assert os.path.isdir(os.path.join(setup_dir, "figures", "subject_1", "block_2"))
    tree = dict(stage["tree"], subject_dirs=stage["tree"]["subject_dirs"][1:], subject_ids=[2])
    drawn = preprocess_main.run(_stage_config(tree, str(tmp_path / "out"), deepcopy(CHAIN)))               # default: true
    assert handover.lookup(os.path.join(drawn, "subject_2")) is None                                        # default: not kept
    figures = sorted(os.path.relpath(os.path.join(b, f), drawn) for b, _d, files in os.walk(os.path.join(drawn, "figures"))
                     for f in files)
    assert figures == [os.path.join("figures", "subject_2", "block_1", "ecog", name) for name in
                       ("step_0_downsample.png", "step_1_frequency_filter.png", "step_2_zscore_rereference.png")]
    assert all(os.path.getsize(os.path.join(drawn, f)) > 1000 for f in figures)
    with np.load(os.path.join(drawn, "subject_2", "B1_ecog.npz")) as a, \
            np.load(os.path.join(stage["setup_dir"], "subject_2", "B1_ecog.npz")) as b:
        assert a["data"].tobytes() == b["data"].tobytes()                                                   # drawing changes nothing


def _collect(stage, out, capsys, monkeypatch):
    """One ``extract_samples.run`` over the stage's directory: (arrays of every subject file, printed lines, files np.load
    opened)."""
    opened, load = [], np.load

    def noted(file, *args, **kwargs):
        opened.append(os.path.basename(str(file)))
        return load(file, *args, **kwargs)

    cfg = {"sample_collection": _collection_config(stage["setup_dir"], str(stage["tmp"] / "tg"), out, overwrite=True)}
    capsys.readouterr()
    with monkeypatch.context() as patch, warnings.catch_warnings():
        warnings.simplefilter("ignore")
        patch.setattr(np, "load", noted)
        result = extract_samples.run(cfg)
    printed = capsys.readouterr().out
    arrays = {}
    for subject in BLOCKS:
        with np.load(os.path.join(result, f"subject_{subject}.npz")) as d:
            arrays[subject] = {k: d[k] for k in d.files}
    return arrays, printed, opened, result


def test_hand_over_equals_the_file_route(stage, tmp_path, capsys, monkeypatch):
    assert all(stage["registry"].values()) and len(handover.registered()) == 2
    out = str(tmp_path / "samples")
    resident, resident_lines, resident_opened, where = _collect(stage, out, capsys, monkeypatch)
    assert not [f for f in resident_opened if f.startswith("B")], resident_opened     # no B*_ecog.npz / B*_audio.npz was read
    subject_block.release(stage["setup_dir"])
    assert handover.registered() == []
    files, file_lines, file_opened, again = _collect(stage, out, capsys, monkeypatch)
    assert again == where
    assert sorted(f for f in file_opened if f.startswith("B")) == ["B1_audio.npz", "B1_audio.npz", "B1_ecog.npz", "B1_ecog.npz",
                                                                    "B2_audio.npz", "B2_ecog.npz"]
    assert resident_lines == file_lines and "ECoG recording length for block 2: 4.0  s" in file_lines
    for subject in BLOCKS:
        a, b = resident[subject], files[subject]
        assert sorted(a) == sorted(b) == ["audio", "audio_sf", "ecog", "ecog_rest", "ecog_sf", "syllable", "tone"]
        for key in a:
            assert a[key].dtype == b[key].dtype and a[key].shape == b[key].shape and a[key].tobytes() == b[key].tobytes(), key
    n = sum(len(_events(s)) for s in BLOCKS[1].values())
    assert resident[1]["ecog"].shape == (n, 2 * CHANNELS, 100) and resident[1]["audio"].shape == (n, 500)
    assert resident[1]["ecog_rest"].shape == (4, 2 * CHANNELS, 100) and np.isfinite(resident[1]["ecog"]).all()
    # the windows are those of the written block
    with np.load(os.path.join(stage["setup_dir"], "subject_1", "B2_ecog.npz")) as block:
        first = len(_events(3.0))
        assert np.array_equal(resident[1]["ecog"][first], block["data"][:, 320:420])


def test_yaml_pipeline_preprocess_to_channel_selection(stage, tmp_path):
    """The stages of the reference's example configuration, named as the reference names them, from raw blocks to channel
    lists.  Without ``preprocess_main`` in the package this stops at the first stage with an ImportError."""
    from decode_tonal_langauge_amd import main
    cfg = _stage_config(stage["tree"], str(tmp_path / "processed"), deepcopy(CHAIN), keep_resident=True, figures=False)
    cfg["sample_collection"] = _collection_config(None, str(stage["tmp"] / "tg"), str(tmp_path / "samples"))
    cfg["channel_selection"] = {"module": "channel_selection_main", "params": {
        "io": {"output_dir": str(tmp_path / "channels")},
        "selections": [{"module": "channel_selection.active", "selection_name": "active_channels",
                        "params": {"p_threshold": 0.05, "active_time_threshold": 0.05}}]}}
    path = tmp_path / "pipeline.yaml"
    path.write_text(yaml.dump(cfg))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        main.run_pipeline(str(path))
    # the name is a digest over the steps as the YAML file gives them (yaml.dump wrote the keys sorted)
    setup = subject_block.generate_setup_name(yaml.safe_load(path.read_text())["preprocess"]["params"]["modalities"])
    assert os.listdir(tmp_path / "processed") == [setup]
    # recording_dir came from the preprocess stage's return value: sample collection names its directory after it
    (samples,) = os.listdir(tmp_path / "samples")
    assert samples.startswith(setup + "__")
    assert sorted(f for f in os.listdir(tmp_path / "samples" / samples) if f.endswith(".npz")) == ["subject_1.npz", "subject_2.npz"]
    (channels,) = os.listdir(tmp_path / "channels")
    assert channels.startswith(samples + "__")
    with open(tmp_path / "channels" / channels / "subject_1.json") as f:
        assert list(json.load(f)) == ["active_channels"]
    # the configuration is carried forward
    with open(tmp_path / "processed" / setup / "config.yaml") as f:
        first = yaml.safe_load(f)
    with open(tmp_path / "samples" / samples / "config.yaml") as f:
        second = yaml.safe_load(f)
    with open(tmp_path / "channels" / channels / "config.yaml") as f:
        third = yaml.safe_load(f)
    assert set(first) == {"preprocess"} and set(second) == {"preprocess", "sample_collection"}
    assert set(third) == {"preprocess", "sample_collection", "channel_selection"}
    assert third["preprocess"] == second["preprocess"] == first["preprocess"]
    assert first["preprocess"]["modalities"] == cfg["preprocess"]["params"]["modalities"]
    assert second["sample_collection"]["params"]["io"]["recording_dir"] == str(tmp_path / "processed" / setup)
    assert third["sample_collection"] == second["sample_collection"]
    # the blocks kept for sample collection were released when that stage was done
    assert handover.lookup(str(tmp_path / "processed" / setup / "subject_1")) is None
    # the same samples as from the files of the stage fixture's run (same raw tree, same chain; the spy step is the identity)
    with np.load(tmp_path / "samples" / samples / "subject_1.npz") as got:
        with np.load(os.path.join(stage["setup_dir"], "subject_1", "B1_ecog.npz")) as block:
            assert np.array_equal(got["ecog"][0], block["data"][:, 320:420]) and float(got["ecog_sf"]) == 400
