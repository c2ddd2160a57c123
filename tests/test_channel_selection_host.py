"""CPU: argument checks of the three ANOVA entries, the host helpers of channel_selection.utils, the stage
(channel_selection_main.run) with a stub selection module, and the stage runner on a reference-style YAML."""
import ctypes as C
import json
import os
import sys
import types

import numpy as np
import pytest
import torch
import yaml


def test_anova_entries_refuse_bad_arguments_without_gpu():
    from decode_tonal_langauge_amd import _lib
    lib = _lib.load()
    cnt = (C.c_int32 * 64)(*([3] * 64))
    # tl_group_moments(x, is_f64, n_rows, cols, idx, n, shift, splits, sum, sumsq, stream)
    assert lib.tl_group_moments(None, 1, 4, 8, 16, 4, 16, 1, 16, 16, None) == -1 and b"null" in lib.tl_last_error()
    assert lib.tl_group_moments(16, 1, 4, 8, None, 4, 16, 1, 16, 16, None) == -1 and b"null" in lib.tl_last_error()
    assert lib.tl_group_moments(16, 1, 4, 8, 16, 4, 16, 1, None, 16, None) == -1 and b"null" in lib.tl_last_error()
    assert lib.tl_group_moments(16, 1, 4, 8, 16, 0, 16, 1, 16, 16, None) == -1 and b"at least 1" in lib.tl_last_error()
    assert lib.tl_group_moments(16, 1, 4, 0, 16, 4, 16, 1, 16, 16, None) == -1 and b"at least 1" in lib.tl_last_error()
    assert lib.tl_group_moments(16, 1, 4, 8, 16, 4, 16, 0, 16, 16, None) == -1 and b"splits" in lib.tl_last_error()
    # tl_anova_finalize(sum, sumsq, counts, k, splits, cols, F, p, stream)
    assert lib.tl_anova_finalize(None, 16, cnt, 4, 1, 8, 16, 16, None) == -1 and b"null" in lib.tl_last_error()
    assert lib.tl_anova_finalize(16, 16, None, 4, 1, 8, 16, 16, None) == -1 and b"null" in lib.tl_last_error()
    assert lib.tl_anova_finalize(16, 16, cnt, 4, 1, 8, 16, None, None) == -1 and b"null" in lib.tl_last_error()
    assert lib.tl_anova_finalize(16, 16, cnt, 1, 1, 8, 16, 16, None) == -1 and b"[2, 64]" in lib.tl_last_error()
    assert lib.tl_anova_finalize(16, 16, cnt, 65, 1, 8, 16, 16, None) == -1 and b"[2, 64]" in lib.tl_last_error()
    assert lib.tl_anova_finalize(16, 16, cnt, 4, 1, 0, 16, 16, None) == -1 and b"cols" in lib.tl_last_error()
    cnt[2] = 0
    assert lib.tl_anova_finalize(16, 16, cnt, 4, 1, 8, 16, 16, None) == -1 and b"at least one sample" in lib.tl_last_error()
    # tl_max_run_below(p, C, T, thr, count, maxrun, stream)
    assert lib.tl_max_run_below(None, 2, 8, 0.05, 16, 16, None) == -1 and b"null" in lib.tl_last_error()
    assert lib.tl_max_run_below(16, 0, 8, 0.05, 16, 16, None) == -1 and b"at least 1" in lib.tl_last_error()
    assert lib.tl_max_run_below(16, 2, 0, 0.05, 16, 16, None) == -1 and b"at least 1" in lib.tl_last_error()


def test_run_length_helpers_on_hand_made_cases():
    from decode_tonal_langauge_amd.channel_selection import find_significant_channels, get_max_length
    assert get_max_length(np.array([4, 5, 6])) == 3                          # a single run
    assert get_max_length(np.array([1, 2, 7, 8, 9, 10])) == 4                # two runs, the later one longer
    assert get_max_length(np.array([0, 1, 2, 3, 8])) == 4                    # run at the start
    assert get_max_length(np.array([2, 7, 8, 9])) == 3                       # run at the end
    assert get_max_length(np.array([5])) == 1 and isinstance(get_max_length(np.array([5])), int)
    with pytest.raises(IndexError):
        get_max_length(np.array([], dtype=int))
    T = 10
    p = np.ones((5, T))
    thr = 0.05 / T                                                           # the Bonferroni threshold of the function
    p[0, 2:6] = thr / 2                                                      # run of 4 inside
    p[1, 0:3] = thr / 2                                                      # run of 3 at the start
    p[2, 7:10] = thr / 2                                                     # run of 3 at the end
    p[3, [1, 3, 5, 7]] = thr / 2                                             # four isolated points
    p[4, 4:8] = thr                                                          # equal to the threshold: not below
    channels, lengths = find_significant_channels(p, pvalue_threshold=0.05, length_threshold=2)
    assert channels == [0, 1, 2] and lengths == []                           # max_lengths comes back empty, as mirrored
    assert find_significant_channels(p, 0.05, 3)[0] == [0]                   # strictly greater than the length
    assert find_significant_channels(p, 0.05, 4)[0] == []
    assert find_significant_channels(p * 0 + 0.04, 0.05, 0)[0] == []         # below 0.05 but not below 0.05 / T
    assert find_significant_channels(np.full((2, T), np.nan), 0.05, 0) == ([], [])


def test_selectors_mirror_the_reference_errors_before_touching_the_gpu():
    from decode_tonal_langauge_amd.channel_selection import active, discriminative
    x = np.zeros((6, 2, 5))
    with pytest.raises(KeyError):
        discriminative.run({"ecog": x, "ecog_sf": 100}, {"active_time_threshold": 0.1})
    with pytest.raises(ValueError, match="sampling frequency"):
        discriminative.run({"ecog": x, "tone": np.arange(6)}, {"target": "tone", "active_time_threshold": 0.1})
    with pytest.raises(KeyError, match="Recording 'hga' not found"):
        discriminative.test_discriminative_power({"ecog": x}, {"target": "tone", "recording_name": "hga"})
    with pytest.raises(ValueError, match="must be a 3D array"):
        discriminative.test_discriminative_power({"ecog": x[0]}, {"target": "tone"})
    with pytest.raises(KeyError, match="Labels 'tone' not found"):
        discriminative.test_discriminative_power({"ecog": x}, {"target": "tone"})
    with pytest.raises(ValueError, match="must be a 1D array"):
        discriminative.test_discriminative_power({"ecog": x, "tone": np.zeros((2, 3), dtype=int)}, {"target": "tone"})
    with pytest.raises(ValueError, match=r"\(5\) does not match"):
        discriminative.test_discriminative_power({"ecog": x, "tone": np.arange(5)}, {"target": "tone"})
    with pytest.raises(ValueError, match="must be integers"):
        discriminative.test_discriminative_power({"ecog": x, "tone": np.arange(6) / 2}, {"target": "tone"})
    prm = {"p_threshold": 0.05, "active_time_threshold": 0.1}
    with pytest.raises(ValueError, match="sampling frequency"):
        active.run({"ecog": x, "ecog_rest": x}, prm)
    with pytest.raises(KeyError, match="Recording 'ecog_rest' not found"):
        active.run({"ecog": x, "ecog_sf": 100}, prm)
    with pytest.raises(KeyError, match="Recording 'erp' not found"):
        active.run({"ecog_rest": x, "ecog_sf": 100}, dict(prm, erp_name="erp"))
    with pytest.raises(ValueError, match="Shape mismatch"):
        active.run({"ecog": x, "ecog_rest": np.zeros((4, 3, 5)), "ecog_sf": 100}, prm)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            active.run({"ecog": x, "ecog_rest": x, "ecog_sf": 100}, prm)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            discriminative.run({"ecog": x, "ecog_sf": 100, "tone": np.arange(6) % 2}, {"target": "tone", "active_time_threshold": 0.1})


def _stub_module(name, calls):
    mod = types.ModuleType(name)

    def run(data, params):
        calls.append(("run", params, sorted(data.keys()), data["ecog"].shape))
        return {"selected_channels": [np.int64(c) for c in params["pick"]], "max_lengths": [], "p_values": None}

    def generate_figures(data, results, params, figure_dir):
        calls.append(("figures", figure_dir))
    mod.run, mod.generate_figures = run, generate_figures
    return mod


def _write_samples(sample_dir, subjects=(1,)):
    from decode_tonal_langauge_amd.data_loading import synthetic
    os.makedirs(sample_dir, exist_ok=True)
    for i, sid in enumerate(subjects):
        np.savez(os.path.join(sample_dir, f"subject_{sid}.npz"),
                 **synthetic.make_subject(n_samples=40, n_channels=4, n_timepoints=20, seed=7 + i))
    with open(os.path.join(sample_dir, "config.yaml"), "w") as f:
        yaml.dump({"sample_collection": {"module": "extract_samples"}}, f)
    with open(os.path.join(sample_dir, "notes.npz.txt"), "w") as f:
        f.write("not a subject file")


def test_stage_with_a_stub_selection_module(tmp_path):
    from decode_tonal_langauge_amd import channel_selection_main
    from decode_tonal_langauge_amd.utils.config import generate_hash_name_from_config, load_config
    calls = []
    sys.modules["stub_selection"] = _stub_module("stub_selection", calls)
    try:
        sample_dir = str(tmp_path / "samples")
        _write_samples(sample_dir, subjects=(1, 2))
        ch_cfg = {"module": "channel_selection_main", "params": {
            "io": {"sample_dir": sample_dir, "output_dir": str(tmp_path / "channels")},
            "selections": [{"module": "stub_selection", "selection_name": "active_channels", "params": {"pick": [0, 2, 3]}},
                           {"module": "stub_selection", "selection_name": "tone_discriminative", "params": {"pick": []}}]}}
        with pytest.warns(UserWarning, match="No active channels found for selection tone_discriminative in subject 1"):
            out = channel_selection_main.run({"channel_selection": ch_cfg})
        assert out == os.path.join(str(tmp_path / "channels"), generate_hash_name_from_config("samples", ch_cfg))
        for sid in (1, 2):
            with open(os.path.join(out, f"subject_{sid}.json")) as f:
                assert json.load(f) == {"active_channels": [0, 2, 3], "tone_discriminative": []}
        carried = load_config(os.path.join(out, "config.yaml"))
        assert carried["sample_collection"] == {"module": "extract_samples"} and carried["channel_selection"] == ch_cfg
        runs = [c for c in calls if c[0] == "run"]
        assert len(runs) == 4 and runs[0][1] == {"pick": [0, 2, 3]} and "ecog_rest" in runs[0][2] and runs[0][3] == (40, 4, 20)
        figs = [c[1] for c in calls if c[0] == "figures"]
        assert os.path.join(out, "figures", "tone_discriminative", "subject_2") in figs and all(os.path.isdir(d) for d in figs)
    finally:
        del sys.modules["stub_selection"]
    # the reference layout's selector names resolve to this package
    for tail in ("active", "discriminative"):
        mod = channel_selection_main.resolve_selection_module(f"channel_selection.{tail}")
        assert mod.__name__ == f"decode_tonal_langauge_amd.channel_selection.{tail}" and hasattr(mod, "run")


def test_stage_runner_picks_the_stage_up_from_a_reference_style_yaml(tmp_path):
    """``channel_selection.module: channel_selection_main`` resolves; its output directory reaches training as
    ``channel_selection_dir`` (the stub training stage records what it was given)."""
    from decode_tonal_langauge_amd.main import run_pipeline
    calls, seen = [], {}
    sys.modules["stub_selection"] = _stub_module("stub_selection", calls)
    trainer = types.ModuleType("stub_training")
    trainer.run = lambda config: seen.update(config["training"]["params"]["io"])
    sys.modules["stub_training"] = trainer
    try:
        sample_dir = str(tmp_path / "samples")
        _write_samples(sample_dir)
        cfg = {"channel_selection": {"module": "channel_selection_main", "params": {
                   "io": {"sample_dir": sample_dir, "output_dir": str(tmp_path / "channels")},
                   "selections": [{"module": "stub_selection", "selection_name": "active_channels", "params": {"pick": [1]}}]}},
               "training": {"module": "stub_training", "params": {"io": {"sample_dir": sample_dir}}}}
        path = str(tmp_path / "cfg.yaml")
        with open(path, "w") as f:
            yaml.dump(cfg, f)
        run_pipeline(path)
        chan_dir = seen["channel_selection_dir"]
        assert os.path.dirname(chan_dir) == str(tmp_path / "channels")
        with open(os.path.join(chan_dir, "subject_1.json")) as f:
            assert json.load(f) == {"active_channels": [1]}
    finally:
        del sys.modules["stub_selection"], sys.modules["stub_training"]
