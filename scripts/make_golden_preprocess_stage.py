#!/usr/bin/env python3
"""Writes tests/golden/preprocess_stage_ref.json: what the REFERENCE implementation's block driver
(``preprocess/pipelines/subject_block.py``) gives for a set of directory names, a set of modality configurations and one run
over a small tree.

    python scripts/make_golden_preprocess_stage.py --reference /path/to/reference/checkout

Host only; run once on a build machine that has the reference checkout, never by a test.  The reference's
``preprocess/io/tdt_blocks.py`` imports the ``tdt`` package at module level and only calls it inside ``load_block``; a stub
module is registered under that name so that its ``save_block`` can be used as it is.  The io module the run is driven with
is a stub defined here (its ``load_block`` makes two small arrays from the block path, its ``save_block`` is the
reference's), and so is the identity preprocessor.  The reference visits a subject's directories in the file system's
order; files are recorded as a sorted list and blocks as a sorted list of (subject, block), which is what the product is
compared on."""
import argparse
import contextlib
import importlib
import io
import json
import os
import sys
import tempfile
import types

import numpy as np
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BLOCK_NAMES = ["HS1-3", "HS12-B7", "HS1-notes", "notes", "B5", "HS3-12", "HS2-B", "HS-2-4", "HS4-B10", "HS1-3.5", "HS1- 6",
               "HS1-B0"]

EXAMPLE_STEPS = [
    {"module": "preprocess.downsample", "params": {"downsample_freq": 400}},
    {"module": "preprocess.frequency_filter", "params": {"bands": [
        {"method": "hilbert", "params": {"freq_ranges": [70, 150], "envelope": True}},
        {"method": "butter", "params": {"freqs": [0.3, 100], "filter_type": "bandpass"}}]}},
    {"module": "preprocess.zscore_rereference", "params": {"rereference_interval": [0., 25.]}},
]

MODALITY_CONFIGS = {
    "no steps": {"ecog": {"type": "signal"}, "audio": {"type": "signal"}},
    "empty": {},
    "example config": {"ecog": {"type": "signal", "preprocessing": {"steps": EXAMPLE_STEPS}}, "audio": {"type": "signal"}},
    "two modalities with steps": {
        "ecog": {"type": "signal", "preprocessing": {"steps": [
            {"module": "preprocess.signal.car_rereference", "params": {}},
            {"module": "preprocess.signal.downsample", "params": {"downsample_freq": 200.5}}]}},
        "audio": {"type": "signal", "preprocessing": {"steps": [
            {"module": "preprocess.signal.channel_zscore", "params": {"zscore_axis": 1}}]}}},
    "a step without params": {"ecog": {"type": "signal", "preprocessing": {"steps": [
        {"module": "preprocess.signal.channel_zscore"}, {"module": "my_lab.steps.notch", "params": {"freq": 50}}]}}},
    "nested params": {"ecog": {"type": "signal", "preprocessing": {"steps": [
        {"module": "plugin_step", "params": {"outer": {"inner": [1, 2.5, "x"], "flag": None}, "name": "a b"}}]}}},
}

# the run: 2 subjects x 2 blocks and one stray directory; flat parameters, so that the reference's config.yaml
# (vars(Namespace)) is a file yaml.safe_load reads
RUN_TREE = {"Sub1/tdt": ["HS1-1", "HS1-B2", "HS1-notes"], "Sub2/tdt": ["HS2-3", "HS2-10"]}
RUN_PIPELINE = {"subject_dirs": ["Sub1/tdt", "Sub2/tdt"], "subject_ids": [1, 2]}
RUN_IO_EXTRA = {"line_noise": 50}
RUN_MODALITIES = MODALITY_CONFIGS["two modalities with steps"]


def tree_listing(root: str) -> list:
    """Sorted relative paths below ``root``; a directory ends in ``/``."""
    out = []
    for base, dirs, files in os.walk(root):
        out += [os.path.relpath(os.path.join(base, d), root).replace(os.sep, "/") + "/" for d in dirs]
        out += [os.path.relpath(os.path.join(base, f), root).replace(os.sep, "/") for f in files]
    return sorted(out)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference checkout")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "preprocess_stage_ref.json"))
    args = ap.parse_args()

    sys.modules["tdt"] = types.ModuleType("tdt")
    sys.path.insert(0, os.path.abspath(args.reference))
    ref = importlib.import_module("preprocess.pipelines.subject_block")
    ref_io = importlib.import_module("preprocess.io.tdt_blocks")
    ref_cfg = importlib.import_module("utils.config")

    golden = {"block_ids": {}, "setup_names": {}}
    with contextlib.redirect_stdout(io.StringIO()):
        for name in BLOCK_NAMES:
            golden["block_ids"][name] = ref.get_block_id(name)
    for label, cfg in MODALITY_CONFIGS.items():
        golden["setup_names"][label] = {"modalities": cfg, "name": ref.generate_setup_name(cfg)}

    seen = []
    stub_io = types.SimpleNamespace(save_block=ref_io.save_block)

    def load_block(block_path):
        seen.append(os.path.basename(block_path))
        n = 4 + len(seen)
        return {"ecog": np.arange(2 * n, dtype=np.float32).reshape(2, n), "audio": np.ones((1, 3), dtype=np.int16),
                "ecog_sf": 1017.25, "audio_sf": 24414.0625}

    stub_io.load_block = load_block
    identity = types.SimpleNamespace(preprocess_modalities=lambda data_dict, modalities_cfg, base_params, figure_dir=None: data_dict)

    with tempfile.TemporaryDirectory() as tmp:
        raw, out = os.path.join(tmp, "raw"), os.path.join(tmp, "processed")
        for subject_dir, names in RUN_TREE.items():
            for name in names:
                os.makedirs(os.path.join(raw, subject_dir, name))
        io_cfg = {"root_dir": raw, "output_dir": out, **RUN_IO_EXTRA}
        with contextlib.redirect_stdout(io.StringIO()) as lines:
            setup_dir = ref.run(ref_cfg.dict_to_namespace(RUN_PIPELINE), ref_cfg.dict_to_namespace(io_cfg), stub_io, identity,
                                RUN_MODALITIES)
        with open(os.path.join(setup_dir, "config.yaml")) as f:
            written = yaml.safe_load(f)
        # the two directories are the only machine-dependent values of the file
        written["preprocess"]["io"]["root_dir"] = "<root_dir>"
        written["preprocess"]["io"]["output_dir"] = "<output_dir>"
        with np.load(os.path.join(setup_dir, "subject_1", "B1_audio.npz")) as saved:
            audio_keys, audio_dtype = sorted(saved.files), str(saved["data"].dtype)
        golden["run"] = {
            "tree": RUN_TREE, "pipeline": RUN_PIPELINE, "io_extra": RUN_IO_EXTRA, "modalities": RUN_MODALITIES,
            "setup_name": os.path.relpath(setup_dir, out),
            "files": tree_listing(setup_dir),
            "config": written,
            "blocks_loaded": sorted(seen),
            "progress_lines": sorted(line for line in lines.getvalue().splitlines() if line.startswith("Processing block")),
            "skipped_lines": sorted(line for line in lines.getvalue().splitlines() if line.startswith("Skipping")),
            "saved_keys": audio_keys, "saved_audio_dtype": audio_dtype,
        }
    with open(args.out, "w") as f:
        json.dump(golden, f, indent=1)                  # key order is data: the setup name depends on it
        f.write("\n")
    print(args.out, os.path.getsize(args.out), "bytes")
    print(json.dumps(golden["block_ids"]), [v["name"] for v in golden["setup_names"].values()], golden["run"]["setup_name"])


if __name__ == "__main__":
    main()
