"""The channel-selection stage (counterpart of reference channel_selection_main.py:19-92).

``run(config)`` reads ``channel_selection.params.io.{sample_dir, output_dir}``, names its output directory by a hash of the
stage configuration, carries the configuration of the earlier stages forward, and for every ``subject_<id>.npz`` runs the
selections listed under ``params.selections`` (``module``, ``selection_name``, ``params``): the module's
``run(data, params)`` and, where it has one, ``generate_figures(data, results, params, figure_dir=...)``.  It writes
``subject_<id>.json`` as ``{selection_name: [channel indices]}`` - the file train_classifier / train_synthesizer read -
and returns the output directory.

Module names of the reference layout (``channel_selection.active``, ``channel_selection.discriminative``) and
``channel_selection.permutation`` resolve to this package's GPU selectors; any other name is imported as it is (the plugin ABI).  A subject's recordings are uploaded once
and shared by that subject's selections."""
from __future__ import annotations

import importlib
import json
import os
import sys
import warnings
from collections.abc import Mapping

import numpy as np

from .utils.config import dict_to_namespace, generate_hash_name_from_config, load_config, update_configuration

_PKG = __name__.rsplit(".", 1)[0]
_SELECTORS = ("active", "discriminative", "permutation")


def resolve_selection_module(name: str):
    """``channel_selection.active`` / ``.discriminative`` / ``.permutation`` map onto this package; anything else is
    imported as is."""
    tail = name.rsplit(".", 1)[-1]
    if tail in _SELECTORS and name == f"channel_selection.{tail}":
        name = f"{_PKG}.channel_selection.{tail}"
    return importlib.import_module(name)


class SubjectData(Mapping):
    """The arrays of one ``subject_<id>.npz`` as a read-only mapping (each array is read from the archive once), plus
    ``device(name)``: the array as a CUDA tensor, uploaded on first use and kept for the subject's other selections."""

    def __init__(self, arrays):
        self._arrays = arrays
        self._host = {}
        self._device = {}

    def __getitem__(self, key):
        if key not in self._host:
            self._host[key] = self._arrays[key]
        return self._host[key]

    def __iter__(self):
        return iter(self._arrays.keys())

    def __len__(self):
        return len(self._arrays.keys())

    def device(self, name: str):
        if name not in self._device:
            from .channel_selection.utils import to_device
            self._device[name] = to_device(self[name], "channel_selection")
        return self._device[name]


def run(config: dict) -> str:
    ch_cfg = config.get("channel_selection", {})
    ch_params = ch_cfg.get("params", {})
    io = dict_to_namespace(ch_params.get("io", {}))
    output_dir = os.path.join(io.output_dir, generate_hash_name_from_config(os.path.basename(io.sample_dir), ch_cfg))
    figure_root = os.path.join(output_dir, "figures")
    os.makedirs(figure_root, exist_ok=True)
    update_configuration(output_path=os.path.join(output_dir, "config.yaml"),
                         previous_config_path=os.path.join(io.sample_dir, "config.yaml"),
                         new_module='channel_selection', new_module_cfg=ch_cfg)

    for file_name in sorted(os.listdir(io.sample_dir)):
        if not file_name.endswith(".npz") or not file_name.startswith("subject_"):
            continue
        subject_id = file_name.split("_")[1].split(".")[0]
        sample_file_path = os.path.join(io.sample_dir, file_name)
        with np.load(sample_file_path) as arrays:
            data = SubjectData(arrays)
            subject_results = {}
            for selection in ch_params.get("selections", []):
                module_name, selection_name = selection["module"], selection["selection_name"]
                module_params = selection.get("params", {})
                print(f'Running {module_name} for subject {subject_id} from file {sample_file_path} ')
                module = resolve_selection_module(module_name)
                results = module.run(data, module_params)
                subject_results[selection_name] = [int(ch) for ch in results["selected_channels"]]
                if len(subject_results[selection_name]) == 0:
                    warnings.warn(f'No active channels found for selection {selection_name} in subject {subject_id}.')
                figure_dir = os.path.join(figure_root, selection_name, f'subject_{subject_id}')
                os.makedirs(figure_dir, exist_ok=True)
                if hasattr(module, 'generate_figures'):
                    module.generate_figures(data, results, module_params, figure_dir=figure_dir)
        output_file = os.path.join(output_dir, f'subject_{subject_id}.json')
        with open(output_file, "w") as f:
            json.dump(subject_results, f, indent=4)
        print(f'Saved results for subject {subject_id} to {output_file}.')
    return output_dir


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit("Usage: python -m decode_tonal_langauge_amd.channel_selection_main <config.yaml>")
    run(load_config(sys.argv[1]))
