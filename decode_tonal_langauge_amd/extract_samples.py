"""The sample-collection stage (counterpart of reference extract_samples.py): TextGrid intervals plus the preprocessed block
recordings of every subject -> ``subject_<id>.npz``, the file channel selection and training read.

``run(config)`` reads ``sample_collection.params.{io, settings, subjects}``:

  io        ``recording_dir`` (output of the preprocess stage: ``subject_<id>/B<block>_<modality>.npz``), ``textgrid_root``,
            ``output_dir``
  settings  ``syllable_identifiers``, optional ``overwrite``, optional ``figures`` (default true: the event figure per block)
  subjects  ``<id>: {textgrid_dir, sample_length, rest_period, start_offset?, tier_list?, blocks?}``

The output directory is ``<basename(recording_dir)>__<md5(yaml.dump(stage config, sort_keys=True))[:6]>``; the configuration
of the earlier stages is carried forward into its ``config.yaml``.  A subject is skipped when its recording directory is
missing, when its output exists and ``overwrite`` is not set, or when its TextGrid directory is missing.  The window copies
run on the GPU (``data_loading/text_align.py``).

Resident hand-over: a subject whose ``subject_path`` the preprocess stage of this process registered
(``preprocess.params.pipeline.params.keep_resident: true``, ``preprocess/handover.py``) is epoched from the blocks that stage
left in memory - visited in the order of their files in a sorted listing - instead of from the files it wrote; results,
``subject_<id>.npz`` and the printed lines are those of the file route.  Without a registration nothing changes."""
from __future__ import annotations

import hashlib
import os
import sys
import warnings

import numpy as np
import yaml

from .data_loading.text_align import extract_ecog_audio, handle_textgrids
from .preprocess import handover
from .utils.config import dict_to_namespace, load_config, update_configuration


def output_dir_name(base_name: str, collection_cfg: dict) -> str:
    digest = hashlib.md5(yaml.dump(collection_cfg, sort_keys=True).encode()).hexdigest()[:6]
    return f"{base_name}__{digest}"


def run(config: dict) -> str:
    collection_cfg = config.get("sample_collection", {})
    params_config = collection_cfg.get("params", {})
    merged = {}
    for section in ("io", "settings"):
        merged.update(params_config.get(section, {}))
    params = dict_to_namespace(merged)
    overwrite = bool(getattr(params, "overwrite", False))
    figures = bool(getattr(params, "figures", True))

    output_dir = os.path.join(params.output_dir, output_dir_name(os.path.basename(params.recording_dir), collection_cfg))
    figure_root = os.path.join(output_dir, "figures")
    os.makedirs(figure_root, exist_ok=True)
    update_configuration(output_path=os.path.join(output_dir, "config.yaml"),
                         previous_config_path=os.path.join(params.recording_dir, "config.yaml"),
                         new_module='sample_collection', new_module_cfg=collection_cfg)

    for subject_id, subject_params in params_config.get("subjects", {}).items():
        subject_path = os.path.join(params.recording_dir, f"subject_{subject_id}")
        if not os.path.exists(subject_path):
            print(f"Recording directory {subject_path} not found. Skipping...")
            continue
        subject_output_path = os.path.join(output_dir, f"subject_{subject_id}.npz")
        if os.path.exists(subject_output_path) and not overwrite:
            print(f"Output file {subject_output_path} already exists. Skipping ...")
            continue
        textgrid_dir = os.path.join(params.textgrid_root, subject_params["textgrid_dir"])
        if not os.path.exists(textgrid_dir):
            print(f"TextGrid directory {textgrid_dir} not found. Skipping...")
            continue
        print(f"Extracting all samples from {subject_path} using textgrids from {textgrid_dir}")
        blocks = subject_params.get("blocks", None)
        intervals = handle_textgrids(textgrid_dir, start_offset=subject_params.get("start_offset", 0.0),
                                     tier_list=subject_params.get("tier_list", None), blocks=blocks)
        if len(intervals) == 0:
            raise ValueError("No intervals found in the TextGrid files. Check the directory and file naming conventions."
                             f"Target blocks: {blocks if blocks else 'all'}")
        print(f"Extracted intervals from TextGrid files: {len(intervals)} blocks found.")
        resident = handover.lookup(subject_path)
        recordings = None
        if resident:                                     # "B10_" sorts before "B1_": the order of the files
            recordings = {block: resident[block] for block in sorted(resident, key=lambda block: f"B{block}_")}
        for block_id, table in intervals.items():
            if figures and len(table):
                plot_block_events(subject_path, subject_id, block_id, table.to_dict("records"),
                                  os.path.join(figure_root, f"subject_{subject_id}"),
                                  recording=(recordings or {}).get(block_id, {}).get("ecog"))
        extract_ecog_audio(intervals, subject_path, syllables=params.syllable_identifiers,
                           length=subject_params["sample_length"], output_path=subject_output_path,
                           rest_period=tuple(subject_params["rest_period"]), recordings=recordings,
                           announce=recordings is not None)
    return output_dir


def plot_block_events(subject_path: str, subject_id, block_id, events: list, fig_dir: str, num_events: int = 3,
                      recording=None) -> None:
    """Three consecutive events of a block on ``min(5, C)`` random channels, the event spans highlighted (host matplotlib;
    outside the tested contract).  Nothing is drawn without matplotlib or without ``B<block>_ecog.npz``; ``recording``
    (``(data, sf)``, a NumPy array or a tensor) is drawn instead of the file when given, and only the span that is drawn is
    copied to the host."""
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except ImportError:
        warnings.warn("matplotlib is not importable: no event figures")
        return
    if recording is not None:
        signal, sf = recording[0], float(recording[1])
    else:
        ecog_path = os.path.join(subject_path, f"B{block_id}_ecog.npz")
        if not os.path.exists(ecog_path):
            return
        with np.load(ecog_path) as ecog:
            signal, sf = ecog["data"], float(ecog["sf"])
    events = sorted(events, key=lambda e: e["start"])
    if len(events) > num_events:
        first = np.random.randint(0, len(events) - num_events + 1)
        events = events[first:first + num_events]
    channels = np.random.choice(signal.shape[0], size=min(5, signal.shape[0]), replace=False)
    lo = int(max(min(e["start"] for e in events) - 0.5, 0) * sf)
    hi = min(int((max(e["end"] for e in events) + 0.5) * sf), signal.shape[1])
    n_samples, span = signal.shape[1], signal[:, lo:hi]
    span = span if isinstance(span, np.ndarray) else span.detach().cpu().numpy()
    fig, axes = plt.subplots(len(channels), 1, figsize=(12, 4 * len(channels)), sharex=True, squeeze=False)
    for ax, ch in zip(axes[:, 0], channels):
        ax.plot(np.arange(lo, hi) / sf, span[ch], label="Offset", color="blue", alpha=0.7)
        for k, e in enumerate(events):
            a, b = int(e["start"] * sf), min(int(e["end"] * sf), n_samples)
            ax.plot(np.arange(a, b) / sf, span[ch, a - lo:b - lo], label="Onset" if k == 0 else None, color="orange")
            ax.axvline(e["start"], color="g", linestyle="--", alpha=0.7, label="Event Start" if k == 0 else None)
            ax.axvline(e["end"], color="r", linestyle="--", alpha=0.7, label="Event End" if k == 0 else None)
        ax.set_title(f"Channel {ch}", fontsize=18)
        ax.set_ylabel("Amplitude", fontsize=16)
        ax.legend(fontsize=14, loc="upper right", bbox_to_anchor=(1.2, 1), borderaxespad=0.)
    axes[-1, 0].set_xlabel("Time (s)", fontsize=16)
    fig.suptitle(f"Subject {subject_id} Block {block_id}", fontsize=20)
    fig.tight_layout()
    fig.subplots_adjust(top=0.93)
    os.makedirs(fig_dir, exist_ok=True)
    fig.savefig(os.path.join(fig_dir, f"block_{block_id}_events.png"), dpi=100)
    plt.close(fig)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit("Usage: python -m decode_tonal_langauge_amd.extract_samples <config.yaml>")
    run(load_config(sys.argv[1]))
