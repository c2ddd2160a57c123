#!/usr/bin/env python
"""The preprocess stage on one synthetic block of real size: ECoG 256 x 366 210 float32 at 3051.7578125 Hz (120 s, the size
``tests/test_gpu_signal_steps.py`` uses), audio 1 x 2 929 687 float32 at 24414.0625 Hz without steps, the chain of the
reference's ``example_config.yaml`` (downsample to 400 Hz, Hilbert envelope 70 - 150 Hz plus Butterworth 0.3 - 100 Hz,
z-score against the first 25 s).

  (a) ``subject_block.run`` over that block, ``resident: true``, no figures: the wall time and its parts - ``load_block``
      (``np.load``), the upload, the steps (HIP events around ``preprocess_modalities``), the download, ``save_block``
      (``np.savez``).  The parts are taken by wrapping the io module and the preprocessor the pipeline is handed; the pipeline
      itself is the product's.
  (b) the same with ``resident: false`` (every step uploads and downloads for itself, as a host preprocessor would be driven),
      and once with ``figures: true``.
  (c) ``extract_samples.run`` over the block the stage wrote: from the files (the code of the parent commit - the baseline)
      against handed over by ``keep_resident``.

    python scripts/bench_preprocess_stage.py [--rounds 3] [--out-dir profiles] [--time-limit 420]

writes ``preprocess_stage.json`` and ``preprocess_stage.md`` into the output directory.  Nothing here is a pass mark."""
from __future__ import annotations

import argparse
import json
import os
import platform
import signal
import sys
import tempfile
import time
import types
import warnings
from copy import deepcopy

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

C, SECONDS, ECOG_SF, AUDIO_SF = 256, 120, 3051.7578125, 24414.0625
CHAIN = [
    {"module": "preprocess.downsample", "params": {"downsample_freq": 400}},
    {"module": "preprocess.frequency_filter", "params": {"bands": [
        {"method": "hilbert", "params": {"freq_ranges": [70., 150.], "envelope": True}},
        {"method": "butter", "params": {"freqs": [0.3, 100], "filter_type": "bandpass"}}]}},
    {"module": "preprocess.zscore_rereference", "params": {"rereference_interval": [0., 25.]}},
]
N_EVENTS, REST = 100, (0.0, 10.0)
PARTS = ("load", "upload", "steps", "download", "save")


def _median(v):
    v = sorted(v)
    return v[len(v) // 2]


def _span(v):
    return f"{_median(v):.1f} ({min(v):.1f} .. {max(v):.1f})"


class _Timed:
    """The io module and the preprocessor ``subject_block.run`` is handed, with a clock around each part."""

    def __init__(self, resident: bool):
        import torch
        from decode_tonal_langauge_amd.preprocess import preprocessor
        from decode_tonal_langauge_amd.preprocess.io import npz_blocks
        from decode_tonal_langauge_amd.preprocess.pipelines import subject_block
        self.torch, self.ms, self.saved = torch, dict.fromkeys(PARTS, 0.0), None
        timed = self

        def load_block(block_path):
            t0 = time.perf_counter()
            data = npz_blocks.load_block(block_path)
            timed.ms["load"] += (time.perf_counter() - t0) * 1e3
            return data

        def save_block(setup_dir, subject_id, block_id, data_dict):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host = {k: v.cpu().numpy() if isinstance(v, torch.Tensor) else v for k, v in data_dict.items()}
            t1 = time.perf_counter()
            npz_blocks.save_block(setup_dir, subject_id, block_id, host)
            timed.ms["download"] += (t1 - t0) * 1e3
            timed.ms["save"] += (time.perf_counter() - t1) * 1e3
            timed.saved = (block_id, data_dict)

        def preprocess_modalities(data_dict, modalities_cfg, base_params, figure_dir=None, resident=False, shard_channels=False):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            out = preprocessor.preprocess_modalities(data_dict, modalities_cfg, base_params, figure_dir=figure_dir,
                                                     resident=resident, shard_channels=shard_channels)
            b.record()
            torch.cuda.synchronize()
            timed.ms["steps"] += a.elapsed_time(b)
            return out

        upload = subject_block._upload

        def timed_upload(data_dict, modalities_cfg):
            t0 = time.perf_counter()
            upload(data_dict, modalities_cfg)
            torch.cuda.synchronize()
            timed.ms["upload"] += (time.perf_counter() - t0) * 1e3

        self.io = types.SimpleNamespace(load_block=load_block, save_block=save_block)
        self.preprocessor = types.SimpleNamespace(preprocess_modalities=preprocess_modalities)
        self.upload, self.resident, self.subject_block = timed_upload, resident, subject_block

    def run(self, tree, out_dir, **pipeline):
        from decode_tonal_langauge_amd.utils.config import dict_to_namespace
        sb, keep = self.subject_block, self.subject_block._upload
        sb._upload = self.upload
        try:
            self.torch.cuda.synchronize()
            t0 = time.perf_counter()
            setup = sb.run(dict_to_namespace({"subject_dirs": tree["subject_dirs"], "subject_ids": tree["subject_ids"],
                                              "resident": self.resident, **pipeline}),
                           dict_to_namespace({"root_dir": tree["root_dir"], "output_dir": out_dir}), self.io, self.preprocessor,
                           {"ecog": {"type": "signal", "preprocessing": {"steps": deepcopy(CHAIN)}}, "audio": {"type": "signal"}})
            self.torch.cuda.synchronize()
            self.ms["total"] = (time.perf_counter() - t0) * 1e3
        finally:
            sb._upload = keep
        return setup


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--time-limit", type=int, default=420, help="seconds after which the run gives up")
    args = ap.parse_args()

    def give_up(*_):
        raise SystemExit(f"bench_preprocess_stage: no result within {args.time_limit} s")
    signal.signal(signal.SIGALRM, give_up)
    signal.alarm(args.time_limit)

    import torch
    from decode_tonal_langauge_amd import extract_samples
    from decode_tonal_langauge_amd.data_loading import synthetic
    from decode_tonal_langauge_amd.preprocess import handover
    arch = torch.cuda.get_device_properties(0).gcnArchName.split(":")[0]
    name = {"gfx950": "MI355X"}.get(arch, arch)
    T = int(SECONDS * ECOG_SF)
    res = {"device": f'{name} ({arch}; the runtime names it "{torch.cuda.get_device_name(0)}")',
           "host": f"{platform.processor() or platform.machine()}, {os.cpu_count()} logical CPUs", "ecog": [C, T],
           "ecog_sf": ECOG_SF, "audio": [1, int(SECONDS * AUDIO_SF)], "audio_sf": AUDIO_SF, "chain": CHAIN, "rounds": args.rounds,
           "stage": {}, "collection": {"files_ms": [], "handed_over_ms": []}}
    keep_out, sys.stdout = sys.stdout, open(os.devnull, "w")                       # the stage prints its progress
    try:
        with tempfile.TemporaryDirectory() as tmp, warnings.catch_warnings():
            warnings.simplefilter("ignore")
            tree = synthetic.write_raw_tree(os.path.join(tmp, "raw"), {1: {1: float(SECONDS)}}, n_channels=C, ecog_sf=ECOG_SF,
                                            audio_sf=AUDIO_SF, seed=16)
            events = [(12.0 + k, 12.6 + k, 1 + k % 4, "ai"[k % 2]) for k in range(N_EVENTS)]
            synthetic.write_block_annotations(os.path.join(tmp, "tg", "s1"), 1, events, seconds=float(SECONDS))
            for label, resident, extra in (("resident", True, {"figures": False}), ("per_step", False, {"figures": False})):
                rows = {k: [] for k in PARTS + ("total",)}
                for r in range(args.rounds + 1):                                   # the first round warms up (coefficient caches)
                    timed = _Timed(resident)
                    setup = timed.run(tree, os.path.join(tmp, "out"), **extra)
                    if r:
                        for k in rows:
                            rows[k].append(timed.ms[k])
                res["stage"][label] = rows
                if resident:
                    kept = timed.saved
            timed = _Timed(True)
            timed.run(tree, os.path.join(tmp, "out_figures"), figures=True)
            res["stage"]["resident_with_figures_total_ms"] = timed.ms["total"]
            with np.load(os.path.join(setup, "subject_1", "B1_ecog.npz")) as block:
                res["written"] = {"ecog": list(block["data"].shape), "dtype": str(block["data"].dtype), "sf": float(block["sf"]),
                                  "bytes": int(block["data"].nbytes)}
            cfg = {"sample_collection": {"module": "extract_samples", "params": {
                "io": {"recording_dir": setup, "textgrid_root": os.path.join(tmp, "tg"), "output_dir": os.path.join(tmp, "samples")},
                "settings": {"syllable_identifiers": ["a", "i"], "figures": False, "overwrite": True},
                "subjects": {1: {"textgrid_dir": "s1", "sample_length": 1.0, "rest_period": list(REST)}}}}}
            subject_dir, results = os.path.join(setup, "subject_1"), {}
            for r in range(args.rounds + 1):
                for key, handed in (("files_ms", False), ("handed_over_ms", True)):
                    handover.release()
                    if handed:
                        handover.register(subject_dir, *kept)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    out = extract_samples.run(deepcopy(cfg))
                    torch.cuda.synchronize()
                    if r:
                        res["collection"][key].append((time.perf_counter() - t0) * 1e3)
                    with np.load(os.path.join(out, "subject_1.npz")) as d:
                        results[key] = {k: d[k].tobytes() for k in d.files}
            handover.release()
            assert results["files_ms"] == results["handed_over_ms"], "the two routes of sample collection differ"
            res["collection"]["windows"] = N_EVENTS
    finally:
        sys.stdout.close()
        sys.stdout = keep_out
    signal.alarm(0)

    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "preprocess_stage.json"), "w") as f:
        json.dump(res, f, indent=1)
    s, p, c, w = res["stage"]["resident"], res["stage"]["per_step"], res["collection"], res["written"]
    parts = sum(_median(s[k]) for k in PARTS)
    lines = [
        "# Preprocess stage: one block of real size", "",
        f"Written by `scripts/bench_preprocess_stage.py` on one {res['device']} (host: {res['host']}): one synthetic block, ECoG",
        f"{C} x {T} float32 at {ECOG_SF} Hz ({C * T * 4 / 1e6:.0f} MB), audio 1 x {res['audio'][1]} float32 without steps, the chain of",
        f"`example_config.yaml`; written: ECoG {w['ecog'][0]} x {w['ecog'][1]} {w['dtype']} at {w['sf']:.0f} Hz ({w['bytes'] / 1e6:.0f} MB).",
        f"Median of {args.rounds} rounds after a warm-up round (min .. max), milliseconds.  None of these figures is a pass mark.", "",
        "| part of `subject_block.run` | `resident: true` | `resident: false` | note |", "|---|---|---|---|",
        f"| `load_block` | {_span(s['load'])} | {_span(p['load'])} | `np.load` of `ecog.npz` and `audio.npz` |",
        f"| upload | {_span(s['upload'])} | {_span(p['upload'])} | the ECoG, once, pageable host memory; `resident: false`: inside the steps |",
        f"| steps | {_span(s['steps'])} | {_span(p['steps'])} | HIP events around `preprocess_modalities`; `resident: false`: with one upload "
        "and one download per step |",
        f"| download | {_span(s['download'])} | {_span(p['download'])} | the processed ECoG, once; `resident: false`: inside the steps |",
        f"| `save_block` | {_span(s['save'])} | {_span(p['save'])} | `np.savez` of both modalities |",
        f"| whole stage | {_span(s['total'])} | {_span(p['total'])} | wall clock; the parts sum to {parts:.1f} |", "",
        f"- The device work is {_median(s['steps']) / _median(s['total']):.2f} of the resident stage; files and the bus are the rest "
        f"(`load_block` + `save_block`: {(_median(s['load']) + _median(s['save'])) / _median(s['total']):.2f}).",
        f"- With `figures: true` (the default, as the reference always draws) the resident stage took "
        f"{res['stage']['resident_with_figures_total_ms']:.0f} ms, one run.", "",
        "| sample collection over that block (`extract_samples.run`, "
        f"{N_EVENTS} windows of 1 s, rest {REST[0]:.0f} - {REST[1]:.0f} s) | ms |", "|---|---|",
        f"| from the files the stage wrote (the parent commit's route: the baseline) | {_span(c['files_ms'])} |",
        f"| handed over (`keep_resident: true`) | {_span(c['handed_over_ms'])} |", "",
        f"- Handed over takes {_median(c['handed_over_ms']) / _median(c['files_ms']):.2f} of the file route; both write the same "
        "`subject_1.npz`, byte for byte (checked in this run), and writing it is part of both figures.", ""]
    with open(os.path.join(args.out_dir, "preprocess_stage.md"), "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
