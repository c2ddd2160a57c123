#!/usr/bin/env python3
"""Recording diagnostics: ``welch_psd`` and ``segment_mean_std`` (utils/diagnostics.py) on the GPU against what the reference
does on the host, on the same box in the same run.  Nothing here is a pass mark.

Sizes (float32): 256 x 24 000 at 400 Hz (60 s of a processed block), 256 x 366 210 and 6 x 366 210 at 3051.7578125 Hz (a
raw-rate block of 120 s).  Welch at the defaults (Hann, nperseg 256, overlap 128, constant detrend), the moments over all
whole seconds.

GPU leg: the recording resident on the device, HIP events around one call (allocation of the outputs and the workspace by the
caching allocator included), median of 5 after a warm-up call.  Beside the time: the bytes of the recording read once over the
time, against the 6.3 TB/s a streaming kernel reaches on an MI355X (HBM3E, 8 TB/s on paper).  With 50 % overlap every sample is
requested twice; the second request is EXPECTED to be served by L2 (neighbouring segments are gathered by the same workgroup
in the same or the next trip).  Nobody has measured that: no counter run is part of this script.

Host legs, ``time.perf_counter`` around one call after one warm-up call, no thread count set by this process:
  * what the reference does: ``matplotlib.mlab.psd`` (the arithmetic of ``plt.psd``) per channel in a Python loop, and the
    NumPy loop over one-second segments (``np.mean`` / ``np.std`` of ``data[:, a:b]``);
  * ``scipy.signal.welch(axis=1)`` at the same settings.

Stage: ``subject_block.run`` over the synthetic 256-channel block of scripts/bench_preprocess_stage.py (its chain, resident, no
figures) with and without ``diagnostics: true``, wall clock, median of ``--rounds`` after a warm-up round: what switching it on
costs.

    python scripts/bench_spectral_diagnostics.py [--out-dir profiles] [--rounds 2] [--no-stage]

writes ``spectral_diagnostics.json`` and prints the tables of ``profiles/spectral_diagnostics.md``."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
import warnings
from copy import deepcopy

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SIZES = [(256, 24000, 400.0), (256, 366210, 3051.7578125), (6, 366210, 3051.7578125)]
REPS = 5
HBM_ACHIEVABLE_TBPS = 6.3


def _gpu_ms(torch, fn):
    fn()
    ms = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def _host_ms(fn):
    fn()
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def _segment_loop(x, L, n):
    means, stds = np.zeros((x.shape[0], n)), np.zeros((x.shape[0], n))
    for i in range(n):
        seg = x[:, i * L:(i + 1) * L]
        means[:, i] = np.mean(seg, axis=1)
        stds[:, i] = np.std(seg, axis=1)
    return means, stds


def _stage(torch, rounds):
    from decode_tonal_langauge_amd.data_loading import synthetic
    from decode_tonal_langauge_amd.preprocess import preprocessor
    from decode_tonal_langauge_amd.preprocess.io import npz_blocks
    from decode_tonal_langauge_amd.preprocess.pipelines import subject_block
    from decode_tonal_langauge_amd.utils.config import dict_to_namespace
    import bench_preprocess_stage as stage
    out = {"off_ms": [], "on_ms": []}
    keep, sys.stdout = sys.stdout, open(os.devnull, "w")                           # the stage prints its progress
    try:
        with tempfile.TemporaryDirectory() as tmp, warnings.catch_warnings():
            warnings.simplefilter("ignore")
            tree = synthetic.write_raw_tree(os.path.join(tmp, "raw"), {1: {1: float(stage.SECONDS)}}, n_channels=stage.C,
                                            ecog_sf=stage.ECOG_SF, audio_sf=stage.AUDIO_SF, seed=16)
            for r in range(rounds + 1):                                            # the first round warms up
                for key, on in (("off_ms", False), ("on_ms", True)):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    setup = subject_block.run(
                        dict_to_namespace({"subject_dirs": tree["subject_dirs"], "subject_ids": tree["subject_ids"],
                                           "figures": False, **({"diagnostics": True} if on else {})}),
                        dict_to_namespace({"root_dir": tree["root_dir"], "output_dir": os.path.join(tmp, key)}), npz_blocks,
                        preprocessor, {"ecog": {"type": "signal", "preprocessing": {"steps": deepcopy(stage.CHAIN)}},
                                       "audio": {"type": "signal"}})
                    torch.cuda.synchronize()
                    if r:
                        out[key].append((time.perf_counter() - t0) * 1e3)
            where = os.path.join(setup, "diagnostics", "subject_1", "block_1", "ecog")
            out["files"] = sorted(os.listdir(where))
            out["bytes"] = sum(os.path.getsize(os.path.join(where, f)) for f in out["files"])
    finally:
        sys.stdout.close()
        sys.stdout = keep
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--no-stage", action="store_true")
    args = ap.parse_args()
    import scipy.signal
    import torch
    from matplotlib import mlab
    from decode_tonal_langauge_amd.utils import diagnostics
    if not torch.cuda.is_available():
        raise SystemExit("bench_spectral_diagnostics: no GPU visible; nothing is measured without one")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "host_cpus": os.cpu_count(), "reps": REPS, "rows": []}
    for C, T, fs in SIZES:
        x = (np.random.default_rng(T + C).standard_normal((C, T)) * 30.0 + 5.0).astype(np.float32)
        xd = torch.from_numpy(x).to(dev)
        L, n = int(fs), T // int(fs)
        welch = _gpu_ms(torch, lambda: diagnostics.welch_psd(xd, fs))
        moments = _gpu_ms(torch, lambda: diagnostics.segment_mean_std(xd, fs, 0.0, float(n)))
        psd = diagnostics.welch_psd(xd, fs)[1].cpu().numpy()
        mean, std = (a.cpu().numpy() for a in diagnostics.segment_mean_std(xd, fs, 0.0, float(n)))
        mlab_ms, theirs = _host_ms(lambda: np.stack([mlab.psd(x[c], NFFT=256, Fs=fs, noverlap=128)[0] for c in range(C)]))
        scipy_ms, sp = _host_ms(lambda: scipy.signal.welch(x.astype(np.float64), fs=fs, nperseg=256, axis=1)[1])
        loop_ms, (m_ref, s_ref) = _host_ms(lambda: _segment_loop(x, L, n))
        row = {"C": C, "T": T, "fs": fs, "n_seg": (T - 128) // 128, "slabs": diagnostics.plan_slabs(
                   (T - 128) // 128, 256, C, torch.cuda.get_device_properties(dev).multi_processor_count)[0],
               "welch_ms": statistics.median(welch), "welch_all_ms": welch, "moments_ms": statistics.median(moments),
               "moments_all_ms": moments, "mlab_per_channel_ms": mlab_ms, "scipy_welch_ms": scipy_ms, "numpy_segment_loop_ms": loop_ms,
               "welch_TBps_of_bytes_read_once": C * T * 4 / statistics.median(welch) / 1e9,
               "moments_TBps_of_bytes_read_once": C * n * L * 4 / statistics.median(moments) / 1e9,
               "welch_vs_scipy_of_row_max": float((np.abs(psd - sp).max(axis=1) / sp.max(axis=1)).max()),
               "moments_vs_numpy_float32_loop": float(max(np.abs(mean - m_ref).max(), np.abs(std - s_ref).max()))}
        res["rows"].append(row)
        print(json.dumps(row), flush=True)
        del xd
    if not args.no_stage:
        res["stage"] = _stage(torch, args.rounds)
        print(json.dumps(res["stage"]), flush=True)
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "spectral_diagnostics.json"), "w") as f:
        json.dump(res, f, indent=1)
    span = lambda v: f"{statistics.median(v):.3f} ({min(v):.3f} .. {max(v):.3f})"
    lines = [f"Device {res['device']}; host legs on {res['host_cpus']} logical CPUs, no thread count set.", "",
             "| C x T | Welch GPU ms | bytes read once / time (of 6.3 TB/s) | mlab.psd per channel ms | scipy.signal.welch(axis=1) ms | "
             "moments GPU ms | bytes / time | NumPy segment loop ms |", "|---|---|---|---|---|---|---|---|"]
    for r in res["rows"]:
        lines.append(f"| {r['C']} x {r['T']} | {span(r['welch_all_ms'])} | {r['welch_TBps_of_bytes_read_once']:.2f} TB/s "
                     f"({r['welch_TBps_of_bytes_read_once'] / HBM_ACHIEVABLE_TBPS:.0%}) | {r['mlab_per_channel_ms']:.0f} | "
                     f"{r['scipy_welch_ms']:.0f} | {span(r['moments_all_ms'])} | {r['moments_TBps_of_bytes_read_once']:.2f} TB/s | "
                     f"{r['numpy_segment_loop_ms']:.1f} |")
    if "stage" in res:
        s = res["stage"]
        lines += ["", f"Stage (256-channel block, resident, no figures), wall ms, median of {args.rounds}: without `diagnostics` "
                      f"{span(s['off_ms'])}, with {span(s['on_ms'])}; {len(s['files'])} files, {s['bytes']} bytes."]
    print("\n".join(lines))


if __name__ == "__main__":
    main()
