#!/usr/bin/env python
"""Sample collection at the size of one real block: a 256 x 240 000 float32 recording (600 s at 400 Hz), 1 s windows
(L = 400), 480 event windows plus 120 rest windows.

  (a) the two ``tl_extract_windows`` launches (events, rest) by HIP events after warm-up, as bytes read plus written per
      second.  Three recordings and three destinations are used in turn (1.5 GB, several times the Infinity Cache), so that
      the rows come from HBM.
  (b) the same cut by NumPy slicing and ``np.array`` on the host, as the reference collects its windows.
  (c) ``extract_ecog_audio`` from block files, and from a recording that already lies on the device with ``to_host=False``.

    python scripts/bench_sample_collection.py [--rounds 5] [--out-dir profiles]

writes ``sample_collection.json`` and ``sample_collection.md`` into the output directory."""
from __future__ import annotations

import argparse
import json
import os
import platform
import sys
import tempfile
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

C, T, SF, L = 256, 240_000, 400.0, 400
N_EVENTS, N_REST = 480, 120
SOUND_SF = 1200.0
GATHER_ROWS_TB_S = 4.7                        # profiles/resident_loader.md: tl_gather_rows, bytes read plus written


def _median(v):
    v = sorted(v)
    return v[len(v) // 2]


def _span(v):
    return f"{_median(v):.3f} ({min(v):.3f} .. {max(v):.3f})"


def kernel_alone(dev, rounds: int) -> dict:
    import torch
    from decode_tonal_langauge_amd.data_loading.epoching import launch_extract
    gen = torch.Generator(device=dev).manual_seed(1)
    recs = [torch.randn(C, T, device=dev, generator=gen) for _ in range(3)]
    ev = torch.arange(N_EVENTS, dtype=torch.int64, device=dev) * L + N_REST * L
    rs = torch.arange(N_REST, dtype=torch.int64, device=dev) * L
    outs = [(torch.empty(N_EVENTS, C, L, device=dev), torch.empty(N_REST, C, L, device=dev)) for _ in range(3)]
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    moved = 2 * (N_EVENTS + N_REST) * C * L * 4

    def pair(k):
        launch_extract(recs[k % 3], ev, L, outs[k % 3][0], err)
        launch_extract(recs[k % 3], rs, L, outs[k % 3][1], err)

    for k in range(6):
        pair(k)
    torch.cuda.synchronize()
    assert int(err.item()) == 0
    assert torch.equal(outs[0][0][7], recs[0][:, (N_REST + 7) * L:(N_REST + 8) * L])
    REPS, times = 12, []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for k in range(REPS):
            pair(k)
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) / REPS * 1e3)                               # us per pair of launches
    return {"us_per_pair": times, "bytes_moved": moved, "tb_per_s": moved / (_median(times) * 1e-6) / 1e12}


def numpy_cut(rec: np.ndarray, rounds: int) -> dict:
    ev = [(N_REST + k) * L for k in range(N_EVENTS)]
    rs = [k * L for k in range(N_REST)]
    times = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        a = np.array([rec[:, s:s + L] for s in ev])
        b = np.array([rec[:, s:s + L] for s in rs])
        times.append((time.perf_counter() - t0) * 1e3)
    assert a.shape == (N_EVENTS, C, L) and b.shape == (N_REST, C, L)
    return {"ms": times}


def stage(rec: np.ndarray, dev, rounds: int) -> dict:
    import pandas as pd
    import torch
    from decode_tonal_langauge_amd.data_loading.text_align import extract_ecog_audio
    starts = [float(N_REST + k) for k in range(N_EVENTS)]
    table = pd.DataFrame({"start": starts, "end": [s + 1.0 for s in starts], "syllable": ["a", "i"] * (N_EVENTS // 2),
                          "tone": [1 + k % 4 for k in range(N_EVENTS)]})
    sound = np.random.default_rng(2).standard_normal((1, int(T / SF * SOUND_SF))).astype(np.float32)
    kwargs = dict(syllables=["a", "i"], length=1.0, rest_period=(0.0, float(N_REST)))
    out = {"files_ms": [], "load_ms": [], "upload_ms": [], "resident_ms": []}
    with tempfile.TemporaryDirectory() as tmp, warnings.catch_warnings():
        warnings.simplefilter("ignore")
        np.savez(os.path.join(tmp, "B1_ecog.npz"), data=rec, sf=SF)
        np.savez(os.path.join(tmp, "B1_sound.npz"), data=sound, sf=SOUND_SF)
        rec_dev, sound_dev = torch.from_numpy(rec).to(dev), torch.from_numpy(sound).to(dev)
        recordings = {1: {"ecog": (rec_dev, np.array(SF)), "sound": (sound_dev, np.array(SOUND_SF))}}
        sys.stdout, keep = open(os.devnull, "w"), sys.stdout                       # the stage prints its shapes
        try:
            for r in range(rounds + 1):                                            # the first round warms up
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                by_file = extract_ecog_audio({1: table}, tmp, **kwargs)
                t1 = time.perf_counter()
                data = np.load(os.path.join(tmp, "B1_ecog.npz"))["data"]
                t2 = time.perf_counter()
                torch.from_numpy(data).to(dev)
                torch.cuda.synchronize()
                t3 = time.perf_counter()
                res = extract_ecog_audio({1: table}, None, recordings=recordings, to_host=False, **kwargs)
                torch.cuda.synchronize()
                t4 = time.perf_counter()
                if r:
                    for key, v in (("files_ms", t1 - t0), ("load_ms", t2 - t1), ("upload_ms", t3 - t2), ("resident_ms", t4 - t3)):
                        out[key].append(v * 1e3)
        finally:
            sys.stdout.close()
            sys.stdout = keep
        assert np.array_equal(res["ecog"].cpu().numpy(), by_file["ecog"]) and by_file["ecog_rest"].shape == (N_REST, C, L)
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    import torch
    dev = torch.device("cuda:0")
    rec = np.random.default_rng(0).standard_normal((C, T)).astype(np.float32)
    arch = torch.cuda.get_device_properties(0).gcnArchName.split(":")[0]
    name = {"gfx950": "MI355X"}.get(arch, arch)
    res = {"device": f'{name} ({arch}; the runtime names it "{torch.cuda.get_device_name(0)}")', "host": f"{platform.processor() or platform.machine()}, "
           f"{os.cpu_count()} logical CPUs", "shape": [C, T], "L": L, "events": N_EVENTS, "rest": N_REST}
    res["kernel"] = kernel_alone(dev, args.rounds)
    res["numpy"] = numpy_cut(rec, args.rounds)
    res["stage"] = stage(rec, dev, args.rounds)
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "sample_collection.json"), "w") as f:
        json.dump(res, f, indent=1)
    k, n, s = res["kernel"], res["numpy"], res["stage"]
    lines = [
        "# Sample collection: window extraction on the device", "",
        f"Written by `scripts/bench_sample_collection.py` on one {res['device']} (host: {res['host']}): a {C} x {T} float32",
        f"recording (600 s at 400 Hz, {C * T * 4 / 1e6:.0f} MB), windows of L = {L} samples, {N_EVENTS} event windows plus "
        f"{N_REST} rest windows.", f"Median of {args.rounds} rounds (min .. max).  None of these figures is a pass mark.", "",
        "| what | time | note |", "|---|---|---|",
        f"| (a) `tl_extract_windows`, events + rest (two launches) | {_span(k['us_per_pair'])} us | HIP events around 12 pairs "
        f"after warm-up; three recordings and destinations in turn, so the rows come from HBM |",
        f"| (b) NumPy slicing + `np.array` on the host | {_span(n['ms'])} ms | the reference's way of collecting the same windows |",
        f"| (c) `extract_ecog_audio` from block files | {_span(s['files_ms'])} ms | `np.load`, upload, three launches, results "
        f"copied to the host |",
        f"| ... of which `np.load` of the ECoG block alone | {_span(s['load_ms'])} ms | measured separately on the same file |",
        f"| ... and its upload alone | {_span(s['upload_ms'])} ms | pageable host memory to the device |",
        f"| (c) `extract_ecog_audio` from a resident recording, `to_host=False` | {_span(s['resident_ms'])} ms | host planning "
        f"(pandas, 480 rows), three launches, `torch.cat` |", "",
        f"- (a) moves {k['bytes_moved'] / 1e6:.1f} MB read plus written per pair: {k['tb_per_s']:.2f} TB/s, beside the "
        f"{GATHER_ROWS_TB_S} TB/s that `profiles/resident_loader.md` records for `tl_gather_rows` "
        f"({k['tb_per_s'] / GATHER_ROWS_TB_S:.2f} of it).  The kernel copies one 4-byte element per lane per access, eight "
        f"in flight per thread; wider destination stores were not tried.",
        f"- (b) / (a): the host cut takes {_median(n['ms']) * 1e3 / _median(k['us_per_pair']):.0f} times the two launches.",
        f"- (c) from files is bound by the file and the bus, as expected: `np.load` plus the upload are "
        f"{(_median(s['load_ms']) + _median(s['upload_ms'])) / _median(s['files_ms']):.2f} of it.  With the recording resident "
        f"the stage takes {_median(s['resident_ms']):.1f} ms, {_median(s['files_ms']) / _median(s['resident_ms']):.0f} times "
        f"less; what is left there is host planning, not the kernel "
        f"({_median(k['us_per_pair']) / 1e3:.3f} ms).", ""]
    with open(os.path.join(args.out_dir, "sample_collection.md"), "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
