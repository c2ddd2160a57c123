#!/usr/bin/env python
"""Whole epochs through the stock ``DataLoader`` of ``split_dataset`` against the device-resident loader
(``split_dataset(..., resident=True)``: one ``tl_gather_rows`` launch per batch), same process, same device, alternating.

Three configurations, the data placed as the public entry points place it:

  * logistic 16 x 100, batch 32: ``ClassifierTrainer(fused=True)._run_epoch`` (tensors on the device, as
    ``training/classifier_pipeline.py`` prepares them);
  * SynthesisLite 32 x 200, two 8-channel classifier inputs, 80 mel values, batch 64: ``SynthesisTrainer.train``
    (stock: four CPU tensors, three of them host copies ``ecog[:, channels, :]``, as ``train_synthesizer.py`` builds them);
  * SynthesisModelCNN 128 x 400, two 16-channel classifier inputs, 80 mel values, batch 256: the same.

80 mel values per sample, the output width of ``bench.py`` and of the recorded step times: both synthesis engines reduce the
output gradient with ``tl_colsum``, which takes at most 1 024 columns, so a 3 840-value target does not run on them.

An epoch is timed by the host clock around work that ends in a device synchronise (both trainers read their statistics once
per epoch).  Next to the two epochs stands the per-step time with the epoch's batches already built on the device - the
convention of ``bench.py`` - and, for the big model's batch, the gather alone by HIP events with the bytes it moves.

    python scripts/bench_resident_loader.py [--rounds 5] [--out-dir profiles]

writes ``resident_loader.json`` and ``resident_loader.md`` into the output directory.  Each configuration runs in a child
process of its own under a timeout."""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 6.3e12                     # what the project takes as achievable
GATHER_BYTES_PER_S = (5.5e12, 5.8e12)        # whole-row gathers into registers, 1 152 .. 2 304-byte rows
TONE_MAP = {"0": [3, 3, 3, 3, 3], "1": [1, 2, 3, 4, 5], "2": [3, 2, 1, 2, 4], "3": [5, 4, 3, 2, 1]}
# samples: 0.8 of them train, a whole number of batches (no ragged last batch: one shape per epoch)
CONFIGS = {
    "logistic_16x100_b32": dict(kind="classifier", channels=16, length=100, batch=32, samples=8000),
    "lite_32x200_b64": dict(kind="lite", channels=32, clf_channels=8, length=200, mel=80, batch=64, samples=3200),
    "full_128x400_b256": dict(kind="full", channels=128, clf_channels=16, length=400, mel=80, batch=256, samples=1280),
}
RATIOS = [0.8, 0.2]


def _median(v):
    v = sorted(v)
    return v[len(v) // 2]


def _timed(fn) -> float:
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def gather_alone(cfg: dict, dev) -> dict:
    """The gather at the big model's batch, by HIP events.  A launch of some tens of microseconds is shorter than the host
    takes to issue the next one, so LAUNCHES of them are captured into one HIP graph and a replay is timed: the events then
    bracket device work only.  Every launch of a replay reads a different batch of a 2 560-sample dataset (0.66 GB, more
    than twice the Infinity Cache; a replay sweeps it twice), so the rows come from HBM."""
    import torch
    from decode_tonal_langauge_amd.data_loading.resident import ResidentDataset
    LAUNCHES, N = 20, 2560
    B, T, C, Cc, D = cfg["batch"], cfg["length"], cfg["channels"], cfg["clf_channels"], cfg["mel"]
    gen = torch.Generator(device=dev).manual_seed(2)
    ecog = torch.randn(N, C + 2 * Cc, T, device=dev, generator=gen)
    mels = torch.randn(N, D, device=dev, generator=gen)
    non, syl, tone = list(range(C)), list(range(C, C + Cc)), list(range(C + Cc, C + 2 * Cc))
    ds = ResidentDataset([(ecog, non), (ecog, syl), (ecog, tone), (mels, None)])
    order = torch.randperm(N, device=dev, generator=gen)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    batch_bytes = sum(t.numel() * t.element_size() for t in ds.gather(order, 0, B, err))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        keep = [ds.gather(order, (i * B) % N, (i * B) % N + B, err) for i in range(LAUNCHES)]
    ms = []
    for i in range(8):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        graph.replay()
        b.record()
        torch.cuda.synchronize()
        if i >= 2:
            ms.append(a.elapsed_time(b) / LAUNCHES)
    assert int(err.item()) == 0 and len(keep) == LAUNCHES
    med = _median(ms)
    return {"batch_bytes": batch_bytes, "bytes_read_plus_written": 2 * batch_bytes, "launches_per_replay": LAUNCHES,
            "median_ms": med, "min_ms": min(ms), "max_ms": max(ms), "read_plus_write_tb_per_s": 2 * batch_bytes / (med * 1e-3) / 1e12,
            "gathered_tb_per_s": batch_bytes / (med * 1e-3) / 1e12, "row_bytes": T * 4, "rows": B * (C + 2 * Cc),
            "dataset_bytes": ecog.numel() * 4 + mels.numel() * 4}


def child(name: str, rounds: int) -> None:
    import torch
    from torch.utils.data import TensorDataset
    from decode_tonal_langauge_amd.data_loading.dataloaders import split_dataset
    from decode_tonal_langauge_amd.data_loading.resident import ResidentDataset
    if not torch.cuda.is_available():
        raise SystemExit("bench_resident_loader: no GPU visible; this script measures on the device only")
    cfg = CONFIGS[name]
    dev = torch.device("cuda:0")
    B, T, N = cfg["batch"], cfg["length"], cfg["samples"]
    g = torch.Generator().manual_seed(1)
    extra = {}
    if cfg["kind"] == "classifier":
        from decode_tonal_langauge_amd.models.classifier_trainer import ClassifierTrainer
        from decode_tonal_langauge_amd.models.simple_classifiers import LogisticRegressionClassifier
        x = torch.randn(N, cfg["channels"], T, generator=g).to(dev)
        y = torch.randint(0, 4, (N,), generator=g).float().to(dev)
        stock_ds = TensorDataset(x, y)
        resident_ds = ResidentDataset.from_tensor_dataset(stock_ds, dev)
        torch.manual_seed(0)
        trainer = ClassifierTrainer(LogisticRegressionClassifier(cfg["channels"] * T, 4).to(dev), 0.0005, 0.01, fused=True)
        epoch = lambda loader: trainer._run_epoch(loader, True)

        def prebuilt(batches):
            for xb, yb in batches:
                trainer.engine.train_batch(xb, yb)
            trainer.engine.epoch_stats()
    else:
        from decode_tonal_langauge_amd.models.simple_classifiers import LogisticRegressionClassifier
        from decode_tonal_langauge_amd.models.synthesis_models import SynthesisLite, SynthesisModelCNN
        from decode_tonal_langauge_amd.models.synthesis_trainer import SynthesisTrainer
        C, Cc, D = cfg["channels"], cfg["clf_channels"], cfg["mel"]
        ecog = torch.randn(N, C + 2 * Cc, T, generator=g)
        mels = 10 * torch.randn(N, D, generator=g)
        non, syl, tone = list(range(C)), list(range(C, C + Cc)), list(range(C + Cc, C + 2 * Cc))
        stock_ds = TensorDataset(ecog[:, non, :], ecog[:, syl, :], ecog[:, tone, :], mels)      # train_synthesizer.py's dataset
        resident_ds = ResidentDataset([(ecog, non), (ecog, syl), (ecog, tone), (mels, None)], device=dev)
        torch.manual_seed(1234)
        model = (SynthesisLite if cfg["kind"] == "lite" else SynthesisModelCNN)(D, C, T)
        trainer = SynthesisTrainer(model, LogisticRegressionClassifier(Cc * T, 4), LogisticRegressionClassifier(Cc * T, 2),
                                   TONE_MAP, device=dev, verbose=False)
        epoch = lambda loader: trainer.train(loader, 1, verbose=False)

        def prebuilt(batches):
            trainer._stats.zero_()
            for b in batches:
                trainer.train_step(*b)
            trainer._stats.tolist()
    stock = split_dataset(stock_ds, RATIOS, [True, False], batch_size=B, seed=42)[0]
    resident = split_dataset(resident_ds, RATIOS, [True, False], batch_size=B, seed=42, resident=True)[0]
    steps = len(stock)
    assert steps == len(resident) == int(N * RATIOS[0]) // B
    batches = [tuple(t.clone() for t in b) for b in resident]            # an epoch's batches, on the device
    for _ in range(2):                                                     # warm-up: every path, every shape
        epoch(stock), epoch(resident), prebuilt(batches)
    times = {"stock": [], "resident": [], "prebuilt": []}
    for _ in range(rounds):
        times["stock"].append(_timed(lambda: epoch(stock)))
        times["resident"].append(_timed(lambda: epoch(resident)))
        times["prebuilt"].append(_timed(lambda: prebuilt(batches)))
    # the loaders alone: the stock loader on the host (plus the upload a CPU batch needs), the resident one's launches
    def drain_stock():
        for b in stock:
            [t.to(dev, non_blocking=True) for t in b]

    def drain_resident():
        for b in resident:
            pass
    loaders = {"stock": [], "resident": []}
    for _ in range(rounds):
        loaders["stock"].append(_timed(drain_stock))
        loaders["resident"].append(_timed(drain_resident))

    if cfg["kind"] == "full":
        extra["gather"] = gather_alone(cfg, dev)
    out = {"config": name, **cfg, "steps_per_epoch": steps, "rounds": rounds, **extra}
    for key, v in times.items():
        out[key] = {"epoch_ms_median": _median(v), "epoch_ms_min": min(v), "epoch_ms_max": max(v),
                    "step_ms_median": _median(v) / steps}
    for key, v in loaders.items():
        out[key]["loader_alone_ms_per_batch"] = _median(v) / steps
    out["resident_over_stock"] = out["resident"]["epoch_ms_median"] / out["stock"]["epoch_ms_median"]
    out["resident_over_prebuilt"] = out["resident"]["epoch_ms_median"] / out["prebuilt"]["epoch_ms_median"]
    out["stock_over_prebuilt"] = out["stock"]["epoch_ms_median"] / out["prebuilt"]["epoch_ms_median"]
    print("RESULT " + json.dumps(out))


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=5, help="timed epochs per path, alternating")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--timeout", type=int, default=420, help="seconds allowed per configuration")
    ap.add_argument("--only", default=None, choices=list(CONFIGS), help="one configuration")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        child(args.child, args.rounds)
        return
    results = []
    for name in ([args.only] if args.only else CONFIGS):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--rounds", str(args.rounds)],
                           capture_output=True, text=True, timeout=args.timeout)
        if r.returncode != 0:           # a fault or abort of one configuration ends the run: nothing more is started on the device
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit(f"bench_resident_loader: configuration {name} exited with {r.returncode}")
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1]
        results.append(json.loads(line[len("RESULT "):]))
        print(line, flush=True)
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "resident_loader.json"), "w") as f:
        json.dump({"hbm_bytes_per_s": HBM_BYTES_PER_S, "gather_bytes_per_s": GATHER_BYTES_PER_S, "results": results}, f, indent=1,
                  sort_keys=True)
    with open(os.path.join(args.out_dir, "resident_loader.md"), "w") as f:
        f.write("\n".join(report(results, args.rounds)) + "\n")


def report(results, rounds):
    rows = ["# Device-resident loader: whole epochs against the stock DataLoader", "",
            "Written by `scripts/bench_resident_loader.py` on one MI355X: whole training epochs through the stock `DataLoader` of",
            "`split_dataset` (the default, unchanged) and through `split_dataset(..., resident=True)`, alternating in one process",
            f"after two warm-up epochs of each; host clock around an epoch that ends in a device synchronise, median of {rounds}.",
            "`pre-built` is the same epoch over batches that already lie on the device (the convention of `bench.py`).",
            "The synthesis configurations carry 80 mel values per sample, the width of `bench.py` and of the recorded step times: the",
            "engines' `tl_colsum` takes at most 1 024 output columns, so a 3 840-value target does not run on them.", "",
            "| configuration | steps / epoch | stock epoch ms | resident epoch ms | pre-built epoch ms | resident / stock | "
            "stock ms / step | resident ms / step | pre-built ms / step |", "|---|---|---|---|---|---|---|---|---|"]
    for r in results:
        s, d, p = r["stock"], r["resident"], r["prebuilt"]
        rows.append(f"| {r['config']} | {r['steps_per_epoch']} | {s['epoch_ms_median']:.2f} ({s['epoch_ms_min']:.2f} .. {s['epoch_ms_max']:.2f}) | "
                    f"{d['epoch_ms_median']:.2f} ({d['epoch_ms_min']:.2f} .. {d['epoch_ms_max']:.2f}) | "
                    f"{p['epoch_ms_median']:.2f} ({p['epoch_ms_min']:.2f} .. {p['epoch_ms_max']:.2f}) | {r['resident_over_stock']:.3f} | "
                    f"{s['step_ms_median']:.3f} | {d['step_ms_median']:.3f} | {p['step_ms_median']:.3f} |")
    rows += ["", "The loaders alone (an epoch of batches fetched and dropped; the stock loader's batches are sent to the device as the",
             "train step would send them), per batch:", "",
             "| configuration | stock loader ms / batch | resident loader ms / batch |", "|---|---|---|"]
    for r in results:
        rows.append(f"| {r['config']} | {r['stock']['loader_alone_ms_per_batch']:.3f} | {r['resident']['loader_alone_ms_per_batch']:.4f} |")
    rows.append("")
    for r in results:
        word = "not slower" if r["resident_over_stock"] <= 1.0 else "SLOWER"
        gap = r["resident"]["step_ms_median"] - r["prebuilt"]["step_ms_median"]
        rows.append(f"- {r['config']}: the resident epoch takes {r['resident_over_stock']:.3f} of the stock epoch ({word}); against "
                    f"pre-built batches it is {r['resident_over_prebuilt']:.3f} x (stock: {r['stock_over_prebuilt']:.3f} x), "
                    f"{gap * 1e3:.1f} us per step are left.")
    for r in results:
        if "gather" not in r:
            continue
        q = r["gather"]
        lo, hi = GATHER_BYTES_PER_S
        rows += ["", f"## The gather alone ({r['config']})", "",
                 f"One `tl_gather_rows` launch for the batch of {r['batch']}: {q['rows']} rows of {q['row_bytes']} B picked by three channel "
                 f"lists out of a {q['dataset_bytes'] / 1e6:.0f} MB dataset, plus the mel rows; {q['batch_bytes'] / 1e6:.1f} MB gathered, "
                 f"{q['bytes_read_plus_written'] / 1e6:.1f} MB read plus written.  {q['launches_per_replay']} such launches, each on another "
                 "batch, are captured into one HIP graph (one launch is shorter than the host takes to issue the next) and HIP events "
                 f"bracket a replay: median {q['median_ms'] * 1e3:.1f} us per launch ({q['min_ms'] * 1e3:.1f} .. {q['max_ms'] * 1e3:.1f}).", "",
                 f"- bytes read plus written over time: {q['read_plus_write_tb_per_s']:.2f} TB/s, "
                 f"{q['read_plus_write_tb_per_s'] * 1e12 / HBM_BYTES_PER_S:.2f} of the 6.3 TB/s taken as achievable;",
                 f"- bytes gathered over time: {q['gathered_tb_per_s']:.2f} TB/s, {q['gathered_tb_per_s'] * 1e12 / lo:.2f} .. "
                 f"{q['gathered_tb_per_s'] * 1e12 / hi:.2f} of the {lo / 1e12:.1f} .. {hi / 1e12:.1f} TB/s measured for whole-row gathers into "
                 "registers (that figure counts the rows read and stores nothing; this kernel also writes every byte it reads)."]
        if q["gathered_tb_per_s"] * 1e12 < 0.5 * lo:
            rows += ["", "That is below half of the gather figure, and has to be: the kernel moves every byte twice - a gather INTO registers "
                     "only reads - so the rate to compare is bytes read plus written over time, the line above it.  What is missing to "
                     f"6.3 TB/s there ({(q['median_ms'] - q['bytes_read_plus_written'] / HBM_BYTES_PER_S * 1e3) * 1e3:.1f} us of "
                     f"{q['median_ms'] * 1e3:.1f} us per launch) was not profiled; against the train step that consumes the batch it does "
                     "not show (table above)."]
    return rows


if __name__ == "__main__":
    main()
