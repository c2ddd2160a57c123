#!/usr/bin/env python
"""Whole training epochs of M logistic (or, ``--model shallow``, M shallow) classifiers: ``ClassifierEnsembleTrainer`` (every
step of the group is the launches of one model's step) against M sequential ``ClassifierTrainer(fused=True)`` epochs over
``ResidentLoader``s - what ``training/classifier_pipeline.py`` runs for the M seeds of an experiment with and without
``training.params.ensemble``.

Configuration of ``scripts/bench_resident_loader.py``: logistic 16 x 100, 4 classes, batch 32, 200 steps per epoch (8 000
samples, 0.8 of them train), one split per member (seed m) over ONE device-resident dataset.  M = 1, 4, 16, 64.  Both legs run
in one process on one GPU, alternating, median of ``--rounds`` epochs after one warm-up epoch each; an epoch is bracketed by HIP
events and by the host clock (it ends in the one device-to-host read of its statistics).

    python scripts/bench_classifier_ensemble.py [--model logistic|shallow] [--rounds 5] [--out-dir profiles]

writes ``classifier_ensemble.json`` and ``classifier_ensemble.md`` into the output directory; the shallow leg
(``ShallowNNClassifier`` with ``hidden_dim`` 800 and ReLU on the same input) writes ``classifier_ensemble_shallow.json`` / ``.md``.
The measuring runs in a child process under ``timeout -k 10``."""
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

CONFIG = dict(channels=16, length=100, classes=4, batch=32, samples=8000, lr=0.0005, weight_decay=0.01)
RATIOS = [0.8, 0.2]
MEMBERS = (1, 4, 16, 64)
HIDDEN = 800                      # the shallow leg's hidden_dim
CLASS_NAMES = {"logistic": "LogisticRegressionClassifier", "shallow": "ShallowNNClassifier"}


def _median(v):
    v = sorted(v)
    return v[len(v) // 2]


def _timed(fn):
    """(HIP-event ms, host-clock ms) of ``fn``, which ends in a device synchronise of its own."""
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), (time.perf_counter() - t0) * 1e3


def child(rounds: int, model: str) -> None:
    import torch
    from torch.utils.data import TensorDataset
    from decode_tonal_langauge_amd.data_loading.dataloaders import split_dataset
    from decode_tonal_langauge_amd.data_loading.resident import ResidentDataset
    from decode_tonal_langauge_amd.models.classifier_ensemble_trainer import ClassifierEnsembleTrainer
    from decode_tonal_langauge_amd.models.classifier_trainer import ClassifierTrainer
    from decode_tonal_langauge_amd.models.simple_classifiers import LogisticRegressionClassifier, ShallowNNClassifier
    if not torch.cuda.is_available():
        raise SystemExit("bench_classifier_ensemble: no GPU visible; this script measures on the device only")
    dev = torch.device("cuda:0")
    c = CONFIG
    g = torch.Generator().manual_seed(1)
    x = torch.randn(c["samples"], c["channels"], c["length"], generator=g).to(dev)
    y = torch.randint(0, c["classes"], (c["samples"],), generator=g).float().to(dev)
    rds = ResidentDataset.from_tensor_dataset(TensorDataset(x, y), dev)
    results = []
    for M in MEMBERS:
        loaders = [split_dataset(rds, RATIOS, [True, False], batch_size=c["batch"], seed=m, resident=True)[0] for m in range(M)]
        steps = len(loaders[0])
        torch.manual_seed(0)
        if model == "shallow":
            one = lambda: ShallowNNClassifier(c["channels"] * c["length"], c["classes"], HIDDEN, "ReLU")
        else:
            one = lambda: LogisticRegressionClassifier(c["channels"] * c["length"], c["classes"])
        build = lambda: [one().to(dev) for _ in range(M)]
        singles = [ClassifierTrainer(model, c["lr"], c["weight_decay"], fused=True) for model in build()]
        group = ClassifierEnsembleTrainer(build(), c["lr"], c["weight_decay"])
        members = list(range(M))

        def sequential():
            for trainer, loader in zip(singles, loaders):
                trainer._run_epoch(loader, True)

        def ensemble():
            group._run_epoch(loaders, True, members)
        sequential(), ensemble()                                   # warm-up: every path, every shape
        t = {"sequential": [], "ensemble": []}
        for _ in range(rounds):
            t["sequential"].append(_timed(sequential))
            t["ensemble"].append(_timed(ensemble))
        row = {"members": M, "steps_per_epoch": steps, "rounds": rounds}
        for key, v in t.items():
            ev, wall = [a for a, _ in v], [b for _, b in v]
            row[key] = {"event_ms_median": _median(ev), "event_ms_min": min(ev), "event_ms_max": max(ev),
                        "wall_ms_median": _median(wall), "wall_ms_min": min(wall), "wall_ms_max": max(wall)}
        seq, ens = row["sequential"], row["ensemble"]
        row["ensemble_over_sequential"] = ens["wall_ms_median"] / seq["wall_ms_median"]          # t_ens(M) / (M t_seq)
        row["ensemble_over_sequential_events"] = ens["event_ms_median"] / seq["event_ms_median"]
        row["sequential_spread"] = (seq["wall_ms_max"] - seq["wall_ms_min"]) / seq["wall_ms_median"]
        row["sequential_ms_per_member"] = seq["wall_ms_median"] / M
        row["ensemble_ms_per_member"] = ens["wall_ms_median"] / M
        results.append(row)
        del singles, group
    config = dict(CONFIG, model=model, **({"hidden_dim": HIDDEN} if model == "shallow" else {}))
    print("RESULT " + json.dumps({"config": config, "results": results}))


def report(out: dict) -> list:
    c, res = out["config"], out["results"]
    rounds = res[0]["rounds"]
    name = CLASS_NAMES[c.get("model", "logistic")]
    shape = f"{c['channels']} x {c['length']}" + (f", hidden_dim {c['hidden_dim']}, ReLU" if "hidden_dim" in c else "")
    rows = ["# Classifier ensemble: M seeds in one pass against M sequential fused runs", "",
            "Written by `scripts/bench_classifier_ensemble.py` on one MI355X: whole training epochs of M",
            f"`{name}`s ({shape}, {c['classes']} classes, batch {c['batch']}, "
            f"{res[0]['steps_per_epoch']} steps per epoch, one split per member over one",
            "device-resident dataset) through `ClassifierEnsembleTrainer` and through M sequential `ClassifierTrainer(fused=True)`",
            f"epochs over `ResidentLoader`s, alternating in one process after one warm-up epoch of each, median of {rounds}",
            "(min .. max).  Host clock around an epoch that ends in its one device-to-host read; the HIP-event time of the same",
            "epoch stands beside it.  `ratio` is t_ens(M) / (M t_seq), the sequential leg being the M epochs as run; `spread` is",
            "(max - min) / median of that leg's repeats.", "",
            "| M | sequential epoch ms | ensemble epoch ms | ratio | spread of the sequential leg | sequential ms / member | "
            "ensemble ms / member | ratio by HIP events |", "|---|---|---|---|---|---|---|---|"]
    for r in res:
        s, e = r["sequential"], r["ensemble"]
        rows.append(f"| {r['members']} | {s['wall_ms_median']:.2f} ({s['wall_ms_min']:.2f} .. {s['wall_ms_max']:.2f}) | "
                    f"{e['wall_ms_median']:.2f} ({e['wall_ms_min']:.2f} .. {e['wall_ms_max']:.2f}) | {r['ensemble_over_sequential']:.3f} | "
                    f"{r['sequential_spread']:.3f} | {r['sequential_ms_per_member']:.2f} | {r['ensemble_ms_per_member']:.2f} | "
                    f"{r['ensemble_over_sequential_events']:.3f} |")
    rows.append("")
    by = {r["members"]: r for r in res}
    if 16 in by:
        r = by[16]
        word = ("below 1 by more than the spread: the ensemble delivers" if r["ensemble_over_sequential"] < 1 - r["sequential_spread"]
                else "NOT below 1 by more than the spread: the ensemble has not delivered")
        rows.append(f"- M = 16: t_ens / (16 t_seq) = {r['ensemble_over_sequential']:.3f} with a spread of {r['sequential_spread']:.3f} "
                    f"in the sequential leg - {word}.")
    if 1 in by:
        r = by[1]
        if abs(r["ensemble_over_sequential"] - 1) <= r["sequential_spread"]:
            word = "inside the spread"
        elif r["ensemble_over_sequential"] < 1:
            word = ("BELOW 1 by more than the spread: the same kernels, but the group's epoch loop issues a batch from a plain range "
                    "over one index table where the sequential loader drives a DataLoader object per batch - the epoch is bound by "
                    "the host, and that is the lighter host loop")
        else:
            word = "ABOVE 1 by more than the spread: a group of one is slower than the single engine"
            if "hidden_dim" in c:
                word += (" (its step is one launch longer: the two bias updates are two `tl_nadam_group` launches where the "
                         "single engine's optimiser puts them into one `tl_nadam_multi`; not measured apart)")
        rows.append(f"- M = 1: t_ens / t_seq = {r['ensemble_over_sequential']:.3f} with a spread of {r['sequential_spread']:.3f} - {word}.")
    return rows


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--model", choices=sorted(CLASS_NAMES), default="logistic", help="the members' class")
    ap.add_argument("--rounds", type=int, default=5, help="timed epochs per leg, alternating")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--timeout", type=int, default=240, help="seconds allowed for the measuring process")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        child(args.rounds, args.model)
        return
    r = subprocess.run(["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child", "--rounds",
                        str(args.rounds), "--model", args.model], capture_output=True, text=True)
    if r.returncode != 0:               # a fault, abort or time limit ends the run: nothing more is started on the device
        sys.stderr.write(r.stdout + r.stderr)
        raise SystemExit(f"bench_classifier_ensemble: the measuring process exited with {r.returncode}")
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1]
    out = json.loads(line[len("RESULT "):])
    print(line, flush=True)
    os.makedirs(args.out_dir, exist_ok=True)
    stem = "classifier_ensemble" + ("" if args.model == "logistic" else "_" + args.model)
    with open(os.path.join(args.out_dir, stem + ".json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    with open(os.path.join(args.out_dir, stem + ".md"), "w") as f:
        f.write("\n".join(report(out)) + "\n")


if __name__ == "__main__":
    main()
