#!/usr/bin/env python
"""Whole training epochs of M ``SynthesisLite`` models: ``SynthesisEnsembleTrainer`` (every step of the group is the launches of
one model's step) against M sequential ``SynthesisTrainer`` epochs over ``ResidentLoader``s - what ``train_synthesizer --repeat M``
runs with and without ``--ensemble``.

32 channels x 200 samples, output 80, logistic tone / syllable classifiers on 8 channels each, 1 280 training samples, at batch 8
(160 steps per epoch) and at batch 64 (20 steps), one split per member (seed m) over ONE device-resident dataset.  M = 1, 4, 8,
16.  Both legs run in one process on one GPU with the HIP graph on, alternating, median of ``--rounds`` epochs after one warm-up
epoch each (which captures the graphs); an epoch is bracketed by HIP events and by the host clock (it ends in the one
device-to-host read of its statistics).

    python scripts/bench_synthesis_ensemble.py [--rounds 3] [--out-dir profiles]

writes ``synthesis_ensemble.json`` and ``synthesis_ensemble.md`` into the output directory.  The measuring runs in a child
process under ``timeout -k 10``."""
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

CONFIG = dict(channels=32, length=200, out_dim=80, classifier_channels=8, samples=1600, lr=0.0005)
RATIOS = [0.8, 0.2]
MEMBERS = (1, 4, 8, 16)
BATCHES = (8, 64)
TONE_MAP = {"0": [3, 3, 3, 3, 3], "1": [1, 2, 3, 4, 5], "2": [3, 2, 1, 2, 4], "3": [5, 4, 3, 2, 1]}


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


def child(rounds: int) -> None:
    import torch
    from decode_tonal_langauge_amd.data_loading.dataloaders import split_dataset
    from decode_tonal_langauge_amd.data_loading.resident import ResidentDataset
    from decode_tonal_langauge_amd.models.simple_classifiers import LogisticRegressionClassifier
    from decode_tonal_langauge_amd.models.synthesis_ensemble_trainer import SynthesisEnsembleTrainer
    from decode_tonal_langauge_amd.models.synthesis_models import SynthesisLite
    from decode_tonal_langauge_amd.models.synthesis_trainer import SynthesisTrainer
    if not torch.cuda.is_available():
        raise SystemExit("bench_synthesis_ensemble: no GPU visible; this script measures on the device only")
    dev = torch.device("cuda:0")
    c = CONFIG
    g = torch.Generator().manual_seed(1)
    n, cc, T = c["samples"], c["classifier_channels"], c["length"]
    rds = ResidentDataset([(torch.randn(n, c["channels"], T, generator=g), None), (torch.randn(n, cc, T, generator=g), None),
                           (torch.randn(n, cc, T, generator=g), None), (10 * torch.randn(n, c["out_dim"], generator=g), None)],
                          device=dev)
    torch.manual_seed(2)
    tone, syl = LogisticRegressionClassifier(cc * T, 4).to(dev), LogisticRegressionClassifier(cc * T, 2).to(dev)
    results = []
    for batch in BATCHES:
        for M in MEMBERS:
            loaders = [split_dataset(rds, RATIOS, [True, False], batch_size=batch, seed=m, resident=True)[0] for m in range(M)]
            steps = len(loaders[0])

            def build():
                out = []
                for m in range(M):
                    torch.manual_seed(m)
                    out.append(SynthesisLite(c["out_dim"], c["channels"], T))
                return out
            singles = [SynthesisTrainer(model, tone, syl, TONE_MAP, device=dev, learning_rate=c["lr"], verbose=False)
                       for model in build()]
            group = SynthesisEnsembleTrainer(build(), tone, syl, TONE_MAP, seeds=list(range(M)), device=dev, learning_rate=c["lr"],
                                             verbose=False)

            def sequential():
                for trainer, loader in zip(singles, loaders):
                    trainer.train(loader, 1, verbose=False)

            def ensemble():
                group.train_loaders(loaders, 1)
            sequential(), ensemble()                                   # warm-up: every path, every shape, the graph captures
            t = {"sequential": [], "ensemble": []}
            for _ in range(rounds):
                t["sequential"].append(_timed(sequential))
                t["ensemble"].append(_timed(ensemble))
            graphs = (sum(1 for tr in singles for v in tr._graphs.values() if v["graph"] is not None),
                      sum(1 for v in group._graphs.values() if v["graph"] is not None))
            row = {"batch": batch, "members": M, "steps_per_epoch": steps, "rounds": rounds, "graphs_sequential": graphs[0],
                   "graphs_ensemble": graphs[1]}
            for key, v in t.items():
                ev, wall = [a for a, _ in v], [b for _, b in v]
                row[key] = {"event_ms_median": _median(ev), "event_ms_min": min(ev), "event_ms_max": max(ev),
                            "wall_ms_median": _median(wall), "wall_ms_min": min(wall), "wall_ms_max": max(wall)}
            seq, ens = row["sequential"], row["ensemble"]
            row["ensemble_over_sequential"] = ens["event_ms_median"] / seq["event_ms_median"]         # t_ens(M) / (M t_single)
            row["ensemble_over_sequential_wall"] = ens["wall_ms_median"] / seq["wall_ms_median"]
            row["sequential_spread"] = (seq["event_ms_max"] - seq["event_ms_min"]) / seq["event_ms_median"]
            row["single_step_ms"] = seq["event_ms_median"] / (M * steps)
            row["ensemble_step_ms"] = ens["event_ms_median"] / steps
            results.append(row)
            del singles, group
            torch.cuda.empty_cache()
    print("RESULT " + json.dumps({"config": CONFIG, "results": results}))


def report(out: dict) -> list:
    c, res = out["config"], out["results"]
    rows = ["# Synthesis ensemble: M SynthesisLite repeats in one pass against M sequential runs", "",
            "Written by `scripts/bench_synthesis_ensemble.py` on one MI355X: whole training epochs of M `SynthesisLite`s",
            f"({c['channels']} ch x {c['length']} t, output {c['out_dim']}, logistic classifiers on {c['classifier_channels']} channels, "
            "one split per member over one",
            "device-resident dataset) through `SynthesisEnsembleTrainer` and through M sequential `SynthesisTrainer` epochs over",
            f"`ResidentLoader`s, HIP graph on for both, alternating in one process after one warm-up epoch of each, median of "
            f"{res[0]['rounds']}",
            "(min .. max) by HIP events around the epoch; the host-clock ratio stands beside it.  `ratio` is",
            "t_ens(M) / (M t_single), the sequential leg being the M epochs as run; `spread` is (max - min) / median of that leg.", "",
            "| batch | M | steps | sequential epoch ms | ensemble epoch ms | ratio | spread | single step ms | group step ms | "
            "ratio by host clock |", "|---|---|---|---|---|---|---|---|---|---|"]
    for r in res:
        s, e = r["sequential"], r["ensemble"]
        rows.append(f"| {r['batch']} | {r['members']} | {r['steps_per_epoch']} | {s['event_ms_median']:.2f} ({s['event_ms_min']:.2f} .. "
                    f"{s['event_ms_max']:.2f}) | {e['event_ms_median']:.2f} ({e['event_ms_min']:.2f} .. {e['event_ms_max']:.2f}) | "
                    f"{r['ensemble_over_sequential']:.3f} | {r['sequential_spread']:.3f} | {r['single_step_ms']:.3f} | "
                    f"{r['ensemble_step_ms']:.3f} | {r['ensemble_over_sequential_wall']:.3f} |")
    rows.append("")
    by = {(r["batch"], r["members"]): r for r in res}
    if (8, 8) in by:
        r = by[(8, 8)]
        word = ("below 1 by more than 5 %: the condition for merging is met" if r["ensemble_over_sequential"] < 0.95
                else "NOT below 1 by more than 5 %: the condition for merging is NOT met")
        rows.append(f"- batch 8, M = 8: t_ens / (8 t_single) = {r['ensemble_over_sequential']:.3f} - {word}.")
    for M in MEMBERS:
        if (64, M) in by:
            rows.append(f"- batch 64, M = {M}: t_ens / ({M} t_single) = {by[(64, M)]['ensemble_over_sequential']:.3f} (reported, not "
                        "conditioned on: the conv kernels already launch 256 workgroups per member).")
    return rows


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=3, help="timed epochs per leg, alternating")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--timeout", type=int, default=420, help="seconds allowed for the measuring process")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        child(args.rounds)
        return
    r = subprocess.run(["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child", "--rounds",
                        str(args.rounds)], capture_output=True, text=True)
    if r.returncode != 0:               # a fault, abort or time limit ends the run: nothing more is started on the device
        sys.stderr.write(r.stdout + r.stderr)
        raise SystemExit(f"bench_synthesis_ensemble: the measuring process exited with {r.returncode}")
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1]
    out = json.loads(line[len("RESULT "):])
    print(line, flush=True)
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "synthesis_ensemble.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    with open(os.path.join(args.out_dir, "synthesis_ensemble.md"), "w") as f:
        f.write("\n".join(report(out)) + "\n")


if __name__ == "__main__":
    main()
