#!/usr/bin/env python
"""Per-step time of the three classifier train engines with and without the data-parallel exchange.

For each engine at its existing benchmark shape (``scripts/bench_classifier_train.py``, ``bench_cnn_classifier_train.py``,
``bench_cnnrnn_classifier_train.py``) three measurements, each in a child process of its own under a timeout:

  single     no process group: the single-process path, the baseline;
  rehearsal  one rank under ``TONAL_DP_FORCE=1``: the sharded code path with the real collectives (RCCL through the process
             group, or the C-ABI handle with ``--backend tl``) on a group of one - what the exchange costs when nothing has to
             move between devices;
  n2         two ranks on two GPUs, when two are visible; otherwise the profile says "N > 1: UNMEASURED".

A step is timed by HIP events after warm-up (median of ``--steps``); the exchange's share is the HIP-event time between the
start of the bucketed all-reduce and the end of the factor gathers (``engine.exchange_events``) over the step time.  No scaling
figure is derived from a rehearsal: a group of one moves no data.

    python scripts/bench_classifier_dp.py [--steps 10] [--warmup 3] [--backend nccl|tl] [--out-dir profiles]

writes ``classifier_dp.json`` and ``classifier_dp.md`` into the output directory."""
from __future__ import annotations

import argparse
import json
import os
import socket
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CASES = {
    "shallow_128x400_b64": dict(model="shallow", channels=128, length=400, batch=64, classes=4),
    "cnn_128x400_b64": dict(model="cnn", channels=128, length=400, batch=64, classes=4),
    "cnnrnn_128x400_l800_b64": dict(model="cnnrnn", channels=128, length=400, lstm_dim=800, batch=64, classes=4),
}


def child(name: str, steps: int, warmup: int) -> None:
    import torch
    from decode_tonal_langauge_amd import parallel
    from decode_tonal_langauge_amd.models.classifier_trainer import ClassifierTrainer
    from decode_tonal_langauge_amd.models.deep_classifiers import CNNClassifier, CNNRNNClassifier
    from decode_tonal_langauge_amd.models.simple_classifiers import ShallowNNClassifier
    if not torch.cuda.is_available():
        raise SystemExit("bench_classifier_dp: no GPU visible; this script measures on the device only")
    rank, world, local = parallel.init_from_env()
    c = CASES[name]
    Cn, T, B, N = c["channels"], c["length"], c["batch"], c["classes"]
    dev = torch.device(f"cuda:{local}")
    torch.cuda.set_device(dev)
    torch.manual_seed(0)
    if c["model"] == "shallow":
        model = ShallowNNClassifier(Cn * T, N, None, "LeakyReLU")
    elif c["model"] == "cnn":
        model = CNNClassifier(Cn, T, N)
    else:
        model = CNNRNNClassifier(Cn, T, N, lstm_dim=c["lstm_dim"])
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, Cn, T, generator=g).to(dev)
    y = torch.randint(0, N, (B,), generator=g).float().to(dev)
    tr = ClassifierTrainer(model.to(dev), 0.0005, 0.01, fused=True)
    tr.model.train()
    eng = tr.engine
    times, share = [], []
    for i in range(warmup + steps):
        eng.exchange_events = [] if eng.dp else None
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        eng.train_batch(x, y)
        b.record()
        torch.cuda.synchronize()
        if i >= warmup:
            times.append(a.elapsed_time(b))
            share.append(sum(e0.elapsed_time(e1) for e0, e1 in (eng.exchange_events or [])))
    eng.epoch_stats()
    ms = sorted(times)
    out = {"case": name, "rank": rank, "world": world, "dp": bool(eng.dp), "median_ms": ms[len(ms) // 2], "min_ms": ms[0],
           "max_ms": ms[-1], "exchange_ms": sorted(share)[len(share) // 2], "backend": os.environ.get("TONAL_DIST_BACKEND", "")}
    if parallel.tl_active():
        parallel.tl_comm_destroy()
    if world > 1 or eng.dp:
        torch.distributed.destroy_process_group()
    if rank == 0:
        print("RESULT " + json.dumps(out))


def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _launch(name: str, mode: str, args) -> dict:
    base = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "TONAL_DP_FORCE")}
    cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--steps", str(args.steps), "--warmup", str(args.warmup)]
    world = {"single": 1, "rehearsal": 1, "n2": 2}[mode]
    port = str(_free_port())
    procs = []
    for r in range(world):
        env = dict(base)
        if mode != "single":
            env.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=port, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK=str(r),
                       TONAL_DIST_BACKEND=args.backend)
        if mode == "rehearsal":
            env["TONAL_DP_FORCE"] = "1"
        procs.append(subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    outs = []
    for p in procs:
        try:
            outs.append(p.communicate(timeout=args.timeout))
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise SystemExit(f"bench_classifier_dp: {name} / {mode} ran past {args.timeout} s")
    for p, (so, se) in zip(procs, outs):
        if p.returncode != 0:           # a fault or abort ends the run: nothing more is started on the device
            sys.stderr.write(so + se)
            raise SystemExit(f"bench_classifier_dp: {name} / {mode} exited with {p.returncode}")
    line = [l for l in outs[0][0].splitlines() if l.startswith("RESULT ")][-1]
    res = json.loads(line[len("RESULT "):])
    res["mode"] = mode
    print(f"{name} {mode}: {res['median_ms']:.3f} ms, exchange {res['exchange_ms']:.3f} ms")
    return res


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--backend", default="nccl", choices=("nccl", "tl"))
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--timeout", type=int, default=420, help="seconds allowed per measurement")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        child(args.child, args.steps, args.warmup)
        return
    n_gpus = int(subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.device_count())"], capture_output=True,
                                text=True, check=True).stdout.strip() or 0)
    if n_gpus < 1:
        raise SystemExit("bench_classifier_dp: no GPU visible; this script measures on the device only")
    modes = ["single", "rehearsal"] + (["n2"] if n_gpus >= 2 else [])
    results = [_launch(name, mode, args) for name in args.cases.split(",") for mode in modes]
    report(results, args, n_gpus)


def report(results, args, n_gpus: int) -> None:
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "classifier_dp.json"), "w") as f:
        json.dump({"results": results, "gpus_visible": n_gpus, "steps": args.steps, "warmup": args.warmup,
                   "backend": args.backend}, f, indent=1, sort_keys=True)
    rows = ["# Classifier train step under the data-parallel exchange", "",
            "Written by `scripts/bench_classifier_dp.py`: one train step of `ClassifierTrainer(fused=True)` per engine at its",
            f"benchmark shape, HIP-event times, median of {args.steps} steps after {args.warmup} warm-up steps, one child process per",
            f"measurement, {n_gpus} GPU(s) visible, collectives over `{args.backend}`.  `single` is the single-process path (no",
            "process group); `rehearsal` is one rank under `TONAL_DP_FORCE=1` - the sharded code path and the real collectives on a",
            "group of one; `exchange` is the HIP-event time from the start of the bucketed all-reduce to the end of the factor",
            "gathers, and its share of the step.", "",
            "| case | mode | ranks | median ms | min .. max ms | exchange ms | exchange share |", "|---|---|---|---|---|---|---|"]
    for r in results:
        rows.append(f"| {r['case']} | {r['mode']} | {r['world']} | {r['median_ms']:.3f} | {r['min_ms']:.3f} .. {r['max_ms']:.3f} | "
                    f"{r['exchange_ms']:.3f} | {r['exchange_ms'] / r['median_ms']:.4f} |")
    rows.append("")
    by = {(r["case"], r["mode"]): r for r in results}
    for case in dict.fromkeys(r["case"] for r in results):
        s, h = by[case, "single"], by[case, "rehearsal"]
        rows.append(f"- {case}: the rehearsal step takes {h['median_ms'] / s['median_ms']:.3f} x the single-process step "
                    f"({h['median_ms'] - s['median_ms']:+.3f} ms).")
    rows.append("")
    if n_gpus < 2:
        rows.append("N > 1: UNMEASURED (one GPU visible).  A rehearsal moves no data between devices; no scaling figure is claimed.")
    else:
        for case in dict.fromkeys(r["case"] for r in results):
            s, t = by[case, "single"], by[case, "n2"]
            rows.append(f"- {case}, N = 2: {t['median_ms']:.3f} ms per step of the same global batch, "
                        f"{s['median_ms'] / t['median_ms']:.2f} x the single-process step's speed.")
    with open(os.path.join(args.out_dir, "classifier_dp.md"), "w") as f:
        f.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    main()
