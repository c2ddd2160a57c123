#!/usr/bin/env python
"""One train step of the simple classifiers: ``ClassifierTrainer(fused=True)`` (tl_ce_loss, tl_head_bwd, FusedNAdam) against
``fused=False`` (autograd, torch.optim.NAdam, the per-batch host reads), same process, same device.

Shapes: LogisticRegressionClassifier on 16 x 100 at batch 32 (BASELINE config C1) and ShallowNNClassifier on 128 x 400 with
hidden = input_dim // 2 at batch 64 (a 5.2 GB hidden weight).  Each shape runs in a child process of its own under a timeout;
a step is timed by HIP events after warm-up, the two paths alternating.  Next to each time stands the least number of bytes
the path has to move and what that takes at the 6.3 TB/s the project takes as achievable HBM bandwidth.

    python scripts/bench_classifier_train.py [--steps 20] [--warmup 3] [--out-dir profiles]

writes ``classifier_train.json`` and ``classifier_train.md`` into the output directory."""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 6.3e12
SHAPES = {
    "logistic_16x100_b32": dict(model="logistic", channels=16, length=100, batch=32, classes=4),
    "shallow_128x400_b64": dict(model="shallow", channels=128, length=400, batch=64, classes=4),
}


def min_bytes(shape: dict) -> dict:
    """Least HBM traffic of one step, fp32.  Every weight matrix of P values is read by the forward pass (4 P).  fused: the
    low-rank update reads and writes p, m, v (24 P) and no gradient exists.  unfused: the backward pass writes dW (4 P) and
    the optimizer reads g, p, m, v and writes p, m, v (28 P) - were it a single pass.  Activations and biases are counted
    once read, once written where they are produced and consumed (they are noise at these shapes)."""
    K, B, N = shape["channels"] * shape["length"], shape["batch"], shape["classes"]
    if shape["model"] == "logistic":
        weights, acts = K * N, B * K + 3 * B * N
    else:
        H = K // 2
        weights = K * H + H * N
        acts = B * K * 2 + 4 * B * H + 3 * B * N          # x (forward, update), h (written, read twice), dh (written, read)
    return {"fused": 4 * (7 * weights + acts), "unfused": 4 * (9 * weights + acts), "weight_values": weights}


def child(name: str, steps: int, warmup: int) -> None:
    import torch
    import torch.nn as nn
    from decode_tonal_langauge_amd.models.classifier_trainer import ClassifierTrainer
    from decode_tonal_langauge_amd.models.simple_classifiers import LogisticRegressionClassifier, ShallowNNClassifier
    if not torch.cuda.is_available():
        raise SystemExit("bench_classifier_train: no GPU visible; this script measures on the device only")
    shape = SHAPES[name]
    K, B, N = shape["channels"] * shape["length"], shape["batch"], shape["classes"]
    dev = torch.device("cuda:0")

    def build():
        torch.manual_seed(0)
        m = LogisticRegressionClassifier(K, N) if shape["model"] == "logistic" else ShallowNNClassifier(K, N, None, "LeakyReLU")
        return m.to(dev)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, shape["channels"], shape["length"], generator=g).to(dev)
    y = torch.randint(0, N, (B,), generator=g).float().to(dev)

    fused = ClassifierTrainer(build(), 0.0005, 0.01, fused=True)
    plain = ClassifierTrainer(build(), 0.0005, 0.01, fused=False)
    cm = torch.zeros(N, N, dtype=torch.long)

    def step_fused():
        fused.engine.train_batch(x, y)

    def step_plain():                                   # the loop body of ClassifierTrainer._run_epoch, host reads included
        yl = y.long()
        logits = plain.model(x)
        loss = plain.criterion(logits, yl)
        plain.optimizer.zero_grad()
        loss.backward()
        plain.optimizer.step()
        float(loss.detach())
        idx = yl.cpu() * N + logits.detach().argmax(1).cpu()
        cm.add_(torch.bincount(idx, minlength=N * N).reshape(N, N))

    plain.model.train()
    times = {"fused": [], "unfused": []}
    for i in range(warmup + steps):
        for key, fn in (("fused", step_fused), ("unfused", step_plain)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            if i >= warmup:
                times[key].append(a.elapsed_time(b))
    fused.engine.epoch_stats()
    out = {"shape": name, **shape, "steps": steps, "warmup": warmup, "min_bytes": min_bytes(shape)}
    for key, ms in times.items():
        ms = sorted(ms)
        med = ms[len(ms) // 2]
        floor_ms = out["min_bytes"][key] / HBM_BYTES_PER_S * 1e3
        out[key] = {"median_ms": med, "min_ms": ms[0], "max_ms": ms[-1], "hbm_floor_ms": floor_ms, "floor_over_median": floor_ms / med}
    out["speedup_median"] = out["unfused"]["median_ms"] / out["fused"]["median_ms"]
    print("RESULT " + json.dumps(out))


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--timeout", type=int, default=240, help="seconds allowed per shape")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        child(args.child, args.steps, args.warmup)
        return
    results = []
    for name in SHAPES:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--steps", str(args.steps), "--warmup",
                            str(args.warmup)], capture_output=True, text=True, timeout=args.timeout)
        if r.returncode != 0:           # a fault or abort of one shape ends the run: nothing more is started on the device
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit(f"bench_classifier_train: shape {name} exited with {r.returncode}")
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1]
        results.append(json.loads(line[len("RESULT "):]))
        print(line)
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "classifier_train.json"), "w") as f:
        json.dump({"hbm_bytes_per_s": HBM_BYTES_PER_S, "results": results}, f, indent=1, sort_keys=True)
    rows = ["# Classifier train step: fused against unfused", "",
            "Written by `scripts/bench_classifier_train.py`: one train step (forward, loss, backward, NAdam) of",
            "`ClassifierTrainer(fused=True)` against `fused=False`, alternating in one process on one MI355X, HIP-event times",
            f"(median of {args.steps} steps after {args.warmup} warm-up steps).  `floor` is the least traffic of the path over 6.3 TB/s.", "",
            "| shape | path | median ms | min .. max ms | least bytes | floor ms | floor / median |", "|---|---|---|---|---|---|---|"]
    for r in results:
        for key in ("fused", "unfused"):
            t = r[key]
            rows.append(f"| {r['shape']} | {key} | {t['median_ms']:.3f} | {t['min_ms']:.3f} .. {t['max_ms']:.3f} | "
                        f"{r['min_bytes'][key] / 1e6:.1f} MB | {t['hbm_floor_ms']:.4f} | {t['floor_over_median']:.2f} |")
    rows.append("")
    for r in results:
        word = "faster" if r["speedup_median"] > 1 else "SLOWER"
        rows.append(f"- {r['shape']}: the fused step is {r['speedup_median']:.2f} x the unfused one's speed ({word}).")
    rows += ["", "The small shape is launch-bound on both paths (its floor is microseconds); the large one streams the hidden weight",
             "and its two moments.  The unfused path also pays one host read of the loss and two copies for the confusion matrix per",
             "batch; the fused path reads once per epoch."]
    with open(os.path.join(args.out_dir, "classifier_train.md"), "w") as f:
        f.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    main()
