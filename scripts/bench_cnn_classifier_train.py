#!/usr/bin/env python
"""One train step of ``CNNClassifier``: ``ClassifierTrainer(fused=True)`` (the conv stack's HIP kernels, tl_ce_scores_loss,
tl_head_bwd, FusedNAdam) against ``fused=False`` (autograd over MIOpen / rocBLAS, torch.optim.NAdam, the per-batch host reads),
same process, same device.

Shapes: 128 x 400 at batch 64 with 4 classes (the syllable decoder's real shape: a 1.2 GB fc1 weight) and 8 x 150 at batch 16.
Each shape runs in a child process of its own under a timeout; a step is timed by HIP events after warm-up, the two paths
alternating, median of ``--steps``.  After the timed steps the fused engine runs a few more with its per-launch timers on.
The trunk's algorithmic FLOPs (direct convolution: forward, input gradient and weight gradient of every stage, no input
gradient for the first) over the step time stand against the dense fp32 MFMA peak.

    python scripts/bench_cnn_classifier_train.py [--steps 20] [--warmup 3] [--out-dir profiles]

writes ``cnn_classifier_train.json`` and ``cnn_classifier_train.md`` into the output directory."""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PEAK_FP32_MFMA_TFLOPS = 157.3          # MI355X, dense fp32 matrix peak (bench.py)
SHAPES = {
    "cnn_8x150_b16": dict(channels=8, length=150, batch=16, classes=4),
    "cnn_128x400_b64": dict(channels=128, length=400, batch=64, classes=4),
}


def trunk_flops(eng, B: int) -> float:
    """Algorithmic FLOPs of the conv stack in one train step (2 per multiply-add of the direct convolution on valid rows)."""
    S = B * eng.C
    total = 2.0 * 2 * eng.k1 * eng.c1 * (2 * eng.tout1) * S          # stage 1: forward + weight gradient
    for st in eng.stages:
        total += 3.0 * 2 * st.cin * st.cout * st.k * st.tc * S
    return total


def child(name: str, steps: int, warmup: int) -> None:
    import torch
    from decode_tonal_langauge_amd.models.classifier_trainer import ClassifierTrainer
    from decode_tonal_langauge_amd.models.deep_classifiers import CNNClassifier
    if not torch.cuda.is_available():
        raise SystemExit("bench_cnn_classifier_train: no GPU visible; this script measures on the device only")
    shape = SHAPES[name]
    Cn, T, B, N = shape["channels"], shape["length"], shape["batch"], shape["classes"]
    dev = torch.device("cuda:0")

    def build():
        torch.manual_seed(0)
        return CNNClassifier(Cn, T, N).to(dev)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, Cn, T, generator=g).to(dev)
    y = torch.randint(0, N, (B,), generator=g).float().to(dev)

    fused = ClassifierTrainer(build(), 0.0005, 0.01, fused=True)
    plain = ClassifierTrainer(build(), 0.0005, 0.01, fused=False)
    cm = torch.zeros(N, N, dtype=torch.long)
    fused.model.train()
    plain.model.train()

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
    eng = fused.engine
    eng.enable_timers()
    for _ in range(3):
        step_fused()
    stages = {k: {"launches_per_step": n // 3, "mean_ms": ms} for k, (n, ms) in sorted(eng.timer_summary().items())}
    eng.enable_timers(False)
    eng.epoch_stats()
    flops = trunk_flops(eng, B)
    out = {"shape": name, **shape, "steps": steps, "warmup": warmup, "wino63": bool(eng.wino63), "trunk_gflop": flops / 1e9,
           "stage_timers": stages, "peak_fp32_mfma_tflops": PEAK_FP32_MFMA_TFLOPS}
    for key, ms in times.items():
        ms = sorted(ms)
        med = ms[len(ms) // 2]
        tf = flops / (med * 1e-3) / 1e12
        out[key] = {"median_ms": med, "min_ms": ms[0], "max_ms": ms[-1], "trunk_algorithmic_tflops": tf,
                    "frac_of_fp32_mfma_peak": tf / PEAK_FP32_MFMA_TFLOPS}
    out["speedup_median"] = out["unfused"]["median_ms"] / out["fused"]["median_ms"]
    print("RESULT " + json.dumps(out))


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--timeout", type=int, default=420, help="seconds allowed per shape")
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
            raise SystemExit(f"bench_cnn_classifier_train: shape {name} exited with {r.returncode}")
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1]
        results.append(json.loads(line[len("RESULT "):]))
        print(line)
    report(results, args.steps, args.warmup, args.out_dir)


def report(results, steps: int, warmup: int, out_dir: str) -> None:
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "cnn_classifier_train.json"), "w") as f:
        json.dump({"results": results}, f, indent=1, sort_keys=True)
    real = results[-1]
    word = "faster than" if real["speedup_median"] > 1 else "SLOWER than"
    rows = ["# CNNClassifier train step: fused against unfused", "",
            f"At {real['shape']} the fused step takes {real['fused']['median_ms']:.1f} ms and the unfused one "
            f"{real['unfused']['median_ms']:.1f} ms: the fused step is {real['speedup_median']:.2f} x the unfused one's speed "
            f"({word} autograd over MIOpen / rocBLAS on the same device).", "",
            "Written by `scripts/bench_cnn_classifier_train.py`: one train step (forward, loss on the sigmoid scores, backward,",
            "NAdam) of `ClassifierTrainer(fused=True)` against `fused=False`, alternating in one process on one MI355X, HIP-event",
            f"times (median of {steps} steps after {warmup} warm-up steps).  `trunk TFLOP/s` is the conv stack's algorithmic FLOPs",
            f"of a train step over the WHOLE step time; `of peak` is that over the dense fp32 MFMA peak ({PEAK_FP32_MFMA_TFLOPS} TFLOP/s).  The FLOPs",
            "counted are the direct convolution's; the Winograd forms issue 0.44 - 0.5 of them, so the ratio is an end-to-end rate and",
            "may exceed 1 - it is not a kernel's share of peak.", "",
            "| shape | path | median ms | min .. max ms | trunk GFLOP | trunk TFLOP/s | of peak |", "|---|---|---|---|---|---|---|"]
    for r in results:
        for key in ("fused", "unfused"):
            t = r[key]
            rows.append(f"| {r['shape']} | {key} | {t['median_ms']:.3f} | {t['min_ms']:.3f} .. {t['max_ms']:.3f} | "
                        f"{r['trunk_gflop']:.1f} | {t['trunk_algorithmic_tflops']:.2f} | {t['frac_of_fp32_mfma_peak']:.3f} |")
    rows.append("")
    for r in results:
        word = "faster" if r["speedup_median"] > 1 else "SLOWER"
        rows.append(f"- {r['shape']}: the fused step is {r['speedup_median']:.2f} x the unfused one's speed ({word}).")
    for r in results:
        rows += ["", f"Per-launch timers of the fused step at {r['shape']} (HIP events around the GEMM launches, mean of 3 steps"
                     f"; F(6,3) stages: {r['wino63']}):", "", "| launch | per step | mean ms |", "|---|---|---|"]
        rows += [f"| {k} | {v['launches_per_step']} | {v['mean_ms']:.3f} |" for k, v in r["stage_timers"].items()]
    with open(os.path.join(out_dir, "cnn_classifier_train.md"), "w") as f:
        f.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    main()
