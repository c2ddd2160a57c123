#!/usr/bin/env python
"""One train step of ``CNNRNNClassifier``: ``ClassifierTrainer(fused=True)`` (LSTM train / BPTT kernels, the 7-tap conv stack,
tl_pool3_fwd / _bwd, tl_conv1_dgrad, tl_ce_scores_loss, tl_head_bwd, FusedNAdam) against ``fused=False`` (autograd over MIOpen /
rocBLAS, torch.optim.NAdam, the per-batch host reads), same process, same device.

Shapes: 8 x 48 with lstm_dim 48 at batch 16 (launch bound) and 128 x 400 with lstm_dim 800 at batch 64, 4 classes (the tone
decoder's real shape).  Each shape runs in a child process of its own under a timeout; a step is timed by HIP events after
warm-up, the two paths alternating, median of ``--steps``.  After the timed steps the fused engine runs a few more with its
per-launch timers on.  The trunk's algorithmic FLOPs (direct convolution: forward, input gradient and weight gradient of the
two wide stages, forward and weight gradient of the first) over the step time stand against the dense fp32 MFMA peak.

    python scripts/bench_cnnrnn_classifier_train.py [--steps 20] [--warmup 3] [--out-dir profiles] [--fused-only SHAPE ...]
                                                    [--f63-backward]

``--fused-only SHAPE`` times the fused step of that shape alone: at 128 x 400 the first unfused step (stock autograd through
MIOpen's 7-tap convolutions over 8 320 sequences) did not return within 7 minutes on an MI355X, twice; a comparison that runs
into ``--timeout`` is reported as unmeasured in the same way, with the fused figures of a child of its own.

``--f63-backward`` also times, alternating with the default in the same process, a second fused trainer built under
``TONAL_KERNELS conv7=wino63bwd`` (both backward passes of the two wide 7-tap stages on F(6,3)) and reports its per-launch
timers, the MFMA FLOPs those launches issue and the workspace it adds beside the default's.

writes ``cnnrnn_classifier_train.json`` and ``cnnrnn_classifier_train.md`` into the output directory."""
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
    "cnnrnn_8x48_l48_b16": dict(channels=8, length=48, lstm_dim=48, batch=16, classes=4),
    "cnnrnn_128x400_l800_b64": dict(channels=128, length=400, lstm_dim=800, batch=64, classes=4),
}


def trunk_flops(eng, B: int) -> float:
    """Algorithmic FLOPs of the conv stack in one train step (2 per multiply-add of the direct convolution on valid rows)."""
    S = B * eng.C                                                     # (the stack's W = w1 + C sequences per batch element)
    total = 2.0 * 2 * eng.k1 * eng.c1 * (2 * eng.tout1) * S          # stage 1: forward + weight gradient
    for st in eng.stages:
        total += 3.0 * 2 * st.cin * st.cout * st.k * st.tc * S
    return total


def f63_backward_issued_flops(eng, B: int) -> dict:
    """MFMA FLOPs the F(6,3) backward launches of the two wide stages issue in one step: 8 products per hex; the weight gradient
    runs three segments (24 per hex), the input gradient's K loop three (24 per hex) - padded hexes included."""
    nhex = B * eng.C * eng.Tp // 6
    return {f"conv{st.idx}_{p}": 2.0 * 24 * nhex * st.cin * st.cout for st in eng.stages for p in ("wgrad", "dgrad")}


def child(name: str, steps: int, warmup: int, compare: bool, f63_backward: bool = False) -> None:
    import torch
    from decode_tonal_langauge_amd.models.classifier_trainer import ClassifierTrainer
    from decode_tonal_langauge_amd.models.deep_classifiers import CNNRNNClassifier
    if not torch.cuda.is_available():
        raise SystemExit("bench_cnnrnn_classifier_train: no GPU visible; this script measures on the device only")
    shape = SHAPES[name]
    Cn, T, B, N, lstm_dim = shape["channels"], shape["length"], shape["batch"], shape["classes"], shape["lstm_dim"]
    dev = torch.device("cuda:0")

    def build():
        torch.manual_seed(0)
        return CNNRNNClassifier(Cn, T, N, lstm_dim=lstm_dim).to(dev)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, Cn, T, generator=g).to(dev)
    y = torch.randint(0, N, (B,), generator=g).float().to(dev)

    fused = ClassifierTrainer(build(), 0.0005, 0.01, fused=True)
    plain = ClassifierTrainer(build(), 0.0005, 0.01, fused=False) if compare else None
    fused63 = None
    if f63_backward:                                    # (the setting is read where the engine is built)
        keep = os.environ.get("TONAL_KERNELS")
        os.environ["TONAL_KERNELS"] = ",".join(filter(None, [keep, "conv7=wino63bwd"]))
        try:
            fused63 = ClassifierTrainer(build(), 0.0005, 0.01, fused=True)
            assert fused63.engine.conv7_bwd
        finally:
            if keep is None:
                del os.environ["TONAL_KERNELS"]
            else:
                os.environ["TONAL_KERNELS"] = keep
        fused63.model.train()
    cm = torch.zeros(N, N, dtype=torch.long)
    fused.model.train()
    if compare:
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

    paths = (("fused", step_fused), ("unfused", step_plain)) if compare else (("fused", step_fused),)
    if fused63 is not None:
        paths += (("fused_wino63bwd", lambda: fused63.engine.train_batch(x, y)),)
    times = {key: [] for key, _ in paths}
    for i in range(warmup + steps):
        for key, fn in paths:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ms = a.elapsed_time(b)
            print(f"[{name}] step {i} {key}: {ms:.1f} ms", file=sys.stderr, flush=True)     # (a time limit still leaves a record)
            if i >= warmup:
                times[key].append(ms)
    eng = fused.engine
    eng.enable_timers()
    for _ in range(3):
        step_fused()
    stages = {k: {"launches_per_step": n // 3, "mean_ms": ms} for k, (n, ms) in sorted(eng.timer_summary().items())}
    eng.enable_timers(False)
    eng.epoch_stats()
    flops = trunk_flops(eng, B)
    out = {"shape": name, **shape, "steps": steps, "warmup": warmup, "conv7_form": eng.conv7_form, "trunk_gflop": flops / 1e9,
           "stage_timers": stages, "peak_fp32_mfma_tflops": PEAK_FP32_MFMA_TFLOPS}
    if fused63 is not None:
        e63 = fused63.engine
        e63.enable_timers()
        for _ in range(3):
            e63.train_batch(x, y)
        t63 = {k: {"launches_per_step": n // 3, "mean_ms": ms} for k, (n, ms) in sorted(e63.timer_summary().items())}
        e63.enable_timers(False)
        e63.epoch_stats()
        issued = f63_backward_issued_flops(e63, B)
        extra = [e63.Y7, *e63.D7]
        out["f63_backward"] = {
            "stage_timers": t63,
            "issued_gflop": {k: v / 1e9 for k, v in issued.items()},
            "issued_tflops": {k: v / (t63[k]["mean_ms"] * 1e-3) / 1e12 for k, v in issued.items()},
            "frac_of_fp32_mfma_peak": {k: v / (t63[k]["mean_ms"] * 1e-3) / 1e12 / PEAK_FP32_MFMA_TFLOPS for k, v in issued.items()},
            "extra_workspace_gb": sum(t.numel() * 4 for t in extra) / 1e9,
            "wgrad_slab_gb": max(3 * e63._splitk((st.cin // 64) * (st.cout // 64), (B * e63.C * e63.Tp + 35) // 36, 4096)
                                 * 32 * st.cin * st.cout for st in e63.stages) / 1e9,
        }
    for key, ms in times.items():
        ms = sorted(ms)
        med = ms[len(ms) // 2]
        tf = flops / (med * 1e-3) / 1e12
        out[key] = {"median_ms": med, "min_ms": ms[0], "max_ms": ms[-1], "trunk_algorithmic_tflops": tf,
                    "frac_of_fp32_mfma_peak": tf / PEAK_FP32_MFMA_TFLOPS}
    out["speedup_median"] = out["unfused"]["median_ms"] / out["fused"]["median_ms"] if compare else None
    print("RESULT " + json.dumps(out))


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--timeout", type=int, default=900, help="seconds allowed per shape")
    ap.add_argument("--fused-only", action="append", default=[], choices=list(SHAPES), metavar="SHAPE",
                    help="time the fused step of this shape alone (no unfused partner)")
    ap.add_argument("--f63-backward", action="store_true",
                    help="also time a fused trainer built under TONAL_KERNELS conv7=wino63bwd beside the default")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--no-compare", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        child(args.child, args.steps, args.warmup, not args.no_compare, args.f63_backward)
        return

    def run(name, compare):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--steps", str(args.steps), "--warmup", str(args.warmup)]
        cmd += ["--f63-backward"] if args.f63_backward else []
        r = subprocess.run(cmd + ([] if compare else ["--no-compare"]), stdout=subprocess.PIPE, text=True, timeout=args.timeout)
        if r.returncode != 0:           # a fault or abort of one shape ends the run: nothing more is started on the device
            sys.stderr.write(r.stdout)
            raise SystemExit(f"bench_cnnrnn_classifier_train: shape {name} exited with {r.returncode}")
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1]
        print(line)
        return json.loads(line[len("RESULT "):])
    results = []
    for name in SHAPES:
        if name in args.fused_only:
            res = run(name, False)
            res["unfused_note"] = "not run: --fused-only, see the docstring of the script"
        else:
            try:
                res = run(name, True)
            except subprocess.TimeoutExpired:
                # the comparison ran into its limit (the child is killed): nothing more is started on the device
                report(results, args.steps, args.warmup, args.out_dir)
                raise SystemExit(f"bench_cnnrnn_classifier_train: the comparison at {name} did not finish within {args.timeout} s; "
                                 f"re-run with --fused-only {name}")
        results.append(res)
    report(results, args.steps, args.warmup, args.out_dir)


def report(results, steps: int, warmup: int, out_dir: str) -> None:
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "cnnrnn_classifier_train.json"), "w") as f:
        json.dump({"results": results}, f, indent=1, sort_keys=True)
    def sentence(r):
        if r["speedup_median"] is None:
            return (f"At {r['shape']} the fused step takes {r['fused']['median_ms']:.1f} ms; the unfused step is UNMEASURED "
                    f"({r.get('unfused_note', 'not run')}): no claim is made that the fused step is faster there.")
        word = "faster than" if r["speedup_median"] > 1 else "SLOWER than"
        return (f"At {r['shape']} the fused step takes {r['fused']['median_ms']:.1f} ms and the unfused one "
                f"{r['unfused']['median_ms']:.1f} ms: the fused step is {r['speedup_median']:.2f} x the unfused one's speed "
                f"({word} autograd over MIOpen / rocBLAS on the same device).")
    rows = ["# CNNRNNClassifier train step: fused against unfused", ""] + [x for r in results for x in (sentence(r), "")] + [
            "Written by `scripts/bench_cnnrnn_classifier_train.py`: one train step (forward, loss on the sigmoid scores, backward,",
            "NAdam) of `ClassifierTrainer(fused=True)` against `fused=False`, alternating in one process on one MI355X, HIP-event",
            f"times (median of {steps} steps after {warmup} warm-up steps).  `algorithmic TFLOP/s` is the conv stack's algorithmic FLOPs",
            f"of a train step over the WHOLE step time; `algorithmic / peak` is that over the dense fp32 MFMA peak ({PEAK_FP32_MFMA_TFLOPS} TFLOP/s).  The FLOPs",
            "counted are the direct convolution's (the F(6,3) forms issue fewer, so for them the ratio is no share of peak and is left",
            "out where all three passes run on F(6,3): the issued-FLOP table further down is the figure to read); the two LSTMs, whose",
            "steps are latency bound, are not counted, so the ratio is an end-to-end rate - it is not a kernel's share of peak.", "",
            "| shape | path | median ms | min .. max ms | trunk GFLOP (algorithmic) | algorithmic TFLOP/s | algorithmic / peak |",
            "|---|---|---|---|---|---|---|"]
    for r in results:
        for key in ("fused", "unfused") + (("fused_wino63bwd",) if "fused_wino63bwd" in r else ()):
            if key not in r:
                rows.append(f"| {r['shape']} | {key} | UNMEASURED | - | {r['trunk_gflop']:.1f} | - | - |")
                continue
            t = r[key]
            rows.append(f"| {r['shape']} | {key} | {t['median_ms']:.3f} | {t['min_ms']:.3f} .. {t['max_ms']:.3f} | "
                        f"{r['trunk_gflop']:.1f} | {t['trunk_algorithmic_tflops']:.2f} | "
                        + ("- |" if key == "fused_wino63bwd" else f"{t['frac_of_fp32_mfma_peak']:.3f} |"))
    rows.append("")
    for r in results:
        if r["speedup_median"] is None:
            rows.append(f"- {r['shape']}: UNMEASURED against the unfused path ({r.get('unfused_note', 'not run')}).")
            continue
        word = "faster" if r["speedup_median"] > 1 else "SLOWER"
        rows.append(f"- {r['shape']}: the fused step is {r['speedup_median']:.2f} x the unfused one's speed ({word}).")
    for r in results:
        rows += ["", f"Per-launch timers of the fused step at {r['shape']} (HIP events around the launches, mean of 3 steps"
                     f"; 7-tap forward: {r['conv7_form']}; an LSTM sequence is one timer over all its step launches):", "", "| launch | per step | mean ms |", "|---|---|---|"]
        rows += [f"| {k} | {v['launches_per_step']} | {v['mean_ms']:.3f} |" for k, v in r["stage_timers"].items()]
        b = r.get("f63_backward")
        if b is None:
            continue
        d, n = r["stage_timers"], b["stage_timers"]
        rows += ["", f"`TONAL_KERNELS conv7=wino63bwd` at {r['shape']} (same process, alternating steps): step "
                     f"{r['fused_wino63bwd']['median_ms']:.1f} ms against {r['fused']['median_ms']:.1f} ms of the default; it adds "
                     f"{b['extra_workspace_gb']:.2f} GB of workspace (Y = A dz and V0 / V1 of the moved dz, sized for the wider stage). "
                     "The weight gradient's three launches leave split-K slabs (3 x sk x 32 C_in C_out bytes, transient: "
                     f"{b['wgrad_slab_gb']:.2f} GB at the wider stage) that are summed, finished and scattered into the seven taps "
                     "under the `_reduce` tag; the direct form's own slab sum and permute carry no tag, so its column is the launch alone. "
                     "A `_xform` tag is the transforms in front of the launch it names (weight gradient: V0 / V1 of the stage input "
                     "where the forward's are gone, and Y; input gradient: V0 / V1 of dz and the tap pack); issued = the MFMA FLOPs "
                     "of the F(6,3) launches (24 products per hex and pass), over the launch time.", "",
                 "| launch | default (direct, J = 7) ms | wino63bwd ms | its transforms ms | its reductions ms | issued GFLOP | issued TFLOP/s | of peak |",
                 "|---|---|---|---|---|---|---|---|"]
        for k in sorted(b["issued_gflop"]):
            red = f"{n[k + '_reduce']['mean_ms']:.3f}" if k + "_reduce" in n else "-"
            rows.append(f"| {k} | {d[k]['mean_ms']:.3f} | {n[k]['mean_ms']:.3f} | {n[k + '_xform']['mean_ms']:.3f} | {red} | "
                        f"{b['issued_gflop'][k]:.1f} | {b['issued_tflops'][k]:.1f} | {b['frac_of_fp32_mfma_peak'][k]:.3f} |")
        total = sum(v["mean_ms"] for k, v in n.items() if k.startswith(("conv2_", "conv3_")))
        rows += ["", f"All backward tags of the two stages together: {sum(d[k]['mean_ms'] for k in b['issued_gflop']):.1f} ms direct "
                     f"(launches alone), {total:.1f} ms under wino63bwd (launches, transforms and reductions)."]
    with open(os.path.join(out_dir, "cnnrnn_classifier_train.md"), "w") as f:
        f.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    main()
