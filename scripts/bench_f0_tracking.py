#!/usr/bin/env python3
"""F0 tracking: ``yin_f0_batch`` (``tl_yin_f0``, utils/audio.py) on the GPU against ``yin_f0`` on the host, on the same box in
the same run, and the observed errors of the kernel against the long-double restatement of tests/yin_ref.py.  Nothing here
is a pass mark.

Size: 2 000 clips x 24 414 samples (one second at the audio rate) of float32, the defaults: frame_length 2048, win_length
1024, hop 512, 60 - 500 Hz, i.e. 48 frames per clip and the lags 0 .. 407.  The clips are harmonic tones (five harmonics,
gliding between two random pitches in 100 - 300 Hz) in noise.

GPU leg: the batch resident on the device, HIP events around one call (allocation of the outputs by the caching allocator
included), median of ``REPS`` after a warm-up call.  Beside the time: the fp64 FMA count N * n_frames * W * (pmax + 1) over
the time, against the fp64 vector peak (78.6 TFLOP/s = 39.3 T FMA/s on paper for an MI355X).  The kernel spends a subtraction
and an FMA per term, so half of that peak is the most this formulation can reach.

Host leg: ``yin_f0`` clip by clip on a pool of 16 threads (NumPy releases the interpreter lock inside its loops),
``time.perf_counter``, over the first ``--host-clips`` clips (default 160), scaled to the batch; the scaling is stated in the
output.

Errors: the four geometries of the tests, both input dtypes, the kernel against ``yin_ref`` in long double.

    python scripts/bench_f0_tracking.py [--out-dir profiles] [--clips 2000] [--host-clips 160]

writes ``f0_tracking.json`` and ``f0_tracking.md`` to the output directory."""
import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SR, S = 24414, 24414
FMIN, FMAX = 60.0, 500.0
REPS = 7
HOST_THREADS = 16
FP64_VECTOR_PEAK_TFMA = 39.3


def _gpu_ms(torch, fn):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def _clips(torch, n, dev):
    g = torch.Generator(device="cpu").manual_seed(0)
    f_a = 100.0 + 200.0 * torch.rand(n, 1, generator=g)
    f_b = 100.0 + 200.0 * torch.rand(n, 1, generator=g)
    noise = 0.01 * torch.randn(n, S, generator=g)
    t = torch.linspace(0.0, 1.0, S).unsqueeze(0)
    phi = 2.0 * np.pi * torch.cumsum((f_a + (f_b - f_a) * t).double(), dim=1) / SR
    x = sum(torch.sin(h * phi) / h for h in range(1, 6)).float() + noise
    return x.to(dev)


def _errors(torch, dev):
    """Observed maxima of the kernel against the long-double restatement on the test geometries."""
    from decode_tonal_langauge_amd.utils import audio
    from tests import yin_ref as yr
    rows = []
    for name, (sr, fl, W, hop, fmin, fmax, Sg) in yr.GEOMETRIES.items():
        pmin, pmax = yr.periods(sr, fl, W, fmin, fmax)
        for dt in ("float32", "float64"):
            ref = yr.reference(name, dt, "longdouble")
            r64 = yr.reference(name, dt, "float64")
            x = torch.from_numpy(yr.clips(sr, Sg).astype(dt)).to(dev)
            got = audio.yin_f0_batch(x, sr, fmin, fmax, fl, W, hop, yr.THRESHOLD, return_cmnd=True)
            c = got.cmnd.cpu().numpy().astype(np.longdouble)
            nz = ref.cmnd != 0
            agree = (got.period_index.cpu().numpy() == ref.period_index)
            f0 = got.f0.cpu().numpy().astype(np.longdouble)
            rms = got.rms.cpu().numpy().astype(np.longdouble)
            live = ref.rms != 0
            rows.append({
                "geometry": name, "input": dt, "frames": int(agree.size), "lags": pmax + 1, "eps_c": yr.eps_c(W, pmax),
                "cmnd_rel_err": float((np.abs(c - ref.cmnd)[nz] / ref.cmnd[nz]).max()),
                "cmnd_rel_err_float64_restatement": float((np.abs(r64.cmnd - ref.cmnd)[nz] / ref.cmnd[nz]).max()),
                "undecidable_frames": int((~ref.decidable).sum()),
                "index_mismatches_on_decidable_frames": int((~agree & ref.decidable).sum()),
                "f0_rel_err_on_agreeing_frames": float((np.abs(f0 - ref.f0) / ref.f0)[agree].max()),
                "f0_rel_err_float64_restatement": float((np.abs(r64.f0 - ref.f0) / ref.f0)[r64.period_index == ref.period_index].max()),
                "rms_rel_err": float((np.abs(rms - ref.rms)[live] / ref.rms[live]).max()),
            })
            print(json.dumps(rows[-1]), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--clips", type=int, default=2000)
    ap.add_argument("--host-clips", type=int, default=160)
    args = ap.parse_args()
    import torch
    from decode_tonal_langauge_amd.utils import audio
    if not torch.cuda.is_available():
        raise SystemExit("bench_f0_tracking: no GPU visible; nothing is measured without one")
    dev = torch.device("cuda:0")
    fl, W, hop, pmin, pmax = audio.yin_geometry(SR, FMIN, FMAX)
    n_frames = audio.yin_n_frames(S, fl, hop, True)
    x = _clips(torch, args.clips, dev)
    gpu = _gpu_ms(torch, lambda: audio.yin_f0_batch(x, SR, FMIN, FMAX))
    gpu_cmnd = _gpu_ms(torch, lambda: audio.yin_f0_batch(x, SR, FMIN, FMAX, return_cmnd=True))
    track = audio.yin_f0_batch(x, SR, FMIN, FMAX)
    fma = args.clips * n_frames * W * (pmax + 1)
    n_host = min(args.host_clips, args.clips)
    host_x = x[:n_host].cpu().numpy()
    audio.yin_f0(host_x[0], SR, FMIN, FMAX)
    t0 = time.perf_counter()
    with ThreadPoolExecutor(HOST_THREADS) as pool:
        host = list(pool.map(lambda row: audio.yin_f0(row, SR, FMIN, FMAX), host_x))
    host_s = time.perf_counter() - t0
    host_idx = np.stack([h.period_index for h in host])
    host_f0 = np.stack([h.f0 for h in host])
    same = track.period_index[:n_host].cpu().numpy() == host_idx
    res = {"device": torch.cuda.get_device_name(0), "host_cpus": os.cpu_count(), "host_threads": HOST_THREADS, "reps": REPS,
           "clips": args.clips, "samples": S, "sr": SR, "frame_length": fl, "win_length": W, "hop": hop, "min_period": pmin,
           "max_period": pmax, "n_frames": n_frames, "fp64_fma": fma, "gpu_ms": statistics.median(gpu), "gpu_all_ms": gpu,
           "gpu_with_cmnd_ms": statistics.median(gpu_cmnd), "gpu_with_cmnd_all_ms": gpu_cmnd,
           "tfma_per_s": fma / statistics.median(gpu) / 1e9,
           "fraction_of_fp64_vector_peak": fma / statistics.median(gpu) / 1e9 / FP64_VECTOR_PEAK_TFMA,
           "host_clips": n_host, "host_s_measured": host_s, "host_s_scaled_to_batch": host_s * args.clips / n_host,
           "frames_with_the_host_index": float(same.mean()),
           "f0_rel_diff_to_host_on_those": float((np.abs(track.f0[:n_host].cpu().numpy() - host_f0) / host_f0)[same].max())}
    print(json.dumps(res), flush=True)
    res["errors"] = _errors(torch, dev)
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "f0_tracking.json"), "w") as f:
        json.dump(res, f, indent=1)
    span = lambda v: f"{statistics.median(v):.3f} ({min(v):.3f} .. {max(v):.3f})"
    lines = [
        "# F0 tracking: `tl_yin_f0` on an MI355X", "",
        f"Written by `scripts/bench_f0_tracking.py`.  Device {res['device']}; host leg on {HOST_THREADS} threads "
        f"({res['host_cpus']} logical CPUs on the box).", "",
        f"{args.clips} clips x {S} samples float32 at {SR} Hz, frame_length {fl}, win_length {W}, hop {hop}, "
        f"{FMIN:.0f} - {FMAX:.0f} Hz: {n_frames} frames per clip, lags 0 .. {pmax}.", "",
        "| | time | |", "|---|---|---|",
        f"| `yin_f0_batch`, HIP events, median (min .. max) of {REPS} after warm-up | {span(gpu)} ms | "
        f"{fma:.3e} fp64 FMA = N n_frames W (pmax + 1): {res['tfma_per_s']:.2f} T FMA/s, "
        f"{res['fraction_of_fp64_vector_peak']:.1%} of the {FP64_VECTOR_PEAK_TFMA} T FMA/s fp64 vector peak (a subtraction "
        "rides with every FMA: 50 % is this formulation's ceiling) |",
        f"| the same with `return_cmnd=True` | {span(gpu_cmnd)} ms | "
        f"{args.clips * n_frames * (pmax - pmin + 1) * 8 / 1e6:.0f} MB more written |",
        f"| `yin_f0` per clip, {HOST_THREADS} host threads | {res['host_s_scaled_to_batch']:.1f} s | measured "
        f"{host_s:.2f} s over the first {n_host} clips, scaled by {args.clips / n_host:.1f} |", "",
        f"Against the host path on those {n_host} clips: {res['frames_with_the_host_index']:.4%} of the frames pick the same "
        f"index; on them f0 differs by at most {res['f0_rel_diff_to_host_on_those']:.1e} relative.", "",
        "## Observed errors against the long-double restatement (tests/yin_ref.py)", "",
        "| geometry | input | frames | lags | CMND rel. error (bound eps_c) | float64 restatement | undecidable frames | index "
        "mismatches on decidable frames | f0 rel. error on agreeing frames | float64 restatement | rms rel. error |",
        "|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in res["errors"]:
        lines.append(f"| {r['geometry']} | {r['input']} | {r['frames']} | {r['lags']} | {r['cmnd_rel_err']:.1e} ({r['eps_c']:.1e}) | "
                     f"{r['cmnd_rel_err_float64_restatement']:.1e} | {r['undecidable_frames']} | "
                     f"{r['index_mismatches_on_decidable_frames']} | {r['f0_rel_err_on_agreeing_frames']:.1e} | "
                     f"{r['f0_rel_err_float64_restatement']:.1e} | {r['rms_rel_err']:.1e} |")
    text = "\n".join(lines) + "\n"
    with open(os.path.join(args.out_dir, "f0_tracking.md"), "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
