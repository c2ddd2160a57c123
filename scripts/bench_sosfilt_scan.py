#!/usr/bin/env python3
"""Causal Butterworth filter (``butter_filter(causal=True)``): the sequential kernel (tl_sosfilt_f64, the default) against the
time-parallel block scan (tl_sosfilt_scan_f64, TONAL_KERNELS=butter=scan).

Protocol: one process, one resident float32 recording per size; the two routes ALTERNATE call by call, each call timed with HIP
events, the median of 5 after a warm-up call of each route.  Every timed call runs under a watchdog of its own: a call that
does not finish within --limit seconds ends the process with status 124 after the results so far are written.  Sizes 256 x
24 000 (the C5 size) and 256 x 240 000; 256 x 2.4 M with both routes only if the sequential time extrapolated from the 240 000
run stays under a minute, otherwise the scan alone (said so in the table).  Designs: band-pass order 4, 70 - 150 Hz at 400 Hz
(4 sections) and low-pass order 16 (8 sections).

Per size and design: the two medians, their ratio, the spread (max - min of the 5) of the sequential leg, and the scan's bytes
per second - against the roof (one read of x, one write of y: 12 B per sample) and counting what the form really moves (the
time-major fp64 work image written once, read twice, rewritten once and read back: 40 B per sample more, plus the block states).

    python scripts/bench_sosfilt_scan.py --out profiles        # writes sosfilt_scan.json / sosfilt_scan.md
"""
import argparse
import json
import os
import statistics
import sys
import threading

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DESIGNS = [("band-pass 4, 70-150 Hz", dict(freqs=[70.0, 150.0], order=4, filter_type="bandpass"), 4),
           ("low-pass 16, 60 Hz", dict(freqs=60.0, order=16, filter_type="lowpass"), 8)]
FS = 400.0
C = 256
REPS = 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles")
    ap.add_argument("--limit", type=float, default=120.0, help="seconds a single timed call may take")
    ap.add_argument("--sizes", type=int, nargs="*", default=[24000, 240000, 2400000])
    args = ap.parse_args()
    import torch
    from decode_tonal_langauge_amd.preprocess.signal import frequency_filter as ff
    if not torch.cuda.is_available():
        raise SystemExit("bench_sosfilt_scan: no GPU visible; nothing is measured without one")
    dev = torch.device("cuda:0")
    results = {"protocol": "alternating routes in one process, HIP events per call, median of 5 after a warm-up of each route; "
                           "float32 recording resident on the device", "device": torch.cuda.get_device_name(0), "rows": []}
    os.makedirs(args.out, exist_ok=True)

    def dump():
        with open(os.path.join(args.out, "sosfilt_scan.json"), "w") as f:
            json.dump(results, f, indent=1)
        with open(os.path.join(args.out, "sosfilt_scan.md"), "w") as f:
            f.write(markdown(results))

    def timed(fn):
        """HIP-event milliseconds of one call, under its own time limit"""
        def expired():
            results["aborted"] = f"a timed call exceeded {args.limit} s"
            dump()
            os._exit(124)
        dog = threading.Timer(args.limit, expired)
        dog.daemon = True
        dog.start()
        try:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1), out
        finally:
            dog.cancel()

    def route(x, kw, scan):
        os.environ["TONAL_KERNELS"] = "butter=scan" if scan else ""
        try:
            return ff.butter_filter(x, kw["freqs"], FS, order=kw["order"], causal=True, filter_type=kw["filter_type"])
        finally:
            os.environ.pop("TONAL_KERNELS", None)

    seq_ms_at = {}
    for T in args.sizes:
        x = torch.randn(C, T, device=dev, dtype=torch.float32, generator=torch.Generator(device=dev).manual_seed(T))
        for name, kw, nsec in DESIGNS:
            with_seq = True
            if T > 240000:
                base = seq_ms_at.get((name, 240000))
                with_seq = base is not None and base * (T / 240000.0) < 60e3
            seq, scan = [], []
            ms, y_scan = timed(lambda: route(x, kw, True))                  # warm-up (matrices, code objects, allocator)
            y_seq = None
            if with_seq:
                ms, y_seq = timed(lambda: route(x, kw, False))
            for _ in range(REPS):
                if with_seq:
                    seq.append(timed(lambda: route(x, kw, False))[0])
                scan.append(timed(lambda: route(x, kw, True))[0])
            L = ff._SCAN_L
            while (T + L - 1) // L > 65535:
                L *= 2
            nb = (T + L - 1) // L
            roof_bytes = C * T * (4 + 8)
            moved_bytes = C * T * (4 + 8 + 5 * 8) + 4 * nb * 2 * nsec * C * 8     # states: written, read, written, read
            scan_med = statistics.median(scan)
            row = {"C": C, "T": T, "design": name, "sections": nsec, "block": L, "scan_ms": scan_med, "scan_all_ms": scan,
                   "scan_roof_GBps": roof_bytes / scan_med / 1e6, "scan_moved_GBps": moved_bytes / scan_med / 1e6}
            if with_seq:
                seq_med = statistics.median(seq)
                seq_ms_at[(name, T)] = seq_med
                scale = float(y_seq.abs().max())
                row.update({"seq_ms": seq_med, "seq_all_ms": seq, "seq_spread_ms": max(seq) - min(seq), "ratio": seq_med / scan_med,
                            "scan_vs_seq_rel": float((y_scan - y_seq).abs().max()) / scale})
            else:
                row["note"] = "scan alone: the sequential leg, extrapolated from 240 000 samples, would pass a minute"
            results["rows"].append(row)
            print(json.dumps(row), flush=True)
            dump()
            del y_scan, y_seq
        del x
        torch.cuda.empty_cache()
    c5 = [r for r in results["rows"] if r["T"] == 24000 and "seq_ms" in r]
    if c5:
        keep = all(r["seq_ms"] - r["scan_ms"] > r["seq_spread_ms"] for r in c5)
        results["keep"] = bool(keep)
    dump()


def markdown(res):
    out = ["# Time-parallel causal Butterworth filter: `tl_sosfilt_scan_f64` against `tl_sosfilt_f64`", "",
           f"Measured by `scripts/bench_sosfilt_scan.py` on {res['device']}: {res['protocol']}.", "",
           "| C x T | design | sections | sequential ms | spread of its 5 (ms) | scan ms | ratio | scan GB/s of the roof (x in, y out) | "
           "scan GB/s moved (with the work image) | scan vs sequential |", "|---|---|---|---|---|---|---|---|---|---|"]
    for r in res["rows"]:
        if "seq_ms" in r:
            out.append(f"| {r['C']} x {r['T']} | {r['design']} | {r['sections']} | {r['seq_ms']:.3f} | {r['seq_spread_ms']:.3f} | "
                       f"{r['scan_ms']:.3f} | {r['ratio']:.1f} x | {r['scan_roof_GBps']:.0f} | {r['scan_moved_GBps']:.0f} | {r['scan_vs_seq_rel']:.1e} |")
        else:
            out.append(f"| {r['C']} x {r['T']} | {r['design']} | {r['sections']} | not measured | - | {r['scan_ms']:.3f} | - | "
                       f"{r['scan_roof_GBps']:.0f} | {r['scan_moved_GBps']:.0f} | - |")
    out.append("")
    for r in res["rows"]:
        if "note" in r:
            out.append(f"* {r['C']} x {r['T']}, {r['design']}: {r['note']}.")
    if "aborted" in res:
        out.append(f"* ABORTED: {res['aborted']}; the rows above are what finished.")
    if "keep" in res:
        out.append("")
        out.append("**Keep condition** (the scan beats the sequential kernel at the C5 size, 256 x 24 000, by more than the spread of the "
                   "sequential leg, for both designs): " + ("**met - the form is kept** (opt-in, `TONAL_KERNELS=butter=scan`)." if res["keep"]
                                                            else "**NOT met - the form should be dropped.**"))
    out.append("")
    return "\n".join(out)


if __name__ == "__main__":
    main()
