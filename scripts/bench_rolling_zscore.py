#!/usr/bin/env python3
"""Rolling z-score: the window kernel (tl_rolling_zscore, ``method: window``, the default) against the blocked route
(tl_rolling_zscore_blocked, ``method: blocked``).

Protocol: one process, one resident float32 recording per size; the two routes ALTERNATE call by call, each call timed with HIP
events, the median of 5 after a warm-up call of each route.  Every timed call runs under a watchdog of its own: a call that
does not finish within --limit seconds ends the process with status 124 after the results so far are written.

Sizes: 64 x 120 000 at W = 256 / 4 000 / 10 000 (the sizes DESIGN quotes the window kernel at) plus W = 512 / 1 024 / 2 048 to
find the smallest W at which the blocked route wins; 256 x 48 000 at W = 4 000 (10 s at the example chain's 400 Hz, 120 s of it);
256 x 366 210 at W = 30 517 (10 s at the raw rate), where the window leg runs ONCE after the blocked leg's five (it is expected
to take seconds; no warm-up, no median).

Per row: the two medians, their ratio, the spread (max - min of the 5) of the window leg, the largest distance between the two
routes' outputs, and the bytes the blocked route moves per sample: x read once by rz_tile_moments and up to three times by the
output kernel (tile, two head samples per lane; 4 B each), y written (8 B), a table row written per tile (64 B / 256 samples)
and W / 256 rows read per tile (W / 1024 B per sample).

    python scripts/bench_rolling_zscore.py --out profiles      # writes rolling_zscore_blocked.json / rolling_zscore_blocked.md
"""
import argparse
import json
import os
import statistics
import sys
import threading
from argparse import Namespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

REPS = 5
#: (C, T, W, window leg: "alternate" or "once")
SIZES = [(64, 120000, 256, "alternate"), (64, 120000, 512, "alternate"), (64, 120000, 1024, "alternate"),
         (64, 120000, 2048, "alternate"), (64, 120000, 4000, "alternate"), (64, 120000, 10000, "alternate"),
         (256, 48000, 4000, "alternate"), (256, 366210, 30517, "once")]
NAME = "rolling_zscore_blocked"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles")
    ap.add_argument("--limit", type=float, default=120.0, help="seconds a single timed call may take")
    ap.add_argument("--skip-raw-window-leg", action="store_true", help="do not run the window kernel at the raw-rate size")
    args = ap.parse_args()
    import torch
    from decode_tonal_langauge_amd.preprocess.signal import rolling_zscore
    if not torch.cuda.is_available():
        raise SystemExit("bench_rolling_zscore: no GPU visible; nothing is measured without one")
    dev = torch.device("cuda:0")
    results = {"protocol": "alternating routes in one process, HIP events per call, median of 5 after a warm-up of each route; "
                           "float32 recording resident on the device; times include the allocation of the output (and of the "
                           "blocked route's table) by the caching allocator",
               "device": torch.cuda.get_device_name(0), "rows": []}
    os.makedirs(args.out, exist_ok=True)

    def dump():
        with open(os.path.join(args.out, NAME + ".json"), "w") as f:
            json.dump(results, f, indent=1)
        with open(os.path.join(args.out, NAME + ".md"), "w") as f:
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

    def route(x, W, method):
        return rolling_zscore.run(x, Namespace(window_length=W, signal_freq=1, preserve_nans=True, method=method))

    x, shape = None, None
    for C, T, W, leg in SIZES:
        if shape != (C, T):
            del x
            torch.cuda.empty_cache()
            x = torch.randn(C, T, device=dev, dtype=torch.float32, generator=torch.Generator(device=dev).manual_seed(T)) + 1.5
            shape = (C, T)
        win, blk = [], []
        _, y_blk = timed(lambda: route(x, W, "blocked"))                   # warm-up (code objects, allocator)
        y_win = None
        if leg == "alternate":
            _, y_win = timed(lambda: route(x, W, "window"))
        for _ in range(REPS):
            if leg == "alternate":
                win.append(timed(lambda: route(x, W, "window"))[0])
            blk.append(timed(lambda: route(x, W, "blocked"))[0])
        if leg == "once" and not args.skip_raw_window_leg:
            ms, y_win = timed(lambda: route(x, W, "window"))
            win.append(ms)
        blk_med = statistics.median(blk)
        bytes_per_sample = 4 + 3 * 4 + 8 + 64.0 / 256 + W / 1024.0
        row = {"C": C, "T": T, "W": W, "blocked_ms": blk_med, "blocked_all_ms": blk, "blocked_spread_ms": max(blk) - min(blk),
               "blocked_bytes_per_sample": bytes_per_sample, "blocked_GBps": C * T * bytes_per_sample / blk_med / 1e6,
               "window_leg": leg}
        if win:
            win_med = statistics.median(win)
            ok = ~(torch.isnan(y_win) | torch.isnan(y_blk))
            row.update({"window_ms": win_med, "window_all_ms": win, "window_spread_ms": max(win) - min(win),
                        "ratio": win_med / blk_med, "same_nan_pattern": bool(torch.equal(torch.isnan(y_win), torch.isnan(y_blk))),
                        "routes_rel_of_largest": float((y_win - y_blk)[ok].abs().max() / y_blk[ok].abs().max())})
        results["rows"].append(row)
        print(json.dumps(row), flush=True)
        dump()
        del y_blk, y_win
    sweep = sorted((r for r in results["rows"] if (r["C"], r["T"]) == (64, 120000) and r["window_leg"] == "alternate"),
                   key=lambda r: r["W"])
    wins = [r["window_ms"] - r["blocked_ms"] > r["window_spread_ms"] for r in sweep]
    results["smallest_winning_W"] = next((r["W"] for i, r in enumerate(sweep) if all(wins[i:])), None)
    at4000 = [r for r in results["rows"] if r["W"] == 4000 and "window_ms" in r]
    if at4000:
        results["faster_at_4000"] = bool(all(r["window_ms"] - r["blocked_ms"] > r["window_spread_ms"] for r in at4000))
    dump()


def markdown(res):
    out = ["# Rolling z-score: `tl_rolling_zscore_blocked` (`method: blocked`) against `tl_rolling_zscore` (`method: window`)", "",
           f"Measured by `scripts/bench_rolling_zscore.py` on {res['device']}: {res['protocol']}.", "",
           "| C x T | W | window ms | spread of its 5 (ms) | blocked ms | spread (ms) | ratio | blocked B / sample | blocked GB/s | "
           "routes apart (of the largest z) |", "|---|---|---|---|---|---|---|---|---|---|"]
    for r in res["rows"]:
        head = f"| {r['C']} x {r['T']} | {r['W']} | "
        tail = (f"{r['blocked_ms']:.3f} | {r['blocked_spread_ms']:.3f} | {{}} | {r['blocked_bytes_per_sample']:.1f} | "
                f"{r['blocked_GBps']:.0f} | {{}} |")
        if "window_ms" in r:
            spread = f"{r['window_spread_ms']:.3f}" if r["window_leg"] == "alternate" else "one run"
            out.append(head + f"{r['window_ms']:.3f} | {spread} | " + tail.format(f"{r['ratio']:.1f} x", f"{r['routes_rel_of_largest']:.1e}"))
        else:
            out.append(head + "not measured | - | " + tail.format("-", "-"))
    out.append("")
    if "aborted" in res:
        out.append(f"* ABORTED: {res['aborted']}; the rows above are what finished.")
    if "smallest_winning_W" in res:
        w = res["smallest_winning_W"]
        out.append("* Smallest W of the 64 x 120 000 sweep from which the blocked route is faster by more than the window leg's spread: "
                   + (f"**{w}**." if w is not None else "**none** - the blocked route does not win in this sweep."))
    if "faster_at_4000" in res:
        out.append("* At W = 4 000 the blocked route is " + ("**faster** than the window kernel by more than the window leg's spread."
                   if res["faster_at_4000"] else "**NOT faster** than the window kernel by more than the window leg's spread: it stays "
                   "opt-in on its accuracy alone."))
    out.append("")
    return "\n".join(out)


if __name__ == "__main__":
    main()
