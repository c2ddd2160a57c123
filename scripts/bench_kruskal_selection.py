"""Rank-based channel selection, measured: a (480, 256, 600) recording, k = 4 classes, float32 and float64.

Timed with HIP events on the launch stream after warm-up, three repeats of each window: tl_rank_columns alone, the whole
kruskal_oneway (ranks, four tl_group_moments launches on them, tl_kruskal_finalize), and anova_oneway on the same input.
scipy.stats.kruskal(axis=0) runs once on the host clock, the channels cut into 16 parts on 16 threads.  The rank kernel's
traffic is set against the HBM rate and its compare-exchange count against the LDS read rate of ds_read_b32 / ds_read_b64.
The ranks of the first two channels must equal scipy.stats.rankdata and H / p must agree with scipy to 1e-9 (H: absolute below 1); the script
exits non-zero if they do not.  Writes profiles/kruskal_selection.md.  Needs a GPU."""
import argparse
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from scipy import stats

from decode_tonal_langauge_amd.channel_selection import utils as cs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
#: HBM3E of the MI355X: 8.0 TB/s on the data sheet, 6.3 TB/s reached by a streaming copy
HBM_SPEC, HBM_COPY = 8.0e12, 6.3e12
#: LDS reads with every CU streaming: ds_read_b32 128 B / clk / CU, ds_read_b64 256 B / clk / CU at about 2.4 GHz on 256 CUs
LDS_READ_RATE = {4: 75e12, 8: 150e12}
HOST_THREADS = 16
#: what the block sizes and tile budgets that did not ship measured when they were built side by side (same shape, same box,
#: 3 windows of 50 calls; those builds are not in the library, so this is a record, not a measurement of this run)
CHOICE_RECORD = (
    "Block size and tile budget, measured side by side before they were fixed (`tl_rank_columns` ms, float32 / float64, fastest "
    "window; a record of that comparison, not a measurement of this run): 256 threads with tiles of up to 80 KiB 1.09 / 1.78; "
    "1 024 threads, 80 KiB 0.92 / 1.72; 512 threads, 80 KiB 0.86 / 1.30; 256 threads, 40 KiB 0.90 / 1.22; 512 threads, 40 KiB "
    "(shipped) 0.89 / 1.20.  Before that, with 256 threads and 80 KiB: one step of the network per pass over LDS 1.86 / 2.65; up to "
    "three steps per pass in registers 1.27 / 1.99; eight row loads in flight per thread on top 1.09 / 1.78.")


def events(fn, iters, warmup=3, repeats=3):
    """ms per call, one figure per repeat."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / iters)
    return out


def scipy_threads(x, lab, k):
    parts = np.array_split(np.arange(x.shape[1]), HOST_THREADS)

    def one(ch):
        res = stats.kruskal(*[x[lab == v][:, ch] for v in range(k)], axis=0)
        return res.statistic, res.pvalue
    t0 = time.perf_counter()
    with ThreadPoolExecutor(HOST_THREADS) as pool:
        out = list(pool.map(one, parts))
    seconds = time.perf_counter() - t0
    return seconds, np.concatenate([o[0] for o in out]), np.concatenate([o[1] for o in out])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kruskal_selection.md"))
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--shape", type=int, nargs=3, default=[480, 256, 600])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_kruskal_selection: no GPU visible; nothing is measured without one")
    N, Cn, T = args.shape
    k, cols = 4, Cn * T
    rng = np.random.default_rng(0)
    x64 = rng.standard_normal((N, Cn, T))
    lab = rng.integers(0, k, N)
    x64[:, :40, 200:330] += 0.8 * lab[:, None, None]
    rows, ok = [], True
    npad = max(2, 1 << (N - 1).bit_length())
    steps = (npad.bit_length() - 1) * npad.bit_length() // 2
    exchanges = cols * (npad // 2) * steps
    for name, x in (("float32", x64.astype(np.float32)), ("float64", x64)):
        xd = torch.from_numpy(x).cuda()
        is_f64 = name == "float64"
        key = 8 if is_f64 else 4
        tile = cs.rank_tile_columns(N, is_f64)
        rank_ms = events(lambda: cs.rank_columns_device([xd]), args.iters)
        kruskal_ms = events(lambda: cs.kruskal_oneway(xd, lab), args.iters)
        anova_ms = events(lambda: cs.anova_oneway(xd, lab), args.iters)
        ranks = cs.rank_columns_device([xd])[:, :2].cpu().numpy()
        same = bool(np.array_equal(ranks, stats.rankdata(x[:, :2], axis=0).astype(np.float32)))
        H, p = (t.cpu().numpy() for t in cs.kruskal_oneway(xd, lab))
        host_s, Hs, ps = scipy_threads(x, lab, k)
        dev_H = float(np.max(np.abs(H - Hs) / np.maximum(np.abs(Hs), 1.0)))          # scipy's H cancels: absolute below H = 1
        dev_p = float(np.max(np.abs(p - ps)[ps > 1e-290] / ps[ps > 1e-290]))
        ok = ok and same and dev_H < 1e-9 and dev_p < 1e-9
        t_rank = min(rank_ms) * 1e-3
        traffic = N * cols * (x.itemsize + 4)
        rows.append(dict(name=name, tile=tile, lds=npad * tile * (key + 2), rank_ms=rank_ms, kruskal_ms=kruskal_ms,
                         anova_ms=anova_ms, host_s=host_s, same=same, dev_H=dev_H, dev_p=dev_p, traffic=traffic,
                         hbm_rate=traffic / t_rank, exch_rate=exchanges / t_rank,
                         lds_read_share=2 * key * exchanges / t_rank / LDS_READ_RATE[key]))
        print(rows[-1], flush=True)
        del xd
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(render(torch.cuda.get_device_name(0), (N, Cn, T), k, npad, steps, exchanges, args.iters, rows))
    if not ok:
        raise SystemExit("bench_kruskal_selection: the device results differ from scipy")


def render(device, shape, k, npad, steps, exchanges, iters, rows):
    N, Cn, T = shape
    fmt = lambda ms: " / ".join(f"{v:.3f}" for v in ms)
    lines = [
        "# Rank-based channel selection: measurement",
        "",
        f"`scripts/bench_kruskal_selection.py` on {device}: a {N} x {Cn} x {T} recording ({Cn * T} columns), k = {k}.  HIP events on "
        f"the launch stream after 3 warm-up calls, 3 windows of {iters} calls each, ms per call of every window; the host figure is "
        f"one run of `scipy.stats.kruskal(axis=0)` on the host clock with the channels cut into {HOST_THREADS} parts on "
        f"{HOST_THREADS} threads.",
        "",
        "| dtype | tile (columns) | LDS per block | `tl_rank_columns` ms | `kruskal_oneway` ms | `anova_oneway` ms | scipy, host s |",
        "|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['name']} | {r['tile']} | {r['lds'] / 1024:.0f} KiB | {fmt(r['rank_ms'])} | {fmt(r['kruskal_ms'])} | "
                     f"{fmt(r['anova_ms'])} | {r['host_s']:.2f} |")
    lines += ["",
              f"The rank kernel against the machine (fastest window).  Traffic = the recording read once and the float32 ranks written "
              f"once.  The bitonic network on npad = {npad} positions has {steps} steps of {npad // 2} compare-exchanges per column: "
              f"{exchanges:.3e} in all.  Counted as two key reads each, they are set against the streaming rate of `ds_read_b32` "
              f"({LDS_READ_RATE[4] / 1e12:.0f} TB/s) or `ds_read_b64` ({LDS_READ_RATE[8] / 1e12:.0f} TB/s); the kernel runs up to "
              "three steps per pass in registers, so it reads fewer keys than that, and the index words and the stores come on top.",
              "",
              "| dtype | bytes moved | HBM rate | of 6.3 TB/s (copy) | of 8.0 TB/s (data sheet) | compare-exchanges / s | key reads, share of the LDS read rate |",
              "|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['name']} | {r['traffic'] / 1e6:.0f} MB | {r['hbm_rate'] / 1e12:.2f} TB/s | {r['hbm_rate'] / HBM_COPY:.2f} | "
                     f"{r['hbm_rate'] / HBM_SPEC:.2f} | {r['exch_rate']:.3e} | {r['lds_read_share']:.2f} |")
    lines += ["",
              "Checked in the same run: the ranks of the first two channels equal `scipy.stats.rankdata` "
              f"({', '.join(str(r['same']) for r in rows)}); the largest distance of H from `scipy.stats.kruskal` (relative; absolute below H = 1) is "
              f"{', '.join('%.1e' % r['dev_H'] for r in rows)}, of p (over p > 1e-290) {', '.join('%.1e' % r['dev_p'] for r in rows)}."]
    lines += ["", CHOICE_RECORD]
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    main()
