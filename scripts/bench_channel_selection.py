"""Channel-selection measurement: discriminative selection of a (n_samples, 256, 600) float64 recording, k = 4 classes, at
480 samples and at 2 000.  Per case one JSON line with three splits - upload (host clock around the host-to-device copy),
kernels (HIP events on the launch stream after warm-up: the k tl_group_moments launches, tl_anova_finalize,
tl_max_run_below), download plus host logic (host clock) - the tl_group_moments launches timed on their own (at the sample split the package picks and at 1, 2, 4 and 8) with the
bytes they must read over that time against the 6.3 TB/s achievable HBM figure, and scipy.stats.f_oneway per channel
timed on the same box.  Needs a GPU; writes the lines to --out as one JSON document."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from scipy import stats

from decode_tonal_langauge_amd import _lib
from decode_tonal_langauge_amd.channel_selection import utils as cs

HBM_ACHIEVABLE = 6.3e12


def events(fn, iters):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters, out


def case(N, C, T, k, iters):
    rng = np.random.default_rng(0)
    x = rng.standard_normal((N, C, T))
    lab = rng.integers(0, k, N)
    x[:, :40, 200:330] += 0.8 * lab[:, None, None]
    thr, length = 0.05 / T, 100
    index_lists = [np.flatnonzero(lab == v).astype(np.int32) for v in range(k)]

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    xd = torch.from_numpy(x).cuda()
    torch.cuda.synchronize()
    upload_s = time.perf_counter() - t0

    def kernels():
        F, p = cs.anova_device([xd] * k, index_lists)
        return p, cs.max_run_below(p, thr)
    kernels_ms, (p, (count, longest)) = events(kernels, iters)

    # the moment launches alone (index lists and slabs prepared outside the timed window)
    lib, cols = _lib.load(), C * T
    splits = cs._splits(cols, min(len(ix) for ix in index_lists))
    idx = [torch.from_numpy(ix).cuda() for ix in index_lists]

    def moments(sp):
        slabs = torch.empty(2, k, sp, cols, dtype=torch.float64, device=xd.device)

        def launch():
            for g in range(k):
                _lib.check(lib.tl_group_moments(xd.data_ptr(), 1, N, cols, idx[g].data_ptr(), len(index_lists[g]), xd.data_ptr(),
                                                sp, slabs[0, g].data_ptr(), slabs[1, g].data_ptr(), _lib.stream_ptr()),
                           "tl_group_moments")
        return events(launch, iters)[0]
    by_splits = {sp: moments(sp) for sp in (1, 2, 4, 8)}            # the split heuristic against its neighbours
    moments_ms = by_splits[splits] if splits in by_splits else moments(splits)
    moment_bytes = N * cols * 8 + 2 * k * splits * cols * 8 + k * cols * 8          # samples once, slabs out, the shift row per launch

    t0 = time.perf_counter()
    c_h, l_h = count.cpu().numpy(), longest.cpu().numpy()
    selected = [int(ch) for ch in np.flatnonzero((c_h > 0) & (l_h > length))]
    p_h = p.cpu().numpy()
    download_s = time.perf_counter() - t0

    t0 = time.perf_counter()
    p_ref = np.empty((C, T))
    for ch in range(C):
        p_ref[ch] = stats.f_oneway(*[x[ix, ch, :] for ix in index_lists]).pvalue
    ref_sel = [ch for ch in range(C) if (p_ref[ch] < thr).any() and cs.get_max_length(np.where(p_ref[ch] < thr)[0]) > length]
    scipy_s = time.perf_counter() - t0
    assert selected == ref_sel, (selected, ref_sel)
    m = p_ref > 1e-290
    gpu_s = upload_s + kernels_ms / 1e3 + download_s
    return {"shape": [N, C, T], "dtype": "float64", "k": k, "splits": splits,
            "upload_ms": round(upload_s * 1e3, 3), "kernels_ms": round(kernels_ms, 4), "download_and_host_ms": round(download_s * 1e3, 3),
            "group_moments_ms": round(moments_ms, 4),
            "group_moments_ms_by_splits": {str(sp): round(ms, 4) for sp, ms in by_splits.items()}, "group_moments_bytes": moment_bytes,
            "group_moments_TBps": round(moment_bytes / (moments_ms * 1e-3) / 1e12, 3),
            "group_moments_frac_of_6.3TBps": round(moment_bytes / (moments_ms * 1e-3) / HBM_ACHIEVABLE, 3),
            "scipy_loop_s": round(scipy_s, 3), "end_to_end_cold_speedup_vs_scipy": round(scipy_s / gpu_s, 1),
            "resident_speedup_vs_scipy": round(scipy_s / (kernels_ms / 1e3 + download_s), 1),
            "selected_channels": len(selected), "max_rel_p_deviation": float(np.max(np.abs(p_h[m] - p_ref[m]) / p_ref[m]))}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "channel_selection_bench.json"))
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_channel_selection: no GPU visible; nothing is measured without one")
    lines = []
    for N in (480, 2000):
        lines.append(case(N, 256, 600, 4, args.iters))
        print(json.dumps(lines[-1]), flush=True)
    with open(args.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "host_threads": os.cpu_count() if "OMP_NUM_THREADS" not in os.environ
                   else int(os.environ["OMP_NUM_THREADS"]), "cases": lines}, f, indent=1)
        f.write("\n")
