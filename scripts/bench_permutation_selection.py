"""Permutation-test measurement: 1 000 labellings (the observed one and 999 relabellings) of a (480, 256, 600) float64
recording, k = 4 classes, cell level 0.05 / 600.  HIP events on the launch stream after warm-up.

The new path (channel_selection.permutation_runs) is timed whole and split into tl_perm_exceed, tl_perm_runs and the rest
(the tl_group_moments pass, tau, the table upload).  The route the package offered before is timed on the same table: one
anova_device + max_run_below call per labelling at the same cell level.  Both routes must give the same runs; the script
exits non-zero if they do not.  Writes profiles/permutation_selection.json and .md.  Needs a GPU."""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from decode_tonal_langauge_amd import _lib
from decode_tonal_langauge_amd.channel_selection import utils as cs

#: AMD Instinct MI355X data sheet: peak FP64 matrix throughput 78.6 TFLOP/s (the FP64 vector peak is the same figure)
FP64_MATRIX_PEAK = 78.6e12
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

#: what the form that did not ship measured when both were built side by side (same script, same box, same table; the
#: VALU kernel is no longer in the library, so this is a record, not a measurement of this run)
OTHER_FORM = {
    "form": "valu_predicated_adds", "new_path_ms": [97.4, 97.7, 97.9], "mfma_new_path_ms_same_runs": [13.2, 13.5, 13.7],
    "agrees": True,
    "text": "The other form, measured side by side before it was dropped: a VALU kernel (a lane owns a column, 16 relabellings "
            "a pass, labels broadcast from LDS, one predicated `v_add_f64` per group and sample) gave the same `runs` and took "
            "97.4 - 97.9 ms for the whole path in three runs in which the MFMA form took 13.2 - 13.7 ms.  Its k selects and "
            "adds per (relabelling, sample, column) cost more VALU issue slots than the MFMA form spends matrix cycles, so the "
            "MFMA form shipped and the VALU kernel is not in the library."}


def events(fn, iters, warmup=1):
    for _ in range(warmup):
        out = fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "permutation_selection"))
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--rows", type=int, default=1000, help="labellings, the observed one included")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_permutation_selection: no GPU visible; nothing is measured without one")
    N, Cn, T, k, P = 480, 256, 600, 4, args.rows
    cols = Cn * T
    rng = np.random.default_rng(0)
    x = rng.standard_normal((N, Cn, T))
    lab = rng.integers(0, k, N)
    x[:, :40, 200:330] += 0.8 * lab[:, None, None]
    alpha_cell = 0.05 / T
    counts = np.bincount(lab, minlength=k).tolist()
    table = cs.permutation_table(lab, P - 1, seed=0)
    xd = torch.from_numpy(x).cuda()
    lib = _lib.load()

    # ---- the new path, whole
    new_ms, (runs, f_crit, theta) = events(lambda: cs.permutation_runs([xd], table, counts, alpha_cell), args.iters)

    # ---- its two kernels on their own, chunked as the package chunks them
    chunk = max(1, cs._PERM_MASK_BYTES // cols)
    chunk -= chunk % 128 if chunk >= 128 else 0
    chunk = min(chunk, P)
    d = xd.reshape(N, cols)
    shift = d[0].contiguous()
    S = (d - shift).sum(dim=0)
    tau = (theta * (((d - shift) ** 2).sum(dim=0) - S * S / N) + S * S / N).contiguous()
    labels = torch.from_numpy(table.copy()).cuda()
    cnt = (C.c_int32 * k)(*counts)
    mask = torch.empty(chunk, cols, dtype=torch.uint8, device="cuda")
    runs2 = torch.empty(P, Cn, dtype=torch.int32, device="cuda")
    spans = [(p0, min(P, p0 + chunk)) for p0 in range(0, P, chunk)]

    def exceed_only():
        for p0, p1 in spans:
            _lib.check(lib.tl_perm_exceed(xd.data_ptr(), N, None, 0, 1, cols, shift.data_ptr(), labels.data_ptr() + p0 * N, p1 - p0,
                                          cnt, k, tau.data_ptr(), mask.data_ptr(), _lib.stream_ptr()), "tl_perm_exceed")

    def runs_only():
        for p0, p1 in spans:
            _lib.check(lib.tl_perm_runs(mask.data_ptr(), (p1 - p0) * Cn, T, runs2[p0:p1].data_ptr(), _lib.stream_ptr()), "tl_perm_runs")
    exceed_ms, _ = events(exceed_only, args.iters)
    runs_ms, _ = events(runs_only, args.iters)

    # ---- the route there was before: one selection per labelling
    def loop_route():
        out = torch.empty(P, Cn, dtype=torch.int32, device="cuda")
        for r in range(P):
            index_lists = [np.flatnonzero(table[r] == g).astype(np.int32) for g in range(k)]
            _, p = cs.anova_device([xd] * k, index_lists)
            out[r] = cs.max_run_below(p, alpha_cell)[1]
        return out
    t0 = time.perf_counter()
    loop_ms, runs_loop = events(loop_route, 1, warmup=0)
    loop_wall_ms = (time.perf_counter() - t0) * 1e3
    same = bool(torch.equal(runs, runs_loop))
    differing = int((runs != runs_loop).sum())

    useful = 2.0 * P * (k - 1) * N * cols                          # the product the test needs (last group = total - others)
    pb, gr = 64, 4                                                  # relabellings per block, groups per tile at k = 4
    issued = 2.0 * sum(-(-(p1 - p0) // pb) * pb for p0, p1 in spans) * gr * (-(-k // gr)) * (-(-N // cs.PERM_SAMPLE_CHUNK) *
                                                                                            cs.PERM_SAMPLE_CHUNK) * (-(-cols // 64) * 64)
    res = {"device": torch.cuda.get_device_name(0), "shape": [N, Cn, T], "dtype": "float64", "k": k, "labellings": P,
           "cell_level": alpha_cell, "f_crit": f_crit, "theta": theta, "perm_chunk": chunk, "form": "mfma_f64_16x16x4",
           "new_path_ms": round(new_ms, 3), "exceed_ms": round(exceed_ms, 3), "runs_ms": round(runs_ms, 3),
           "rest_ms": round(new_ms - exceed_ms - runs_ms, 3),
           "exceed_useful_TFLOPs": round(useful / (exceed_ms * 1e-3) / 1e12, 2),
           "exceed_issued_TFLOPs": round(issued / (exceed_ms * 1e-3) / 1e12, 2),
           "exceed_issued_frac_of_fp64_matrix_peak": round(issued / (exceed_ms * 1e-3) / FP64_MATRIX_PEAK, 3),
           "fp64_matrix_peak_TFLOPs": FP64_MATRIX_PEAK / 1e12,
           "loop_route_ms_events": round(loop_ms, 2), "loop_route_ms_host_clock": round(loop_wall_ms, 2),
           "loop_over_new": round(loop_ms / new_ms, 1), "routes_agree": same, "runs_differing": differing,
           "observed_runs_max": int(runs[0].max()), "null_max_of_max": int(runs[1:].max()) if P > 1 else 0,
           "other_form": OTHER_FORM}
    print(json.dumps(res), flush=True)
    with open(args.out + ".json", "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    with open(args.out + ".md", "w") as f:
        f.write(render(res))
    if not same:
        raise SystemExit(f"bench_permutation_selection: the two routes differ in {differing} runs")


def render(r):
    N, Cn, T = r["shape"]
    other = r["other_form"]
    lines = [
        "# Permutation test for channel selection: measurement",
        "",
        f"`scripts/bench_permutation_selection.py` on {r['device']}: {r['labellings']} labellings (the observed one and "
        f"{r['labellings'] - 1} relabellings) of a {N} x {Cn} x {T} {r['dtype']} recording, k = {r['k']}, cell level "
        f"{r['cell_level']:.3e} (F_crit {r['f_crit']:.4f}, theta {r['theta']:.5f}); HIP events after warm-up.",
        "",
        "| route | ms |",
        "|---|---|",
        f"| new path, whole (`permutation_runs`, {r['perm_chunk']} labellings per launch) | {r['new_path_ms']} |",
        f"| - `tl_perm_exceed` | {r['exceed_ms']} |",
        f"| - `tl_perm_runs` | {r['runs_ms']} |",
        f"| - the rest (one `tl_group_moments` pass, tau, table upload, allocations) | {r['rest_ms']} |",
        f"| before: `anova_device` + `max_run_below` per labelling, events | {r['loop_route_ms_events']} |",
        f"| before, host clock | {r['loop_route_ms_host_clock']} |",
        "",
        f"The loop takes **{r['loop_over_new']} x** the new path.  Both routes give the same `runs`: "
        f"**{r['routes_agree']}** ({r['runs_differing']} of {r['labellings'] * Cn} entries differ; longest observed run "
        f"{r['observed_runs_max']}, longest run of any relabelling {r['null_max_of_max']}).",
        "",
        f"Float64 rate of `tl_perm_exceed`: {r['exceed_useful_TFLOPs']} TFLOP/s of the product the test needs "
        f"(2 P (k - 1) N C T), {r['exceed_issued_TFLOPs']} TFLOP/s of MFMA work issued (all k groups, padded tiles) = "
        f"{r['exceed_issued_frac_of_fp64_matrix_peak']} of the {r['fp64_matrix_peak_TFLOPs']} TFLOP/s FP64 matrix peak "
        "(AMD Instinct MI355X data sheet).",
        "",
        f"Kernel form shipped: `{r['form']}` (one-hot operand formed in registers from label bytes in LDS, samples staged "
        "32 at a time through LDS, 4 x 4 tiles of 16 x 16 per wave)."]
    if other:
        lines += ["", other.get("text", "")]
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    main()
