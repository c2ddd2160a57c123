"""Mel front-end measurement: one ``audio_to_mel_batch`` call on 2048 trials x 24 414 samples (one second each, float32),
n_mels = 80 and the defaults (n_fft 2048, hop 512, dB).  HIP events on the launch stream around the call on device-resident
audio (tables cached by the warm-up call): one warm-up, then the median of five; the two kernels timed apart the same way;
the call from a NumPy array (upload and download included) by the host clock; and the host loop
(``audio_to_mel`` per trial) over the first 64 trials on the same box, scaled to 2048.  Needs a GPU; prints one JSON line
and writes it to --out."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from decode_tonal_langauge_amd import _lib
from decode_tonal_langauge_amd.utils import audio as au


def median_ms(fn, reps=5):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return statistics.median(times), times


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--trials", type=int, default=2048)
    ap.add_argument("--samples", type=int, default=24414)
    ap.add_argument("--host-trials", type=int, default=64)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mel_frontend: no GPU visible; nothing is measured without one")
    sr, kw = 24414, {"n_mels": 80}
    N, S = args.trials, args.samples
    rng = np.random.default_rng(0)
    t = np.arange(S) / sr
    x = (0.1 * np.sin(2 * np.pi * 220.0 * t)[None, :] * rng.uniform(0.1, 1.0, (N, 1))
         + 1e-3 * rng.standard_normal((N, S))).astype(np.float32)
    xd = torch.from_numpy(x).cuda()

    call_ms, call_all = median_ms(lambda: au.audio_to_mel_batch(xd, sr, mel_kwargs=kw))
    out = au.audio_to_mel_batch(xd, sr, mel_kwargs=kw)
    n_fft, hop, n_mels = 2048, 512, 80
    n_frames = 1 + S // hop
    assert out.shape == (N, n_mels * n_frames)

    # the two kernels apart, on the tables and buffers the call itself would use
    lib = _lib.load()
    win, tw, bands, weights, n_w = au._mel_batch_tables(str(xd.device), float(sr), n_fft, n_fft, n_mels, 0.0, None)
    work = torch.empty(N, n_mels, n_frames, dtype=torch.float64, device=xd.device)
    rowmax = torch.empty(N, dtype=torch.float64, device=xd.device)
    res = torch.empty(N, n_mels * n_frames, dtype=torch.float32, device=xd.device)
    power_ms, _ = median_ms(lambda: _lib.check(lib.tl_mel_power(
        xd.data_ptr(), 0, S, win.data_ptr(), tw.data_ptr(), bands.data_ptr(), weights.data_ptr(), n_w, work.data_ptr(),
        rowmax.data_ptr(), N, S, n_fft, n_fft, hop, 1, 2, n_mels, n_frames, _lib.stream_ptr()), "tl_mel_power"))
    finish_ms, _ = median_ms(lambda: _lib.check(lib.tl_mel_finish(
        work.data_ptr(), rowmax.data_ptr(), res.data_ptr(), N, n_mels, n_frames, 1, _lib.stream_ptr()), "tl_mel_finish"))
    assert torch.equal(res, out)

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    from_numpy = au.audio_to_mel_batch(x, sr, mel_kwargs=kw)
    numpy_call_s = time.perf_counter() - t0

    H = min(args.host_trials, N)
    t0 = time.perf_counter()
    host = np.stack([au.audio_to_mel(row, sr, mel_kwargs=kw) for row in x[:H]])
    host_s = time.perf_counter() - t0
    dev = float(np.abs(from_numpy[:H].astype(np.float64) - host.astype(np.float64)).max())

    frames = N * n_frames
    line = {"device": torch.cuda.get_device_name(0), "trials": N, "samples": S, "n_fft": n_fft, "hop": hop, "n_mels": n_mels,
            "frames": frames, "call_ms_median_of_5": round(call_ms, 4), "call_ms_all": [round(v, 4) for v in call_all],
            "tl_mel_power_ms": round(power_ms, 4), "tl_mel_finish_ms": round(finish_ms, 4),
            "audio_GBps_over_call": round(x.nbytes / (call_ms * 1e-3) / 1e9, 2),
            "frames_per_s_over_call": round(frames / (call_ms * 1e-3)),
            "frames_per_s_tl_mel_power": round(frames / (power_ms * 1e-3)),
            "call_from_numpy_s": round(numpy_call_s, 4),
            "host_loop_trials": H, "host_loop_s": round(host_s, 4), "host_loop_s_scaled_to_all": round(host_s * N / H, 3),
            "host_threads": int(os.environ.get("OMP_NUM_THREADS", os.cpu_count())),
            "speedup_resident_vs_host": round(host_s * N / H / (call_ms * 1e-3), 1),
            "speedup_from_numpy_vs_host": round(host_s * N / H / numpy_call_s, 1),
            "max_abs_dB_deviation_first_host_trials": dev}
    print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(line, f, indent=1)
            f.write("\n")
