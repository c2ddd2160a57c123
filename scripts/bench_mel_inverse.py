"""Mel inverse measurement: one ``mel_to_audio_batch`` call on 2048 trials x 48 frames of dB mels (n_mels 128, n_fft 2048,
hop 512, 32 Griffin-Lim iterations, the default FISTA count) made from one second of a tone plus noise per trial.  HIP events on
the launch stream around the call on device-resident mels (tables cached by the warm-up call): one warm-up, then the median of
three; the kernels timed apart the same way (``tl_mel_invert`` once, one ``tl_gl_synth`` + ``tl_gl_analyse`` iteration,
``tl_gl_overlap_add``) on one workspace chunk; and the host ``mel_to_audio`` over the first few trials on the same box, scaled
to all.  Needs a GPU; prints one JSON line and writes it to --out."""
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


def median_ms(fn, reps=3):
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
    ap.add_argument("--host-trials", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mel_inverse: no GPU visible; nothing is measured without one")
    sr, n_mels, n_fft, hop, n_iter = 24414, 128, 2048, 512, 32
    N, S = args.trials, args.samples
    rng = np.random.default_rng(0)
    t = np.arange(S) / sr
    x = (0.1 * np.sin(2 * np.pi * 220.0 * t)[None, :] * rng.uniform(0.1, 1.0, (N, 1))
         + 1e-3 * rng.standard_normal((N, S))).astype(np.float32)
    mels = au.audio_to_mel_batch(torch.from_numpy(x).cuda(), sr, mel_kwargs={"n_mels": n_mels})       # dB, (N, n_mels * T)
    T = mels.shape[1] // n_mels
    n_bins = n_fft // 2 + 1

    call = lambda: au.mel_to_audio_batch(mels, n_mels, sr, length=S)
    call_ms, call_all = median_ms(call)
    wave = call()
    assert wave.shape == (N, S) and bool(torch.isfinite(wave).all())

    # the kernels apart, on what the call itself uses
    lib, dev = _lib.load(), mels.device
    p = (0.0001 * torch.pow(10.0, 0.1 * mels.double())).reshape(N, n_mels, T).contiguous()
    invert_ms, _ = median_ms(lambda: au.mel_invert_batch(p, sr, n_fft, n_mels))
    mag = au.mel_invert_batch(p, sr, n_fft, n_mels)
    per_trial = T * (8 * n_fft + 8 * n_bins + 2 * 16 * n_bins)
    c = max(1, min(N, 65535, au.GL_WORKSPACE_BYTES // per_trial))
    win, tw = au._stft_batch_tables(str(dev), n_fft, n_fft)
    mag_t = mag[:c].transpose(1, 2).contiguous()
    frames = torch.empty(c, T, n_fft, dtype=torch.float64, device=dev)
    angles = torch.zeros(c, T, n_bins, 2, dtype=torch.float64, device=dev)
    angles[..., 0] = 1.0
    tprev = torch.zeros_like(angles)
    wsum = torch.ones(n_fft + hop * (T - 1), dtype=torch.float64, device=dev)
    out = torch.empty(c, S, dtype=torch.float64, device=dev)
    synth_ms, _ = median_ms(lambda: _lib.check(lib.tl_gl_synth(
        mag_t.data_ptr(), angles.data_ptr(), 0, win.data_ptr(), tw.data_ptr(), frames.data_ptr(), c, n_fft, T,
        _lib.stream_ptr()), "tl_gl_synth"))
    analyse_ms, _ = median_ms(lambda: _lib.check(lib.tl_gl_analyse(
        frames.data_ptr(), wsum.data_ptr(), win.data_ptr(), tw.data_ptr(), angles.data_ptr(), tprev.data_ptr(), c, n_fft, n_fft,
        hop, T, S, 0.99, 0, _lib.stream_ptr()), "tl_gl_analyse"))
    ola_ms, _ = median_ms(lambda: _lib.check(lib.tl_gl_overlap_add(
        frames.data_ptr(), wsum.data_ptr(), out.data_ptr(), c, n_fft, n_fft, hop, T, S, _lib.stream_ptr()), "tl_gl_overlap_add"))

    mels_host = mels.cpu().numpy()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    from_numpy = au.mel_to_audio_batch(mels_host, n_mels, sr, length=S)
    numpy_call_s = time.perf_counter() - t0
    assert from_numpy.shape == (N, S)

    H = min(args.host_trials, N)
    t0 = time.perf_counter()
    for row in mels_host[:H]:
        au.mel_to_audio(row, n_mels, sr, length=S)
    host_s = time.perf_counter() - t0

    chunks = -(-N // c)
    line = {"device": torch.cuda.get_device_name(0), "trials": N, "frames_per_trial": T, "n_fft": n_fft, "hop": hop,
            "n_mels": n_mels, "nnls_iter": au.NNLS_ITER_DEFAULT, "griffinlim_iter": n_iter,
            "call_ms_median_of_3": round(call_ms, 3), "call_ms_all": [round(v, 3) for v in call_all],
            "tl_mel_invert_ms_all_trials": round(invert_ms, 3), "trials_per_chunk": c, "chunks": chunks,
            "tl_gl_synth_ms_per_chunk": round(synth_ms, 4), "tl_gl_analyse_ms_per_chunk": round(analyse_ms, 4),
            "tl_gl_overlap_add_ms_per_chunk": round(ola_ms, 4),
            "griffinlim_ms_estimate_all_trials": round(N / c * ((n_iter + 1) * synth_ms + n_iter * analyse_ms + ola_ms), 3),
            "frames_per_s_tl_mel_invert": round(N * T / (invert_ms * 1e-3)),
            "call_from_numpy_s": round(numpy_call_s, 4),
            "host_trials": H, "host_s": round(host_s, 3), "host_s_scaled_to_all": round(host_s * N / H, 1),
            "host_threads": int(os.environ.get("OMP_NUM_THREADS", os.cpu_count())),
            "speedup_resident_vs_host": round(host_s * N / H / (call_ms * 1e-3), 1),
            "speedup_from_numpy_vs_host": round(host_s * N / H / numpy_call_s, 1)}
    print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(line, f, indent=1)
            f.write("\n")
