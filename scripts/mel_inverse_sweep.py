"""CPU measurements behind the mel-inverse defaults and test bounds (profiles/mel_inverse.md); no GPU involved.

1. Iteration sweep: per-frame relative residual ``||fb x - p|| / ||p||`` of ``mel_to_linear`` at several iteration counts
   against ``scipy.optimize.nnls`` - on one trial of 24 414 samples at n_mels 128 / n_fft 2048 and n_mels 80 / n_fft 1024,
   true mels and mels times 3 dB Gaussian noise, and on the small cases of the tests.
2. Spread of ``mel_to_linear`` when every iteration's gradient is perturbed by 1e-15 relative, on the test cases.
3. Spread of ``griffinlim`` when every iteration's resynthesised signal is perturbed by 1e-15 relative, on the test cases.
Prints markdown tables."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from scipy.optimize import nnls

from decode_tonal_langauge_amd.utils import audio as au
from tests import mel_inverse_cases as mc

COUNTS = (100, 200, 300, 400, 500, 600, 700, 800, 900, 1000, 1200)


def fista(p, fb, counts, rel_noise=0.0, seed=0):
    """``mel_to_linear`` at each of ``counts`` (the iterates do not depend on the count) with an optional relative
    perturbation of each gradient."""
    rng = np.random.default_rng(seed)
    perturb = (lambda g: g * (1.0 + rel_noise * rng.standard_normal(g.shape))) if rel_noise else None
    if len(counts) == 1:
        return {counts[0]: au.mel_to_linear(p, fb, counts[0], _perturb=perturb)}
    return {k: au.mel_to_linear(p, fb, k) for k in counts}


def griffinlim_perturbed(mag, n_iter, rel_noise, seed, **kw):
    """``au.griffinlim`` with the resynthesised signal of every iteration times (1 + rel_noise * gaussian)."""
    noise = np.random.default_rng(seed)
    angles = np.exp(2j * np.pi * np.random.default_rng(0).random(mag.shape))
    n_fft, length = 2 * (mag.shape[0] - 1), kw.pop("length", None)
    tprev = None
    for _ in range(n_iter):
        inverse = au.istft(mag * angles, length=length, **kw)
        if rel_noise:
            inverse = inverse * (1.0 + rel_noise * noise.standard_normal(inverse.shape))
        rebuilt = au.stft(inverse, n_fft=n_fft, **kw)
        rebuilt = rebuilt[:, :mag.shape[1]] if rebuilt.shape[1] >= mag.shape[1] else \
            np.pad(rebuilt, ((0, 0), (0, mag.shape[1] - rebuilt.shape[1])))
        angles = rebuilt - (0.99 / 1.99) * tprev if tprev is not None else rebuilt.copy()
        angles /= np.abs(angles) + 1e-16
        tprev = rebuilt
    return au.istft(mag * angles, length=length, **kw)


def sweep_row(label, fb, p, every=1):
    frames = np.arange(0, p.shape[1], every)
    ref = np.array([np.linalg.norm(fb @ nnls(fb, p[:, t])[0] - p[:, t]) / np.linalg.norm(p[:, t]) for t in frames])
    xs = fista(p, fb, COUNTS)
    cells = []
    for k in COUNTS:
        excess = mc.relative_residual(fb, xs[k], p)[frames] - ref
        cells.append(f"{excess.max():.1e}")
    print(f"| {label} | {p.shape[1]} | {ref.max():.1e} | " + " | ".join(cells) + " |", flush=True)


if __name__ == "__main__":
    print("### Iteration sweep: worst per-frame excess of the relative residual over scipy.optimize.nnls\n")
    print("| input | frames | scipy worst residual | " + " | ".join(str(k) for k in COUNTS) + " |")
    print("|---|---|---|" + "---|" * len(COUNTS))
    x = np.array(mc.signals(1, 24414))[0]
    for n_mels, n_fft in ((128, 2048), (80, 1024)):
        kw = dict(n_mels=n_mels, n_fft=n_fft)
        fb = mc.bank(kw)
        p = au.audio_to_mel(x, mc.SR, mel_in_db=False, mel_kwargs=kw).reshape(n_mels, -1).astype(np.float64)
        sweep_row(f"true, n_mels {n_mels}, n_fft {n_fft}", fb, p)
        noisy = p * np.power(10.0, 0.3 * np.random.default_rng(1).standard_normal(p.shape))
        sweep_row(f"3 dB noise, n_mels {n_mels}, n_fft {n_fft}", fb, noisy)
    for name, (N, S, kw, _) in mc.CASES.items():
        fb = mc.bank(kw)
        for noisy in (False, True):
            p = np.concatenate(list(mc.mel_power(name, noisy)), axis=1)
            sweep_row(f"{name}{', 3 dB noise' if noisy else ''}", fb, p)

    print("\n### mel_to_linear under a 1e-15 relative perturbation of every gradient\n")
    print("| case | max abs change / max x of the trial, worst of 3 seeds and both inputs |")
    print("|---|---|")
    worst_all = 0.0
    for name, (N, S, kw, _) in mc.CASES.items():
        fb, worst = mc.bank(kw), 0.0
        for noisy in (False, True):
            for p in mc.mel_power(name, noisy):
                base = fista(p, fb, (au.NNLS_ITER_DEFAULT,))[au.NNLS_ITER_DEFAULT]
                for seed in (1, 2, 3):
                    got = fista(p, fb, (au.NNLS_ITER_DEFAULT,), 1e-15, seed)[au.NNLS_ITER_DEFAULT]
                    worst = max(worst, float(np.abs(got - base).max() / base.max()))
        worst_all = max(worst_all, worst)
        print(f"| {name} | {worst:.2e} |", flush=True)
    print(f"\nworst {worst_all:.2e}; 1 000 x = {1000 * worst_all:.2e}")

    print("\n### griffinlim under a 1e-15 relative perturbation of every resynthesised signal\n")
    print("| case | n_iter | max abs change / peak of the row, worst of 3 seeds |")
    print("|---|---|---|")
    for name, (N, S, kw, keep) in mc.CASES.items():
        power = kw.get("power", 2.0)
        gl = {k: kw[k] for k in ("hop_length", "win_length") if k in kw}
        gl["length"] = S if keep else None
        for n_iter in (4, 32):
            worst = 0.0
            for lin in mc.host_linear(name):
                mag = np.power(lin, 1.0 / power)
                base = griffinlim_perturbed(mag, n_iter, 0.0, 0, **gl)
                assert np.array_equal(base, au.griffinlim(mag, n_iter=n_iter, **gl))
                for seed in (1, 2, 3):
                    got = griffinlim_perturbed(mag, n_iter, 1e-15, seed, **gl)
                    worst = max(worst, float(np.abs(got - base).max() / np.abs(base).max()))
            print(f"| {name} | {n_iter} | {worst:.2e} |", flush=True)
