"""The p-value routine of csrc/tonal_anova.hip against 60-digit arithmetic, on the host (no GPU needed).

Builds scripts/f_survival_host.cpp with hipcc (the routine is __host__ __device__; the host pass uses the host's libm, so this
checks the algorithm, not the device's log / exp / lgamma), feeds it F in [1e-6, 1e3] plus a few fixed values for
(dfn, dfd) pairs up to (63, 2000), and prints the largest relative error over p > 1e-290 of the routine and of
scipy.special.fdtrc against mpmath.betainc, and of the two against each other.  Needs mpmath."""
import os
import subprocess
import sys
import tempfile

import numpy as np
from scipy import special

try:
    import mpmath
except ImportError:
    raise SystemExit("check_f_survival: mpmath is not importable; nothing is checked")

HERE = os.path.dirname(os.path.abspath(__file__))
rng = np.random.default_rng(1)
cases = []
for dfb, dfw in [(3, 476), (1, 478), (1, 2), (39, 40), (39, 440), (3, 1996), (63, 2000), (1, 8), (2, 5), (63, 64), (10, 10)]:
    for F in list(np.exp(rng.uniform(np.log(1e-6), np.log(1e3), 60))) + [0.5, 1.0, 150.0, 1e3, 1e5]:
        cases.append((float(F), dfb, dfw))

with tempfile.TemporaryDirectory() as tmp:
    exe = os.path.join(tmp, "f_survival_host")
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O2", "-std=c++17", "--offload-arch=gfx950",
                           "-Wno-unused-function", os.path.join(HERE, "f_survival_host.cpp"), "-o", exe], stderr=subprocess.DEVNULL)
    out = subprocess.run([exe], input="\n".join("%.17g %d %d" % c for c in cases), capture_output=True, text=True, check=True).stdout
mine = np.array([float(v) for v in out.split()])
scipy_p = np.array([special.fdtrc(dfb, dfw, F) for F, dfb, dfw in cases])
mpmath.mp.dps = 60
exact = np.array([float(mpmath.betainc(mpmath.mpf(dfw) / 2, mpmath.mpf(dfb) / 2, 0, dfw / (dfw + dfb * mpmath.mpf(F)), regularized=True))
                  for F, dfb, dfw in cases])
ok = exact > 1e-290
rel = lambda a, b: float(np.max(np.abs(a[ok] - b[ok]) / b[ok]))
print(f"{int(ok.sum())} of {len(cases)} points with p > 1e-290, smallest {exact[ok].min():.3e}")
print(f"f_survival (host build) vs 60-digit: {rel(mine, exact):.3e}")
print(f"scipy.special.fdtrc      vs 60-digit: {rel(scipy_p, exact):.3e}")
print(f"f_survival vs scipy.special.fdtrc:    {rel(mine, scipy_p):.3e}")
sys.exit(0 if rel(mine, exact) < 1e-12 else 1)
