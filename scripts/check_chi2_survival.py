"""The chi-square tail of csrc/tonal_anova.hip (the p-value of tl_kruskal_finalize) against 60-digit arithmetic, on the host (no
GPU needed).

Builds scripts/chi2_survival_host.cpp with hipcc (the routine is __host__ __device__; the host pass uses the host's libm, so this
checks the algorithm, not the device's log / exp / lgamma), feeds it H in [1e-6, 1300] plus fixed values around the switch from
the series to the continued fraction for 1 to 63 degrees of freedom, and prints the largest relative error over p > 1e-290 of
the routine and of scipy.special.chdtrc against mpmath.gammainc.  Needs mpmath."""
import os
import subprocess
import sys
import tempfile

import numpy as np
from scipy import special

try:
    import mpmath
except ImportError:
    raise SystemExit("check_chi2_survival: mpmath is not importable; nothing is checked")

HERE = os.path.dirname(os.path.abspath(__file__))
rng = np.random.default_rng(1)
cases = []
for df in (1, 2, 3, 4, 7, 20, 39, 63):
    for H in list(np.exp(rng.uniform(np.log(1e-6), np.log(1300.0), 80))) + [0.5, 1.0, df + 1.9999, df + 2.0, df + 2.0001, 150.0,
                                                                            400.0, 1000.0]:
        cases.append((float(H), df))

with tempfile.TemporaryDirectory() as tmp:
    exe = os.path.join(tmp, "chi2_survival_host")
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O2", "-std=c++17", "--offload-arch=gfx950",
                           "-Wno-unused-function", os.path.join(HERE, "chi2_survival_host.cpp"), "-o", exe], stderr=subprocess.DEVNULL)
    out = subprocess.run([exe], input="\n".join("%.17g %d" % c for c in cases), capture_output=True, text=True, check=True).stdout
mine = np.array([float(v) for v in out.split()])
scipy_p = np.array([special.chdtrc(df, H) for H, df in cases])
mpmath.mp.dps = 60
exact = np.array([float(mpmath.gammainc(mpmath.mpf(df) / 2, mpmath.mpf(H) / 2, mpmath.inf, regularized=True)) for H, df in cases])
ok = exact > 1e-290
rel = lambda a, b: float(np.max(np.abs(a[ok] - b[ok]) / b[ok]))
print(f"{int(ok.sum())} of {len(cases)} points with p > 1e-290, smallest {exact[ok].min():.3e}")
print(f"chi2_survival (host build) vs 60-digit: {rel(mine, exact):.3e}")
print(f"scipy.special.chdtrc       vs 60-digit: {rel(scipy_p, exact):.3e}")
sys.exit(0 if rel(mine, exact) < 1e-12 else 1)
