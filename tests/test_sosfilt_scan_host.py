"""CPU: the host side of the time-parallel causal Butterworth filter (``TONAL_KERNELS=butter=scan`` with ``causal=True``,
tl_sosfilt_scan_f64) - no GPU.

* ``_sos_scan_matrices`` returns the exact rational powers A^(L 2^m) of the cascade's zero-input transition matrix, rounded once;
* the device's block scan restated in NumPy with those matrices (tests/sosfilt_scan_ref.py), against ``scipy.signal.sosfilt``
  and against the same loop in long double: the scan may stand at most 20 x as far from scipy as scipy stands from 64-bit-mantissa
  arithmetic.  THIS TEST CHOSE THE MATRIX FORMAT: with plain fp64 matrices the ratio reaches 18.0 (band-pass 1 - 50 Hz at
  24 414 Hz) and 19.6 (high-pass 0.5 Hz on a DC level of 1000) at 40 000 samples and grows with the length - no margin - so the
  matrices are (hi, lo) pairs and the products compensated; observed then: at most 2.1;
* every refusal of the C entry returns -1 with its message before anything is launched.
"""
from fractions import Fraction

import numpy as np
import pytest
import scipy.signal as sps

from tests import sosfilt_scan_ref as R
from tests.parity_record import record

RATIO_BOUND = 20.0          # set by the issue: three times the worst ratio of its plain-fp64 table (6.6)
L = 128


def _exact_A(sos):
    """the transition matrix by pushing unit states through one zero-input sample of scipy's statements, in rationals"""
    nsec = sos.shape[0]
    ns = 2 * nsec
    A = [[Fraction(0)] * ns for _ in range(ns)]
    for col in range(ns):
        z = [Fraction(int(k == col)) for k in range(ns)]
        v = Fraction(0)
        for q in range(nsec):
            b0, b1, b2, _a0, a1, a2 = (Fraction(float(c)) for c in sos[q])
            yv = b0 * v + z[2 * q]
            z[2 * q] = (b1 * v - a1 * yv) + z[2 * q + 1]
            z[2 * q + 1] = b2 * v - a2 * yv
            v = yv
        for r in range(ns):
            A[r][col] = z[r]
    return A


@pytest.mark.parametrize("order,ftype,freqs,Lb", [(2, "lowpass", 60.0, 8), (4, "bandpass", [2.0, 60.0], 8), (4, "bandpass", [2.0, 60.0], 11),
                                                 (8, "bandpass", [70.0, 150.0], 8), (16, "lowpass", 60.0, 9)])
def test_scan_matrices_are_the_exact_powers_rounded_once(order, ftype, freqs, Lb):
    from decode_tonal_langauge_amd.preprocess.signal.frequency_filter import _sos_scan_matrices
    sos = R.design(order, freqs, 400.0, ftype)
    ns = 2 * sos.shape[0]
    nlev = 3
    M = _sos_scan_matrices(sos, Lb, nlev)
    assert M.shape == (nlev, 16, 16, 2) and M.dtype == np.float64
    A = _exact_A(sos)
    mm = lambda X, Y: [[sum(X[i][k] * Y[k][j] for k in range(ns)) for j in range(ns)] for i in range(ns)]
    P = [[Fraction(int(i == j)) for j in range(ns)] for i in range(ns)]
    for _ in range(Lb):
        P = mm(P, A)
    for m in range(nlev):
        for i in range(16):
            for j in range(16):
                want = P[i][j] if i < ns and j < ns else Fraction(0)
                hi = float(want)                                          # (Fraction -> float rounds correctly)
                assert M[m, i, j, 0] == hi, (m, i, j)
                assert M[m, i, j, 1] == float(want - Fraction(hi)), (m, i, j)
        # lower block-triangular: a section never sees the states of the sections behind it
        assert all(P[i][j] == 0 for i in range(ns) for j in range(ns) if j // 2 > i // 2)
        P = mm(P, P)


def test_block_scan_restated_in_numpy_stays_near_scipys_own_rounding():
    from decode_tonal_langauge_amd.preprocess.signal.frequency_filter import _sos_scan_matrices
    assert R.has_long_double(), "the yardstick needs a long double wider than double on this host"
    obs = {}
    worst = 0.0
    for name, (order, freqs, fs, ftype, dc) in R.DESIGNS.items():
        sos = R.design(order, freqs, fs, ftype)
        nsec = sos.shape[0]
        blk, nlev = (128, 7) if nsec <= 4 else (64, 6)                     # the device's chunk of the prefix
        M = _sos_scan_matrices(sos, L, nlev)
        for T in (3000, 40000):                                           # 24 and 313 blocks: one chunk, and 3 - 5 of them
            x = np.random.default_rng(T + order).standard_normal(T) + dc
            ref = sps.sosfilt(sos, x)
            assert np.array_equal(R.sosfilt_loop(sos, x[None, :2000], np.float64)[0], ref[:2000])   # the loop IS scipy's
            yard = R.yardstick(sos, x[None], ref[None])
            got = R.scan_restated(sos, x, L, M, blk)
            assert np.array_equal(got[:L], ref[:L])                       # the first block: same statements, zero state
            dev = float(np.abs(got - ref).max() / np.abs(ref).max())
            ratio = dev / yard
            obs[f"{name} ({nsec} sections) T={T} scipy-vs-long-double"] = yard
            obs[f"{name} ({nsec} sections) T={T} scan-vs-scipy"] = dev
            obs[f"{name} ({nsec} sections) T={T} ratio"] = ratio
            worst = max(worst, ratio)
            print(f"{name} T={T}: scipy vs long double {yard:.3e}, scan vs scipy {dev:.3e}, ratio {ratio:.2f}")
    obs["largest ratio"] = worst
    record("sosfilt_scan_restated", obs)
    bad = {k: v for k, v in obs.items() if k.endswith("ratio") and v > RATIO_BOUND}
    assert not bad, bad


def test_entry_is_declared_bound_and_exported():
    import os
    import re
    from decode_tonal_langauge_amd import _lib
    lib = _lib.load()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "tonal_hip.h")) as f:
        header = f.read()
    assert re.search(r"\bint\s+tl_sosfilt_scan_f64\s*\(", header)
    assert "tl_sosfilt_scan_f64" in _lib.SIGNATURES and hasattr(lib, "tl_sosfilt_scan_f64")
    assert len(_lib.SIGNATURES["tl_sosfilt_scan_f64"][1]) == 13


def test_entry_refuses_bad_arguments_without_gpu():
    """(x, x_is_f64, sos, M, nlev, y, work, swork, C, T, nsec, L, stream): every refusal comes before the first launch, so
    the dummy pointers are never touched"""
    from decode_tonal_langauge_amd import _lib
    lib = _lib.load()
    f, err = lib.tl_sosfilt_scan_f64, lib.tl_last_error
    ok = dict(x=16, f64=1, sos=16, M=16, nlev=7, y=16, work=16, swork=16, C=2, T=5000, nsec=4, L=128)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a["x"], a["f64"], a["sos"], a["M"], a["nlev"], a["y"], a["work"], a["swork"], a["C"], a["T"], a["nsec"], a["L"], None)

    for name in ("x", "sos", "M", "y", "work", "swork"):
        assert call(**{name: None}) == -1 and b"null pointer" in err(), name
    for nsec in (0, 9, -1):
        assert call(nsec=nsec) == -1 and b"sosfilt: nsec must be 1..8" in err(), nsec
    assert lib.tl_sosfilt_f64(16, 1, 16, 16, 2, 5000, 9, None) == -1
    seq_words = err()
    assert call(nsec=9) == -1 and err() == seq_words                      # the sequential entry's own words
    for C in (0, -3, 65536):
        assert call(C=C) == -1 and b"bad sizes" in err(), C
    for T in (0, -1):
        assert call(T=T) == -1 and b"bad sizes" in err(), T
    for Lb in (7, 0, -128):
        assert call(L=Lb) == -1 and b"at least 8 samples" in err(), Lb
    assert call(T=65535 * 128 + 1) == -1 and b"65 535 blocks" in err()
    assert call(T=65536 * 8, L=8) == -1 and b"65 535 blocks" in err()
    assert call(nsec=4, nlev=6) == -1 and b"7 matrix levels" in err()     # chunks of 128 blocks up to four sections
    assert call(nsec=5, nlev=5) == -1 and b"6 matrix levels" in err()     # chunks of 64 beyond
    assert call(nsec=8, nlev=0) == -1 and b"matrix levels" in err()
