"""Shared by the host and the GPU tests of the time-parallel sosfilt (``TONAL_KERNELS=butter=scan``, ``causal=True``): scipy's
``_sosfilt`` loop in any dtype (the long-double yardstick), the device's block scan restated in NumPy, and the designs."""
import numpy as np
import scipy.signal as sps

#: name -> (order, freqs, fs, filter_type, DC level of the recording)
DESIGNS = {
    "bp4 70-150 @400": (4, [70.0, 150.0], 400.0, "bandpass", 0.0),
    "bp8 70-150 @400": (8, [70.0, 150.0], 400.0, "bandpass", 0.0),
    "bp4 1-50 @24414": (4, [1.0, 50.0], 24414.0, "bandpass", 0.0),
    "bp4 70-150 @24414 dc1000": (4, [70.0, 150.0], 24414.0, "bandpass", 1000.0),
    "lp8 100 @24414 dc1000": (8, 100.0, 24414.0, "lowpass", 1000.0),
    "hp4 0.5 @400 dc1000": (4, 0.5, 400.0, "highpass", 1000.0),
    "lp16 60 @400": (16, 60.0, 400.0, "lowpass", 0.0),
}


def design(order, freqs, fs, ftype):
    """the section coefficients exactly as ``butter_filter`` designs them"""
    wn = np.asarray(freqs, dtype=float) / (0.5 * fs)
    return np.ascontiguousarray(sps.butter(order, wn, btype=ftype, output="sos"), dtype=np.float64)


def sosfilt_loop(sos, x, dt):
    """scipy's ``_sosfilt`` loop - same statements, same order - in dtype ``dt`` on a (C, T) recording, zero initial state"""
    s = np.asarray(sos).astype(dt)
    x = np.asarray(x).astype(dt)
    nsec = s.shape[0]
    z = np.zeros((nsec, 2, x.shape[0]), dt)
    y = np.empty_like(x)
    for i in range(x.shape[1]):
        v = x[:, i]
        for q in range(nsec):
            yv = s[q, 0] * v + z[q, 0]
            z[q, 0] = (s[q, 1] * v - s[q, 4] * yv) + z[q, 1]
            z[q, 1] = s[q, 2] * v - s[q, 5] * yv
            v = yv
        y[:, i] = v
    return y


def has_long_double():
    return np.finfo(np.longdouble).nmant > 52


def yardstick(sos, x, ref=None):
    """max |scipy - the same loop in long double| over a (C, T) recording, relative to the largest output sample"""
    ref = sps.sosfilt(sos, x, axis=-1) if ref is None else ref
    wide = sosfilt_loop(sos, x, np.longdouble).astype(np.float64)
    return float(np.abs(wide - ref).max() / np.abs(ref).max())


def _two_prod_err(a, b, p):
    """a * b - p exactly, p = fl(a * b): Dekker's split (what the device gets from one fma)"""
    def split(v):
        t = 134217729.0 * v
        hi = t - (t - v)
        return hi, v - hi
    a, b = np.broadcast_arrays(a, b)
    ah, al = split(a)
    bh, bl = split(b)
    return ((ah * bh - p) + ah * bl + al * bh) + al * bl


def scan_restated(sos, x, L, M, blk):
    """The three device steps of ``tl_sosfilt_scan_f64`` for ONE channel in fp64: blocks of ``L`` samples from a zero state,
    the Hillis-Steele scan over chunks of ``blk`` blocks with the host's matrices ``M`` (levels, 16, 16) and the carry from
    chunk to chunk, the blocks again from their true start states.  A row of ``M u + v`` is v + M_0 u_0 + M_1 u_1 + ..., left
    to right, unfused - the device's statements."""
    nsec = sos.shape[0]
    ns = 2 * nsec
    N = len(x)
    nb = (N + L - 1) // L
    xp = np.concatenate([np.asarray(x, np.float64), np.zeros(nb * L - N)]).reshape(nb, L)

    def run(zs):
        z = zs.copy()
        y = np.empty_like(xp)
        for t in range(L):
            v = xp[:, t]
            for q in range(nsec):
                yv = sos[q, 0] * v + z[:, 2 * q]
                z[:, 2 * q] = (sos[q, 1] * v - sos[q, 4] * yv) + z[:, 2 * q + 1]
                z[:, 2 * q + 1] = sos[q, 2] * v - sos[q, 5] * yv
                v = yv
            y[:, t] = v
        return y, z

    def row_mv(Mm, u, v):                      # u, v (n, ns): rows of  M u + v
        if Mm.ndim == 2:                       # plain doubles, summed left to right (kept for the comparison of the two formats)
            acc = v.copy()
            for k in range(ns):
                acc = acc + Mm[None, :ns, k] * u[:, k:k + 1]
            return acc
        s, e = v.copy(), np.zeros_like(v)      # (hi, lo) pairs: the device's compensated dot product (scan_row)
        for k in range(ns):
            mh, ml, uk = Mm[None, :ns, k, 0], Mm[None, :ns, k, 1], u[:, k:k + 1]
            pr = mh * uk
            pe = _two_prod_err(mh, uk, pr)
            s2 = s + pr
            bv = s2 - s
            se = (s - (s2 - bv)) + (pr - bv)
            s = s2
            e = e + ((pe + se) + ml * uk)
        return s + e

    _, s = run(np.zeros((nb, ns)))
    Z = np.zeros((nb, ns))
    carry = np.zeros(ns)
    for c0 in range(0, nb, blk):
        nact = min(blk, nb - c0)
        v = s[c0:c0 + nact].copy()
        Z[c0] = carry
        v[0:1] = row_mv(M[0], carry[None, :], v[0:1])
        lev, d = 0, 1
        while d < nact:
            prev = v.copy()
            v[d:] = row_mv(M[lev], prev[:-d], prev[d:])
            lev, d = lev + 1, d * 2
        Z[c0 + 1:c0 + nact] = v[:nact - 1]
        if c0 + nact < nb:
            Z[c0 + nact] = v[nact - 1]
        carry = v[nact - 1]
    y, _ = run(Z)
    return y.reshape(-1)[:N]
