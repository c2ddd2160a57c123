"""NumPy restatement of the blocked rolling z-score (tl_rolling_zscore_blocked) - TEST INFRASTRUCTURE ONLY.

The same tiling and the same pair arithmetic as the kernels in csrc/tonal_steps.hip, operation for operation and in the
same order, on whole arrays: a moment is the tuple (n, S1 hi, S1 lo, S2 hi, S2 lo, min, max) of a set of samples, NaN
samples and samples outside the recording are the identity, the 256 lanes of a tile are the last axis.  NumPy has no fma:
the exact product comes from Dekker's split, which yields the same two words."""
import numpy as np

TILE = 256
_INF = np.inf


def _two_sum(a, b):
    s = a + b
    bv = s - a
    return s, (a - (s - bv)) + (b - bv)


def _fast_two_sum(a, b):
    s = a + b
    return s, b - (s - a)


def _dd_add(ah, al, bh, bl):
    s, e = _two_sum(ah, bh)
    t, f = _two_sum(al, bl)
    s, e = _fast_two_sum(s, e + t)
    return _fast_two_sum(s, e + f)


def _split(a):
    c = 134217729.0 * a                                          # 2^27 + 1
    hi = c - (c - a)
    return hi, a - hi


def _prod_plus(a, b, c):
    """(a b) + c as a pair: a b = p + e exactly, c joins the error word."""
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    return _fast_two_sum(p, e + c)


def _sample(v):
    ok = ~np.isnan(v)
    v0 = np.where(ok, v, 0.0)
    s2h, s2l = _prod_plus(v0, v0, 0.0)
    return (ok.astype(np.int64), v0, np.zeros_like(v0), s2h, s2l, np.where(ok, v, _INF), np.where(ok, v, -_INF))


def _combine(a, b):
    s1 = _dd_add(a[1], a[2], b[1], b[2])
    s2 = _dd_add(a[3], a[4], b[3], b[4])
    return (a[0] + b[0], s1[0], s1[1], s2[0], s2[1], np.minimum(a[5], b[5]), np.maximum(a[6], b[6]))


def _cut(m, idx):
    return tuple(f[idx] for f in m)


def _block_scan(m, rev=False):
    """Inclusive scan along the last axis (256 lanes; rev: from lane 255 down): Hillis-Steele in each 64-lane wave, then the
    totals of the waves before (after) this one, the nearest added last, go in front (behind)."""
    lead = m[0].shape[:-1]
    m = tuple(np.array(f).reshape(lead + (4, 64)) for f in m)
    off = 1
    while off < 64:
        if rev:
            new = _combine(_cut(m, np.s_[..., :-off]), _cut(m, np.s_[..., off:]))
            m = tuple(np.concatenate([n_, f[..., -off:]], axis=-1) for n_, f in zip(new, m))
        else:
            new = _combine(_cut(m, np.s_[..., :-off]), _cut(m, np.s_[..., off:]))
            m = tuple(np.concatenate([f[..., :off], n_], axis=-1) for n_, f in zip(new, m))
        off *= 2
    tot = _cut(m, np.s_[..., 0 if rev else 63])                  # lead + (4,)
    waves = [_cut(m, np.s_[..., w, :]) for w in range(4)]
    wt = [_cut(tot, np.s_[..., w:w + 1]) for w in range(4)]
    if rev:
        for w in range(3):
            p = wt[3]
            for k in range(2, w, -1):
                p = _combine(wt[k], p)
            waves[w] = _combine(waves[w], p)
    else:
        for w in range(1, 4):
            p = wt[0]
            for k in range(1, w):
                p = _combine(p, wt[k])
            waves[w] = _combine(p, waves[w])
    return tuple(np.concatenate([waves[w][i] for w in range(4)], axis=-1) for i in range(7))


def _identity_where(mask, m):
    ident = (0, 0.0, 0.0, 0.0, 0.0, _INF, -_INF)
    return tuple(np.where(mask, f, i) for f, i in zip(m, ident))


def blocked_rolling_zscore(x: np.ndarray, window: int, preserve_nans: bool = True) -> np.ndarray:
    x = np.asarray(x)
    assert x.ndim == 2 and x.dtype in (np.float32, np.float64)
    x = x.astype(np.float64)
    C, T = x.shape
    W = min(int(window), T)
    assert W >= TILE, "the blocked route needs min(window, T) >= 256"
    nt = -(-T // TILE)
    lanes = np.arange(TILE)

    def gather(idx):                                             # x[:, idx], NaN outside the recording
        ok = (idx >= 0) & (idx < T)
        return np.where(ok, x[:, np.clip(idx, 0, T - 1)], np.nan)

    t0 = np.arange(nt)[:, None] * TILE                           # (nt, 1)
    xv = gather(t0 + lanes)                                      # (C, nt, 256)
    a = _block_scan(_sample(xv))                                 # (a), and the table: its last lane
    table = _cut(a, np.s_[..., TILE - 1])                        # (C, nt) each
    pos = t0 + TILE - W > 0
    k0 = np.where(pos, -(-(t0 + TILE - W) // TILE), 0)           # (nt, 1)
    h0 = t0 - W + 1
    L = np.where(pos, k0 * TILE - h0, 0)
    c = _block_scan(_sample(np.where(lanes < L, gather(h0 + lanes), np.nan)), rev=True)          # (c)
    p = _sample(np.where(TILE + lanes < L, gather(h0 + TILE + lanes), np.nan))
    j = np.arange(nt)[:, None]
    m = 0
    while True:                                                  # (b): lane i adds rows k0 + i, k0 + i + 256, ...
        k = k0 + m + lanes
        live = k < j
        if not live.any():
            break
        rows = _cut(table, (slice(None), np.clip(k, 0, nt - 1)))
        p = _combine(p, _identity_where(live, rows))
        m += TILE
    M = _cut(_block_scan(p), np.s_[..., TILE - 1:TILE])
    w = _combine(_combine(c, M), a)
    n = w[0].astype(np.float64)
    ok = ~np.isnan(xv) & (w[0] >= 2) & (w[5] != w[6])
    x0 = np.where(ok, xv, 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        ah, al = _prod_plus(n, w[3], n * w[4])
        bh, bl = _prod_plus(w[1], w[1], 2.0 * (w[1] * w[2]))
        qh, ql = _dd_add(ah, al, -bh, -bl)
        ah, al = _prod_plus(n, x0, 0.0)
        dh, dl = _dd_add(ah, al, -w[1], -w[2])
        z = ((dh + dl) / n) / np.sqrt(((qh + ql) / n) / (n - 1.0))
    out = np.where(ok, z, np.nan).reshape(C, nt * TILE)[:, :T]
    if not preserve_nans:
        out = np.where(np.isnan(out), 0.0, out)
    return np.ascontiguousarray(out)
