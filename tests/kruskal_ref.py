"""CPU references of the Kruskal-Wallis tests - TEST INFRASTRUCTURE (no reference-project code).

NumPy, scipy and mpmath.  ``midranks`` is ``scipy.stats.rankdata(axis=0)``; ``scipy_kruskal`` is ``scipy.stats.kruskal(axis=0)``,
the yardstick; ``h_identity`` restates H as the ANOVA decomposition of the midranks, ``H = (N - 1) ssb / sst`` (tie correction
included); ``exact`` evaluates that identity in rational arithmetic on the doubled ranks (integers) and the chi-square tail
with mpmath at 50 digits.  The distance of scipy from ``exact`` is the yardstick's own floor.  ``perm_expected`` decides
``sum_g S_g^2 / n_g > tau`` of every relabelling in rational arithmetic.  The inputs of both test files are built here."""
import functools
import warnings
from fractions import Fraction

import numpy as np
from scipy import special, stats

HARD_CAP = 1e-9
ULP = 2.0 ** -52
PERM_MARGIN = 1e-12
SHARE_CAP = 1e-4


def _groups(x, labels):
    if labels is None:
        return [np.asarray(g) for g in x]
    x = np.asarray(x)
    return [x[labels == v] for v in np.unique(labels)]


def midranks(x, x1=None):
    """float32 midranks down axis 0 (a column with a NaN is NaN throughout), of x or of x followed by x1."""
    x = np.asarray(x) if x1 is None else np.concatenate([np.asarray(x), np.asarray(x1)])
    return stats.rankdata(x, method="average", axis=0).astype(np.float32)


def scipy_kruskal(x, labels=None):
    """(H, p) of scipy.stats.kruskal along axis 0, in the dtype's own values."""
    groups = _groups(x, labels)
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        res = stats.kruskal(*groups, axis=0)
    return np.asarray(res.statistic, dtype=np.float64), np.asarray(res.pvalue, dtype=np.float64)


def _ranks_and_index(x, labels):
    groups = _groups(x, labels)
    sizes = [g.shape[0] for g in groups]
    r = stats.rankdata(np.concatenate(groups), method="average", axis=0)
    starts = np.concatenate(([0], np.cumsum(sizes)))
    return r, [np.arange(starts[g], starts[g + 1]) for g in range(len(sizes))]


def h_identity(x, labels=None):
    """(H, p) in float64 from the ANOVA decomposition of the midranks; p from scipy.special.chdtrc."""
    r, index = _ranks_and_index(x, labels)
    N, k = r.shape[0], len(index)
    with np.errstate(all="ignore"):
        d = r - r.mean(axis=0)
        sst = (d * d).sum(axis=0)
        ssb = sum(d[ix].sum(axis=0) ** 2 / len(ix) for ix in index)
        H = (N - 1) * ssb / sst
        return H, special.chdtrc(k - 1, H)


def exact(x, labels=None):
    """(H, p) rounded once from exact values: H as a Fraction of the doubled ranks, p = Q((k - 1)/2, H/2) at 50 digits.
    NaN where the column holds a NaN or all its values are identical."""
    import mpmath
    r, index = _ranks_and_index(x, labels)
    N, k = r.shape[0], len(index)
    shape = r.shape[1:]
    r = r.reshape(N, -1)
    H, p = np.full(r.shape[1], np.nan), np.full(r.shape[1], np.nan)
    with mpmath.workdps(50):
        for c in range(r.shape[1]):
            if np.isnan(r[:, c]).any():
                continue
            d = [int(v) for v in np.rint(2 * r[:, c])]
            assert all(v == 2 * w for v, w in zip(d, r[:, c]))
            total = sum(d)
            mean_sq = Fraction(total * total, N)
            sst = sum(v * v for v in d) - mean_sq
            if sst == 0:
                continue
            ssb = sum(Fraction(sum(d[i] for i in ix) ** 2, len(ix)) for ix in index) - mean_sq
            h = (N - 1) * ssb / sst
            H[c] = float(h)
            hm = mpmath.mpf(h.numerator) / mpmath.mpf(h.denominator)
            p[c] = float(mpmath.gammainc(mpmath.mpf(k - 1) / 2, hm / 2, mpmath.inf, regularized=True))
    return H.reshape(shape), p.reshape(shape)


def rel(a, b, mask):
    """max |a - b| / |b| over mask."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    with np.errstate(all="ignore"):
        r = np.abs(a - b) / np.abs(b)
    r = np.where(a == b, 0.0, r)
    return float(np.max(r[mask])) if mask.any() else 0.0


def longest_runs(below):
    """Longest run of True per row, by counting."""
    out = []
    for row in below:
        best = run = 0
        for v in row:
            run = run + 1 if v else 0
            best = max(best, run)
        out.append(best)
    return out


def selection(p, threshold, length_threshold):
    """(selected channels, longest run per channel, cells within 1e-9 relative of the threshold) on a p-value array."""
    with np.errstate(all="ignore"):
        below = p < threshold
        near = np.abs(p - threshold) <= HARD_CAP * threshold
    runs = longest_runs(below)
    return [c for c, r in enumerate(runs) if r > length_threshold], runs, near


# ---- the inputs -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def heavy_tail_input():
    """The input of the issue: 120 samples in 3 shuffled equal classes, 8 channels, 60 timepoints, an effect of 0.9 per class
    step in channels 0-3 at timepoints 20-49, and 4 % of the (sample, channel) pairs off by +-40 over the whole window."""
    rng = np.random.default_rng(7)
    N, C, T = 120, 8, 60
    lab = rng.permutation(np.arange(N) % 3)
    x = rng.standard_normal((N, C, T))
    x[:, :4, 20:50] += 0.9 * lab[:, None, None]
    hit = rng.random((N, C)) < 0.04
    x += (hit * rng.choice([-40.0, 40.0], size=(N, C)))[:, :, None]
    x.setflags(write=False)
    return x, lab


@functools.lru_cache(maxsize=None)
def heavy_tail_rest_erp():
    """Rest and ERP with the same tails: 70 and 50 samples, the ERP 1.2 higher in channels 0-3 at timepoints 20-49."""
    rng = np.random.default_rng(8)
    C, T = 8, 60
    rest, erp = rng.standard_normal((70, C, T)), rng.standard_normal((50, C, T))
    erp[:, :4, 20:50] += 1.2
    for a in (rest, erp):
        hit = rng.random(a.shape[:2]) < 0.04
        a += (hit * rng.choice([-40.0, 40.0], size=a.shape[:2]))[:, :, None]
        a.setflags(write=False)
    return rest, erp


@functools.lru_cache(maxsize=None)
def ragged_labelled():
    rng = np.random.default_rng(21)
    N, C, T = 50, 3, 77
    lab = rng.permutation(np.arange(N) % 3) * 3 - 1
    x = rng.standard_normal((N, C, T))
    x[:, :2, 10:50] += 1.5 * (lab[:, None, None] == lab.max())
    x = np.round(x * 4) / 4                                   # ties
    x.setflags(write=False)
    return x, lab


@functools.lru_cache(maxsize=None)
def ragged_rest_erp():
    rng = np.random.default_rng(22)
    rest, erp = rng.standard_normal((31, 5, 65)), rng.standard_normal((23, 5, 65))
    erp[:, 1:3, 5:40] += 1.6
    rest, erp = rest.astype(np.float32), erp.astype(np.float32)
    rest.setflags(write=False)
    erp.setflags(write=False)
    return rest, erp


HP_VARIANTS = ("float64", "tied", "float32")


@functools.lru_cache(maxsize=None)
def hp_input(variant):
    """480 samples in 4 classes, 6 channels of 50 timepoints; an effect of 1.5 per class step in two channels."""
    rng = np.random.default_rng(0)
    N, C, T = 480, 6, 50
    lab = rng.integers(0, 4, N)
    x = rng.standard_normal((N, C, T))
    x[:, :2, 10:40] += 1.5 * lab[:, None, None]
    if variant == "tied":
        x = np.round(x * 2) / 2
    elif variant == "float32":
        x = x.astype(np.float32)
    x.setflags(write=False)
    return x, lab


@functools.lru_cache(maxsize=None)
def hp_refs(variant):
    """(scipy (H, p), exact (H, p)) of hp_input(variant)."""
    x, lab = hp_input(variant)
    return scipy_kruskal(x, lab), exact(x, lab)


# ranks: every N with the column counts 1, 37 and a tile multiple plus 3 whose tile boundary falls inside a channel
RANK_N = (2, 63, 64, 65, 257, 480, 1000)


def rank_shapes(tile):
    """[(C, T)]: 1 column, 37 columns, and m * tile + 3 = C * T >= 9 columns with T no divisor of the tile."""
    for m in range(1, 64):
        cols = m * tile + 3
        for C in range(2, cols if cols >= 9 else 0):
            if cols % C == 0 and cols // C >= 2 and tile % (cols // C) != 0:
                return [(1, 1), (1, 37), (C, cols // C)]
    raise AssertionError(tile)


def rank_input(N, C, T, dtype, seed=0):
    """(N, C, T) standard normal in ``dtype`` with, where the columns exist: column 0 quantised to 8 levels, 2 all equal,
    3 mixing -0.0 and +0.0 with other values, 4 with +-inf, 6 with one NaN (5 and 7 stay intact), 8 = 1 + j 2^-40 shuffled
    (distinct in float64, one value in float32), and the last column quantised again."""
    rng = np.random.default_rng(1000 * seed + N)
    cols = C * T
    x = rng.standard_normal((N, cols))
    quant = lambda v: np.clip(np.floor(v * 2), -4, 3) / 2
    x[:, 0] = quant(x[:, 0])
    x[:, -1] = quant(x[:, -1])
    if cols > 8:
        x[:, 2] = 3.25
        x[:, 3] = rng.choice([-0.0, 0.0, -1.0, 1.0, 0.0, -0.0], size=N)
        x[rng.random(N) < 0.3, 4] = np.inf
        x[rng.random(N) < 0.3, 4] = -np.inf
        x[N // 2, 6] = np.nan
        x[:, 8] = 1.0 + rng.permutation(N) * 2.0 ** -40
    x = x.reshape(N, C, T).astype(dtype)
    x.setflags(write=False)
    return x


# ---- permutation test on the ranks ----------------------------------------------------------------------------------
# (samples, channels, timepoints), group sizes, rows P of the table, cell level, dtype, ties
PERM_CASES = {
    "n31_k2": dict(shape=(31, 3, 40), counts=(15, 16), P=33, cell=0.01, dtype="float64", seed=1),
    "n32_k3_tied": dict(shape=(32, 3, 40), counts=(10, 11, 11), P=33, cell=0.02, dtype="float64", seed=2, tied=True),
    "n33_k3_f32": dict(shape=(33, 2, 70), counts=(11, 11, 11), P=20, cell=0.02, dtype="float32", seed=3),
    "n97_k2_tied": dict(shape=(97, 2, 33), counts=(40, 57), P=33, cell=0.005, dtype="float64", seed=4, tied=True),
    "n97_k3": dict(shape=(97, 4, 20), counts=(30, 33, 34), P=17, cell=0.005, dtype="float64", seed=5),
}


def table_ref(group_index, n_permutations, seed):
    rng = np.random.default_rng(seed)
    rows = [np.asarray(group_index)] + [rng.permutation(group_index) for _ in range(n_permutations)]
    return np.stack(rows).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def perm_case(name):
    spec = PERM_CASES[name]
    N, C, T = spec["shape"]
    counts = tuple(spec["counts"])
    assert sum(counts) == N
    rng = np.random.default_rng(spec["seed"])
    group_index = rng.permutation(np.repeat(np.arange(len(counts)), counts))
    x = rng.standard_normal((N, C, T))
    x[:, :2, T // 4:T - T // 4] += 1.2 * group_index[:, None, None]
    if spec.get("tied"):
        x = np.round(x * 2) / 2
    x = x.astype(spec["dtype"])
    table = table_ref(group_index, spec["P"] - 1, seed=100 + spec["seed"])
    chi2_crit = float(stats.chi2.isf(spec["cell"], len(counts) - 1))
    out = dict(x=x, table=table, counts=counts, k=len(counts), cell=spec["cell"], chi2_crit=chi2_crit,
               theta=chi2_crit / (N - 1), group_index=group_index)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def perm_expected(name):
    """(mask, excluded), both bool (P, C, T): where ssb > theta sst under each relabelling, decided in rational arithmetic
    on the doubled ranks with theta the float the package forms, and the cells whose exact relative margin
    |ssb - theta sst| / (theta sst) is below 1e-12 (left out of the comparison)."""
    c = perm_case(name)
    N, C, T = c["x"].shape
    d = np.rint(2 * stats.rankdata(c["x"].reshape(N, C * T), method="average", axis=0)).astype(np.int64)
    theta = Fraction(c["theta"])
    P = c["table"].shape[0]
    mask, excluded = np.zeros((P, C * T), dtype=bool), np.zeros((P, C * T), dtype=bool)
    onehot = [(c["table"] == g).astype(np.int64) for g in range(c["k"])]
    sums = [oh @ d for oh in onehot]                                       # (P, cols) integers, exact
    total, squares = d.sum(axis=0), (d * d).sum(axis=0)
    for col in range(C * T):
        mean_sq = Fraction(int(total[col]) ** 2, N)
        bound = theta * (int(squares[col]) - mean_sq)
        for r in range(P):
            ssb = sum(Fraction(int(sums[g][r, col]) ** 2, n_g) for g, n_g in enumerate(c["counts"])) - mean_sq
            mask[r, col] = ssb > bound
            excluded[r, col] = bound > 0 and abs(ssb - bound) < Fraction(PERM_MARGIN) * bound
    return mask.reshape(P, C, T), excluded.reshape(P, C, T)
