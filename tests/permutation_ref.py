"""CPU oracle of the label-permutation test for channel selection - TEST INFRASTRUCTURE (no reference-project code).

Plain NumPy float64.  ``exceed_ref`` restates "the ANOVA at this cell has p < alpha'" as ``ssb > theta * sst`` from group sums
taken after subtracting the column mean (the host test checks that statement against ``scipy.stats.f_oneway`` cell for
cell); ``runs_ref`` counts; ``p_values_ref`` forms both permutation p-vectors; ``margin`` is the smallest relative distance
of any cell from the threshold - the exclusion rule of the GPU tests, which demand equality: an input belongs to the tests
only if the oracle alone puts every cell at least 1e-7 away from the decision.  ``CASES`` are the inputs both test files
use."""
import functools
import warnings

import numpy as np
from scipy import stats

MARGIN_FLOOR = 1e-7
SAMPLE_CHUNK = 32                       # samples per LDS stage of tl_perm_exceed (channel_selection.utils.PERM_SAMPLE_CHUNK)


def theta_of(alpha_cell, k, n):
    """(f_crit, theta): p < alpha_cell is F > f_crit is ssb > theta sst."""
    dfb, dfw = k - 1, n - k
    f_crit = float(stats.f.isf(alpha_cell, dfb, dfw))
    return f_crit, f_crit * dfb / (dfw + f_crit * dfb)


def _ssb_sst(x, table, counts):
    """ssb (P, cols) under every row of table, sst (cols), from column-mean-centred float64 data x (N, cols)."""
    with np.errstate(all="ignore"):
        d = x - x.mean(axis=0)
        sst = (d * d).sum(axis=0)
        ssb = np.zeros((table.shape[0], x.shape[1]))
        for g, n_g in enumerate(counts):
            s = (table == g).astype(np.float64) @ d
            ssb += s * s / n_g
    return ssb, sst


def exceed_ref(x, table, counts, theta):
    """bool (P, C, T): ssb > theta * sst under every labelling of table (P, N); x (N, C, T).  False where NaN."""
    x = np.asarray(x, dtype=np.float64)
    N, C, T = x.shape
    ssb, sst = _ssb_sst(x.reshape(N, C * T), np.asarray(table), counts)
    with np.errstate(all="ignore"):
        return (ssb > theta * sst).reshape(-1, C, T)


def margin(x, table, counts, theta):
    """Smallest |ssb - theta sst| / (theta sst) over all cells with finite sst > 0."""
    x = np.asarray(x, dtype=np.float64)
    N = x.shape[0]
    ssb, sst = _ssb_sst(x.reshape(N, -1), np.asarray(table), counts)
    ok = np.isfinite(sst) & (sst > 0)
    if not ok.any():
        return np.inf
    return float(np.min(np.abs(ssb[:, ok] - theta * sst[ok]) / (theta * sst[ok])))


def scipy_exceed(x, table, k, alpha_cell):
    """bool (P, C, T): scipy.stats.f_oneway(...).pvalue < alpha_cell under every labelling."""
    x = np.asarray(x, dtype=np.float64)
    N, C, T = x.shape
    flat = x.reshape(N, C * T)
    out = np.zeros((table.shape[0], C * T), dtype=bool)
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        for r, row in enumerate(table):
            out[r] = stats.f_oneway(*[flat[row == g] for g in range(k)], axis=0).pvalue < alpha_cell
    return out.reshape(-1, C, T)


def runs_ref(mask):
    """int32 (P, C): longest run of True along the last axis, by counting."""
    P, C, T = mask.shape
    out = np.zeros((P, C), dtype=np.int32)
    for p in range(P):
        for c in range(C):
            best = run = 0
            for v in mask[p, c]:
                run = run + 1 if v else 0
                best = max(best, run)
            out[p, c] = best
    return out


def p_values_ref(runs):
    """(p_channel, p_max), each (C,) float64: (1 + #{pi >= 1: null >= observed}) / P."""
    P, C = runs.shape
    p_channel, p_max = np.empty(C), np.empty(C)
    for c in range(C):
        p_channel[c] = (1 + sum(1 for r in range(1, P) if runs[r, c] >= runs[0, c])) / P
        p_max[c] = (1 + sum(1 for r in range(1, P) if runs[r].max() >= runs[0, c])) / P
    return p_channel, p_max


def table_ref(group_index, n_permutations, seed):
    """The relabelling table as the issue defines it (independent of the package's permutation_table)."""
    rng = np.random.default_rng(seed)
    rows = [np.asarray(group_index)] + [rng.permutation(group_index) for _ in range(n_permutations)]
    return np.stack(rows).astype(np.uint8)


def selection_ref(runs, alpha, correction):
    p_channel, p_max = p_values_ref(runs)
    p = p_max if correction == "max" else p_channel
    return [int(c) for c in np.flatnonzero((runs[0] > 0) & (p <= alpha))], p


# ---- the inputs of the tests: (samples, channels, timepoints), group sizes, total rows P, selector-level p_threshold
# (the cell level is p_threshold / T), dtype, DC offset, samples in the first of two arrays (None: one array).  Planted
# effects sit in the first two channels over the middle half of the timepoints.
CASES = {
    "three_groups_loose": dict(shape=(24, 5, 37), counts=(7, 8, 9), P=33, p_threshold=1.0, dtype="float64", seed=1),
    "three_groups_strict": dict(shape=(24, 5, 37), counts=(7, 8, 9), P=33, p_threshold=0.05, dtype="float64", seed=1),
    "rest_erp_offset_1e4": dict(shape=(24, 3, 70), counts=(11, 13), P=40, p_threshold=28.0, dtype="float64", seed=2,
                                offset=1e4, n0=11),
    "four_groups_f64": dict(shape=(30, 4, 130), counts=(6, 7, 8, 9), P=50, p_threshold=39.0, dtype="float64", seed=3),
    "four_groups_f32": dict(shape=(30, 4, 130), counts=(6, 7, 8, 9), P=50, p_threshold=2.0, dtype="float32", seed=3),
    "two_groups_ragged_rows": dict(shape=(21, 2, 200), counts=(10, 11), P=65, p_threshold=70.0, dtype="float32", seed=4),
    "chunk_plus_one_T257": dict(shape=(SAMPLE_CHUNK + 1, 1, 257), counts=(1, 8, 8, 8, 8), P=20, p_threshold=51.4,
                                dtype="float64", seed=5),
    "chunk_plus_one_T33": dict(shape=(SAMPLE_CHUNK + 1, 2, 33), counts=(1, 8, 8, 8, 8), P=20, p_threshold=6.6,
                               dtype="float64", seed=6),
    "nan_and_constant_channels": dict(shape=(24, 4, 40), counts=(12, 12), P=30, p_threshold=8.0, dtype="float64", seed=7,
                                      nan_channel=2, constant_channel=3),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(x (N, C, T) in its dtype, x64, table, counts, k, alpha_cell, f_crit, theta, n0) of a named case; cached, read-only."""
    spec = CASES[name]
    N, C, T = spec["shape"]
    counts = tuple(spec["counts"])
    assert sum(counts) == N
    rng = np.random.default_rng(spec["seed"])
    group_index = np.repeat(np.arange(len(counts)), counts)
    if "n0" not in spec:
        group_index = rng.permutation(group_index)           # two arrays: rest first, then ERP, as the selector lays them out
    x = rng.standard_normal((N, C, T))
    x[:, :min(2, C), T // 4:T - T // 4] += 1.5 * group_index[:, None, None]
    x = (x + spec.get("offset", 0.0)).astype(spec["dtype"])
    if "nan_channel" in spec:
        x[:, spec["nan_channel"], :] = np.nan
        x[:, spec["constant_channel"], :] = 3.25
    table = table_ref(group_index, spec["P"] - 1, seed=100 + spec["seed"])
    alpha_cell = spec["p_threshold"] / T
    f_crit, theta = theta_of(alpha_cell, len(counts), N)
    out = dict(x=x, x64=x.astype(np.float64), table=table, counts=counts, k=len(counts), alpha_cell=alpha_cell, f_crit=f_crit,
               theta=theta, n0=spec.get("n0"), group_index=group_index)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def expected(name):
    """(mask, runs, p_channel, p_max) of a named case from the oracle; computed once."""
    c = case(name)
    mask = exceed_ref(c["x64"], c["table"], c["counts"], c["theta"])
    runs = runs_ref(mask)
    return (mask, runs) + p_values_ref(runs)
