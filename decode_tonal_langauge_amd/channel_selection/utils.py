"""Helpers of the channel selectors (mirror of reference channel_selection/utils.py:4-76) and the device entry points.

``get_max_length`` / ``find_significant_channels`` are host NumPy with the reference's behaviour.  ``anova_oneway`` is the
low-level entry to the kernels of ``csrc/tonal_anova.hip``: a one-way ANOVA (``scipy.stats.f_oneway`` along axis 0) at every
trailing position of the samples, F and p computed on the device in float64.  ``max_run_below`` is the device form of
``get_max_length`` over the rows of a p-value array.  ``permutation_table`` / ``permutation_runs`` / ``permutation_p_values``
are the label-permutation test of the longest significant run (``tl_perm_exceed``, ``tl_perm_runs``).  The input checks
(``rest_erp_inputs``, ``labelled_inputs``), the dispatch on the ``test`` key (``group_test``) and the run rule
(``channels_by_run``) that the selectors share live here too.  No CPU fallback: without a GPU the device entries raise."""
from __future__ import annotations

import ctypes as C
from typing import Mapping, Optional, Sequence, Tuple

import numpy as np

#: below this many columns per launch the samples of a group are split over gridDim.y to fill the chip (at 153 600 columns one
#: slab measured 1 - 2 % faster than two, four or eight: scripts/bench_channel_selection.py)
_FILL_COLUMNS = 1 << 16


def get_max_length(indices: np.ndarray) -> int:
    """Longest stretch of consecutive integers in the sorted, non-empty ``indices``."""
    indices = np.asarray(indices)
    if indices.size == 0:
        raise IndexError("get_max_length: empty index array")            # the reference fails on indices[0]
    breaks = np.flatnonzero(np.diff(indices) != 1)
    edges = np.concatenate(([-1], breaks, [len(indices) - 1]))
    return int(np.diff(edges).max())


def find_significant_channels(p_values: np.ndarray, pvalue_threshold: float = 0.05, length_threshold: int = 10):
    """Channels whose longest run of ``p < pvalue_threshold / n_timepoints`` (Bonferroni) is strictly longer than
    ``length_threshold``.  Returns ``(significant_channels, max_lengths)``; as in the reference ``max_lengths`` is never
    filled and comes back empty."""
    below = np.asarray(p_values) < pvalue_threshold / p_values.shape[1]                # NaN compares false
    keep = [ch for ch, row in enumerate(below) if row.any() and get_max_length(np.flatnonzero(row)) > length_threshold]
    return keep, []


def lookup(data, key: str, kind: str):
    """``data[key]``, or the reference's KeyError: ``kind`` is "Recording" or "Labels"."""
    if key not in data:
        raise KeyError(f"{kind} '{key}' not found in data.Available keys: {list(data.keys())}")
    return data[key]


# ---- the selectors' input checks: the reference's, with its messages ---------------------------------------------------
_NO_SF = "ECoG sampling frequency (ecog_sf) not found in the data."


def rest_erp_inputs(data: Mapping, params: dict):
    """The checks of the rest-against-ERP form (reference active.py): ``(rest name, ERP name, rest, erp)``, the recordings
    as ``data`` holds them.  One check goes beyond the reference, which fails inside scipy on such a pair: recordings with
    different numbers of timepoints are refused here, before anything is uploaded."""
    erp_name, rest_name = params.get('erp_name', 'ecog'), params.get('rest_name', 'ecog_rest')
    if "ecog_sf" not in data:
        raise ValueError(_NO_SF)
    rest = lookup(data, rest_name, "Recording")
    erp = lookup(data, erp_name, "Recording")
    if erp.shape[1:2] != rest.shape[1:2]:
        raise ValueError(f"Shape mismatch between '{erp_name}' and '{rest_name}': {erp.shape[1:2]} vs {rest.shape[1:2]}.")
    if erp.shape[2:] != rest.shape[2:]:
        raise ValueError(f"'{erp_name}' and '{rest_name}' must have the same number of timepoints: "
                         f"{erp.shape[2:]} vs {rest.shape[2:]}.")
    return rest_name, erp_name, rest, erp


def labelled_inputs(data: Mapping, params: dict, need_sf: bool = True):
    """The checks of the labelled form (reference discriminative.py:122-164): ``(recording name, recording, labels)`` with
    the labels a 1D integer array, one per sample.  ``need_sf`` asks for the key ``<recording>_sf`` first."""
    name = params.get('recording_name', 'ecog')
    target = params['target']
    if need_sf and f"{name}_sf" not in data:
        raise ValueError(_NO_SF)
    series = lookup(data, name, "Recording")
    if series.ndim != 3:
        raise ValueError(f"Recording '{name}' must be a 3D array (n_samples, n_channels, n_timepoints).")
    labels = np.asarray(lookup(data, target, "Labels")).squeeze()
    if labels.ndim != 1:
        raise ValueError(f"Labels '{target}' must be a 1D array (n_samples,) or 2D array with shape (1, n_samples)"
                         " or (n_samples, 1).")
    n_labels, n_samples = labels.shape[0], series.shape[0]
    if n_labels != n_samples:
        raise ValueError(f"Number of samples in '{target}' ({n_labels}) does not match number of samples in "
                         f"'{name}' ({n_samples}).")
    if not np.issubdtype(labels.dtype, np.integer):
        raise ValueError(f"Labels for '{target}' must be integers.")
    return name, series, labels


# ---- device side ---------------------------------------------------------------------------------------------------
def to_device(a, what: str):
    """NumPy array -> CUDA tensor (uploaded, float32 / float64 kept, anything else becomes float64); CUDA tensor -> itself."""
    from .. import _lib
    return _lib.to_gpu(a, what)[0]


def device_recording(data, name: str, what: str):
    """The recording ``data[name]`` on the GPU.  The stage hands the selectors a mapping with a ``device(name)`` method that
    uploads a recording once per subject; a plain dict / NpzFile is uploaded here."""
    getter = getattr(data, "device", None)
    if callable(getter):
        return getter(name)
    return to_device(data[name], what)


def promote(tensors: Sequence) -> list:
    """The tensors as they are where their dtypes agree, all of them widened to float64 where not."""
    tensors = list(tensors)
    if len({t.dtype for t in tensors}) > 1:
        tensors = [t.double() for t in tensors]
    return tensors


def _sample_arrays(arrays: Sequence, what: str, ndim: Optional[int] = None) -> list:
    """One or two CUDA tensors whose samples follow each other, checked and made contiguous: one trailing shape, dtype
    (float32 or float64) and device.  Any trailing shape passes; ``ndim=3`` asks for (n, C, T)."""
    import torch
    from .. import _lib
    arrays = list(arrays)
    if not 1 <= len(arrays) <= 2:
        raise ValueError(f"{what}: one or two sample arrays")
    x0 = arrays[0]
    shape = "must share trailing shape" if ndim is None else "must be (n, C, T) of one trailing shape"
    for a in arrays:
        _lib.require_gpu(a, what)
        bad_rank = a.dim() < 1 if ndim is None else a.dim() != ndim
        if bad_rank or a.shape[1:] != x0.shape[1:] or a.dtype != x0.dtype or a.device != x0.device:
            raise ValueError(f"{what}: arrays {shape}, dtype and device")
    if x0.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"{what}: float32 or float64 samples")
    return [a.contiguous() for a in arrays]


def _splits(cols: int, n_min: int) -> int:
    return int(max(1, min(-(-_FILL_COLUMNS // cols), n_min, 1024)))


def _group_counts(what: str, index_lists: Sequence[np.ndarray], trailing: Sequence[int] = ()) -> list:
    """The sizes of between 2 and 64 groups of at least one sample each, in columns of a non-empty ``trailing`` shape."""
    k = len(index_lists)
    if not 2 <= k <= 64:
        raise ValueError(f"{what}: needs between 2 and 64 groups, got {k}")
    counts = [int(len(ix)) for ix in index_lists]
    if min(counts) < 1 or not all(trailing):
        raise ValueError(f"{what}: every group needs at least one sample and one column")
    return counts


def _group_test(finalize: str, arrays: Sequence, index_lists: Sequence[np.ndarray], counts: Sequence[int]):
    """``(statistic, p)``, float64 CUDA tensors of the trailing shape: ``tl_group_moments`` once per group ``g`` over the rows
    ``index_lists[g]`` (``counts[g]`` of them) of ``arrays[g]``, then the entry point ``finalize``.  ``arrays`` are contiguous
    CUDA tensors (n_g_rows, ...) of one dtype, trailing shape and device."""
    import torch
    from .. import _lib
    from .._lib import check, ptr, stream_ptr
    x0, k = arrays[0], len(counts)
    trailing = tuple(x0.shape[1:])
    cols = int(np.prod(trailing, dtype=np.int64))
    lib = _lib.load()
    splits = _splits(cols, min(counts))
    sums = torch.empty(2, k, splits, cols, dtype=torch.float64, device=x0.device)
    idx = torch.from_numpy(np.concatenate([np.asarray(ix, dtype=np.int32) for ix in index_lists])).to(x0.device)
    is_f64 = int(x0.dtype == torch.float64)
    # one row of the first array for every group: the sums share a frame
    shift = x0.data_ptr() + int(index_lists[0][0]) * cols * x0.element_size()
    off = 0
    with torch.cuda.device(x0.device):
        for g, a in enumerate(arrays):
            check(lib.tl_group_moments(ptr(a), is_f64, a.shape[0], cols, idx.data_ptr() + 4 * off, counts[g], shift, splits,
                                       ptr(sums[0, g]), ptr(sums[1, g]), stream_ptr()), "tl_group_moments")
            off += counts[g]
        out = torch.empty(2, cols, dtype=torch.float64, device=x0.device)
        cnt = (C.c_int32 * k)(*counts)
        check(getattr(lib, finalize)(ptr(sums[0]), ptr(sums[1]), cnt, k, splits, cols, ptr(out[0]), ptr(out[1]), stream_ptr()),
              finalize)
    return out[0].reshape(trailing), out[1].reshape(trailing)


def anova_device(arrays: Sequence, index_lists: Sequence[np.ndarray]):
    """F and p (float64 CUDA tensors of the trailing shape) of the groups ``arrays[g][index_lists[g]]``.  ``arrays`` are
    CUDA tensors (n_g_rows, ...) of one dtype and one trailing shape - the same tensor k times for a labelled recording."""
    counts = _group_counts("anova_oneway", index_lists, tuple(arrays[0].shape[1:]) if len(arrays) else ())
    x0 = arrays[0]
    for a in arrays:
        if a.shape[1:] != x0.shape[1:] or a.dtype != x0.dtype or a.device != x0.device:
            raise ValueError("anova_oneway: groups must share trailing shape, dtype and device")
    return _group_test("tl_anova_finalize", arrays, index_lists, counts)


# ---- rank form: Kruskal-Wallis ---------------------------------------------------------------------------------------
#: most samples tl_rank_columns sorts in one column (RK_MAX_N of csrc/tonal_anova.hip)
RANK_MAX_SAMPLES = 8192
#: most LDS of one block of tl_rank_columns (RK_LDS_BYTES), of a tile of several columns (RK_TILE_BYTES), its widest tile (RK_MAX_TW)
_RANK_LDS_BYTES, _RANK_TILE_BYTES, _RANK_MAX_TILE = 81920, 40960, 64
STATISTICS = ("anova", "kruskal")


def check_statistic(value, key: str = "statistic") -> str:
    if value not in STATISTICS:
        raise ValueError(f"Unknown {key} '{value}': expected one of {list(STATISTICS)}.")
    return value


def rank_tile_columns(n: int, is_f64: bool) -> int:
    """Columns a block of ``tl_rank_columns`` sorts for ``n`` samples: the entry point's rule, restated for tests and the
    bench script."""
    npad = max(2, 1 << (int(n) - 1).bit_length())
    per = npad * (10 if is_f64 else 6)
    tile = 1
    while tile < _RANK_MAX_TILE and per * tile * 2 <= _RANK_TILE_BYTES:
        tile *= 2
    return tile


def rank_columns_device(arrays: Sequence):
    """Midranks (N, ...) float32 on the device of one CUDA tensor (N, ...) or of two whose samples follow each other."""
    import torch
    from .. import _lib
    from .._lib import check, ptr, stream_ptr
    arrays = _sample_arrays(arrays, "rank_columns")
    x0 = arrays[0]
    n0, n1 = int(x0.shape[0]), int(arrays[1].shape[0]) if len(arrays) == 2 else 0
    cols = int(np.prod(tuple(x0.shape[1:]), dtype=np.int64))
    if n0 < 1 or cols < 1 or (len(arrays) == 2 and n1 < 1):
        raise ValueError("rank_columns: every array needs at least one sample and one column")
    if n0 + n1 > RANK_MAX_SAMPLES:
        raise ValueError(f"rank_columns: at most {RANK_MAX_SAMPLES} samples (got {n0 + n1})")
    ranks = torch.empty((n0 + n1,) + tuple(x0.shape[1:]), dtype=torch.float32, device=x0.device)
    with torch.cuda.device(x0.device):
        check(_lib.load().tl_rank_columns(ptr(arrays[0]), n0, ptr(arrays[1]) if n1 else None, n1,
                                          int(x0.dtype == torch.float64), cols, ptr(ranks), stream_ptr()), "tl_rank_columns")
    return ranks


def rank_columns(x, x1=None):
    """``scipy.stats.rankdata(x, method='average', axis=0)`` as float32 (a midrank is a multiple of 0.5): the rank of every
    sample within its column, ties sharing the mean of their positions.  With ``x1`` the samples of both arrays are ranked
    as one, ``x`` first.  ``-0.0`` and ``+0.0`` tie, infinities rank as values, a column that holds a NaN is NaN throughout;
    float64 input is ranked on its float64 values.  At most ``RANK_MAX_SAMPLES`` samples.  NumPy in, NumPy out; CUDA
    tensors stay on the device."""
    import torch
    given = [x] if x1 is None else [x, x1]
    on_device = all(isinstance(a, torch.Tensor) for a in given)
    n = sum(int(a.shape[0]) for a in given)
    if n > RANK_MAX_SAMPLES:                                   # before anything is uploaded
        raise ValueError(f"rank_columns: at most {RANK_MAX_SAMPLES} samples (got {n})")
    ranks = rank_columns_device(promote(to_device(a, "rank_columns") for a in given))
    return ranks if on_device else ranks.cpu().numpy()


def kruskal_device(arrays: Sequence, index_lists: Sequence[np.ndarray]):
    """H and p (float64 CUDA tensors of the trailing shape) of the Kruskal-Wallis test between the groups ``index_lists``:
    row numbers into the samples of ``arrays``, one CUDA tensor or two that follow each other.  Every sample belongs to
    exactly one group.  ``tl_rank_columns`` once, ``tl_group_moments`` per group on the ranks, ``tl_kruskal_finalize``."""
    counts = _group_counts("kruskal_oneway", index_lists)
    n = sum(int(a.shape[0]) for a in arrays)
    members = np.concatenate([np.asarray(ix, dtype=np.int64) for ix in index_lists])
    if members.size != n or not np.array_equal(np.sort(members), np.arange(n)):
        raise ValueError("kruskal_oneway: the groups must hold every sample exactly once")
    return _group_test("tl_kruskal_finalize", [rank_columns_device(arrays)] * len(counts), index_lists, counts)


def group_test(test: str, arrays: Sequence, classes: Optional[Sequence[np.ndarray]] = None):
    """``(statistic, p)`` of ``test`` on the device: F of the ANOVA or H of the Kruskal-Wallis test, float64 CUDA tensors of
    the trailing shape.  Without ``classes`` every CUDA tensor of ``arrays`` is one group (rest and ERP); with them ``arrays``
    holds one tensor and ``classes`` the row numbers of each of its groups."""
    import torch
    arrays = list(arrays)
    if classes is None:
        sizes = [int(a.shape[0]) for a in arrays]
        starts = np.cumsum([0] + sizes[:-1]) if test == "kruskal" else [0] * len(sizes)     # the ranks' rows count through
        classes = [np.arange(s, s + n, dtype=np.int32) for s, n in zip(starts, sizes)]
        if test == "kruskal" and len(arrays) > 2:
            arrays = [torch.cat(arrays)]                   # the ranks are those of the pooled sample
    elif test == "anova":
        arrays = arrays * len(classes)
    return (kruskal_device if test == "kruskal" else anova_device)(arrays, classes)


def _oneway(test: str, groups_or_array, labels, limit: Optional[int] = None) -> Tuple:
    """The two calling forms of ``anova_oneway`` / ``kruskal_oneway``: upload, common dtype, groups, test, and NumPy back
    unless every sample array came as a tensor.  More than ``limit`` samples are refused before anything is uploaded."""
    import torch
    what = f"{test}_oneway"
    given = list(groups_or_array) if labels is None else [groups_or_array]
    on_device = all(isinstance(g, torch.Tensor) for g in given)
    if limit is not None:
        n = sum(int(g.shape[0]) for g in given)
        if n > limit:
            raise ValueError(f"{what}: at most {limit} samples (got {n})")
    arrays = promote(to_device(g, what) for g in given)
    classes = None
    if labels is not None:
        lab = labels.detach().cpu().numpy() if isinstance(labels, torch.Tensor) else np.asarray(labels)
        lab = lab.squeeze()
        if lab.ndim != 1 or lab.shape[0] != arrays[0].shape[0]:
            raise ValueError(f"{what}: {arrays[0].shape[0]} samples but labels of shape {lab.shape}")
        classes = [np.flatnonzero(lab == v).astype(np.int32) for v in np.unique(lab)]
    stat, p = group_test(test, arrays, classes)
    if on_device:
        return stat, p
    return stat.cpu().numpy(), p.cpu().numpy()


def anova_oneway(groups_or_array, labels=None) -> Tuple:
    """One-way ANOVA along axis 0 at every trailing position: ``(F, p)`` as ``scipy.stats.f_oneway`` defines them.

    ``anova_oneway([g0, g1, ...])`` takes one array ``(n_g, ...)`` per group; ``anova_oneway(x, labels)`` takes one array
    ``(n, ...)`` and an integer label per sample (groups in the order of ``np.unique(labels)``).  NumPy arrays are uploaded
    and the result comes back as NumPy; CUDA tensors are used in place and the result stays on the device.  float32 input
    is read as it is and widened in registers; every sum and the p-value are float64."""
    return _oneway("anova", groups_or_array, labels)


def kruskal_oneway(groups_or_array, labels=None) -> Tuple:
    """Kruskal-Wallis H-test along axis 0 at every trailing position: ``(H, p)`` as ``scipy.stats.kruskal`` defines them
    (tie-corrected H, chi-square tail with k - 1 degrees of freedom), float64.

    The calling forms and return conventions of ``anova_oneway``: one array per group, or one array and a label per
    sample.  A column whose values are all identical gives NaN (scipy raises there), as does a column that holds a NaN.
    At most ``RANK_MAX_SAMPLES`` samples in all."""
    return _oneway("kruskal", groups_or_array, labels, limit=RANK_MAX_SAMPLES)


def max_run_below(p, threshold: float):
    """Per row of the CUDA float64 tensor ``p (C, T)``: ``(count, longest_run)`` of ``p < threshold`` as int32 CUDA tensors -
    ``get_max_length(np.where(p[c] < threshold)[0])`` for every channel at once (0 where no point is below)."""
    import torch
    from .. import _lib
    from .._lib import check, ptr, stream_ptr
    _lib.require_gpu(p, "max_run_below")
    if p.dim() != 2 or p.dtype != torch.float64:
        raise ValueError("max_run_below: expected a float64 tensor of shape (n_channels, n_timepoints)")
    p = p.contiguous()
    out = torch.empty(2, p.shape[0], dtype=torch.int32, device=p.device)
    with torch.cuda.device(p.device):
        check(_lib.load().tl_max_run_below(ptr(p), p.shape[0], p.shape[1], float(threshold), ptr(out[0]), ptr(out[1]),
                                           stream_ptr()), "tl_max_run_below")
    return out[0], out[1]


def channels_by_run(p, cell_threshold: float, length_threshold: int) -> Tuple[list, list]:
    """``(channels, lengths)`` on the host: the rows of the CUDA p-values ``p (C, T)`` whose longest run of
    ``p < cell_threshold`` is strictly longer than ``length_threshold``, and the length of that run for each of them."""
    count, longest = max_run_below(p, cell_threshold)
    count, longest = count.cpu().numpy(), longest.cpu().numpy()
    channels = [int(ch) for ch in np.flatnonzero((count > 0) & (longest > length_threshold))]
    return channels, [int(longest[ch]) for ch in channels]


# ---- label-permutation test ----------------------------------------------------------------------------------------
#: samples per LDS stage of tl_perm_exceed (PX_KC of csrc/tonal_anova.hip): the tests place sample counts around it
PERM_SAMPLE_CHUNK = 32
#: the exceedance mask of one chunk of relabellings stays below this many bytes (one byte per relabelling and column)
_PERM_MASK_BYTES = 64 << 20


def permutation_table(group_index, n_permutations: int, seed: int = 0) -> np.ndarray:
    """``(1 + n_permutations, N)`` uint8, on the host: row 0 is the observed labelling ``group_index`` (integers in
    [0, k), k <= 64), rows 1.. are ``np.random.default_rng(seed).permutation(group_index)`` drawn in order."""
    g = np.asarray(group_index)
    if g.ndim != 1 or g.size < 1 or not np.issubdtype(g.dtype, np.integer):
        raise ValueError("permutation_table: group_index must be a non-empty 1D integer array")
    if g.min() < 0 or g.max() >= 64:
        raise ValueError("permutation_table: group indices must lie in [0, 64)")
    if n_permutations < 0:
        raise ValueError("permutation_table: n_permutations must not be negative")
    g = g.astype(np.uint8)
    rng = np.random.default_rng(seed)
    table = np.empty((1 + int(n_permutations), g.size), dtype=np.uint8)
    table[0] = g
    for r in range(1, table.shape[0]):
        table[r] = rng.permutation(g)
    return table


def critical_values(p_threshold: float, k: int, n: int, statistic: str = "anova") -> Tuple[float, float]:
    """``(f_crit, theta)`` of the cell level ``p_threshold``: ``p < p_threshold`` is ``F > f_crit`` is
    ``ssb > theta * sst`` with ``theta = f_crit dfb / (dfw + f_crit dfb)``; ``scipy.stats.f.isf`` once, on the host.

    ``statistic="kruskal"``: ``(chi2_crit, theta)`` with ``chi2_crit = scipy.stats.chi2.isf(p_threshold, k - 1)`` and
    ``theta = chi2_crit / (n - 1)``, since ``H = (n - 1) ssb / sst`` of the midranks.  H never exceeds n - 1: a level with
    ``chi2_crit >= n - 1`` can be passed by no cell and raises a ``ValueError``."""
    from scipy import stats
    check_statistic(statistic)
    dfb, dfw = k - 1, n - k
    if dfw < 1:
        raise ValueError(f"permutation test: {n} samples in {k} groups leave no degrees of freedom within the groups")
    if not 0.0 < p_threshold < 1.0:
        raise ValueError(f"permutation test: the cell level must lie in (0, 1), got {p_threshold}")
    if statistic == "kruskal":
        chi2_crit = float(stats.chi2.isf(p_threshold, dfb))
        if chi2_crit >= n - 1:
            raise ValueError(f"permutation test: no cell can reach the level {p_threshold} with {n} samples in {k} groups: "
                             f"H is at most {n - 1}, the level needs H > {chi2_crit:.6g}")
        return chi2_crit, chi2_crit / (n - 1)
    f_crit = float(stats.f.isf(p_threshold, dfb, dfw))
    return f_crit, f_crit * dfb / (dfw + f_crit * dfb)


def _perm_masks(arrays, table, counts, p_threshold, perm_chunk, statistic):
    """The work shared by ``permutation_runs`` and ``permutation_exceedances``: the checks, the threshold of every column and
    the upload of the table.  Returns ``(f_crit, theta, (P, C, T), chunks)`` (``critical_values`` of ``statistic``); ``chunks``
    yields ``(p0, p1, mask)`` per chunk of relabellings, ``mask`` (p1 - p0, C * T) uint8 on the device, overwritten by the
    next chunk.  ``"kruskal"`` ranks the samples once - a relabelling does not change them - and runs the same launches on
    the ranks."""
    import torch
    from .. import _lib
    from .._lib import check, ptr, stream_ptr
    check_statistic(statistic)
    arrays = _sample_arrays(arrays, "permutation test", ndim=3)
    x0 = arrays[0]
    Cn, T = int(x0.shape[1]), int(x0.shape[2])
    cols = Cn * T
    N = sum(int(a.shape[0]) for a in arrays)
    table = np.array(table, dtype=np.uint8, order="C")                      # a copy: the upload needs a writable array
    counts = [int(c) for c in counts]
    k = len(counts)
    if table.ndim != 2 or table.shape[0] < 1 or table.shape[1] != N:
        raise ValueError(f"permutation test: the table must be (P, {N}), got {table.shape}")
    if not 2 <= k <= 64 or min(counts) < 1 or sum(counts) != N or cols < 1:
        raise ValueError("permutation test: between 2 and 64 groups of at least one sample each, adding up to the samples")
    f_crit, theta = critical_values(p_threshold, k, N, statistic)
    if statistic == "kruskal":
        arrays = [rank_columns_device(arrays)]                              # (N, C, T) float32
        x0 = arrays[0]
    P = table.shape[0]
    if perm_chunk is None:
        perm_chunk = max(1, _PERM_MASK_BYTES // cols)
        if perm_chunk >= 128:
            perm_chunk -= perm_chunk % 128                   # whole blocks of relabellings for both kernel forms
    perm_chunk = int(perm_chunk)
    if perm_chunk < 1:
        raise ValueError("permutation test: perm_chunk must be at least 1")
    perm_chunk = min(perm_chunk, P)
    lib = _lib.load()
    is_f64 = int(x0.dtype == torch.float64)
    with torch.cuda.device(x0.device):
        # total and sst of the observed data: one tl_group_moments pass over all samples, in the frame of sample 0
        shift = x0[0].reshape(cols)
        S = torch.zeros(cols, dtype=torch.float64, device=x0.device)
        Q = torch.zeros(cols, dtype=torch.float64, device=x0.device)
        for a in arrays:
            n = int(a.shape[0])
            splits = _splits(cols, n)
            sums = torch.empty(2, splits, cols, dtype=torch.float64, device=x0.device)
            idx = torch.arange(n, dtype=torch.int32, device=x0.device)
            check(lib.tl_group_moments(ptr(a), is_f64, n, cols, ptr(idx), n, ptr(shift), splits, ptr(sums[0]), ptr(sums[1]),
                                       stream_ptr()), "tl_group_moments")
            S += sums[0].sum(dim=0)
            Q += sums[1].sum(dim=0)
        mean_sq = S * S / N
        tau = (theta * (Q - mean_sq) + mean_sq).contiguous()          # theta sst + total^2 / N
        labels = torch.from_numpy(table).to(x0.device)
    cnt = (C.c_int32 * k)(*counts)
    x1 = arrays[1] if len(arrays) == 2 else None

    def chunks():
        with torch.cuda.device(x0.device):
            mask = torch.empty(perm_chunk, cols, dtype=torch.uint8, device=x0.device)
            for p0 in range(0, P, perm_chunk):
                p1 = min(P, p0 + perm_chunk)
                check(lib.tl_perm_exceed(ptr(x0), x0.shape[0], ptr(x1), 0 if x1 is None else x1.shape[0], is_f64, cols,
                                         ptr(shift), labels.data_ptr() + p0 * N, p1 - p0, cnt, k, ptr(tau), ptr(mask),
                                         stream_ptr()), "tl_perm_exceed")
                yield p0, p1, mask[:p1 - p0]
    return f_crit, theta, (P, Cn, T), chunks()


def permutation_runs(arrays: Sequence, table, counts: Sequence[int], p_threshold: float, perm_chunk: Optional[int] = None,
                     statistic: str = "anova"):
    """``(runs, f_crit, theta)``: ``runs (P, C)`` int32 on the device is, per row of ``table`` (``permutation_table``) and
    channel, the longest run of timepoints at which the one-way ANOVA under that labelling has ``p < p_threshold``
    (the CELL level - a selector divides its ``p_threshold`` by T first).

    ``arrays`` is one CUDA tensor (N, C, T) or two, (n0, C, T) and (n1, C, T), whose samples follow each other (rest, then
    ERP); ``counts`` the k group sizes of the observed labelling.  No p-value is evaluated: a relabelling keeps the group
    sizes, so ``p < p_threshold`` is ``sum_g S_g^2 / n_g > theta sst + total^2 / N`` with one host ``scipy.stats.f.isf``.
    The relabellings go through ``tl_perm_exceed`` / ``tl_perm_runs`` in chunks of ``perm_chunk`` (default: a mask of at
    most 64 MiB); the result does not depend on the chunking.

    ``statistic="kruskal"``: the Kruskal-Wallis test in place of the ANOVA, ``(runs, chi2_crit, theta)``.  The samples are
    ranked once (``tl_rank_columns``) and the same path runs on the ranks with ``theta = chi2_crit / (N - 1)``."""
    import torch
    from .. import _lib
    from .._lib import check, ptr, stream_ptr
    lib = _lib.load()
    f_crit, theta, (P, Cn, T), chunks = _perm_masks(arrays, table, counts, p_threshold, perm_chunk, statistic)
    runs = torch.empty(P, Cn, dtype=torch.int32, device=arrays[0].device)
    for p0, p1, mask in chunks:
        check(lib.tl_perm_runs(ptr(mask), (p1 - p0) * Cn, T, ptr(runs[p0:p1]), stream_ptr()), "tl_perm_runs")
    return runs, f_crit, theta


def permutation_exceedances(arrays: Sequence, table, counts: Sequence[int], p_threshold: float,
                            perm_chunk: Optional[int] = None, statistic: str = "anova"):
    """The boolean ``(P, C, T)`` CUDA mask behind ``permutation_runs`` (same arguments): where ``p < p_threshold`` under
    each labelling.  P * C * T bytes: for tests and small inputs."""
    import torch
    _, _, shape, chunks = _perm_masks(arrays, table, counts, p_threshold, perm_chunk, statistic)
    out = torch.empty(shape, dtype=torch.bool, device=arrays[0].device)
    for p0, p1, mask in chunks:
        out[p0:p1] = mask.reshape(out[p0:p1].shape) != 0
    return out


def permutation_p_values(runs):
    """``(p_channel, p_max)``, both (C,) float64 NumPy, from ``runs (P, C)`` with the observed labelling in row 0:
    ``p_channel[c] = (1 + #{pi >= 1: runs[pi, c] >= runs[0, c]}) / P`` and ``p_max[c]`` the same count against the
    relabelling's maximum over the channels (family-wise)."""
    r = runs.detach().cpu().numpy() if hasattr(runs, "detach") else np.asarray(runs)
    if r.ndim != 2 or r.shape[0] < 1:
        raise ValueError("permutation_p_values: runs must be (P, C)")
    P = r.shape[0]
    obs, null = r[0], r[1:]
    p_channel = (1 + (null >= obs[None, :]).sum(axis=0)) / P
    p_max = (1 + (null.max(axis=1, initial=0)[:, None] >= obs[None, :]).sum(axis=0)) / P
    return p_channel.astype(np.float64), p_max.astype(np.float64)
