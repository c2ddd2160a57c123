"""Helpers of the channel selectors (mirror of reference channel_selection/utils.py:4-76) and the device entry points.

``get_max_length`` / ``find_significant_channels`` are host NumPy with the reference's behaviour.  ``anova_oneway`` is the
low-level entry to the kernels of ``csrc/tonal_anova.hip``: a one-way ANOVA (``scipy.stats.f_oneway`` along axis 0) at every
trailing position of the samples, F and p computed on the device in float64.  ``max_run_below`` is the device form of
``get_max_length`` over the rows of a p-value array.  No CPU fallback: without a GPU both raise."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

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


# ---- device side ---------------------------------------------------------------------------------------------------
def to_device(a, what: str):
    """NumPy array -> CUDA tensor (uploaded, float32 / float64 kept, anything else becomes float64); CUDA tensor -> itself."""
    import torch
    from .. import _lib
    if isinstance(a, torch.Tensor):
        _lib.require_gpu(a, what)
        t = a
    else:
        if not torch.cuda.is_available():
            raise RuntimeError(f"{what} (MI355X build): no GPU visible; this package has no CPU fallback")
        arr = np.asarray(a)
        if arr.dtype not in (np.float32, np.float64):
            arr = arr.astype(np.float64)
        t = torch.from_numpy(np.ascontiguousarray(arr)).to(torch.device("cuda", torch.cuda.current_device()))
    if t.dtype not in (torch.float32, torch.float64):
        t = t.double()
    return t.contiguous()


def _splits(cols: int, n_min: int) -> int:
    return int(max(1, min(-(-_FILL_COLUMNS // cols), n_min, 1024)))


def anova_device(arrays: Sequence, index_lists: Sequence[np.ndarray]):
    """F and p (float64 CUDA tensors of the trailing shape) of the groups ``arrays[g][index_lists[g]]``.  ``arrays`` are
    CUDA tensors (n_g_rows, ...) of one dtype and one trailing shape - the same tensor k times for a labelled recording."""
    import torch
    from .. import _lib
    from .._lib import check, ptr, stream_ptr
    k = len(arrays)
    if not 2 <= k <= 64:
        raise ValueError(f"anova_oneway: needs between 2 and 64 groups, got {k}")
    x0 = arrays[0]
    trailing = tuple(x0.shape[1:])
    cols = int(np.prod(trailing, dtype=np.int64))
    counts = [int(len(ix)) for ix in index_lists]
    if min(counts) < 1 or cols < 1:
        raise ValueError("anova_oneway: every group needs at least one sample and one column")
    for a in arrays:
        if tuple(a.shape[1:]) != trailing or a.dtype != x0.dtype or a.device != x0.device:
            raise ValueError("anova_oneway: groups must share trailing shape, dtype and device")
    lib = _lib.load()
    splits = _splits(cols, min(counts))
    sums = torch.empty(2, k, splits, cols, dtype=torch.float64, device=x0.device)
    idx = torch.from_numpy(np.concatenate([np.asarray(ix, dtype=np.int32) for ix in index_lists])).to(x0.device)
    is_f64 = int(x0.dtype == torch.float64)
    shift_row = int(index_lists[0][0])                 # one row of the data for every group: the sums share a frame
    off = 0
    with torch.cuda.device(x0.device):
        for g, a in enumerate(arrays):
            check(lib.tl_group_moments(ptr(a), is_f64, a.shape[0], cols, idx.data_ptr() + 4 * off, counts[g],
                                       x0.data_ptr() + shift_row * cols * x0.element_size(), splits,
                                       ptr(sums[0, g]), ptr(sums[1, g]), stream_ptr()), "tl_group_moments")
            off += counts[g]
        out = torch.empty(2, cols, dtype=torch.float64, device=x0.device)
        cnt = (C.c_int32 * k)(*counts)
        check(lib.tl_anova_finalize(ptr(sums[0]), ptr(sums[1]), cnt, k, splits, cols, ptr(out[0]), ptr(out[1]),
                                    stream_ptr()), "tl_anova_finalize")
    return out[0].reshape(trailing), out[1].reshape(trailing)


def anova_oneway(groups_or_array, labels=None) -> Tuple:
    """One-way ANOVA along axis 0 at every trailing position: ``(F, p)`` as ``scipy.stats.f_oneway`` defines them.

    ``anova_oneway([g0, g1, ...])`` takes one array ``(n_g, ...)`` per group; ``anova_oneway(x, labels)`` takes one array
    ``(n, ...)`` and an integer label per sample (groups in the order of ``np.unique(labels)``).  NumPy arrays are uploaded
    and the result comes back as NumPy; CUDA tensors are used in place and the result stays on the device.  float32 input
    is read as it is and widened in registers; every sum and the p-value are float64."""
    import torch
    if labels is None:
        groups = list(groups_or_array)
        on_device = all(isinstance(g, torch.Tensor) for g in groups)
        dev = [to_device(g, "anova_oneway") for g in groups]
        if len({d.dtype for d in dev}) > 1:
            dev = [d.double() for d in dev]
        index_lists = [np.arange(d.shape[0], dtype=np.int32) for d in dev]
    else:
        on_device = isinstance(groups_or_array, torch.Tensor)
        x = to_device(groups_or_array, "anova_oneway")
        lab = labels.detach().cpu().numpy() if isinstance(labels, torch.Tensor) else np.asarray(labels)
        lab = lab.squeeze()
        if lab.ndim != 1 or lab.shape[0] != x.shape[0]:
            raise ValueError(f"anova_oneway: {x.shape[0]} samples but labels of shape {lab.shape}")
        index_lists = [np.flatnonzero(lab == v).astype(np.int32) for v in np.unique(lab)]
        dev = [x] * len(index_lists)
    F, p = anova_device(dev, index_lists)
    if on_device:
        return F, p
    return F.cpu().numpy(), p.cpu().numpy()


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


def device_recording(data, name: str, what: str):
    """The recording ``data[name]`` on the GPU.  The stage hands the selectors a mapping with a ``device(name)`` method that
    uploads a recording once per subject; a plain dict / NpzFile is uploaded here."""
    getter = getattr(data, "device", None)
    if callable(getter):
        return getter(name)
    return to_device(data[name], what)
