"""Rolling z-score (mirror of reference preprocess/signal/rolling_zscore.py:5-51): pandas
``rolling(window, min_periods=1)`` mean and sample std (ddof=1) per channel; float64 out.

``method`` (default ``window``) selects the kernel.  ``window`` gives every output a walk over its own window, O(W) per
sample.  ``blocked`` builds every window from per-tile moments kept as (hi, lo) pairs, O(1) per sample, where
min(window, T) >= 256; smaller windows run on the window kernel under either setting and keep its bits."""
import torch

from ... import _lib
from ..._lib import check, ptr
from ._common import ret, stream, to_device

METHODS = ("window", "blocked")
BLOCKED_TILE = 256            # outputs per workgroup; the smallest window the blocked route takes


def run(data, params: object):
    window_length = getattr(params, "window_length", 10)
    window_size = int(window_length * params.signal_freq)
    preserve_nans = getattr(params, "preserve_nans", True)
    method = getattr(params, "method", "window")
    if method not in METHODS:
        raise ValueError(f"rolling_zscore: method must be 'window' or 'blocked' (got {method!r})")
    if window_size <= 1:
        raise ValueError("window_size must be greater than 1.")
    x, was_np = to_device(data, "rolling_zscore")
    C, T = x.shape
    y = torch.empty(C, T, dtype=torch.float64, device=x.device)
    if method == "blocked" and min(window_size, T) >= BLOCKED_TILE:
        work = torch.empty(8 * C * ((T + BLOCKED_TILE - 1) // BLOCKED_TILE), dtype=torch.float64, device=x.device)
        check(_lib.load().tl_rolling_zscore_blocked(ptr(x), int(x.dtype == torch.float64), ptr(y), ptr(work), work.numel(),
                                                    C, T, window_size, int(not preserve_nans), stream()),
              "tl_rolling_zscore_blocked")
    else:
        check(_lib.load().tl_rolling_zscore(ptr(x), int(x.dtype == torch.float64), ptr(y), C, T, window_size,
                                            int(not preserve_nans), stream()), "tl_rolling_zscore")
    return ret(y, was_np)
