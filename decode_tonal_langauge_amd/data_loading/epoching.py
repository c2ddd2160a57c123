"""Window extraction on the device: ``out[i, c, :] = recording[c, s_i : s_i + L]`` for a table of starts, ONE
``tl_extract_windows`` launch (``csrc/tonal_loader.hip``).

Three loops of the reference are this one operation: the event windows and the rest segments of
``data_loading/text_align.py: extract_ecog_audio`` and the sliding windows of
``data_loading/dataloaders.py: collect_unlabelled_samples``.  ``tl_gather_rows`` cannot do it: it picks whole samples by
index and takes its access width from alignments that hold for every unit; a window starts at an arbitrary sample.

``plan_starts``      host half: times in seconds -> first samples and the window length, truncated where the reference truncates.
``extract_windows``  device half: recording (C, T) + starts -> (n, C, L).  No CPU fallback.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np

from .. import _lib

#: bit of the error word that ``tl_extract_windows`` sets for a window outside the recording (include/tonal_hip.h)
BAD_WINDOW = 2


def plan_starts(times: Sequence[float], sf, length_s: float, n_samples: Optional[int] = None) -> Tuple[np.ndarray, int]:
    """``(starts int64 (n,), L)`` with ``starts[i] = int(times[i] * sf)`` and ``L = int(length_s * sf)``.

    ``sf`` is the NumPy scalar as loaded from the recording file: each product is the float64 product the reference forms
    (``row['start'] * sampling_rate``), so the truncation falls where the reference's falls.  With ``n_samples`` a window that
    starts before the recording or passes its end raises ``ValueError`` naming the window."""
    starts = np.array([int(t * sf) for t in times], dtype=np.int64).reshape(-1)
    length = int(length_s * sf)
    if n_samples is not None:
        if length < 1 or length > n_samples:
            raise ValueError(f"plan_starts: window length {length} samples ({length_s} s at {sf} Hz) does not fit a "
                             f"recording of {n_samples} samples")
        for i, s in enumerate(starts.tolist()):
            if s < 0 or s + length > n_samples:
                raise ValueError(f"plan_starts: window {i} (time {times[i]} s) covers samples [{s}, {s + length}) of a "
                                 f"recording of {n_samples} samples")
    return starts, length


def to_recording(recording, what: str = "extract_windows"):
    """A (C, T) recording as a CUDA tensor whose last dimension is contiguous: a NumPy array is uploaded once, a CUDA tensor
    is taken as it is (any row stride)."""
    rec, _ = _lib.to_gpu(recording, what, floats=False, rows="strided")
    if rec.dim() != 2:
        raise ValueError(f"{what}: the recording must be (n_channels, n_timepoints), got shape {tuple(rec.shape)}")
    if rec.element_size() not in (1, 2, 4, 8) or rec.is_complex():
        raise ValueError(f"{what}: dtype {rec.dtype} is not a 1-, 2-, 4- or 8-byte element")
    if rec.shape[0] < 1 or rec.shape[1] < 1:
        raise ValueError(f"{what}: empty recording of shape {tuple(rec.shape)}")
    return rec


def launch_extract(rec, starts_dev, length: int, out, err) -> None:
    """The bare launch on the current stream: nothing is read back.  ``starts_dev`` int64 CUDA vector, ``out`` (n, C, L)
    contiguous, ``err`` int32 CUDA word (bit ``BAD_WINDOW`` is ORed in for a window outside the recording)."""
    import torch
    C_, T = rec.shape
    ld = rec.stride(0) if C_ > 1 else T
    with torch.cuda.device(rec.device):
        _lib.check(_lib.load().tl_extract_windows(rec.data_ptr(), C_, T, ld, starts_dev.data_ptr(), starts_dev.numel(),
                                                  int(length), rec.element_size(), out.data_ptr(), err.data_ptr(),
                                                  _lib.stream_ptr()), "tl_extract_windows")


def extract_windows(recording, starts, length: int, out=None, check: bool = True):
    """``(n, C, length)`` of the recording's dtype on its device: ``out[i, c, :] = recording[c, starts[i] : starts[i] + length]``.

    ``recording``  CUDA tensor (C, T) of any 1-, 2-, 4- or 8-byte dtype, last dimension contiguous, any row stride; a NumPy
                   array is uploaded once.  ``RuntimeError`` where no GPU is visible.
    ``starts``     a sequence, a NumPy array or an int64 CUDA tensor.
    ``out``        optional destination, contiguous, of that shape, dtype and device.
    ``check``      the error word is read once after the launch (the one host synchronisation) and a window outside the
                   recording raises ``IndexError`` naming the first offending window; its destination is left unwritten.
                   ``False``: nothing is read back - for starts that were validated on the host (``plan_starts``)."""
    import torch
    rec = to_recording(recording)
    length = int(length)
    C_, T = rec.shape
    if isinstance(starts, torch.Tensor):
        if starts.dtype != torch.int64 or starts.dim() != 1:
            raise ValueError("extract_windows: a tensor of starts must be an int64 vector")
        st = starts.to(rec.device).contiguous()
    else:
        host = np.asarray(starts)
        if host.size and not np.issubdtype(host.dtype, np.integer):
            raise ValueError(f"extract_windows: starts must be integers, got dtype {host.dtype}")
        # from pinned memory and asynchronous: the launch below is ordered behind the copy on the stream, and the host does
        # not wait for either
        st = torch.from_numpy(np.ascontiguousarray(host.reshape(-1).astype(np.int64)))
        st = st.pin_memory().to(rec.device, non_blocking=True) if st.numel() else st.to(rec.device)
    n = st.numel()
    if length < 1 or length > T:
        raise ValueError(f"extract_windows: window length {length} does not fit a recording of {T} samples")
    if out is None:
        out = torch.empty((n, C_, length), dtype=rec.dtype, device=rec.device)
    elif (tuple(out.shape) != (n, C_, length) or out.dtype != rec.dtype or out.device != rec.device
          or not out.is_contiguous()):
        raise ValueError(f"extract_windows: out must be a contiguous {rec.dtype} tensor of shape {(n, C_, length)} on "
                         f"{rec.device}")
    if n == 0:
        return out
    err = torch.zeros(1, dtype=torch.int32, device=rec.device)
    launch_extract(rec, st, length, out, err)
    if check and int(err.item()):                          # the one read
        host = st.cpu().numpy()
        bad = np.flatnonzero((host < 0) | (host > T - length))
        first = int(bad[0]) if bad.size else -1
        raise IndexError(f"extract_windows: window {first} (start {int(host[first])}, length {length}) lies outside the "
                         f"recording of {T} samples; {bad.size} such window(s) were not written")
    return out
