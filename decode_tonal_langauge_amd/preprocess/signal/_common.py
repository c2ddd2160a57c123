"""Shared host plumbing of the signal steps: NumPy in -> device -> NumPy out, or CUDA tensor in/out (``_lib.to_gpu``)."""
from ... import _lib
from ..._lib import stream_ptr as stream  # noqa: F401  (the name the sibling steps import; one function, _lib's)


def to_device(data, what: str):
    t, was_np = _lib.to_gpu(data, what)
    if t.dim() != 2:
        raise ValueError("expected data of shape (n_channels, n_timepoints)")
    return t, was_np


def ret(t, was_np):
    return t.cpu().numpy() if was_np else t
