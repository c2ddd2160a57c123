"""Launch plumbing shared by the host engines: the only place that fills ``NtParams`` / ``TnParams`` and calls
``tl_permute_reduce``, plus the cache of packed weights and the HIP-event timers.  Everything launches on torch's current
stream, looked up per launch unless the caller hands over the one it has read (``stream=``)."""
from __future__ import annotations

import ctypes as C

import torch

from ._lib import NtParams, TnParams, check, ptr

# bm = 256 (8-wave workgroups) exists but measured slower than two independent 4-wave workgroups per CU (conv2 fwd 127 vs
# 129, dgrad 114 vs 124 TFLOP/s): not selected.
_NT_DEFAULTS = dict(splitk=1, bm=128, J=1, Tp=1, slope=0.0)
_TN_DEFAULTS = dict(splitk=1, J=1, Tp=1, Tvalid=1)
_NT_FIELDS = frozenset(name for name, _ in NtParams._fields_)
_TN_FIELDS = frozenset(name for name, _ in TnParams._fields_)


def r4(n: int) -> int:
    return (n + 3) // 4 * 4


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _launch(lib, fn, struct, names, defaults, fields, stream, *group) -> None:
    """``group``: nothing, or the member count, the member strides and the mask of a ``_group`` entry.  ``stream``: the stream
    to launch on where the caller has read it already (an engine reads it once a pass), None: torch's current stream."""
    if not names.issuperset(fields):       # (a ctypes.Structure takes any attribute: a misspelt field would reach the kernel as 0)
        raise TypeError(f"{struct.__name__} has no field {', '.join(sorted(set(fields) - names))}")
    p = struct(**{**defaults, **fields})
    check(getattr(lib, fn)(C.byref(p), *group, _stream() if stream is None else stream), fn)


def launch_nt(lib, fn: str = "tl_gemm_nt_window", *, stream=None, **fields) -> None:
    """One NT windowed-GEMM launch (fields of ``NtParams`` by keyword; the rest: splitk = J = Tp = 1, bm = 128, else 0)."""
    _launch(lib, fn, NtParams, _NT_FIELDS, _NT_DEFAULTS, fields, stream)


def launch_nt_group(lib, members: int, s_A: int, s_Bw: int, s_bias: int, s_out: int, active, /, stream=None, **fields) -> None:
    """``launch_nt`` for ``members`` members (positional: ``M`` is a field, the rows of one member): the fields describe member
    0, member m lies ``s_*`` elements behind it (``tl_gemm_nt_window_group``; ``active``: the device mask words or None)."""
    _launch(lib, "tl_gemm_nt_window_group", NtParams, _NT_FIELDS, _NT_DEFAULTS, fields, stream, members, s_A, s_Bw, s_bias, s_out,
            ptr(active))


def launch_nt_group_fc(lib, members: int, s_A: int, s_Bw: int, s_bias: int, s_aux: int, s_out: int, active, /, stream=None,
                       **fields) -> None:
    """``launch_nt_group`` on ``tl_gemm_nt_window_group_fc``: the entry of the small fully connected layers, whose ``aux``
    operand (MASK epilogue) has a member stride too and whose split-K slabs lie inside a member's ``s_out``."""
    _launch(lib, "tl_gemm_nt_window_group_fc", NtParams, _NT_FIELDS, _NT_DEFAULTS, fields, stream, members, s_A, s_Bw, s_bias, s_aux,
            s_out, ptr(active))


def launch_tn(lib, fn: str = "tl_gemm_tn_window", *, stream=None, **fields) -> None:
    """One TN windowed-GEMM launch (fields of ``TnParams`` by keyword; the rest: splitk = J = Tp = Tvalid = 1, else 0)."""
    _launch(lib, fn, TnParams, _TN_FIELDS, _TN_DEFAULTS, fields, stream)


def launch_tn_group(lib, members: int, s_A: int, s_B: int, s_slab: int, s_colsum: int, active, /, stream=None, **fields) -> None:
    """``launch_tn`` for ``members`` members (``tl_gemm_tn_window_group``: the short-reduction kernel only): the fields describe
    member 0, member m lies ``s_*`` elements behind it; ``active``: the device mask words or None."""
    _launch(lib, "tl_gemm_tn_window_group", TnParams, _TN_FIELDS, _TN_DEFAULTS, fields, stream, members, s_A, s_B, s_slab, s_colsum,
            ptr(active))


def permute_reduce(lib, src, dst, dims, strides, lims=None, nz=1, zs=0, src_off=0, bias=None, stream=None) -> None:
    """dst = (sum over ``nz`` slabs ``zs`` floats apart of) a 4-d strided view of ``src`` from float ``src_off`` on (+ bias)."""
    d = (C.c_int64 * 4)(*dims)
    s = (C.c_int64 * 4)(*strides)
    l = (C.c_int64 * 4)(*(lims if lims is not None else dims))
    check(lib.tl_permute_reduce(src.data_ptr() + 4 * src_off, dst.data_ptr(), d, s, l, nz, zs, ptr(bias),
                                _stream() if stream is None else stream),
          "tl_permute_reduce")


class PackCache:
    """Packed copies of weights, each rebuilt when a tensor it was made from was written to or replaced: the key is
    ``(_version, data_ptr())`` of every one of them.  Torch's in-place operations and ``FusedNAdam`` both move ``_version``
    (of the parameter and its ``.detach()`` - ``.data`` has a counter of its own and never shows a write), so an engine
    needs no word from whoever updated the weights."""

    def __init__(self):
        self._packed = {}

    def get(self, key, params, build, into=None):
        """The pack ``key`` of ``params`` (a tensor or a tuple of them): ``build()`` makes it; with ``into`` a stale pack is
        kept and ``into(pack)`` fills it again (``build()`` then only allocates: ``into`` fills the first one too)."""
        params = params if isinstance(params, tuple) else (params,)
        ver = tuple((p._version, p.data_ptr()) for p in params)
        hit = self._packed.get(key)
        if hit is None or hit[0] != ver:
            pack = build() if hit is None or into is None else hit[1]
            if into is not None:
                into(pack)
            hit = self._packed[key] = (ver, pack)
        return hit[1]


class LaunchTimers:
    """Per-launch HIP-event timing (bench.py roofline leg).  Events are recorded on the stream the kernels are launched on
    (torch's current stream)."""
    timers = None

    def enable_timers(self, on: bool = True):
        self.timers = {} if on else None

    def _tick(self, name):
        if self.timers is None or name is None:
            return None
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        self.timers.setdefault(name, []).append(ev)
        ev[0].record()
        return ev

    def timer_summary(self):
        """{name: (launches, mean ms)} - synchronises."""
        torch.cuda.synchronize()
        out = {}
        for k, evs in (self.timers or {}).items():
            ms = [a.elapsed_time(b) for a, b in evs]
            out[k] = (len(ms), sum(ms) / max(len(ms), 1))
        return out
