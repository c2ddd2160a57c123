"""Device-resident batch loader: the dataset is uploaded once, every batch is ONE ``tl_gather_rows`` launch.

The stock loader of ``split_dataset`` indexes the dataset sample by sample in Python and collates with ``torch.stack``; with
CPU tensors each batch is then copied host-to-device from pageable memory inside the train step.  Here the tensors live on
the device, a split and every epoch's order are drawn exactly as the stock loader draws them (same samples in the same
batches for a seed, same state of torch's global generator after every epoch), and a batch is gathered by an index vector
that was uploaded once for the epoch: no per-batch host-to-device copy, no host synchronisation between the first and the
last batch.

``ResidentDataset``  ordered fields ``(tensor, optional channel list)``; several fields may share one tensor (``ecog`` stored
                     once and read through three channel lists).
``ResidentLoader``   iterable over one subset of it, ``len()`` = number of batches; yields tuples of fresh device tensors.
"""
from __future__ import annotations

import ctypes as C
from typing import Iterator, List, Optional, Sequence, Tuple

import torch
from torch.utils.data import DataLoader, RandomSampler, TensorDataset

from .. import _lib

MAX_FIELDS = 4        # segments of one tl_gather_rows launch


class ResidentDataset:
    """Fields ``(tensor, channels)``: field f of sample i is ``tensor[i]`` (``channels`` None) or ``tensor[i][channels]``.

    ``device`` given: every distinct tensor that is not there yet is uploaded once (a ``RuntimeError`` states the bytes
    needed when they do not fit in free device memory - there is no fallback to the host path).  Channel lists are validated
    here, on the host, and uploaded as int32."""

    def __init__(self, fields: Sequence[Tuple[torch.Tensor, Optional[Sequence[int]]]], device=None) -> None:
        fields = [(f, None) if isinstance(f, torch.Tensor) else tuple(f) for f in fields]
        if not fields:
            raise ValueError("ResidentDataset: no fields")
        if len(fields) > MAX_FIELDS:
            raise ValueError(f"ResidentDataset: {len(fields)} fields; one gather launch serves at most {MAX_FIELDS}")
        n = fields[0][0].shape[0] if fields[0][0].dim() > 0 else -1
        lists: List[Optional[List[int]]] = []
        for k, (t, chan) in enumerate(fields):
            if t.dim() < 1 or t.shape[0] != n:
                raise ValueError(f"ResidentDataset: field {k} has shape {tuple(t.shape)}; every field needs {n} samples")
            if t.numel() == 0:
                raise ValueError(f"ResidentDataset: field {k} is empty (shape {tuple(t.shape)})")
            if chan is None:
                lists.append(None)
                continue
            if t.dim() < 2:
                raise ValueError(f"ResidentDataset: field {k} has a channel list but its tensor has no channel dimension")
            chan = [c.item() if hasattr(c, "item") else c for c in chan]
            n_c = t.shape[1]
            if not chan:
                raise ValueError(f"ResidentDataset: field {k} has an empty channel list")
            for c in chan:
                if isinstance(c, bool) or not isinstance(c, int) or not 0 <= c < n_c:
                    raise ValueError(f"ResidentDataset: field {k}: channel {c!r} is not an integer in [0, {n_c})")
            lists.append([int(c) for c in chan])
        tensors = [t for t, _ in fields]
        if device is not None:
            tensors = self._upload(tensors, torch.device(device))
        # one contiguous copy per distinct tensor (the kernel addresses sample i at base + i * sample bytes)
        same = {}
        self._tensors = [same.setdefault(id(t), t.contiguous()) for t in tensors]
        self._lists = lists
        dev = self._tensors[0].device
        if any(t.device != dev for t in self._tensors):
            raise ValueError("ResidentDataset: the fields are on different devices; pass device=")
        self._chan = [None if c is None else torch.tensor(c, dtype=torch.int32).to(dev) for c in lists]
        self._n = int(n)
        self._abi = None

    @staticmethod
    def _upload(tensors: List[torch.Tensor], device: torch.device) -> List[torch.Tensor]:
        todo = {}
        for t in tensors:
            if t.device != device:
                todo.setdefault(id(t), t)
        if device.type == "cuda" and todo:
            need = sum(t.numel() * t.element_size() for t in todo.values())
            free, _total = torch.cuda.mem_get_info(device)
            if need > free:
                raise RuntimeError(f"ResidentDataset: the dataset needs {need} bytes on {device}, {free} bytes are free; "
                                   "use the stock loader (resident=False) or a smaller dataset")
        moved = {k: t.to(device) for k, t in todo.items()}
        return [moved.get(id(t), t) for t in tensors]

    @classmethod
    def from_tensor_dataset(cls, tds: TensorDataset, device=None) -> "ResidentDataset":
        """CPU tensors are uploaded once, tensors already on ``device`` are taken as they are."""
        return cls([(t, None) for t in tds.tensors], device=device)

    def __len__(self) -> int:
        return self._n

    @property
    def device(self) -> torch.device:
        return self._tensors[0].device

    @property
    def n_fields(self) -> int:
        return len(self._tensors)

    def batch_shape(self, k: int, rows: int) -> Tuple[int, ...]:
        t, chan = self._tensors[k], self._lists[k]
        return (rows,) + tuple(t.shape[1:]) if chan is None else (rows, len(chan)) + tuple(t.shape[2:])

    def _tables(self):
        if self._abi is None:              # the tables of the launch that do not change from batch to batch
            src, chan = (C.c_void_p * 4)(), (C.c_void_p * 4)()
            src_rows, n_c, inner, n_chan = (C.c_int64 * 4)(), (C.c_int64 * 4)(), (C.c_int64 * 4)(), (C.c_int64 * 4)()
            for k, t in enumerate(self._tensors):
                src[k], src_rows[k] = t.data_ptr(), self._n
                sample_bytes = (t.numel() // self._n) * t.element_size()
                if self._chan[k] is None:          # a whole sample is one contiguous copy
                    n_c[k], inner[k], n_chan[k], chan[k] = 1, sample_bytes, 0, None
                else:
                    n_c[k], inner[k] = t.shape[1], sample_bytes // t.shape[1]
                    n_chan[k], chan[k] = len(self._lists[k]), self._chan[k].data_ptr()
            self._abi = (src, src_rows, n_c, inner, chan, n_chan, _lib.load().tl_gather_rows)
        return self._abi

    def gather(self, idx: torch.Tensor, start: int, stop: int, err: torch.Tensor) -> Tuple[torch.Tensor, ...]:
        """Rows ``idx[start:stop]`` (int64, on the device, a pointer offset - no slice kernel) of every field, one launch on
        the current stream.  ``err``: int32 device word, bit 0 / 1 set for an index / channel out of range."""
        for t in self._tensors:
            _lib.require_gpu(t, "ResidentDataset.gather")
        if not (idx.is_cuda and idx.dtype == torch.int64 and idx.is_contiguous() and 0 <= start < stop <= idx.numel()):
            raise ValueError("ResidentDataset.gather: idx must be a contiguous int64 device vector and 0 <= start < stop <= len")
        rows, n = stop - start, self.n_fields
        out = tuple(torch.empty(self.batch_shape(k, rows), dtype=self._tensors[k].dtype, device=self.device) for k in range(n))
        src, src_rows, n_c, inner, chan, n_chan, launch = self._tables()
        dst = (C.c_void_p * 4)(*[t.data_ptr() for t in out])
        _lib.check(launch(src, dst, src_rows, n_c, inner, chan, n_chan, n, idx.data_ptr() + 8 * start, rows, err.data_ptr(),
                          _lib.stream_ptr()), "tl_gather_rows")
        return out

    def gather_group(self, table: torch.Tensor, start: int, stop: int, err: torch.Tensor,
                     active: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, ...]:
        """``gather`` for M index vectors at once (``tl_gather_rows_group``): ``table`` is an (M, n) int64 device table, member
        m's batch is rows ``table[m][start:stop]``, and field k comes back stacked as (M, rows, ...).  ``active``: M int32
        device words; the batch of a member whose word is 0 is neither read nor written (its rows are left uninitialised)."""
        for t in self._tensors:
            _lib.require_gpu(t, "ResidentDataset.gather_group")
        if not (table.is_cuda and table.dtype == torch.int64 and table.dim() == 2 and table.is_contiguous()
                and 0 <= start < stop <= table.shape[1]):
            raise ValueError("ResidentDataset.gather_group: table must be a contiguous (M, n) int64 device table and "
                             "0 <= start < stop <= n")
        M, rows, n = table.shape[0], stop - start, self.n_fields
        out = tuple(torch.empty((M,) + self.batch_shape(k, rows), dtype=self._tensors[k].dtype, device=self.device)
                    for k in range(n))
        src, src_rows, n_c, inner, chan, n_chan, _single = self._tables()
        dst = (C.c_void_p * 4)(*[t.data_ptr() for t in out])
        stride = (C.c_int64 * 4)(*[t.stride(0) * t.element_size() for t in out])
        _lib.check(_lib.load().tl_gather_rows_group(src, dst, stride, src_rows, n_c, inner, chan, n_chan, n,
                                                    table.data_ptr() + 8 * start, table.shape[1], rows, M,
                                                    None if active is None else active.data_ptr(), err.data_ptr(),
                                                    _lib.stream_ptr()), "tl_gather_rows_group")
        return out


class _EpochSampler:
    """Sampler of the loader: ``__iter__`` is a generator function, so the ``DataLoader`` that drives it draws its base seed
    first and the order is drawn at the first ``next`` - the sequence of the stock loader (``RandomSampler`` draws its own
    seed from the global generator, then permutes with a private one).  Host only.  ``order`` / ``batches`` hold the last
    epoch's global sample numbers."""

    def __init__(self, indices: torch.Tensor, batch_size: int, shuffle: bool) -> None:
        self.indices = indices                         # int64, host: the subset's sample numbers
        self.batch_size, self.shuffle = int(batch_size), bool(shuffle)
        self.epoch = 0
        self.positions: Optional[torch.Tensor] = None  # the epoch's order as positions inside the subset (None: in order)
        self.order: Optional[torch.Tensor] = None

    def __len__(self) -> int:
        return (len(self.indices) + self.batch_size - 1) // self.batch_size

    @property
    def batches(self) -> List[List[int]]:
        order = self.order.tolist()
        return [order[i:i + self.batch_size] for i in range(0, len(order), self.batch_size)]

    def __iter__(self) -> Iterator[Tuple[int, int]]:
        n = len(self.indices)
        if self.shuffle:
            self.positions = torch.tensor(list(RandomSampler(range(n))), dtype=torch.int64)
            self.order = self.indices[self.positions]
        else:
            self.positions, self.order = None, self.indices
        self.epoch += 1
        for start in range(0, n, self.batch_size):
            yield start, min(start + self.batch_size, n)


class _GatherView:
    """Map-style dataset over ``(start, stop)`` keys: the epoch's order goes to the device at its first batch."""

    def __init__(self, loader: "ResidentLoader") -> None:
        self.loader = loader
        self.epoch = -1
        self.idx: Optional[torch.Tensor] = None

    def __getitem__(self, key: Tuple[int, int]):
        lo, sampler = self.loader, self.loader.sampler
        if self.epoch != sampler.epoch:
            if lo._subset_dev is None:
                lo._subset_dev = sampler.indices.to(lo.dataset.device)          # the subset, once
                lo._err = torch.zeros(1, dtype=torch.int32, device=lo.dataset.device)
            if sampler.positions is None:
                self.idx = lo._subset_dev
            else:
                self.idx = lo._subset_dev[sampler.positions.to(lo.dataset.device)]   # the epoch's order, once
            self.epoch = sampler.epoch
        return lo.dataset.gather(self.idx, key[0], key[1], lo._err)


class _IndexView:
    def __init__(self, sampler: _EpochSampler) -> None:
        self.sampler = sampler

    def __getitem__(self, key: Tuple[int, int]) -> List[int]:
        return self.sampler.order[key[0]:key[1]].tolist()


class _EpochIter:
    def __init__(self, inner, at_end) -> None:
        self.inner, self.at_end = inner, at_end

    def __iter__(self):
        return self

    def __next__(self):
        try:
            return next(self.inner)
        except StopIteration:
            at_end, self.at_end = self.at_end, None
            if at_end is not None:
                at_end()
            raise


class ResidentLoader:
    """Batches of ``dataset[indices]``: ``batch_size`` rows each (the last one ragged), reshuffled every epoch when
    ``shuffle``.  The error word of the gather is read once, when an epoch's iterator is exhausted (``IndexError``)."""

    def __init__(self, dataset: ResidentDataset, indices: Sequence[int], batch_size: int = 8, shuffle: bool = False) -> None:
        if int(batch_size) <= 0:
            raise ValueError("ResidentLoader: batch_size must be positive")
        idx = torch.as_tensor(list(indices) if not isinstance(indices, torch.Tensor) else indices, dtype=torch.int64).cpu()
        if idx.dim() != 1:
            raise ValueError("ResidentLoader: indices must be a vector")
        if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= len(dataset)):
            raise ValueError(f"ResidentLoader: subset indices must be in [0, {len(dataset)}); "
                             f"got {int(idx.min())}..{int(idx.max())}")
        self.dataset = dataset
        self.batch_size = int(batch_size)
        self.sampler = _EpochSampler(idx, batch_size, shuffle)
        self._subset_dev: Optional[torch.Tensor] = None
        self._err: Optional[torch.Tensor] = None

    def __len__(self) -> int:
        return len(self.sampler)

    def _check(self) -> None:
        if self._err is None:
            return
        bits = int(self._err.item())               # the one read of the epoch
        if bits:
            self._err.zero_()
            what = " and ".join(w for b, w in ((1, "a sample index"), (2, "a channel number")) if bits & b)
            raise IndexError(f"ResidentLoader: {what} was out of range during the epoch; those rows were not written")

    def __iter__(self):
        return _EpochIter(iter(DataLoader(_GatherView(self), batch_size=None, sampler=self.sampler)), self._check)

    def iter_indices(self):
        """The same epoch - same draws from torch's global generator - yielding each batch's global sample numbers instead of
        launching the gather (host only)."""
        return iter(DataLoader(_IndexView(self.sampler), batch_size=None, sampler=self.sampler, collate_fn=lambda b: b))
