"""CPU: the device-resident loader's host side - the split and every epoch's order are the stock loader's (same batches,
same state of torch's global generator), host validation, and the argument checks of tl_gather_rows (no launch is reached)."""
import ctypes as C

import pytest
import torch
from torch.utils.data import DataLoader, Subset, TensorDataset

from decode_tonal_langauge_amd.data_loading.dataloaders import split_dataset
from decode_tonal_langauge_amd.data_loading.resident import ResidentDataset, ResidentLoader

RATIOS = [0.74, 0.15, 0.11]           # 203 samples -> 150 / 30 / 23
SHUFFLE = [True, False, False]


def _dataset():
    return TensorDataset(torch.arange(203), torch.arange(203) * 2)


@pytest.mark.parametrize("seed", [0, 7, 42])
def test_order_and_random_stream_match_the_stock_loader(seed):
    tds = _dataset()
    stock = split_dataset(tds, RATIOS, SHUFFLE, batch_size=16, seed=seed)
    assert [len(l.dataset) for l in stock] == [150, 30, 23]
    stock_batches, stock_states = [], []
    for _epoch in range(3):
        for loader in stock:
            stock_batches.append([b[0].tolist() for b in loader])      # the dataset holds arange: values are global indices
        stock_states.append(torch.get_rng_state())
    resident = split_dataset(tds, RATIOS, SHUFFLE, batch_size=16, seed=seed, resident=True, device="cpu")
    assert all(isinstance(l, ResidentLoader) for l in resident)
    assert [len(l) for l in resident] == [len(l) for l in stock] == [10, 2, 2]
    k = 0
    for epoch in range(3):
        for loader in resident:
            got = list(loader.iter_indices())
            assert got == stock_batches[k], (seed, epoch, k)
            assert loader.sampler.batches == got                        # what the gather of that epoch would read
            k += 1
        assert torch.equal(torch.get_rng_state(), stock_states[epoch]), (seed, epoch)


def test_default_split_is_the_stock_loader():
    loaders = split_dataset(_dataset(), RATIOS, SHUFFLE, batch_size=16, seed=3)
    assert all(type(l) is DataLoader and isinstance(l.dataset, Subset) for l in loaders)
    again = split_dataset(_dataset(), RATIOS, SHUFFLE, batch_size=16, seed=3, resident=False)
    assert all(type(l) is DataLoader and isinstance(l.dataset, Subset) for l in again)
    assert [l.dataset.indices for l in loaders] == [l.dataset.indices for l in again]
    assert [l.batch_size for l in again] == [16, 16, 16]


def test_host_validation():
    x = torch.zeros(10, 6, 5)
    for bad in ([0, 6], [-1], [1.5], []):
        with pytest.raises(ValueError, match="channel"):
            ResidentDataset([(x, bad)])
    with pytest.raises(ValueError, match="at most 4"):
        ResidentDataset([(x, None)] * 5)
    with pytest.raises(ValueError, match="samples"):
        ResidentDataset([(x, None), (torch.zeros(9), None)])
    ds = ResidentDataset([(x, [5, 0, 3]), (x, None), (torch.arange(10), None)])
    assert len(ds) == 10 and ds.n_fields == 3
    assert ds.batch_shape(0, 4) == (4, 3, 5) and ds.batch_shape(1, 4) == (4, 6, 5) and ds.batch_shape(2, 4) == (4,)
    for bad in ([0, 10], [-1, 2]):
        with pytest.raises(ValueError, match="subset indices"):
            ResidentLoader(ds, bad, batch_size=4)
    loader = ResidentLoader(ds, [9, 0, 0, 4, 2], batch_size=2, shuffle=False)          # repeats are fine
    assert len(loader) == 3 and list(loader.iter_indices()) == [[9, 0], [0, 4], [2]]
    # no fallback to the host: a gather of tensors that are not on the GPU is an error
    with pytest.raises(RuntimeError, match="no CPU"):
        next(iter(loader))


def test_gather_rows_abi_validation_without_gpu():
    from decode_tonal_langauge_amd import _lib
    lib = _lib.load()
    P4, L4 = C.c_void_p * 4, C.c_int64 * 4
    ptrs, ones, none, zeros = P4(16, 16, 16, 16), L4(1, 1, 1, 1), P4(), L4()
    assert lib.tl_gather_rows(ptrs, ptrs, ones, ones, ones, none, zeros, 5, 16, 4, 16, None) == -1
    assert b"at most 4" in lib.tl_last_error()
    assert lib.tl_gather_rows(None, None, None, None, None, None, None, 2, 16, 4, 16, None) == -1
    assert b"null table" in lib.tl_last_error()
    assert lib.tl_gather_rows(ptrs, ptrs, ones, ones, ones, none, ones, 1, 16, 4, 16, None) == -1
    assert b"null chan" in lib.tl_last_error()
    for sizes in ((zeros, ones, ones), (ones, zeros, ones), (ones, ones, zeros)):
        assert lib.tl_gather_rows(ptrs, ptrs, *sizes, none, zeros, 2, 16, 4, 16, None) == -1
        assert b"positive" in lib.tl_last_error()
    assert lib.tl_gather_rows(ptrs, ptrs, ones, ones, ones, none, zeros, 1, 16, 0, 16, None) == -1 and b"n_idx" in lib.tl_last_error()
    assert lib.tl_gather_rows(ptrs, ptrs, ones, ones, ones, none, zeros, 1, None, 4, 16, None) == -1
    assert lib.tl_gather_rows(ptrs, ptrs, ones, ones, ones, none, zeros, 1, 16, 4, None, None) == -1
    assert b"null index vector or error word" in lib.tl_last_error()
