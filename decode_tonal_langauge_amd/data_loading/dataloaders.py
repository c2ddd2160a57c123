"""``split_dataset`` (mirror of reference data_loading/dataloaders.py:11-74): the seeded
``random_split`` + DataLoader construction that fixes batch composition for a seed.

``resident=True`` (off by default) returns ``ResidentLoader``s instead (``data_loading/resident.py``): the dataset lives on the
device and a batch is one gather launch; same split, same batches and the same state of torch's global generator for a seed."""
from typing import List

import torch
from torch.utils.data import DataLoader, TensorDataset, random_split


def split_dataset(dataset: TensorDataset, ratios: List[float], shuffling: List[bool], batch_size: int = 8,
                  seed: int = 42, resident: bool = False, device=None) -> List[DataLoader]:
    torch.manual_seed(seed)
    n_samples = len(dataset)
    sizes: List[int] = []
    for i, ratio in enumerate(ratios):
        if ratio <= 0 or ratio >= 1:
            raise ValueError("All ratios must be between 0 and 1 (exclusive).")
        sizes.append(n_samples - sum(sizes) if i == len(ratios) - 1 else int(n_samples * ratio))
    subsets = random_split(dataset, sizes)
    if resident:
        from .resident import ResidentDataset, ResidentLoader
        rds = dataset if isinstance(dataset, ResidentDataset) else ResidentDataset.from_tensor_dataset(
            dataset, device if device is not None else ("cuda" if not dataset.tensors[0].is_cuda else None))
        return [ResidentLoader(rds, sub.indices, batch_size=batch_size, shuffle=shuffling[i]) for i, sub in enumerate(subsets)]
    return [DataLoader(sub, batch_size=batch_size, shuffle=shuffling[i]) for i, sub in enumerate(subsets)]
