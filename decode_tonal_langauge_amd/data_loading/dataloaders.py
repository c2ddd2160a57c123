"""``split_dataset`` (mirror of reference data_loading/dataloaders.py:11-74): the seeded
``random_split`` + DataLoader construction that fixes batch composition for a seed.

``resident=True`` (off by default) returns ``ResidentLoader``s instead (``data_loading/resident.py``): the dataset lives on the
device and a batch is one gather launch; same split, same batches and the same state of torch's global generator for a seed.

``collect_unlabelled_samples`` (mirror of reference data_loading/dataloaders.py:77-170): sliding windows over every recording of
a folder, cut into patches - one ``tl_extract_windows`` launch per file."""
import os
from typing import List, Optional

import numpy as np
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


def collect_unlabelled_samples(dataset_folder: str, patch_size: int, segment_length: int, step_size: Optional[int] = None,
                               kwords: Optional[List[str]] = None, verbose: bool = False) -> np.ndarray:
    """``(n_samples, n_channels, n_patches, patch_size)``: the windows ``data[:, s : s + segment_length]`` for
    ``s in range(0, T - segment_length + 1, step_size)`` of every ``.npz`` file under ``dataset_folder`` whose name holds every
    keyword, each window cut into ``segment_length // patch_size`` patches.  ``step_size`` defaults to half a segment.

    The signature and the errors are the reference's.  Directories and files are walked in sorted order (the reference takes
    the file system's), each recording is uploaded once and its windows are one launch; the result is a NumPy array."""
    from .epoching import extract_windows
    from .utils import match_filename
    if step_size is None:
        step_size = segment_length // 2
    if segment_length % patch_size != 0:
        raise ValueError(f"segment_length ({segment_length}) must be divisible by patch_size ({patch_size}).")
    n_patches = segment_length // patch_size
    all_samples = []
    for root, dirs, files in os.walk(dataset_folder):
        dirs.sort()
        for file in sorted(files):
            if not match_filename(file, 'npz', kwords) or not file.endswith('.npz'):
                continue
            file_path = os.path.join(root, file)
            if verbose:
                print(f"Processing file: {file_path}")
            dataset = np.load(file_path)
            if 'data' not in dataset:
                raise KeyError(f'Key data cannot be found in {file_path}, Available keys: {list(dataset.keys())}')
            data = dataset['data']
            n_channels, n_timepoints = data.shape
            starts = np.arange(0, n_timepoints - segment_length + 1, step_size, dtype=np.int64)
            if starts.size == 0:
                raise ValueError(f"need at least one array to stack: {file_path} has {n_timepoints} timepoints, fewer than "
                                 f"segment_length ({segment_length}).")
            windows = extract_windows(data, starts, segment_length, check=False)       # starts are in range by construction
            samples = windows.view(len(starts), n_channels, n_patches, patch_size).cpu().numpy()
            if verbose:
                print('Collected {} samples with shape {}'.format(len(samples), samples.shape[1:]))
            all_samples.append(samples)
    all_samples = np.concatenate(all_samples, axis=0)
    if verbose:
        print('Total samples collected: ', len(all_samples))
    return all_samples
