"""Blocks kept as NumPy archives (no reference counterpart): a block directory ``HS<subject>-<block>/`` holds one
``<modality>.npz`` per modality with ``data (C, T)`` and ``sf``.  ``load_block`` returns the dict ``tdt_blocks.load_block``
returns - ``{<modality>: data, <modality>_sf: sf}`` -, so a recording exported from any acquisition system runs through the
stage without the ``tdt`` package.  ``data_loading.synthetic.write_raw_tree`` writes such a tree."""
from __future__ import annotations

import os

import numpy as np

from .tdt_blocks import save_block  # noqa: F401  (the stage's one writer)


def load_block(block_path: str) -> dict:
    data = {}
    for file in sorted(os.listdir(block_path)):
        if not file.endswith(".npz"):
            continue
        modality = file[:-len(".npz")]
        with np.load(os.path.join(block_path, file)) as archive:
            for key in ("data", "sf"):
                if key not in archive:
                    raise KeyError(f"Expected key '{key}' not found in {os.path.join(block_path, file)}. "
                                   f"Existing keys {list(archive.keys())}.")
            data[modality] = archive["data"]
            sf = archive["sf"]
            data[f"{modality}_sf"] = sf.item() if sf.ndim == 0 else sf
    if not data:
        raise FileNotFoundError(f"No <modality>.npz file in block directory {block_path}")
    for key, value in data.items():
        if not key.endswith("sf"):
            print(f"Shape of {key}: ", value.shape)
    return data
