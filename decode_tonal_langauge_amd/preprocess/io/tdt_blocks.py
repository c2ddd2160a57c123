"""TDT block reader and the block writer of the preprocess stage (counterpart of reference preprocess/io/tdt_blocks.py).

``load_block`` reads a TDT tank through the ``tdt`` package, imported when a block is read, not when this module is: the
package is optional, and ``save_block`` - the writer every io module of the stage shares - needs nothing of it.  There is no
tank parser of this package's own."""
from __future__ import annotations

import os

import numpy as np


def load_block(block_path: str) -> dict:
    """``{"ecog": streams.EOG1.data, "audio": streams.ANIN.data[:1, :], "ecog_sf", "audio_sf"}`` of one TDT block."""
    try:
        import tdt
    except ImportError as e:
        raise ImportError("preprocess.io.tdt_blocks.load_block reads TDT tanks through the 'tdt' package, which is not "
                          "installed.  Install it, or convert the blocks to <modality>.npz files (data (C, T), sf) and "
                          "name preprocess.io.npz_blocks as the io module.") from e
    block_data = tdt.read_block(block_path)
    data = {
        "ecog": block_data.streams.EOG1.data,
        "audio": block_data.streams.ANIN.data[:1, :],
        "ecog_sf": block_data.streams.EOG1.fs,
        "audio_sf": block_data.streams.ANIN.fs,
    }
    for key, value in data.items():
        if not key.endswith("sf"):
            print(f"Shape of {key}: ", value.shape)
    return data


def save_block(setup_dir: str, subject_id, block_id, data_dict: dict) -> None:
    """``<setup_dir>/subject_<id>/B<block>_<key>.npz`` with ``data`` and ``sf`` (``<key>_sf``) for every key that does not
    end in ``_sf``.  A tensor is written as the array it holds (one copy to the host, here)."""
    subject_output_dir = os.path.join(setup_dir, f"subject_{subject_id}")
    os.makedirs(subject_output_dir, exist_ok=True)
    for key, value in data_dict.items():
        if key.endswith("_sf"):
            continue
        if not isinstance(value, np.ndarray) and hasattr(value, "detach"):
            value = value.detach().cpu().numpy()
        file_path = os.path.join(subject_output_dir, f"B{block_id}_{key}.npz")
        np.savez(file_path, data=value, sf=data_dict.get(f"{key}_sf"))
        print(f"Saved {key} data to: {file_path}")
