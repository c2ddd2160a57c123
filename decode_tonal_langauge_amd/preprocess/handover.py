"""Resident hand-over from the preprocess stage to sample collection (no reference counterpart).

With ``pipeline.params.keep_resident: true`` ``pipelines/subject_block.run`` still writes every ``B<block>_<modality>.npz``
and also keeps what it wrote here, keyed by the subject's output directory, in the shape
``extract_ecog_audio(recordings=...)`` documents: ``block -> {"ecog": (data, sf), "sound": (data, sf)}``.  ``data`` is the
CUDA tensor the steps left on the device (or, for a modality without steps, the host array that was never uploaded), ``sf``
the rate as ``np.load`` returns it from the written file.  ``extract_samples.run`` of the same process epochs a registered
subject from these instead of reading and uploading the files again; ``release(setup_dir)`` drops them
(``main.run_pipeline`` calls it after the ``sample_collection`` stage)."""
from __future__ import annotations

import os
from typing import Dict, Optional

import numpy as np

_REGISTRY: Dict[str, Dict[int, dict]] = {}

#: key of a recording in a registry entry <- the word its modality name (and its file name) carries.  The reference's
#: preprocess stage calls the modality "audio" (tdt_blocks.py), its sample collection looks for "sound" files.
KINDS = (("ecog", "ecog"), ("sound", "sound"), ("audio", "sound"))


def kind_of(modality: str) -> Optional[str]:
    for word, kind in KINDS:
        if word in modality:
            return kind
    return None


def _key(path: str) -> str:
    return os.path.normpath(os.path.abspath(path))


def register(subject_dir: str, block_id: int, data_dict: dict) -> None:
    """Keep the ECoG and the sound modality of one saved block.  Modalities are taken in sorted order, the order of their
    files in a sorted listing; the first of a kind wins, as the first file does in ``extract_ecog_audio``."""
    entry = _REGISTRY.setdefault(_key(subject_dir), {}).setdefault(int(block_id), {})
    for modality in sorted(k for k in data_dict if not k.endswith("_sf")):
        kind = kind_of(modality)
        if kind is not None and kind not in entry:
            entry[kind] = (data_dict[modality], np.asarray(data_dict.get(f"{modality}_sf")))


def lookup(subject_dir: str) -> Optional[Dict[int, dict]]:
    """The blocks registered for ``subject_dir`` (``block -> {"ecog": (data, sf), "sound": (data, sf)}``), or
    None."""
    return _REGISTRY.get(_key(subject_dir))


def registered() -> list:
    return sorted(_REGISTRY)


def release(setup_dir: Optional[str] = None) -> None:
    """Forget every subject under ``setup_dir`` (None: everything)."""
    if setup_dir is None:
        _REGISTRY.clear()
        return
    root = _key(setup_dir)
    for key in [k for k in _REGISTRY if k == root or k.startswith(root + os.sep)]:
        del _REGISTRY[key]
