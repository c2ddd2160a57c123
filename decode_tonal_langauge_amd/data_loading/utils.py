"""Label and file-name helpers (mirror of reference data_loading/utils.py)."""
import re
from typing import Dict, List, Optional

import numpy as np


def extract_block_id(filename: str) -> int:
    """The block number of a file name: the digits behind the first ``B`` that has digits behind it (``HS25_B1.wav`` -> 1,
    ``B5_16000.TextGrid`` -> 5).  ``ValueError`` when there is none."""
    found = re.search(r"B(\d+)", filename)
    if found is None:
        raise ValueError(f"No block ID found in filename: {filename}")
    return int(found.group(1))


def match_filename(file: str, file_format: str, kwords: Optional[List[str]] = None) -> bool:
    """True when ``file`` ends with ``file_format`` and contains every keyword."""
    return file.endswith(file_format) and all(word in file for word in (kwords or ()))


def prepare_tone_dynamics(tone_dynamic_mapping: Dict[str, List[int]], tone_labels: np.ndarray,
                          syllable_labels: np.ndarray) -> np.ndarray:
    """Host version kept for API parity; the trainer uses the device gather ``tl_tone_dynamics``."""
    if len(tone_labels) != len(syllable_labels):
        raise ValueError("Length of tone labels and syllable labels must match.")
    dynamics = []
    for tone, syllable in zip(tone_labels, syllable_labels):
        try:
            tone_dynamic = tone_dynamic_mapping[str(tone)]
        except KeyError:
            raise ValueError(f"Tone {str(tone)} not found in tone_dynamic_mapping."
                             f"Available tones in mapping: {list(tone_dynamic_mapping.keys())}")
        dynamics.append(np.array([[syllable] * len(tone_dynamic), tone_dynamic]))
    return np.array(dynamics)


def select_non_discriminative_channels(channel_selections: dict, discriminative_keys: List[str]) -> list:
    keep = set(channel_selections['active_channels'])
    drop = set()
    for label in discriminative_keys:
        drop.update(channel_selections[label])
    return sorted(keep - drop)
