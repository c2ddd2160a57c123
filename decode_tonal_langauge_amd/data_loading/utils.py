"""Label and file-name helpers (mirror of reference data_loading/utils.py)."""
import re
from typing import Dict, List, Optional

import numpy as np

from ..utils.audio import yin_f0_batch


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


def _longest_run(mask: np.ndarray):
    """(start, stop) of the longest run of True in a 1-D mask (the first of equals), (0, 0) if there is none."""
    edges = np.flatnonzero(np.diff(np.concatenate(([0], mask.astype(np.int8), [0]))))
    starts, stops = edges[0::2], edges[1::2]
    if starts.size == 0:
        return 0, 0
    k = int(np.argmax(stops - starts))
    return int(starts[k]), int(stops[k])


def estimate_tone_dynamics(audio, tone_labels, sr: float, n_dynamics: int, device=None, fmin: float = 60.0,
                           fmax: float = 500.0, voicing_threshold: float = 0.1, silence_db: float = 40.0,
                           **yin_kwargs) -> Dict[str, List[float]]:
    """A ``tone_dynamic_mapping`` measured from the speaker's own audio, the counterpart of the hand-set table of
    ``config.json``: the F0 of all (N, S) clips in one ``yin_f0_batch`` call; per clip the longest voiced run of ``log2 f0``,
    resampled to ``n_dynamics`` points by linear interpolation and mapped to the five-level tone scale
    ``1 + 4 (l - l05) / (l95 - l05)`` clipped to [1, 5], ``l05`` / ``l95`` being the 5th / 95th percentile of every voiced
    ``log2 f0`` of the call (the speaker's range); per tone the median over its clips.  Returns ``{str(tone): [level, ...]}``,
    which ``SynthesisTrainer`` takes as it is.  A tone none of whose clips has a voiced frame raises ``ValueError`` by name.
    ``yin_kwargs`` go to the tracker (frame_length, win_length, hop_length, trough_threshold, center)."""
    from ..utils.metrics import f0_voicing
    tone_labels = np.asarray(tone_labels).reshape(-1)
    if np.ndim(audio) != 2 or len(tone_labels) != np.shape(audio)[0]:
        raise ValueError("audio must be (clips, samples) with one tone label per clip.")
    if n_dynamics < 1:
        raise ValueError(f"n_dynamics = {n_dynamics} must be at least 1")
    track = yin_f0_batch(audio, sr, fmin, fmax, device=device, **yin_kwargs)
    f0, aper, pidx, rms = (np.asarray(t.cpu() if hasattr(t, "cpu") else t) for t in track[:4])
    voiced = f0_voicing((f0, aper, pidx, rms), voicing_threshold, silence_db)
    tones = sorted(set(int(t) for t in tone_labels))
    if not voiced.any():
        raise ValueError(f"no voiced frame in any clip: tones {tones} cannot be estimated")
    logf = np.log2(f0)
    l05, l95 = np.percentile(logf[voiced], [5.0, 95.0])
    span = l95 - l05
    contours: Dict[int, list] = {t: [] for t in tones}
    for n, tone in enumerate(tone_labels):
        lo, hi = _longest_run(voiced[n])
        if hi == lo:
            continue
        run = logf[n, lo:hi]
        at = np.interp(np.linspace(0.0, hi - lo - 1.0, int(n_dynamics)), np.arange(hi - lo), run)
        level = 1.0 + 4.0 * (at - l05) / span if span > 0 else np.full(int(n_dynamics), 3.0)
        contours[int(tone)].append(np.clip(level, 1.0, 5.0))
    silent = [t for t in tones if not contours[t]]
    if silent:
        raise ValueError(f"tone(s) {silent} have no clip with a voiced frame: their dynamics cannot be estimated")
    return {str(t): [float(v) for v in np.median(np.stack(contours[t]), axis=0)] for t in tones}
