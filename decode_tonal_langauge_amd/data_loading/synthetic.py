"""Synthetic data in the reference's on-disk schemas (no recordings ship with either repository).

Schemas:
  * ``subject_<id>.npz``   ``ecog (N, C, T) float32``, ``ecog_sf``, ``audio (N, S)``, ``audio_sf``, ``mel (N, n_mels)``,
                           ``syllable (N,)``, ``tone (N,)``, ``ecog_rest (N, C, T)``
                           (reference data_loading/text_align.py:446-459; ``mel`` as consumed by train_synthesizer)
  * ``subject_<id>.json``  channel selections ``{active_channels, tone_discriminative, syllable_discriminative}``
                           (reference channel_selection_main.py:86-88)
  * ``config.json``        ``{mel_kwargs, n_syllables, n_tones, tone_dynamic_mapping}`` (reference train_synthesizer.py:171-177)
  * ``B<block>_<modality>.npz``  ``data (C, T)``, ``sf`` (reference preprocess/io/tdt_blocks.py:33-34)
  * ``HS<subject>-<block>/<modality>.npz``  ``data (C, T)``, ``sf``: a raw block as ``preprocess/io/npz_blocks.py`` reads it
  * ``B<block>.TextGrid``  one interval tier whose reading intervals are marked ``<tone digit><syllable character>``
                           (read by data_loading/text_align.py)

The ECoG carries a learnable class pattern: tone k lifts a group of channels, syllable 1 adds a slow
ramp, so classifiers and the synthesiser have something to fit."""
from __future__ import annotations

import json
import os
from typing import Dict, List, Optional, Sequence

import numpy as np

DEFAULT_TONE_DYNAMICS = {"0": [3, 3, 3, 3, 3], "1": [1, 2, 3, 4, 5], "2": [3, 2, 1, 2, 4], "3": [5, 4, 3, 2, 1]}


def make_subject(n_samples: int = 400, n_channels: int = 16, n_timepoints: int = 100, n_tones: int = 4,
                 n_syllables: int = 2, n_mels: int = 80, ecog_sf: int = 100, audio_sf: int = 16000,
                 seed: int = 2024) -> Dict[str, np.ndarray]:
    """Arrays of one ``subject_<id>.npz``."""
    rng = np.random.default_rng(seed)
    tone = rng.integers(0, n_tones, n_samples)
    syllable = rng.integers(0, n_syllables, n_samples)
    ecog = rng.standard_normal((n_samples, n_channels, n_timepoints)).astype(np.float32)
    group = max(1, n_channels // n_tones)
    for k in range(n_tones):
        ecog[tone == k, k * group:(k + 1) * group, :] += 0.5
    ecog[syllable == 1] += np.linspace(-0.4, 0.4, n_timepoints, dtype=np.float32)
    n_audio = int(n_timepoints / ecog_sf * audio_sf)
    t = np.arange(n_audio) / audio_sf
    f0 = 110.0 * (1 + tone[:, None]) * (1 + 0.1 * syllable[:, None])
    audio = (0.1 * np.sin(2 * np.pi * f0 * t[None, :])).astype(np.float32)
    mel = (10 * rng.standard_normal((n_samples, n_mels)) + 5 * tone[:, None]).astype(np.float32)
    return {"ecog": ecog, "ecog_sf": np.array(ecog_sf), "audio": audio, "audio_sf": np.array(audio_sf), "mel": mel,
            "syllable": syllable, "tone": tone,
            "ecog_rest": rng.standard_normal((n_samples, n_channels, n_timepoints)).astype(np.float32)}


def write_dataset(root: str, subject_ids=(1,), channels: Optional[Dict[str, List[int]]] = None,
                  tone_dynamic_mapping: Optional[Dict[str, List[int]]] = None, **subject_kwargs) -> Dict[str, str]:
    """Write ``samples/subject_<id>.npz``, ``channels/subject_<id>.json`` and ``samples/config.json`` under
    ``root``.  Returns the directories / files written."""
    sample_dir, chan_dir = os.path.join(root, "samples"), os.path.join(root, "channels")
    os.makedirs(sample_dir, exist_ok=True)
    os.makedirs(chan_dir, exist_ok=True)
    n_mels = subject_kwargs.get("n_mels", 80)
    for i, sid in enumerate(subject_ids):
        subj = make_subject(seed=subject_kwargs.pop("seed", 2024) + i, **subject_kwargs)
        np.savez(os.path.join(sample_dir, f"subject_{sid}.npz"), **subj)
        C = subj["ecog"].shape[1]
        sel = channels or {"active_channels": list(range(C)), "tone_discriminative": list(range(0, C // 2)),
                           "syllable_discriminative": list(range(C // 2, C))}
        with open(os.path.join(chan_dir, f"subject_{sid}.json"), "w") as f:
            json.dump(sel, f)
    cfg = {"mel_kwargs": {"n_mels": n_mels}, "n_syllables": subject_kwargs.get("n_syllables", 2),
           "n_tones": subject_kwargs.get("n_tones", 4),
           "tone_dynamic_mapping": tone_dynamic_mapping or DEFAULT_TONE_DYNAMICS}
    config_file = os.path.join(sample_dir, "config.json")
    with open(config_file, "w") as f:
        json.dump(cfg, f)
    return {"sample_dir": sample_dir, "channel_selection_dir": chan_dir, "config_file": config_file}


def write_raw_block(root: str, block: int = 1, modality: str = "ecog", n_channels: int = 256, seconds: float = 60.0,
                    sf: float = 400.0, seed: int = 0) -> str:
    """``B<block>_<modality>.npz`` with ``data (C, T) float32`` and ``sf`` - the input of the preprocess steps."""
    rng = np.random.default_rng(seed)
    data = rng.standard_normal((n_channels, int(seconds * sf))).astype(np.float32)
    os.makedirs(root, exist_ok=True)
    path = os.path.join(root, f"B{block}_{modality}.npz")
    np.savez(path, data=data, sf=sf)
    return path


def write_raw_tree(root: str, blocks: Dict, n_channels: int = 6, ecog_sf: float = 1017.25, audio_sf: float = 2000.5,
                   audio_samples: Optional[int] = None, seed: int = 0, subject_dir: str = "Sub{subject}/raw",
                   stray: Sequence[str] = ()) -> Dict:
    """A raw tree for the preprocess stage with ``preprocess.io.npz_blocks``: ``<root>/<subject_dir>/HS<subject>-<block>/``
    holding ``ecog.npz`` (``data (n_channels, int(seconds * ecog_sf)) float32``, ``sf``) and ``audio.npz``
    (``data (1, audio_samples or int(seconds * audio_sf)) float32``, ``sf``).  ``blocks`` is ``{subject: {block: seconds}}``;
    the data of (subject, block) are drawn from ``default_rng([seed, subject, block])``, and the default ECoG rate is not an
    integer, as a TDT rate is not.  Every name in ``stray`` becomes an empty directory beside each subject's blocks (the
    pipeline skips what does not parse as a block).  Returns ``{"root_dir", "subject_dirs", "subject_ids", "blocks":
    {(subject, block): block directory}}`` - the first three are the pipeline's parameters."""
    out = {"root_dir": root, "subject_dirs": [], "subject_ids": [], "blocks": {}}
    for subject, lengths in blocks.items():
        rel = subject_dir.format(subject=subject)
        out["subject_dirs"].append(rel)
        out["subject_ids"].append(subject)
        for name in stray:
            os.makedirs(os.path.join(root, rel, name), exist_ok=True)
        for block, seconds in lengths.items():
            rng = np.random.default_rng([seed, int(subject), int(block)])
            path = os.path.join(root, rel, f"HS{subject}-{block}")
            os.makedirs(path, exist_ok=True)
            ecog = (rng.standard_normal((n_channels, int(seconds * ecog_sf))) * 30.0 + 5.0).astype(np.float32)
            audio = rng.standard_normal((1, audio_samples or int(seconds * audio_sf))).astype(np.float32)
            np.savez(os.path.join(path, "ecog.npz"), data=ecog, sf=ecog_sf)
            np.savez(os.path.join(path, "audio.npz"), data=audio, sf=audio_sf)
            out["blocks"][(subject, block)] = path
    return out


def write_block_annotations(root: str, block: int, events: Sequence, tier: str = "words", seconds: Optional[float] = None,
                            short: bool = False, encoding: str = "utf-8") -> str:
    """``B<block>.TextGrid`` for a ``write_raw_block`` recording: ``events`` are ``(start_s, end_s, tone, syllable)`` in
    time order, without overlap; each becomes an interval marked ``f"{tone}{syllable}"`` on the tier ``tier`` and the gaps
    between them (and up to ``seconds``, the recording's length) are filled with empty intervals, as Praat writes them."""
    from .textgrid_io import write_textgrid
    rows, at = [], 0.0
    for start, end, tone, syllable in events:
        start, end = float(start), float(end)
        if start < at or end <= start:
            raise ValueError(f"write_block_annotations: event ({start}, {end}) overlaps its predecessor or is empty")
        if not 0 <= int(tone) <= 9 or len(str(syllable)) != 1:
            raise ValueError("write_block_annotations: a tone is one digit and a syllable one character")
        if start > at:
            rows.append((at, start, ""))
        rows.append((start, end, f"{int(tone)}{syllable}"))
        at = end
    if seconds is not None and float(seconds) > at:
        rows.append((at, float(seconds), ""))
    os.makedirs(root, exist_ok=True)
    return write_textgrid(os.path.join(root, f"B{block}.TextGrid"), [(tier, rows)], short=short, encoding=encoding)
