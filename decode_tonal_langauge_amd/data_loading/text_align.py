"""TextGrid intervals -> epoched ECoG / audio samples (counterpart of reference data_loading/text_align.py).

``handle_textgrids``    the interval table of every block of a TextGrid directory.
``read_textgrid``       one TextGrid -> ``DataFrame(start, end, syllable, tone)``.
``get_textgrid_time``   the latest interval end of the chosen tiers.
``extract_ecog_audio``  cuts the event windows, the rest segments and the audio windows of every block and merges them
                        into the arrays of a ``subject_<id>.npz``.

Every window copy - events, rest segments, audio - is one ``tl_extract_windows`` launch (``data_loading/epoching.py``): one
upload per recording, one launch per (block, modality, kind).  The planning (times -> sample numbers, range checks, labels)
stays on the host and is finished before anything is launched.  No CPU fallback.

Behaviour of the reference kept on purpose is named in the docstrings below.  One deliberate difference: directories are
visited in ``sorted(os.listdir(...))`` order, so the block order of the output does not depend on the file system."""
from __future__ import annotations

import os
import warnings
from typing import Dict, List, Mapping, Optional, Tuple

import numpy as np
import pandas as pd

from .epoching import extract_windows, plan_starts, to_recording
from .textgrid_io import TextGrid, read_textgrid_file
from .utils import extract_block_id, match_filename


def handle_textgrids(data_dir: str, start_offset: float = 0.0, end_offset: float = 0.0,
                     tier_list: Optional[List[str]] = None, blocks: Optional[List[int]] = None) -> Dict[int, pd.DataFrame]:
    """``{block: interval table}`` of the ``*.TextGrid`` files of ``data_dir`` (block number from ``B<number>`` in the file
    name; a block is read once, from its first file in sorted order; ``blocks`` restricts the blocks read)."""
    intervals: Dict[int, pd.DataFrame] = {}
    for file in sorted(os.listdir(data_dir)):
        if not file.endswith(".TextGrid"):
            continue
        block = extract_block_id(file)
        if (blocks is not None and block not in blocks) or block in intervals:
            continue
        tg = read_textgrid_file(os.path.join(data_dir, file))
        intervals[block] = read_textgrid(tg, start_offset, end_offset, tier_list)
        print(f"Maximum time for block {block}:", get_textgrid_time(tg, tier_list), " s")
    return intervals


def read_textgrid(tg: TextGrid, start_offset: float, end_offset: float, tier_list: Optional[List[str]] = None) -> pd.DataFrame:
    """The intervals whose mark starts with a digit (the true reading times) as rows ``start, end, syllable, tone``.

    Kept from the reference on purpose:
      * a tier is taken when ``tier.name.lower() in tier_list``; with ``tier_list=None`` the list is the tiers' own names,
        NOT lower-cased - a tier named "Phones" is therefore skipped by default;
      * ``tone = int(mark[0])``, ``syllable = mark[1]`` (one character); empty marks and marks that do not start with a digit
        are skipped;
      * ``start = minTime - start_offset``, ``end = maxTime + end_offset``, both rounded with ``np.around(., 1)``; an interval
        whose unrounded start lies below the previous kept interval's rounded end is skipped with a warning.
    A mark that is a single digit raises ``ValueError`` naming the interval (the reference: a bare ``IndexError``)."""
    rows = []
    if tier_list is None:
        tier_list = [tier.name for tier in tg.tiers]
    for tier in tg.tiers:
        if tier.name.lower() not in tier_list:
            continue
        for interval in tier.intervals:
            mark = interval.mark
            if len(mark) == 0 or not mark[0].isdigit():
                continue
            if len(mark) < 2:
                raise ValueError(f"Mark {mark!r} of the interval [{interval.minTime}, {interval.maxTime}] in tier "
                                 f"'{tier.name}' has a tone but no syllable character.")
            tone, syllable = int(mark[0]), mark[1]
            start, end = interval.minTime - start_offset, interval.maxTime + end_offset
            if rows and start < rows[-1]["end"]:
                warnings.warn(f"Overlapping intervals detected in tier '{tier.name}' at time {interval.minTime:.2f} for "
                              f"syllable '{syllable}', previous end time was {rows[-1]['end']:.2f}. Skipping this interval ... ")
                continue
            rows.append({"start": np.around(start, decimals=1), "end": np.around(end, decimals=1), "syllable": syllable,
                         "tone": tone})
    return pd.DataFrame(rows)


def get_textgrid_time(tg: TextGrid, tier_list: Optional[List[str]] = None) -> float:
    """The latest ``maxTime`` over the tiers whose lower-cased name is in ``tier_list`` (None: every tier)."""
    if tier_list is None:
        tier_list = [tier.name.lower() for tier in tg.tiers]
    latest = 0.0
    for tier in tg.tiers:
        if tier.name.lower() in tier_list:
            for interval in tier.intervals:
                latest = max(latest, interval.maxTime)
    return latest


def plan_rest(rest_period: Tuple[float, float], earliest_start: float, sf, length_s: float, block) -> Tuple[np.ndarray, int]:
    """Starts of the rest segments of one block: ``range(int(r0 * sf), rest_end, int(length_s * sf))``, whole segments only.
    When ``rest_period[1]`` exceeds the block's earliest event start, ``rest_end`` is cut to ``int(earliest_start * sf)``
    with a warning (kept from the reference)."""
    segment = int(length_s * sf)
    rest_start, rest_end = int(rest_period[0] * sf), int(rest_period[1] * sf)
    if rest_period[1] > earliest_start:
        warnings.warn(f"Rest period end ({rest_period[1]} s) is after the earliest interval start for block {block} "
                      f"(earliest event time: {earliest_start} s). Reducing rest period end ...")
        rest_end = int(earliest_start * sf)
    if segment < 1:
        raise ValueError(f"Sample length {length_s} s is shorter than one sample at {sf} Hz.")
    starts = [i for i in range(rest_start, rest_end, segment) if i + segment <= rest_end]
    return np.asarray(starts, dtype=np.int64), segment


def _load_recording(path: str, file: str, what: str):
    dataset = np.load(path)
    for key, meaning in (("data", f"the {what} data"), ("sf", "the sampling frequency")):
        if key not in dataset:
            raise KeyError(f"Expected key '{key}' not found in the npz file {file}. Ensure {meaning} is correctly stored."
                           f"Existing keys {list(dataset.keys())}.")
    return dataset["data"], dataset["sf"]


def plan_event_windows(table: pd.DataFrame, sf, length_s: float, n_samples: int, block, what: str) -> Tuple[np.ndarray, int]:
    """``plan_starts`` for the ``start`` column of a block's table, refused on the host when a window passes the end of the
    ``what`` ("ECoG" / "audio") recording of ``n_samples`` samples."""
    starts, length = plan_starts(table["start"].tolist(), sf, length_s)
    if length < 1:
        raise ValueError(f"Sample length {length_s} s is shorter than one sample of the {what} data at {sf} Hz.")
    for k, start in enumerate(starts.tolist()):
        end = start + length
        if end > n_samples or start < 0:          # a negative start: beyond the reference, which slices it from the end
            raise ValueError(f"Requested sample length exceeds {what} data length for block {block}. "
                             f"Start: {start}, End: {end}, Data length: {n_samples}. \n"
                             f"Corresponding interval: {table.iloc[k]}. ")
    return starts, length


def syllable_codes(table: pd.DataFrame, syllables: List[str]) -> np.ndarray:
    """int8 codes: the index of each syllable in ``syllables``, -1 for one that is not listed."""
    return np.array(pd.Categorical(table["syllable"], categories=syllables).codes)


def merge_tone_labels(per_block: List[np.ndarray]) -> np.ndarray:
    """The blocks' tone columns in one int64 vector, shifted to start at 0 when the lowest tone is above 0."""
    tones = np.concatenate(per_block, axis=0)
    lowest = np.min(tones)
    if lowest > 0:
        tones -= lowest
    return tones


def extract_ecog_audio(intervals: Dict[int, pd.DataFrame], recording_dir: Optional[str], syllables: List[str],
                       length: float = 1.0, output_path: Optional[str] = None,
                       rest_period: Optional[Tuple[float, float]] = None, recording_format: str = "npz",
                       recordings: Optional[Mapping] = None, to_host: bool = True, announce: bool = False) -> dict:
    """The samples of one subject: ``ecog (n, C, L)``, ``ecog_sf``, ``audio (n, S)``, ``audio_sf``, ``syllable (n,)``,
    ``tone (n,)`` and, with ``rest_period``, ``ecog_rest (m, C, L)``; saved with ``np.savez`` when ``output_path`` is given.

    ``recording_dir`` holds ``B<block>...ecog...npz`` and ``B<block>...sound...npz`` files with the keys ``data (C, T)`` and
    ``sf``; a file named ``...audio...`` is a sound recording too (the preprocess stage writes ``B<block>_audio.npz``: the
    reference's two stages disagree on the word).  ``recordings`` is used instead when given: a mapping
    ``block -> {"ecog": (data, sf), "sound": (data, sf)}`` of NumPy arrays or CUDA tensors, visited in the mapping's order
    and, within a block, in the entry's (``announce=True`` prints the recording-length line the file walk prints for each).
    ``to_host=False`` leaves ``ecog`` / ``audio`` / ``ecog_rest`` as CUDA tensors (the channel selectors take them as they
    are); with CUDA recordings nothing then crosses to the host and the host never waits for the device.

    Kept from the reference on purpose:
      * a window is ``[int(start * sf), int(start * sf) + int(length * sf))`` in the float64 arithmetic of the reference; a
        window past the end of its recording raises ``ValueError`` (checked on the host before any launch);
      * syllable codes are ``pd.Categorical(..., categories=syllables).codes``: int8, -1 for an unknown syllable; tone labels
        are int64 with the minimum subtracted when it is above 0;
      * rest segments: see ``plan_rest``;
      * audio is row 0 of the sound recording; ``ecog_sf`` / ``audio_sf`` are those of the last block read; the merged block
        order is the order in which the sound recordings were met;
      * ``KeyError`` for a missing ``data`` / ``sf`` key, ``ValueError`` for mismatched ECoG / audio block sets or no block.
    Beyond the reference: files are visited in sorted order; a block without events or without a whole rest segment raises a
    ``ValueError`` naming the block (the reference fails inside ``np.concatenate``)."""
    import torch
    erp: Dict[int, "torch.Tensor"] = {}
    rest: Dict[int, "torch.Tensor"] = {}
    audio: Dict[int, "torch.Tensor"] = {}
    syllable_labels: Dict[int, np.ndarray] = {}
    tone_labels: Dict[int, np.ndarray] = {}
    ecog_sf = audio_sf = None
    print("Syllable mapping used: ", dict(enumerate(syllables)))

    def ecog_block(block, data, sf):
        nonlocal ecog_sf
        table = intervals[block]
        if len(table) == 0:
            raise ValueError(f"Block {block} has no intervals to extract.")
        rec = to_recording(data, "extract_ecog_audio")
        starts, n_len = plan_event_windows(table, sf, length, rec.shape[1], block, "ECoG")
        rest_starts = None
        if rest_period is not None:
            rest_starts, seg = plan_rest(rest_period, table["start"].min(), sf, length, block)
            if rest_starts.size == 0:
                raise ValueError(f"Block {block} yields no whole rest segment of {seg} samples inside the rest period "
                                 f"{tuple(rest_period)}.")
            if int(rest_starts[0]) < 0 or int(rest_starts[-1]) + seg > rec.shape[1]:
                raise ValueError(f"Rest period {tuple(rest_period)} exceeds ECoG data length for block {block}. "
                                 f"Data length: {rec.shape[1]}.")
        erp[block] = extract_windows(rec, starts, n_len, check=False)          # validated above: no read-back
        if rest_starts is not None:
            rest[block] = extract_windows(rec, rest_starts, seg, check=False)
        tone_labels[block] = table["tone"].to_numpy()
        syllable_labels[block] = syllable_codes(table, syllables)
        ecog_sf = sf

    def sound_block(block, data, sf):
        nonlocal audio_sf
        table = intervals[block]
        if len(table) == 0:
            raise ValueError(f"Block {block} has no intervals to extract.")
        rec = to_recording(data, "extract_ecog_audio")
        starts, n_len = plan_event_windows(table, sf, length, rec.shape[1], block, "audio")
        audio[block] = extract_windows(rec[0:1], starts, n_len, check=False).reshape(len(starts), n_len)   # mono: row 0
        audio_sf = sf

    if recordings is not None:
        for block, entry in recordings.items():
            if block not in intervals:
                continue
            for kind in entry:                                      # the entry's order: the file order of a registered block
                if kind not in ("ecog", "sound"):
                    continue
                what, work = ("ECoG", ecog_block) if kind == "ecog" else ("audio", sound_block)
                data, sf = entry[kind]
                if announce:
                    print(f"{what} recording length for block {block}:", data.shape[1] / sf, " s")
                work(block, data, sf)
    else:
        for file in sorted(os.listdir(recording_dir)):
            for kword, done, what, work in (("ecog", erp, "ECoG", ecog_block), ("sound", audio, "audio", sound_block),
                                            ("audio", audio, "audio", sound_block)):
                if not match_filename(file, recording_format, [kword]):
                    continue
                block = extract_block_id(file)
                if block not in intervals:
                    break
                if block in done:
                    warnings.warn(f"Found multiple {what} files for block {block}, skipping file {file}. ")
                    break
                data, sf = _load_recording(os.path.join(recording_dir, file), file, what)
                print(f"{what} recording length for block {block}:", data.shape[1] / sf, " s")
                work(block, data, sf)
                break

    blocks = list(audio.keys())
    if erp.keys() != audio.keys():
        raise ValueError("Mismatch between ECoG and audio samples blocks. Ensure both ECoG and audio files are present for "
                         f"each block. ECoG blocks found: {erp.keys()}, Audio blocks found: {audio.keys()}.")
    if len(blocks) == 0:
        raise ValueError("No valid blocks found in the specified directories."
                         f"Blocks in textgrids: {list(intervals.keys())}. ")

    tones = merge_tone_labels([tone_labels[b] for b in blocks])
    output = {"ecog": torch.cat([erp[b] for b in blocks], dim=0), "ecog_sf": ecog_sf,
              "audio": torch.cat([audio[b] for b in blocks], dim=0), "audio_sf": audio_sf,
              "syllable": np.concatenate([syllable_labels[b] for b in blocks], axis=0), "tone": tones}
    if rest_period is not None:
        output["ecog_rest"] = torch.cat([rest[b] for b in blocks], dim=0)
    for key in ("ecog", "audio", "ecog_rest"):
        if key in output:
            print(f"{key} samples shape:", tuple(output[key].shape))
    if to_host:
        for key in ("ecog", "audio", "ecog_rest"):
            if key in output:
                output[key] = output[key].cpu().numpy()
    if output_path is not None:
        np.savez(output_path, **{k: v.cpu().numpy() if isinstance(v, torch.Tensor) else v for k, v in output.items()})
        print(f"ECoG and audio samples saved to {output_path}")
    return output
