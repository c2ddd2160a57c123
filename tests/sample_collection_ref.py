"""NumPy references of the sample-collection tests (written for the tests; shared by the host and the GPU file)."""
import numpy as np


def starts_ref(times, sf, length_s):
    """The sample numbers the reference's loops form: python float x the file's 0-d ``sf`` array, truncated."""
    return [int(t * sf) for t in times], int(length_s * sf)


def rest_starts_ref(rest_period, earliest, sf, length_s):
    seg = int(length_s * sf)
    a, b = int(rest_period[0] * sf), int(rest_period[1] * sf)
    if rest_period[1] > earliest:
        b = int(earliest * sf)
    out = []
    for i in range(a, b, seg):
        if i + seg > b:
            break
        out.append(i)
    return out, seg


def cut(rec, starts, length):
    """(n, C, L) by slicing, the way the reference collects windows."""
    return np.array([rec[:, s:s + length] for s in starts]).reshape(len(starts), rec.shape[0], length)


def sliding_ref(arrays, patch_size, segment_length, step_size=None):
    if step_size is None:
        step_size = segment_length // 2
    n_patches = segment_length // patch_size
    out = []
    for data in arrays:
        rows = [data[:, s:s + segment_length].reshape(data.shape[0], n_patches, patch_size)
                for s in range(0, data.shape[1] - segment_length + 1, step_size)]
        out.append(np.stack(rows, axis=0))
    return np.concatenate(out, axis=0)


def write_golden_blocks(golden, folder):
    """The block files of tests/golden/sample_collection_ref.npz, its interval tables, and the call's settings."""
    import os
    import pandas as pd
    intervals = {}
    for block in (1, 2):
        for modality in ("ecog", "sound"):
            np.savez(os.path.join(folder, f"B{block}_{modality}.npz"), data=golden[f"b{block}_{modality}"],
                     sf=golden[f"b{block}_{modality}_sf"])
        intervals[block] = pd.DataFrame({"start": golden[f"b{block}_start"], "end": golden[f"b{block}_end"],
                                         "syllable": [str(s) for s in golden[f"b{block}_syllable"]],
                                         "tone": golden[f"b{block}_tone"]})
    return intervals, dict(syllables=[str(s) for s in golden["syllables"]], length=float(golden["length"]),
                           rest_period=tuple(float(x) for x in golden["rest_period"]))
