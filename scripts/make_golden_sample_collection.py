#!/usr/bin/env python3
"""Writes tests/golden/sample_collection_ref.npz: the inputs of a two-block sample collection and what the REFERENCE
implementation's ``extract_ecog_audio`` returns for them.

    python scripts/make_golden_sample_collection.py --reference /path/to/reference/checkout

Host only; run once on a build machine that has the reference checkout, never by a test.  The reference's
``data_loading/text_align.py`` imports the ``textgrid`` package at module level but only calls it inside
``handle_textgrids``; a stub module is registered under that name so the import succeeds, and the interval tables are
built here as DataFrames of the columns ``read_textgrid`` produces.  ``os.listdir`` is wrapped to return sorted names while
the reference runs, so that its block order is the sorted one the product uses.

Data are integer-valued float32 so that the archive compresses; the rates are non-integer (401.5 Hz ECoG, 24414.0625 / 20 Hz
sound), the second syllable list entry is missing from the table's syllables ("u" is unknown -> -1), tones start at 1, and
``rest_period = (0.5, 2.6)`` is cut by block 1's first event at 2.3 s."""
import argparse
import importlib
import os
import sys
import tempfile
import types
import warnings

import numpy as np
import pandas as pd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ECOG_SF, SOUND_SF, SECONDS, LENGTH = 401.5, 24414.0625 / 20, 12.0, 0.5
SYLLABLES = ["a", "i"]
REST = (0.5, 2.6)
TABLES = {
    1: [(2.3, 2.9, "a", 1), (4.1, 4.6, "i", 3), (6.6, 7.1, "u", 2), (7.7, 8.3, "a", 4)],
    2: [(4.1, 4.7, "i", 2), (5.9, 6.4, "a", 1), (7.7, 8.2, "i", 4), (9.3, 9.9, "u", 3), (11.4, 11.5, "a", 2)],
}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference checkout")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "sample_collection_ref.npz"))
    args = ap.parse_args()

    stub = types.ModuleType("textgrid")
    stub.TextGrid = type("TextGrid", (), {})
    sys.modules["textgrid"] = stub
    sys.path.insert(0, os.path.abspath(args.reference))
    ref = importlib.import_module("data_loading.text_align")

    rng = np.random.default_rng(20261019)
    golden = {"syllables": np.array(SYLLABLES), "length": np.array(LENGTH), "rest_period": np.array(REST)}
    intervals = {}
    with tempfile.TemporaryDirectory() as tmp:
        for block, rows in TABLES.items():
            intervals[block] = pd.DataFrame([{"start": np.around(s, 1), "end": np.around(e, 1), "syllable": syl, "tone": tone}
                                             for s, e, syl, tone in rows])
            golden[f"b{block}_start"] = intervals[block]["start"].to_numpy()
            golden[f"b{block}_end"] = intervals[block]["end"].to_numpy()
            golden[f"b{block}_syllable"] = np.array([r[2] for r in rows])
            golden[f"b{block}_tone"] = intervals[block]["tone"].to_numpy()
            for modality, rows_n, sf in (("ecog", 3, ECOG_SF), ("sound", 1, SOUND_SF)):
                data = rng.integers(-500, 500, (rows_n, int(SECONDS * sf))).astype(np.float32)
                np.savez(os.path.join(tmp, f"B{block}_{modality}.npz"), data=data, sf=sf)
                golden[f"b{block}_{modality}"] = data
                golden[f"b{block}_{modality}_sf"] = np.array(sf)
        listdir = os.listdir
        os.listdir = lambda path: sorted(listdir(path))
        try:
            with warnings.catch_warnings(record=True) as caught:
                warnings.simplefilter("always")
                out = ref.extract_ecog_audio(intervals, tmp, syllables=SYLLABLES, length=LENGTH, rest_period=REST)
        finally:
            os.listdir = listdir
    golden["n_warnings"] = np.array(len(caught))
    for key, value in out.items():
        golden[f"out_{key}"] = np.asarray(value)
        print(key, golden[f"out_{key}"].dtype, golden[f"out_{key}"].shape)
    np.savez_compressed(args.out, **golden)
    print(args.out, os.path.getsize(args.out), "bytes;", len(caught), "warning(s) from the reference")


if __name__ == "__main__":
    main()
