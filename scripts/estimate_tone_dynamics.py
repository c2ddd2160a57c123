#!/usr/bin/env python3
"""A ``tone_dynamic_mapping`` measured from a subject's sample file (``data_loading.utils.estimate_tone_dynamics``).

    python scripts/estimate_tone_dynamics.py --sample_path samples/subject_1.npz [--config_file config.json]
                                             [--n_dynamics 5] [--frame_length 2048] [--device cuda:0]
                                             [--output tone_dynamics.json]

The sample file holds ``audio (n, S)``, ``tone (n,)`` and ``audio_sf`` (what the sample collection stage writes; ``--sr``
overrides or replaces ``audio_sf``).  Prints the mapping as JSON (and writes it to ``--output``).  With ``--config_file`` the
length of the table comes from its ``tone_dynamic_mapping`` and the distance to that table is printed per tone: the mean and the
largest absolute difference in tone levels."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def table_distance(estimated: dict, table: dict) -> dict:
    """Per tone present in both: (mean, max) absolute difference of the levels."""
    out = {}
    for tone in sorted(set(estimated) & set(table), key=int):
        diff = np.abs(np.asarray(estimated[tone], dtype=float) - np.asarray(table[tone], dtype=float))
        out[tone] = (float(diff.mean()), float(diff.max()))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--sample_path", required=True)
    ap.add_argument("--config_file", default=None)
    ap.add_argument("--n_dynamics", type=int, default=None)
    ap.add_argument("--sr", type=float, default=None)
    ap.add_argument("--device", default=None)
    ap.add_argument("--fmin", type=float, default=60.0)
    ap.add_argument("--fmax", type=float, default=500.0)
    ap.add_argument("--frame_length", type=int, default=2048)
    ap.add_argument("--output", default=None)
    args = ap.parse_args(argv)
    from decode_tonal_langauge_amd.data_loading.utils import estimate_tone_dynamics
    data = np.load(args.sample_path)
    table = None
    if args.config_file:
        with open(args.config_file) as f:
            table = json.load(f)["tone_dynamic_mapping"]
    n_dynamics = args.n_dynamics or (len(next(iter(table.values()))) if table else 5)
    sr = args.sr if args.sr is not None else float(data["audio_sf"])
    mapping = estimate_tone_dynamics(data["audio"], data["tone"], sr, n_dynamics, device=args.device, fmin=args.fmin,
                                     fmax=args.fmax, frame_length=args.frame_length)
    print(json.dumps(mapping, indent=1))
    if args.output:
        with open(args.output, "w") as f:
            json.dump(mapping, f, indent=1)
    if table:
        for tone, (mean, worst) in table_distance(mapping, table).items():
            print(f"tone {tone}: config {table[tone]} - mean |difference| {mean:.2f} levels, largest {worst:.2f}")
        missing = sorted(set(table) ^ set(mapping), key=int)
        if missing:
            print(f"tones in one table only: {missing}")
    return mapping


if __name__ == "__main__":
    main()
