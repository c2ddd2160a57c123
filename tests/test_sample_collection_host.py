"""CPU: the host half of the sample-collection stage - the TextGrid reader, the interval table, the window and rest planning,
the labels, the argument checks of tl_extract_windows (no launch is reached) and the stage's plumbing."""
import ctypes as C
import os
import sys
import types
import warnings

import numpy as np
import pandas as pd
import pytest
import yaml

from decode_tonal_langauge_amd.data_loading import text_align, textgrid_io
from decode_tonal_langauge_amd.data_loading.epoching import plan_starts
from decode_tonal_langauge_amd.data_loading.synthetic import write_block_annotations
from decode_tonal_langauge_amd.data_loading.utils import extract_block_id, match_filename
from tests import sample_collection_ref as ref

WORDS = [(0.0, 1.04, ""), (1.04, 1.56, "3a"), (1.56, 2.25, 'say "ma" twice'), (2.25, 2.75, "1ü"),
         (2.75, 4.125, "two\nlines"), (4.125, 6.5, "4i")]
PHONES = [(0.0, 5.0, ""), (5.0, 6.5, "4a")]
RATES = [np.array(3051.7578125), np.array(24414.0625), np.array(401.5)]          # 0-d arrays, as np.load returns ``sf``
TIMES = [2.3, 4.1, 7.7, 0.0, 0.1, 0.7, 1.1, 9.9, 11.4]


def _triples(tier):
    return [tuple(i) for i in tier.intervals]


# ---- TextGrid reader ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["annotations_long_B3.TextGrid", "annotations_short_B3.TextGrid",
                                  "annotations_utf16_B3.TextGrid"])
def test_reader_formats_and_encodings(golden_dir, name):
    tg = textgrid_io.read_textgrid_file(os.path.join(golden_dir, name))
    assert [t.name for t in tg.tiers] == ["words", "Phones"]                       # the point tier is parsed and skipped
    assert _triples(tg.tiers[0]) == WORDS and _triples(tg.tiers[1]) == PHONES      # "" undone, a mark over two lines, non-ASCII
    assert (tg.minTime, tg.maxTime) == (0.0, 6.5)
    assert (tg.tiers[0].minTime, tg.tiers[0].maxTime) == (0.0, 6.5)
    iv = tg.tiers[0].intervals[1]
    assert (iv.minTime, iv.maxTime, iv.mark) == (1.04, 1.56, "3a")


def test_reader_rejects_a_truncated_file(golden_dir):
    path = os.path.join(golden_dir, "annotations_truncated_B3.TextGrid")
    with pytest.raises(ValueError) as e:
        textgrid_io.read_textgrid_file(path)
    assert path in str(e.value) and "line 21" in str(e.value) and "xmax of interval 2" in str(e.value)


@pytest.mark.parametrize("text, what", [
    ('File type = "ooTextFile"\nObject class = "Sound"\n', "line 2"),
    ('File type = "ooTextFile"\nObject class = "TextGrid"\n0\n1\n<exists>\n1\n"IntervalTier"\n"w"\n0\n1\n1\n0\n"x"\n', "line 13"),
    ('File type = "ooTextFile"\nObject class = "TextGrid"\n0\n1\n<exists>\n1\n"IntervalTier"\n"w\n0\n1\n', "not closed"),
    ('File type = "ooTextFile"\nObject class = "TextGrid"\n0\n1\n<exists>\n1\n"Spectrum"\n"w"\n0\n1\n0\n', "unknown tier class"),
])
def test_reader_names_file_and_line_of_a_malformed_file(tmp_path, text, what):
    path = tmp_path / "bad_B1.TextGrid"
    path.write_text(text, encoding="utf-8")
    with pytest.raises(ValueError) as e:
        textgrid_io.read_textgrid_file(str(path))
    assert str(path) in str(e.value) and what in str(e.value)


@pytest.mark.parametrize("short", [False, True])
@pytest.mark.parametrize("encoding", ["utf-8", "utf-16"])
def test_write_read_round_trip(tmp_path, short, encoding):
    tiers = [("words", WORDS), textgrid_io.PointTier("clicks", [(0.5, 'a "click"')], maxTime=6.5), ("Phones", PHONES),
             ("odd", [(0.1 + 0.2, 1 / 3, "x")])]                                   # times that need all their digits
    path = textgrid_io.write_textgrid(str(tmp_path / "rt_B1.TextGrid"), tiers, short=short, encoding=encoding)
    raw = open(path, "rb").read()
    assert raw.startswith(b"\xff\xfe") == (encoding == "utf-16")
    tg = textgrid_io.read_textgrid_file(path)
    assert [t.name for t in tg.tiers] == ["words", "Phones", "odd"]
    assert _triples(tg.tiers[0]) == WORDS and _triples(tg.tiers[1]) == PHONES
    assert _triples(tg.tiers[2]) == [(0.1 + 0.2, 1 / 3, "x")]


def test_synthetic_annotations_round_trip(tmp_path):
    path = write_block_annotations(str(tmp_path), 7, [(1.0, 1.5, 3, "a"), (1.5, 2.0, 1, "i"), (4.25, 4.75, 2, "a")], seconds=6.0)
    assert os.path.basename(path) == "B7.TextGrid" and extract_block_id(path) == 7
    tables = text_align.handle_textgrids(str(tmp_path), start_offset=0.0)
    assert list(tables) == [7]
    assert tables[7].to_dict("list") == {"start": [1.0, 1.5, 4.2], "end": [1.5, 2.0, 4.8], "syllable": ["a", "i", "a"],
                                         "tone": [3, 1, 2]}
    assert text_align.handle_textgrids(str(tmp_path), blocks=[1]) == {}
    with pytest.raises(ValueError, match="overlaps"):
        write_block_annotations(str(tmp_path), 8, [(1.0, 2.0, 1, "a"), (1.5, 2.5, 1, "a")])


def test_file_name_helpers():
    assert extract_block_id("HS25_B1.wav") == 1 and extract_block_id("B12_ecog_B3.npz") == 12
    with pytest.raises(ValueError, match="No block ID"):
        extract_block_id("ecog.npz")
    assert match_filename("B1_ecog.npz", "npz", ["ecog"]) and match_filename("B1_ecog.npz", "npz")
    assert not match_filename("B1_ecog.npz", "npz", ["ecog", "sound"]) and not match_filename("B1_ecog.npy", "npz", ["ecog"])


# ---- read_textgrid on built objects: the rows are what the reference returns for this input ------------------------------
def _grid():
    words = textgrid_io.IntervalTier("words", [(0, 1.04, ""), (1.04, 1.56, "3a"), (1.5, 2.0, "2i"), (2.26, 2.74, "xx"),
                                               (2.74, 3.31, "1i")])
    phones = textgrid_io.IntervalTier("Phones", [(5, 6, "4a")])
    return textgrid_io.TextGrid([words, phones])


def _rows(table):
    return [tuple(r) for r in table[["start", "end", "syllable", "tone"]].itertuples(index=False, name=None)]


def test_read_textgrid_rows_and_overlap_warning():
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        table = text_align.read_textgrid(_grid(), 0.2, 0.0, None)
    assert _rows(table) == [(0.8, 1.6, "a", 3), (2.5, 3.3, "i", 1)]               # "Phones" skipped: names are not lower-cased
    assert len(caught) == 1 and "Overlapping intervals" in str(caught[0].message)
    assert table["start"].dtype == np.float64 and table["tone"].dtype == np.int64


def test_read_textgrid_tier_list():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        table = text_align.read_textgrid(_grid(), 0.2, 0.0, ["words", "phones"])
        only = text_align.read_textgrid(_grid(), 0.2, 0.0, ["phones"])
    assert _rows(table) == [(0.8, 1.6, "a", 3), (2.5, 3.3, "i", 1), (4.8, 6.0, "a", 4)]
    assert _rows(only) == [(4.8, 6.0, "a", 4)]
    assert text_align.get_textgrid_time(_grid()) == 6.0 and text_align.get_textgrid_time(_grid(), ["words"]) == 3.31


def test_read_textgrid_single_digit_mark_is_a_value_error():
    tg = textgrid_io.TextGrid([textgrid_io.IntervalTier("words", [(0, 1, "3a"), (1.5, 2.5, "4")])])
    with pytest.raises(ValueError, match=r"'4'.*1\.5, 2\.5.*words"):
        text_align.read_textgrid(tg, 0.0, 0.0)


# ---- planning -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sf", RATES, ids=lambda r: str(float(r)))
@pytest.mark.parametrize("length_s", [1.0, 0.5, 0.3])
def test_plan_starts_truncates_like_the_reference(sf, length_s):
    starts, length = plan_starts(TIMES, sf, length_s)
    want, want_len = ref.starts_ref(TIMES, sf, length_s)
    assert starts.dtype == np.int64 and starts.tolist() == want and length == want_len and isinstance(length, int)


def test_plan_starts_products_are_not_trivial():
    # the float64 product decides: at 401.5 Hz 2.3 s is sample 923 (923.45), at 3051.7578125 Hz 4.1 s is 12512 (12512.207...)
    assert plan_starts([2.3, 4.1, 7.7], RATES[2], 1.0)[0].tolist() == [923, 1646, 3091]
    s, length = plan_starts([2.3, 4.1, 7.7], RATES[0], 1.0)
    assert s.tolist() == [int(2.3 * 3051.7578125), int(4.1 * 3051.7578125), int(7.7 * 3051.7578125)] and length == 3051
    with pytest.raises(ValueError, match="window 1"):
        plan_starts([0.0, 11.5], RATES[2], 1.0, n_samples=4818)
    with pytest.raises(ValueError, match="window 0"):
        plan_starts([-0.5], RATES[2], 1.0, n_samples=4818)
    assert plan_starts([0.0, 11.0], RATES[2], 1.0, n_samples=4818)[0].tolist() == [0, 4416]


@pytest.mark.parametrize("sf", RATES, ids=lambda r: str(float(r)))
def test_rest_planning(sf):
    with warnings.catch_warnings(record=True) as caught:                          # the rest period ends before the first event
        warnings.simplefilter("always")
        starts, seg = text_align.plan_rest((0.5, 2.6), 4.1, sf, 0.5, block=2)
    assert not caught
    assert (starts.tolist(), seg) == ref.rest_starts_ref((0.5, 2.6), 4.1, sf, 0.5)
    with pytest.warns(UserWarning, match="Reducing rest period end"):            # cut by an event at 2.3 s
        cut, seg = text_align.plan_rest((0.5, 2.6), 2.3, sf, 0.5, block=1)
    assert (cut.tolist(), seg) == ref.rest_starts_ref((0.5, 2.6), 2.3, sf, 0.5)
    assert len(cut) < len(starts)
    # the incomplete last segment is dropped: every kept segment ends inside the (cut) period
    assert cut[-1] + seg <= int(2.3 * sf) < cut[-1] + 2 * seg
    assert starts.dtype == np.int64


def test_rest_planning_at_401_5_hz():
    starts, seg = text_align.plan_rest((0.5, 2.6), 4.1, RATES[2], 0.5, block=2)
    assert seg == 200 and starts.tolist() == [200, 400, 600, 800]                 # 1000 + 200 > int(2.6 * 401.5) = 1043
    with pytest.warns(UserWarning):
        starts, _ = text_align.plan_rest((0.5, 2.6), 2.3, RATES[2], 0.5, block=1)
    assert starts.tolist() == [200, 400, 600]                                     # 800 + 200 > int(2.3 * 401.5) = 923
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert text_align.plan_rest((0.5, 2.6), 0.6, RATES[2], 0.5, block=1)[0].size == 0


def test_window_past_the_end_is_a_value_error():
    table = pd.DataFrame({"start": [2.3, 11.6], "end": [2.9, 12.0], "syllable": ["a", "i"], "tone": [1, 2]})
    starts, length = text_align.plan_event_windows(table, RATES[2], 0.5, 4858, 5, "ECoG")
    assert starts.tolist() == [923, 4657] and length == 200
    with pytest.raises(ValueError) as e:
        text_align.plan_event_windows(table, RATES[2], 0.5, 4856, 5, "ECoG")
    msg = str(e.value)
    assert "exceeds ECoG data length for block 5" in msg and "Start: 4657, End: 4857" in msg and "Data length: 4856" in msg


# ---- labels -------------------------------------------------------------------------------------------------------------
def test_labels():
    table = pd.DataFrame({"start": [1.0, 2.0, 3.0], "end": [1.5, 2.5, 3.5], "syllable": ["i", "u", "a"], "tone": [3, 1, 4]})
    codes = text_align.syllable_codes(table, ["a", "i"])
    assert codes.dtype == np.int8 and codes.tolist() == [1, -1, 0]
    tones = text_align.merge_tone_labels([table["tone"].to_numpy(), np.array([2, 4])])
    assert tones.dtype == np.int64 and tones.tolist() == [2, 0, 3, 1, 3]
    assert table["tone"].tolist() == [3, 1, 4]                                    # the table is not shifted in place
    assert text_align.merge_tone_labels([np.array([0, 2]), np.array([3])]).tolist() == [0, 2, 3]


# ---- C ABI without a GPU ------------------------------------------------------------------------------------------------
def test_extract_windows_abi_validation_without_gpu():
    from decode_tonal_langauge_amd import _lib
    lib = _lib.load()
    assert "tl_extract_windows" in _lib.SIGNATURES
    fn = lib.tl_extract_windows
    assert fn.restype is C.c_int and len(fn.argtypes) == 11 and fn.argtypes[1] is C.c_int64 and fn.argtypes[7] is C.c_int
    P = 4096                                                                       # never dereferenced: every call is refused

    def call(src=P, c=3, t=40, ld=40, starts=P, n=2, length=8, eb=4, dst=P, err=P):
        return fn(src, c, t, ld, starts, n, length, eb, dst, err, None)

    for kw, text in ((dict(src=None), b"null"), (dict(starts=None), b"null"), (dict(dst=None), b"null"), (dict(err=None), b"null"),
                     (dict(c=0), b"positive"), (dict(t=0, ld=0), b"positive"), (dict(length=0), b"positive"),
                     (dict(c=-1), b"positive"), (dict(ld=39), b"row stride"), (dict(length=41), b"window length"),
                     (dict(eb=3), b"elem_bytes"), (dict(eb=0), b"elem_bytes"), (dict(eb=16), b"elem_bytes"),
                     (dict(src=P + 2), b"aligned"), (dict(dst=P + 1, eb=2), b"aligned"), (dict(src=P + 4, eb=8), b"aligned"),
                     (dict(n=-1), b"negative"), (dict(n=1 << 31), b"2^31"), (dict(c=1 << 20, n=1 << 11), b"2^31")):
        assert call(**kw) == -1, kw
        assert text in lib.tl_last_error(), (kw, lib.tl_last_error())
    assert call(src=P + 1, dst=P + 3, eb=1, n=-1) == -1                            # a byte recording needs no alignment
    assert b"negative" in lib.tl_last_error()
    assert call(n=0) == 0                                                          # no launch, hence no device needed
    assert call(n=0, src=None, starts=None, dst=None, err=None) == 0
    assert call(n=0, length=41) == -1                                              # the shape checks do not depend on n


def test_extract_windows_needs_a_gpu_tensor():
    import torch
    from decode_tonal_langauge_amd.data_loading.epoching import extract_windows
    with pytest.raises(RuntimeError, match="no CPU"):
        extract_windows(torch.zeros(2, 10), [0], 4)


# ---- stage plumbing -----------------------------------------------------------------------------------------------------
def _stage_tree(tmp_path):
    rec = tmp_path / "preprocessed_run"
    for sid in ("1", "2"):
        (rec / f"subject_{sid}").mkdir(parents=True)
    (rec / "config.yaml").write_text(yaml.dump({"preprocess": {"module": "preprocess_main", "marker": 5}}))
    tg_root = tmp_path / "textgrids"
    write_block_annotations(str(tg_root / "s1"), 1, [(1.0, 1.5, 3, "a"), (2.0, 2.5, 1, "i")], seconds=4.0)
    write_block_annotations(str(tg_root / "s2"), 2, [(1.0, 1.5, 2, "a")], seconds=4.0)
    cfg = {"sample_collection": {"module": "extract_samples", "params": {
        "io": {"recording_dir": str(rec), "textgrid_root": str(tg_root), "output_dir": str(tmp_path / "samples")},
        "settings": {"syllable_identifiers": ["a", "i"], "figures": False},
        "subjects": {"1": {"textgrid_dir": "s1", "sample_length": 0.5, "rest_period": [0.1, 0.9], "start_offset": 0.2},
                     "2": {"textgrid_dir": "s2", "sample_length": 0.5, "rest_period": [0.1, 0.9], "blocks": [2]},
                     "3": {"textgrid_dir": "s1", "sample_length": 0.5, "rest_period": [0.1, 0.9]},      # no recordings
                     "4": {"textgrid_dir": "missing", "sample_length": 0.5, "rest_period": [0.1, 0.9]}}}}}
    (rec / "subject_4").mkdir()
    return cfg, rec


def _patch_extract(monkeypatch, calls):
    from decode_tonal_langauge_amd import extract_samples

    def fake(intervals, recording_dir, syllables, length=1.0, output_path=None, rest_period=None, **kw):
        calls.append(dict(blocks=list(intervals), rows={b: len(t) for b, t in intervals.items()}, recording_dir=recording_dir,
                          syllables=syllables, length=length, output_path=output_path, rest_period=rest_period,
                          first_start=float(next(iter(intervals.values()))["start"].iloc[0])))
        np.savez(output_path, ecog=np.zeros((1, 1, 1), np.float32))
        return {}
    monkeypatch.setattr(extract_samples, "extract_ecog_audio", fake)
    return extract_samples


def test_stage_plumbing(tmp_path, monkeypatch):
    import hashlib
    calls = []
    stage = _patch_extract(monkeypatch, calls)
    cfg, rec = _stage_tree(tmp_path)
    out = stage.run(cfg)
    digest = hashlib.md5(yaml.dump(cfg["sample_collection"], sort_keys=True).encode()).hexdigest()[:6]
    assert out == os.path.join(str(tmp_path / "samples"), f"preprocessed_run__{digest}")
    carried = yaml.safe_load(open(os.path.join(out, "config.yaml")))
    assert carried["preprocess"] == {"module": "preprocess_main", "marker": 5}
    assert carried["sample_collection"] == cfg["sample_collection"]
    # subject 3 has no recording directory, subject 4 no TextGrid directory
    assert [os.path.basename(c["recording_dir"]) for c in calls] == ["subject_1", "subject_2"]
    assert calls[0]["blocks"] == [1] and calls[0]["rows"] == {1: 2} and calls[0]["first_start"] == 0.8      # start_offset
    assert calls[1]["blocks"] == [2] and calls[1]["first_start"] == 1.0
    assert calls[0]["output_path"] == os.path.join(out, "subject_1.npz") and calls[0]["rest_period"] == (0.1, 0.9)
    assert calls[0]["syllables"] == ["a", "i"] and calls[0]["length"] == 0.5
    assert sorted(f for f in os.listdir(out) if f.endswith(".npz")) == ["subject_1.npz", "subject_2.npz"]
    # existing outputs are kept without ``overwrite`` (the hash, hence the directory, is the configuration's)
    del calls[:]
    assert stage.run(cfg) == out and calls == []
    cfg["sample_collection"]["params"]["settings"]["overwrite"] = True
    os.makedirs(stage.run(cfg), exist_ok=True)
    assert len(calls) == 2


def test_stage_without_intervals_names_the_subjects_blocks(tmp_path, monkeypatch):
    stage = _patch_extract(monkeypatch, [])
    cfg, _rec = _stage_tree(tmp_path)
    cfg["sample_collection"]["params"]["subjects"] = {"1": {"textgrid_dir": "s1", "sample_length": 0.5, "rest_period": [0.1, 0.9],
                                                            "blocks": [9]}}
    with pytest.raises(ValueError, match=r"No intervals found.*Target blocks: \[9\]"):
        stage.run(cfg)


def test_pipeline_wires_the_stage(tmp_path, monkeypatch):
    from decode_tonal_langauge_amd import main
    calls, seen = [], {}
    _patch_extract(monkeypatch, calls)
    cfg, rec = _stage_tree(tmp_path)
    del cfg["sample_collection"]["params"]["io"]["recording_dir"]                  # to be filled from the preprocess stage
    before = types.ModuleType("sc_stub_preprocess")
    before.run = lambda config: str(rec)
    after = types.ModuleType("sc_stub_selection")
    after.run = lambda config: seen.update(io=dict(config["channel_selection"]["params"]["io"]))
    monkeypatch.setitem(sys.modules, "sc_stub_preprocess", before)
    monkeypatch.setitem(sys.modules, "sc_stub_selection", after)
    cfg["preprocess"] = {"module": "sc_stub_preprocess"}
    cfg["channel_selection"] = {"module": "sc_stub_selection", "params": {"io": {"output_dir": str(tmp_path / "channels")}}}
    path = tmp_path / "pipeline.yaml"
    path.write_text(yaml.dump(cfg))
    main.run_pipeline(str(path))
    assert [os.path.dirname(c["recording_dir"]) for c in calls] == [str(rec), str(rec)]
    out = os.path.dirname(calls[0]["output_path"])
    assert os.path.basename(out).startswith("preprocessed_run__") and seen["io"]["sample_dir"] == out
