"""GPU: tl_extract_windows and everything built on it - extract_windows, extract_ecog_audio (against the reference's own
output, tests/golden/sample_collection_ref.npz), the resident chain into channel selection, collect_unlabelled_samples and
the sample-collection stage.  Every comparison is bit for bit against NumPy / torch slicing (byte views: any dtype)."""
import json
import os
import warnings
from argparse import Namespace

import numpy as np
import pytest
import torch
import yaml

from decode_tonal_langauge_amd import _lib
from decode_tonal_langauge_amd.data_loading import epoching, synthetic, text_align
from decode_tonal_langauge_amd.data_loading.epoching import extract_windows
from tests import sample_collection_ref as ref

pytestmark = pytest.mark.gpu

PAD, FRONT, BACK, PREFILL = 0xEE, 0xF1, 0xD7, 0xCB      # canary bytes; the data bytes are all below 200


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


class _Case:
    """A (C, T) recording of ``dtype`` with row stride ``ld`` whose storage ends with the last sample of the last row; the
    padding columns hold PAD.  The recording starts one element behind a 16-byte boundary."""

    def __init__(self, dtype, C, T, ld, dev, seed=0):
        self.dtype, self.C, self.T, self.ld = dtype, C, T, ld
        self.eb = eb = torch.empty((), dtype=dtype).element_size()
        self.lead = 16 + eb
        n_el = (C - 1) * ld + T
        raw = np.random.default_rng(seed).integers(0, 200, self.lead + n_el * eb).astype(np.uint8)
        el = raw[self.lead:].reshape(n_el, eb)
        for c in range(C - 1):
            el[c * ld + T:(c + 1) * ld] = PAD
        self.host = np.stack([el[c * ld:c * ld + T] for c in range(C)])            # (C, T, eb) bytes
        self.raw = torch.from_numpy(raw).to(dev)
        self.src_ptr = self.raw.data_ptr() + self.lead
        assert (self.src_ptr - eb) % 16 == 0
        self.tensor = torch.as_strided(self.raw[self.lead:].view(dtype), (C, T), (ld, 1))
        assert self.tensor.data_ptr() == self.src_ptr

    def want(self, starts, L):
        return np.stack([self.host[:, s:s + L] for s in starts]).reshape(-1)       # (n, C, L, eb) bytes, flat

    def launch(self, starts, L):
        """The raw entry point into a destination one element behind a 16-byte boundary, between canaries.  Returns
        (destination bytes on the host, error word)."""
        n, dev = len(starts), self.raw.device
        n_bytes = n * self.C * L * self.eb
        buf = torch.full((self.lead + n_bytes + 64,), PREFILL, dtype=torch.uint8, device=dev)
        buf[:self.lead] = FRONT
        buf[self.lead + n_bytes:] = BACK
        st = torch.tensor(list(starts), dtype=torch.int64, device=dev)
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        dst_ptr = buf.data_ptr() + self.lead
        assert (dst_ptr - self.eb) % 16 == 0
        _lib.check(_lib.load().tl_extract_windows(self.src_ptr, self.C, self.T, self.ld, st.data_ptr(), n, L, self.eb, dst_ptr,
                                                  err.data_ptr(), _lib.stream_ptr()), "tl_extract_windows")
        out = buf.cpu().numpy()
        assert (out[:self.lead] == FRONT).all() and (out[self.lead + n_bytes:] == BACK).all(), "wrote outside dst"
        return out[self.lead:self.lead + n_bytes], int(err.item())


def _starts(T, L):
    """0, T - L (the last window: on the last row it ends with the allocation), every residue mod 4, a repeated start (6, 6)
    and overlapping windows (5, 6, 7)."""
    return [s for s in (0, T - L, 1, 2, 3, 4, 5, 6, 6, 7, T - L) if 0 <= s <= T - L]


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int16, torch.float32, torch.float64], ids=str)
@pytest.mark.parametrize("C", [3, 1])
def test_kernel_at_the_smallest_shapes(dev, dtype, C):
    T, ld = 37, 40
    case = _Case(dtype, C, T, ld, dev, seed=C)
    for L in (1, 3, 4, 5, 16, 17, 37):
        starts = _starts(T, L)
        assert {s % 4 for s in starts} >= ({0, 1, 2, 3} if T - L >= 3 else {0}) and T - L in starts
        got, err = case.launch(starts, L)
        assert err == 0
        assert not (got == PAD).any() and not (got == PREFILL).any(), (L, "padding read or destination not written")
        assert np.array_equal(got, case.want(starts, L)), (str(dtype), C, L)
        one, err = case.launch([T - L], L)                                          # n = 1
        assert err == 0 and np.array_equal(one, case.want([T - L], L))
        # the Python entry on the strided tensor
        out = extract_windows(case.tensor, starts, L)
        assert out.shape == (len(starts), C, L) and out.dtype == dtype and out.device == case.tensor.device
        assert np.array_equal(out.cpu().numpy().view(np.uint8).reshape(-1), case.want(starts, L))


@pytest.mark.parametrize("L", [5, 17])
def test_kernel_rows_share_waves_and_several_workgroups(dev, L):
    case = _Case(torch.float32, 3, 37, 40, dev, seed=9)
    starts = [(7 * i) % (37 - L + 1) for i in range(257)]                           # 257 * 3 * L elements: 2 and 7 workgroups
    got, err = case.launch(starts, L)
    assert err == 0 and np.array_equal(got, case.want(starts, L))
    table = torch.tensor(starts, dtype=torch.int64, device=dev)
    out = extract_windows(case.tensor, table, L)
    assert torch.equal(out.view(torch.uint8), torch.stack([case.tensor[:, s:s + L] for s in starts]).view(torch.uint8))
    into = torch.empty_like(out)
    assert extract_windows(case.tensor, np.asarray(starts), L, out=into) is into
    assert torch.equal(into.view(torch.uint8), out.view(torch.uint8))


def test_bad_windows_are_flagged_and_left_unwritten(dev):
    T, L = 37, 5
    case = _Case(torch.float32, 3, T, 40, dev, seed=3)
    starts = [4, -1, T - L + 1, 2 ** 40, 0]
    got, err = case.launch(starts, L)
    assert err == epoching.BAD_WINDOW == 2                                          # bit 1 of the error word
    got = got.reshape(5, -1)
    assert np.array_equal(got[0], case.want([4], L)) and np.array_equal(got[4], case.want([0], L))
    assert (got[1:4] == PREFILL).all()
    with pytest.raises(IndexError, match=r"window 1 \(start -1"):
        extract_windows(case.tensor, starts, L)
    with pytest.raises(ValueError, match="window length"):
        extract_windows(case.tensor, [0], T + 1)
    assert extract_windows(case.tensor, [], L).shape == (0, 3, L)


def test_offsets_beyond_4_gib(dev):
    T, L, tail = 2 ** 29 + 1000, 400, 1000
    rec = torch.empty((2, T), dtype=torch.float32, device=dev)                      # 4.3 GB; row 1 ends behind 2^32 bytes
    known = torch.from_numpy(np.random.default_rng(4).standard_normal((2, tail)).astype(np.float32)).to(dev)
    rec[:, T - tail:] = known
    starts = [T - tail, T - 517, T - L]
    try:
        out = extract_windows(rec, starts, L)
        want = torch.stack([known[:, s - (T - tail):s - (T - tail) + L] for s in starts])
        assert torch.equal(out, want)
    finally:
        del rec
        torch.cuda.empty_cache()


def test_medium_size_without_a_device_read(dev):
    rng = np.random.default_rng(5)
    host = rng.standard_normal((64, 4096)).astype(np.float32)
    starts = rng.integers(0, 4096 - 400 + 1, 100)
    rec, table = torch.from_numpy(host).to(dev), torch.from_numpy(starts).to(dev)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = extract_windows(rec, table, 400, check=False)                         # starts on the device, no error word read
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert np.array_equal(out.cpu().numpy(), ref.cut(host, starts, 400))
    assert torch.equal(extract_windows(rec, table, 400), out)                       # the checked call: same result


# ---- extract_ecog_audio -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden(golden_dir):
    with np.load(os.path.join(golden_dir, "sample_collection_ref.npz")) as g:
        return {k: g[k] for k in g.files}


def _assert_is_the_reference(got, golden):
    keys = [k[4:] for k in golden if k.startswith("out_")]
    assert sorted(got) == sorted(keys)
    for k in keys:
        want, have = golden[f"out_{k}"], np.asarray(got[k])
        assert have.dtype == want.dtype and have.shape == want.shape and np.array_equal(have, want), k


def test_extract_ecog_audio_equals_the_reference(dev, golden, tmp_path):
    assert os.path.getsize(os.path.join(os.path.dirname(__file__), "golden", "sample_collection_ref.npz")) < 300_000
    intervals, settings = ref.write_golden_blocks(golden, str(tmp_path))
    assert sorted(os.listdir(tmp_path)) == ["B1_ecog.npz", "B1_sound.npz", "B2_ecog.npz", "B2_sound.npz"]
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        got = text_align.extract_ecog_audio(intervals, str(tmp_path), output_path=str(tmp_path / "subject_1.npz"), **settings)
    assert len(caught) == int(golden["n_warnings"]) == 1 and "Reducing rest period end" in str(caught[0].message)
    _assert_is_the_reference(got, golden)
    assert got["syllable"].tolist().count(-1) == 2 and got["tone"].min() == 0       # unknown syllable; tones started at 1
    with np.load(tmp_path / "subject_1.npz") as saved:
        _assert_is_the_reference({k: saved[k] for k in saved.files}, golden)
    # the same recordings handed over in memory, results left on the device
    recordings = {b: {m: (golden[f"b{b}_{m}"], golden[f"b{b}_{m}_sf"]) for m in ("ecog", "sound")} for b in (1, 2)}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = text_align.extract_ecog_audio(intervals, None, recordings=recordings, to_host=False, **settings)
    assert all(isinstance(res[k], torch.Tensor) and res[k].is_cuda for k in ("ecog", "audio", "ecog_rest"))
    _assert_is_the_reference({k: v.cpu().numpy() if isinstance(v, torch.Tensor) else v for k, v in res.items()}, golden)


def test_extract_ecog_audio_errors(dev, golden, tmp_path):
    intervals, settings = ref.write_golden_blocks(golden, str(tmp_path))
    os.remove(tmp_path / "B2_sound.npz")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.raises(ValueError, match="Mismatch between ECoG and audio"):
            text_align.extract_ecog_audio(intervals, str(tmp_path), **settings)
        with pytest.raises(ValueError, match="No valid blocks"):
            text_align.extract_ecog_audio({7: intervals[1]}, str(tmp_path), **settings)
        np.savez(tmp_path / "B2_sound.npz", signal=golden["b2_sound"], sf=golden["b2_sound_sf"])
        with pytest.raises(KeyError, match="Expected key 'data'"):
            text_align.extract_ecog_audio(intervals, str(tmp_path), **settings)
        late = {1: intervals[1].assign(start=intervals[1]["start"] + 4.0)}
        with pytest.raises(ValueError, match=r"exceeds ECoG data length for block 1.*Start: 4697, End: 4897, Data length: 4818"):
            text_align.extract_ecog_audio(late, str(tmp_path), **settings)
        with pytest.raises(ValueError, match="Block 1 yields no whole rest segment"):
            text_align.extract_ecog_audio({1: intervals[1]}, str(tmp_path), **{**settings, "rest_period": (2.0, 2.3)})


def _resident_inputs(tmp_path, dev):
    from decode_tonal_langauge_amd.preprocess.preprocessor import preprocess_signal
    root = str(tmp_path / "raw")
    events = [(3.1 + 0.9 * k, 3.6 + 0.9 * k, 1 + k % 3, "ai"[k % 2]) for k in range(9)]
    raw = np.load(synthetic.write_raw_block(root, block=1, modality="ecog", n_channels=8, seconds=12.0, sf=400.0, seed=1))["data"]
    for start, end, _tone, _syl in events:
        raw[:4, int(start * 400):int(end * 400)] += 20.0                            # channels 0-3 respond to the events
    steps = [{"module": "preprocess.frequency_filter", "params": {"bands": [
        {"method": "butter", "params": {"freqs": [0.3, 100], "filter_type": "bandpass"}}]}},
        {"module": "preprocess.channel_zscore"}]
    filtered, sf = preprocess_signal(torch.from_numpy(raw).to(dev), steps, Namespace(signal_freq=400.0), resident=True)
    assert isinstance(filtered, torch.Tensor) and filtered.is_cuda
    sound = np.load(synthetic.write_raw_block(root, block=1, modality="sound", n_channels=1, seconds=12.0, sf=1200.5, seed=2))
    synthetic.write_block_annotations(str(tmp_path / "tg"), 1, events, seconds=12.0)
    intervals = text_align.handle_textgrids(str(tmp_path / "tg"))
    return filtered, sf, sound["data"], sound["sf"], intervals


def test_resident_chain_into_channel_selection(dev, tmp_path):
    from decode_tonal_langauge_amd.channel_selection import active
    filtered, sf, sound, sound_sf, intervals = _resident_inputs(tmp_path, dev)
    params = {"p_threshold": 0.05, "active_time_threshold": 0.05}
    kwargs = dict(syllables=["a", "i"], length=0.5, rest_period=(0.0, 3.0))
    # the file route: write, read, upload
    files = tmp_path / "files"
    files.mkdir()
    np.savez(files / "B1_ecog.npz", data=filtered.cpu().numpy(), sf=sf)
    np.savez(files / "B1_sound.npz", data=sound, sf=sound_sf)
    by_file = text_align.extract_ecog_audio(intervals, str(files), **kwargs)
    want = active.run(by_file, params)
    # the resident route: nothing of a recording crosses to the host, the host never waits for the device
    recordings = {1: {"ecog": (filtered, np.array(sf)), "sound": (torch.from_numpy(sound).to(dev), sound_sf)}}
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        resident = text_align.extract_ecog_audio(intervals, None, recordings=recordings, to_host=False, **kwargs)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for key in ("ecog", "audio", "ecog_rest"):
        assert resident[key].is_cuda and np.array_equal(resident[key].cpu().numpy(), by_file[key]), key
    assert np.array_equal(resident["tone"], by_file["tone"]) and np.array_equal(resident["syllable"], by_file["syllable"])
    got = active.run(resident, params)
    assert got["selected_channels"] == want["selected_channels"] and got["max_lengths"] == want["max_lengths"]
    assert np.array_equal(got["p_values"], want["p_values"])
    print("active channels:", got["selected_channels"], got["max_lengths"])
    assert len(got["selected_channels"]) > 0 and set(got["selected_channels"]) <= {0, 1, 2, 3}


def test_collect_unlabelled_samples(dev, tmp_path):
    from decode_tonal_langauge_amd.data_loading.dataloaders import collect_unlabelled_samples
    rng = np.random.default_rng(6)
    a, b, c = (rng.standard_normal((3, T)).astype(np.float32) for T in (101, 64, 90))
    os.makedirs(tmp_path / "sub")
    np.savez(tmp_path / "B2_ecog_rest.npz", data=a, sf=400.0)
    np.savez(tmp_path / "sub" / "B1_ecog_rest.npz", data=b, sf=400.0)
    np.savez(tmp_path / "B3_sound_rest.npz", data=c, sf=400.0)                      # filtered out by the keywords
    got = collect_unlabelled_samples(str(tmp_path), patch_size=4, segment_length=16, step_size=5, kwords=["ecog", "rest"])
    assert isinstance(got, np.ndarray) and got.dtype == np.float32
    assert np.array_equal(got, ref.sliding_ref([a, b], 4, 16, 5)) and got.shape == (18 + 10, 3, 4, 4)
    half = collect_unlabelled_samples(str(tmp_path), patch_size=8, segment_length=16, kwords=["ecog"])
    assert np.array_equal(half, ref.sliding_ref([a, b], 8, 16, None))
    everything = collect_unlabelled_samples(str(tmp_path), patch_size=16, segment_length=16, step_size=16)
    assert np.array_equal(everything, ref.sliding_ref([a, c, b], 16, 16, 16))      # sorted walk: top folder, then sub/
    with pytest.raises(ValueError, match=r"segment_length \(16\) must be divisible by patch_size \(5\)"):
        collect_unlabelled_samples(str(tmp_path), patch_size=5, segment_length=16)
    np.savez(tmp_path / "B4_ecog_rest.npz", signal=a)
    with pytest.raises(KeyError, match="Key data cannot be found"):
        collect_unlabelled_samples(str(tmp_path), patch_size=4, segment_length=16, kwords=["ecog"])


def test_stage_end_to_end_and_on_into_channel_selection(dev, tmp_path):
    from decode_tonal_langauge_amd import main
    rec = tmp_path / "preprocessed"
    events = {1: [(1.5 + 0.9 * k, 2.0 + 0.9 * k, 1 + k % 3, "aiu"[k % 3]) for k in range(10)],
              2: [(2.3 + 0.8 * k, 2.7 + 0.8 * k, 2 + k % 2, "ia"[k % 2]) for k in range(8)]}
    raw = {}
    for block, rows in events.items():
        root = str(rec / "subject_1")
        synthetic.write_raw_block(root, block=block, modality="ecog", n_channels=6, seconds=12.0, sf=401.5, seed=block)
        synthetic.write_raw_block(root, block=block, modality="sound", n_channels=1, seconds=12.0, sf=1220.703125, seed=9 + block)
        synthetic.write_block_annotations(str(tmp_path / "tg" / "s1"), block, rows, seconds=12.0, short=block == 2)
        raw[block] = (np.load(os.path.join(root, f"B{block}_ecog.npz")), np.load(os.path.join(root, f"B{block}_sound.npz")))
    (rec / "config.yaml").write_text(yaml.dump({"preprocess": {"module": "preprocess_main"}}))
    cfg = {
        "sample_collection": {"module": "extract_samples", "params": {
            "io": {"recording_dir": str(rec), "textgrid_root": str(tmp_path / "tg"), "output_dir": str(tmp_path / "samples")},
            "settings": {"syllable_identifiers": ["a", "i"], "figures": False},
            "subjects": {1: {"textgrid_dir": "s1", "sample_length": 0.5, "rest_period": [0.0, 1.6], "start_offset": 0.1},
                         2: {"textgrid_dir": "s1", "sample_length": 0.5, "rest_period": [0.0, 1.6]}}}},      # no recordings
        "channel_selection": {"module": "channel_selection_main", "params": {
            "io": {"output_dir": str(tmp_path / "channels")},
            "selections": [{"module": "channel_selection.active", "selection_name": "active_channels",
                            "params": {"p_threshold": 0.05, "active_time_threshold": 0.05}}]}}}
    path = tmp_path / "pipeline.yaml"
    path.write_text(yaml.dump(cfg))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        main.run_pipeline(str(path))
    (out,) = [d for d in os.listdir(tmp_path / "samples") if d.startswith("preprocessed__")]
    out = tmp_path / "samples" / out
    assert sorted(f for f in os.listdir(out) if f.endswith(".npz")) == ["subject_1.npz"]
    carried = yaml.safe_load(open(out / "config.yaml"))
    assert set(carried) == {"preprocess", "sample_collection"}
    with np.load(out / "subject_1.npz") as d:
        got = {k: d[k] for k in d.files}
    # the same subject by slicing on the host
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        tables = text_align.handle_textgrids(str(tmp_path / "tg" / "s1"), start_offset=0.1)
    ecog, audio, rest = [], [], []
    for block in (1, 2):
        e, s = raw[block]
        starts, L = ref.starts_ref(tables[block]["start"].tolist(), e["sf"], 0.5)
        ecog.append(ref.cut(e["data"], starts, L))
        starts, L = ref.starts_ref(tables[block]["start"].tolist(), s["sf"], 0.5)
        audio.append(ref.cut(s["data"], starts, L)[:, 0])
        starts, L = ref.rest_starts_ref((0.0, 1.6), tables[block]["start"].min(), e["sf"], 0.5)
        rest.append(ref.cut(e["data"], starts, L))
    assert np.array_equal(got["ecog"], np.concatenate(ecog)) and got["ecog"].shape == (18, 6, 200)
    assert np.array_equal(got["audio"], np.concatenate(audio)) and np.array_equal(got["ecog_rest"], np.concatenate(rest))
    assert got["syllable"].dtype == np.int8 and got["syllable"].tolist()[:3] == [0, 1, -1]
    assert got["tone"].dtype == np.int64 and got["tone"].min() == 0 and float(got["ecog_sf"]) == 401.5
    # channel selection took the stage's directory
    (chan,) = os.listdir(tmp_path / "channels")
    assert chan.startswith(os.path.basename(out) + "__")
    with open(tmp_path / "channels" / chan / "subject_1.json") as f:
        assert list(json.load(f)) == ["active_channels"]
