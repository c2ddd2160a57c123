"""GPU: the ANOVA kernels (tl_group_moments, tl_anova_finalize, tl_max_run_below) and the channel-selection stage against
scipy.stats.f_oneway run per channel (tests/anova_ref.py).

How the numeric bounds are formed.  ``closed_form`` and ``scipy_loop`` are two float64 CPU evaluations of the same test that
differ in summation order; their largest relative distance over the points with scipy p > 1e-290 is the yardstick's own
floor on that input.  The GPU is allowed 100 times that floor (a third summation order, and the device's log / exp / lgamma
at a few ulp each entering an exponent of magnitude up to ~700), and never more than the hard cap 1e-9, on which the
exclusion rule of the decision tests rests.  Every numeric comparison uses that rule - the main, offset and float32 inputs,
the ragged shapes and the per-group calling form alike; only a floor that comes out as exactly zero is replaced by one ulp
(2^-52), so that the bound is never zero."""
import functools
import json
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

from tests import anova_ref as ar
from tests import parity_record

pytestmark = pytest.mark.gpu
HARD_CAP = 1e-9
ULP = 2.0 ** -52


@functools.lru_cache(maxsize=None)
def _main_input():
    rng = np.random.default_rng(0)
    N, C, T = 480, 256, 600
    x = rng.standard_normal((N, C, T))
    lab = rng.integers(0, 4, N)
    x[:, :40, 200:330] += 0.8 * lab[:, None, None]
    return x, lab


@functools.lru_cache(maxsize=None)
def _main_refs(offset: float):
    x, lab = _main_input()
    x = x + offset if offset else x
    return ar.scipy_loop(x, lab), ar.closed_form(x, lab)


def _deviation(got, ref, mask):
    return ar.rel_floor(np.asarray(got), ref, mask)


def _check_numbers(F, p, scipy_ref, closed, tag):
    """Prints every figure, records it, then asserts GPU deviation <= min(100 x floor, 1e-9) for F and p."""
    Fs, ps = scipy_ref
    mask = np.isfinite(ps) & (ps > 1e-290) & np.isfinite(Fs)
    floor_F = max(ar.rel_floor(closed[0], Fs, mask), ULP)
    floor_p = max(ar.rel_floor(closed[1], ps, mask), ULP)
    dev_F, dev_p = _deviation(F, Fs, mask), _deviation(p, ps, mask)
    print(f"[{tag}] points {int(mask.sum())}  F: floor {floor_F:.3e} gpu {dev_F:.3e}   p: floor {floor_p:.3e} gpu {dev_p:.3e}"
          f"   min scipy p {float(ps[mask].min()):.3e}")
    parity_record.record(f"channel_selection_{tag}", {"F_floor": floor_F, "F_gpu": dev_F, "p_floor": floor_p, "p_gpu": dev_p,
                                                     "points": int(mask.sum())})
    assert np.array_equal(np.isnan(np.asarray(F)), np.isnan(Fs)) and np.array_equal(np.isnan(np.asarray(p)), np.isnan(ps))
    assert dev_F <= 100 * floor_F and dev_F < HARD_CAP, (tag, dev_F, floor_F)
    assert dev_p <= 100 * floor_p and dev_p < HARD_CAP, (tag, dev_p, floor_p)
    return dev_F, dev_p


# ---------------------------------------------------------------------------------------------- numbers
def test_main_input_matches_scipy_within_100_floors():
    from decode_tonal_langauge_amd.channel_selection import anova_oneway
    x, lab = _main_input()
    F, p = anova_oneway(x, lab)
    assert isinstance(F, np.ndarray) and F.shape == p.shape == (256, 600) and F.dtype == p.dtype == np.float64
    scipy_ref, closed = _main_refs(0.0)
    assert scipy_ref[1].min() < 1e-70 and scipy_ref[1].max() > 0.99            # the p-values span 1e-80 .. 1
    _check_numbers(F, p, scipy_ref, closed, "main")


def test_offset_1e4_keeps_the_digits():
    """The main input plus 1e4: raw sums of squares would lose ~8 digits of ss_within; the kernels sum x - shift."""
    from decode_tonal_langauge_amd.channel_selection import anova_oneway
    x, lab = _main_input()
    F, p = anova_oneway(x + 1e4, lab)
    scipy_ref, closed = _main_refs(1e4)
    _check_numbers(F, p, scipy_ref, closed, "offset_1e4")


def test_float32_input_against_scipy_on_the_float64_cast():
    from decode_tonal_langauge_amd.channel_selection import anova_oneway
    x, lab = _main_input()
    x32 = x[:, :64, :].astype(np.float32)
    F, p = anova_oneway(torch.from_numpy(x32).cuda(), lab)
    assert F.is_cuda and F.dtype == torch.float64
    x64 = x32.astype(np.float64)
    _check_numbers(F.cpu().numpy(), p.cpu().numpy(), ar.scipy_loop(x64, lab), ar.closed_form(x64, lab), "float32_input")


_SHAPES = [  # (tag, N, C, T, k)
    ("T_not_multiple_of_64", 50, 3, 77, 3),
    ("one_channel", 40, 1, 130, 4),
    ("two_samples_per_group", 10, 4, 33, 5),
    ("two_groups", 31, 5, 65, 2),
    ("forty_groups", 200, 2, 50, 40),
    ("no_sample_split", 12, 512, 520, 3),        # 266 240 columns: the one-slab path; everything above splits the samples
]


@pytest.mark.parametrize("tag,N,C,T,k", _SHAPES, ids=[s[0] for s in _SHAPES])
def test_ragged_shapes(tag, N, C, T, k):
    from decode_tonal_langauge_amd.channel_selection import anova_oneway
    from decode_tonal_langauge_amd.channel_selection.utils import _splits
    rng = np.random.default_rng(100 + N)
    x = rng.standard_normal((N, C, T))
    lab = rng.permutation(np.arange(N) % k) * 3 - 1                   # every class present; labels need not be 0..k-1
    x += 0.5 * (lab[:, None, None] == lab.min()) * (np.arange(T) < T // 2)
    assert (_splits(C * T, int(np.bincount(lab + 1).max())) == 1) == (tag == "no_sample_split")
    F, p = anova_oneway(x, lab)
    _check_numbers(F, p, ar.scipy_loop(x, lab), ar.closed_form(x, lab), tag)


def test_degenerate_columns_come_out_as_scipy_returns_them():
    from decode_tonal_langauge_amd.channel_selection import anova_oneway
    rng = np.random.default_rng(5)
    N, C, T = 24, 2, 40
    lab = np.arange(N) % 3
    x = rng.standard_normal((N, C, T))
    x[5, 0, 7] = np.nan                              # a NaN in one sample
    x[:, 1, 3] = 2 * lab + 1                         # integer-valued, constant within each group, groups differ
    x[:, 1, 4] = 3.5                                 # constant everywhere
    F, p = anova_oneway(x, lab)
    Fs, ps = ar.scipy_loop(x, lab)
    assert np.isnan(F[0, 7]) and np.isnan(p[0, 7])
    assert F[1, 3] == np.inf and p[1, 3] == 0.0
    assert np.isnan(F[1, 4]) and np.isnan(p[1, 4])
    for got, ref in ((F, Fs), (p, ps)):
        assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(np.isinf(got), np.isinf(ref))
    assert ps[1, 3] == 0.0
    ok = np.isfinite(Fs)
    assert np.max(np.abs(F[ok] - Fs[ok]) / np.abs(Fs[ok])) < HARD_CAP and np.max(np.abs(p[ok] - ps[ok]) / ps[ok]) < HARD_CAP
    # every group of size 1: N = k, NaN (scipy: all-NaN with a warning)
    F1, p1 = anova_oneway(x[:3], np.arange(3))
    assert np.isnan(F1).all() and np.isnan(p1).all()


def test_cuda_tensors_in_cuda_tensors_out():
    from decode_tonal_langauge_amd.channel_selection import anova_oneway
    rng = np.random.default_rng(9)
    x = rng.standard_normal((60, 6, 90))
    lab = rng.integers(0, 3, 60)
    F_np, p_np = anova_oneway(x, lab)
    xd = torch.from_numpy(x).cuda()
    F, p = anova_oneway(xd, torch.from_numpy(lab).cuda())
    assert F.is_cuda and p.is_cuda and F.shape == (6, 90)
    assert np.array_equal(F.cpu().numpy(), F_np) and np.array_equal(p.cpu().numpy(), p_np)
    # one tensor per group (unequal sizes), the scipy.stats.f_oneway calling form
    groups = [xd[lab == v] for v in range(3)]
    Fg, pg = anova_oneway(groups)
    assert Fg.is_cuda and pg.is_cuda
    host_groups = [x[lab == v] for v in range(3)]
    _check_numbers(Fg.cpu().numpy(), pg.cpu().numpy(), ar.scipy_loop(host_groups), ar.closed_form(host_groups), "per_group_form")
    with pytest.raises(RuntimeError, match="no CPU"):
        anova_oneway(torch.from_numpy(x), lab)
    # two groups of different dtype (4 and 6 samples of the smallest ragged shape): float32 widens exactly, so both tests
    # return, bit for bit, what they return on the float64 casts
    from decode_tonal_langauge_amd.channel_selection import kruskal_oneway
    _, N, C, T, _ = min(_SHAPES, key=lambda s: s[1] * s[2] * s[3])
    y = np.random.default_rng(100 + N).standard_normal((N, C, T))
    y[:4] += 0.5
    mixed = [y[:4].astype(np.float32), y[4:]]
    for oneway in (anova_oneway, kruskal_oneway):
        got, want = oneway(mixed), oneway([g.astype(np.float64) for g in mixed])
        assert got[0].shape == (C, T) and np.isfinite(want[1]).all() and want[1].min() < want[1].max()
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


# ---------------------------------------------------------------------------------------------- run lengths
def test_max_run_below_against_get_max_length():
    from decode_tonal_langauge_amd.channel_selection import get_max_length, max_run_below
    rng = np.random.default_rng(11)
    for C, T, thr in ((37, 600, 0.5), (5, 1, 0.5), (9, 63, 0.9), (9, 64, 0.9), (9, 65, 0.9), (12, 1000, 0.97), (3, 4097, 0.995),
                      (130, 640, 0.8)):
        p = rng.random((C, T))
        p[0, :] = 0.0                                                  # all below: one run through every lane chunk
        if C > 2:
            p[1, :] = 1.0                                              # none below
            p[2, T // 3:] = 0.0                                        # a run to the end, across chunk boundaries
        if T > 20:
            p[-1, 5:17] = np.nan                                       # NaN is not below
            p[-1, 17] = thr                                            # equal is not below
        count, longest = max_run_below(torch.from_numpy(p).cuda(), thr)
        assert count.dtype == longest.dtype == torch.int32 and count.shape == (C,)
        count, longest = count.cpu().numpy(), longest.cpu().numpy()
        for c in range(C):
            below = np.where(p[c] < thr)[0]
            assert count[c] == len(below), (C, T, c)
            assert longest[c] == (get_max_length(below) if len(below) else 0) == (ar.max_length(below) if len(below) else 0), (C, T, c)


# ---------------------------------------------------------------------------------------------- decisions
def test_discriminative_decisions_equal_the_reference_logic_on_scipy_p_values():
    """Length thresholds below (128), at (129, 130) and above (256) the planted run of 130 samples."""
    from decode_tonal_langauge_amd.channel_selection import discriminative, max_run_below
    x, lab = _main_input()
    (_, ps), _ = _main_refs(0.0)
    data = {"ecog": x, "ecog_sf": np.array(128), "tone": lab[:, None]}
    thr = 0.05 / 600
    picked = {}
    for att in (1.0, 129 / 128, 130 / 128, 2.0):
        res = discriminative.run(data, {"target": "tone", "p_threshold": 0.05, "active_time_threshold": att})
        selected, runs, near = ar.reference_selection(ps, thr, int(att * 128))
        assert near == 0                                               # no point is left out of the comparison
        assert res["selected_channels"] == selected and res["max_lengths"] == []
        assert all(isinstance(c, int) for c in res["selected_channels"])
        assert res["p_values"].shape == (256, 600)
        _, longest = max_run_below(torch.from_numpy(res["p_values"]).cuda(), thr)
        assert longest.cpu().numpy().tolist() == runs
        picked[int(att * 128)] = selected
    assert picked[128] == picked[129] == list(range(40)) and picked[130] == picked[256] == []
    out = discriminative.test_discriminative_power(data, {"target": "tone"})
    assert set(out) == {"f_stat", "p_value"} and np.array_equal(out["p_value"], res["p_values"])


def _active_input():
    rng = np.random.default_rng(3)
    C, T = 64, 200
    rest = rng.standard_normal((300, C, T))
    erp = rng.standard_normal((200, C, T))
    erp[:, :10, 50:120] += 0.6                                         # a response of 70 samples in 10 channels
    erp[:, 10:14, 80:100] += 0.6                                       # a short one of 20 samples in 4 more
    return rest, erp


def test_active_decisions_equal_the_reference_logic_on_scipy_p_values():
    from decode_tonal_langauge_amd.channel_selection import active
    rest, erp = _active_input()
    _, ps = ar.scipy_loop([rest, erp])
    thr = 0.05 / 200
    data = {"ecog": erp, "ecog_rest": rest, "ecog_sf": np.array(100)}
    expected = {}
    for att in (0.1, 0.5, 0.9):                                        # lengths 10 (both responses), 50 (the long one, where noise has not cut it), 90
        res = active.run(data, {"p_threshold": 0.05, "active_time_threshold": att})
        length = int(att * 100)
        selected, runs, near = ar.reference_selection(ps, thr, length)
        assert near == 0
        assert res["selected_channels"] == selected and res["max_lengths"] == [runs[c] for c in selected]
        mask = ps[-1] > 1e-290
        assert res["p_values"].shape == (200,) and ar.rel_floor(res["p_values"], ps[-1], mask) < HARD_CAP   # last channel only
        expected[length] = selected
    assert expected[10] == list(range(14)) and 0 < len(expected[50]) <= 10 and max(expected[50]) < 10 and expected[90] == []
    with pytest.raises(ValueError, match="Shape mismatch"):
        active.run({"ecog": erp[:, :5], "ecog_rest": rest, "ecog_sf": 100}, {"p_threshold": 0.05, "active_time_threshold": 0.1})


# ---------------------------------------------------------------------------------------------- the stage
def test_stage_end_to_end_equals_the_json_built_from_scipy(tmp_path, monkeypatch):
    from decode_tonal_langauge_amd import channel_selection_main, train_classifier
    from decode_tonal_langauge_amd.channel_selection import utils as cs_utils
    from decode_tonal_langauge_amd.data_loading import synthetic
    from decode_tonal_langauge_amd.data_loading.sample_loading import ClassificationSampleHandler
    written = synthetic.write_dataset(str(tmp_path / "data"))
    sample_dir = written["sample_dir"]
    selections = [
        {"module": "channel_selection.active", "selection_name": "active_channels",
         "params": {"p_threshold": 0.05, "active_time_threshold": 0.05}},
        {"module": "channel_selection.discriminative", "selection_name": "tone_discriminative",
         "params": {"target": "tone", "recording_name": "ecog", "p_threshold": 0.05, "active_time_threshold": 0.1}},
        {"module": "channel_selection.discriminative", "selection_name": "syllable_discriminative",
         "params": {"target": "syllable", "recording_name": "ecog", "p_threshold": 0.05, "active_time_threshold": 0.1}}]
    uploads = []
    real_to_device = cs_utils.to_device
    monkeypatch.setattr(cs_utils, "to_device", lambda a, what: uploads.append(what) or real_to_device(a, what))
    out = channel_selection_main.run({"channel_selection": {"module": "channel_selection_main", "params": {
        "io": {"sample_dir": sample_dir, "output_dir": str(tmp_path / "channels")}, "selections": selections}}})
    assert len(uploads) == 2                                           # ecog and ecog_rest once each for three selections
    with open(os.path.join(out, "subject_1.json")) as f:
        got = json.load(f)
    d = np.load(os.path.join(sample_dir, "subject_1.npz"))
    ecog, rest = d["ecog"].astype(np.float64), d["ecog_rest"].astype(np.float64)
    T, sf = ecog.shape[2], int(d["ecog_sf"])
    want, near_total = {}, 0
    _, p_active = ar.scipy_loop([rest, ecog])
    want["active_channels"], _, near = ar.reference_selection(p_active, 0.05 / T, int(0.05 * sf))
    near_total += near
    for target in ("tone", "syllable"):
        _, p_t = ar.scipy_loop(ecog, d[target])
        want[f"{target}_discriminative"], _, near = ar.reference_selection(p_t, 0.05 / T, int(0.1 * sf))
        near_total += near
    assert near_total == 0
    assert got == want and len(want["tone_discriminative"]) > 0
    assert os.path.isfile(os.path.join(out, "config.yaml")) and os.path.isdir(os.path.join(out, "figures", "active_channels", "subject_1"))
    # the training stage's loader takes the directory as channel_selection_dir
    sp = train_classifier._prepare_subject_params(Namespace(sample_dir=sample_dir, channel_selection_dir=out), "1")
    assert sp.channel_file == os.path.join(out, "subject_1.json")
    sp.targets, sp.features = ["tone"], "ecog"
    loaded = ClassificationSampleHandler(sp).load_data()
    assert loaded["selected_channels"].tolist() == want["tone_discriminative"]
    assert loaded["features"].shape == (ecog.shape[0], len(want["tone_discriminative"]), T)
