"""GPU: the label-permutation test for channel selection (tl_perm_exceed, tl_perm_runs, the helpers of
channel_selection.utils, the selector and the stage) against the NumPy oracle of tests/permutation_ref.py.

Everything is compared for EQUALITY: the mask cell for cell, the runs, both p-vectors, the selections.  That is sound because
of the exclusion rule the host tests enforce on the same inputs (tests/test_permutation_selection_host.py): the oracle alone
puts every cell at least 1e-7 (relative) away from the decision - the margins observed are >= 1.6e-5 - while the float64 sums
of the kernel and of the oracle differ by rounding only, about 1e-13 after the cancellation in ssb."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from tests import parity_record
from tests import permutation_ref as pr

pytestmark = pytest.mark.gpu


def _arrays(c):
    x = torch.tensor(c["x"]).cuda()                                        # a copy: the cached case is read-only
    return [x] if c["n0"] is None else [x[:c["n0"]].contiguous(), x[c["n0"]:].contiguous()]


@pytest.mark.parametrize("name", list(pr.CASES))
def test_mask_runs_and_p_values_equal_the_oracle(name):
    from decode_tonal_langauge_amd.channel_selection import permutation_p_values, permutation_runs
    from decode_tonal_langauge_amd.channel_selection.utils import permutation_exceedances
    c = pr.case(name)
    want_mask, want_runs, want_pc, want_pm = pr.expected(name)
    arrays = _arrays(c)
    assert len(arrays) == (1 if c["n0"] is None else 2) and str(arrays[0].dtype).endswith(pr.CASES[name]["dtype"])
    mask = permutation_exceedances(arrays, c["table"], c["counts"], c["alpha_cell"])
    assert mask.is_cuda and mask.dtype == torch.bool and mask.shape == want_mask.shape
    runs, f_crit, theta = permutation_runs(arrays, c["table"], c["counts"], c["alpha_cell"])
    assert runs.is_cuda and runs.dtype == torch.int32 and runs.shape == want_runs.shape
    mask, runs = mask.cpu().numpy(), runs.cpu().numpy()
    p_channel, p_max = permutation_p_values(runs)
    wrong = int((mask != want_mask).sum())
    print(f"[{name}] cells {mask.size} set {int(want_mask.sum())} wrong {wrong}  runs wrong {int((runs != want_runs).sum())}"
          f"  observed runs {want_runs[0].tolist()}  f_crit {f_crit:.6g} theta {theta:.6g}")
    parity_record.record(f"permutation_selection_{name}", {
        "cells": mask.size, "cells_set": int(want_mask.sum()), "cells_wrong": wrong,
        "runs_wrong": int((runs != want_runs).sum()), "oracle_margin": pr.margin(c["x64"], c["table"], c["counts"], c["theta"])})
    assert (f_crit, theta) == (c["f_crit"], c["theta"])
    assert np.array_equal(mask, want_mask)
    assert np.array_equal(runs, want_runs)
    assert np.array_equal(p_channel, want_pc) and np.array_equal(p_max, want_pm)
    if "nan_channel" in pr.CASES[name]:
        assert not mask[:, 2:].any() and (p_channel[2:] == 1.0).all() and (p_max[2:] == 1.0).all()


@pytest.mark.parametrize("name", ["two_groups_ragged_rows", "four_groups_f64", "rest_erp_offset_1e4"])
def test_chunks_of_16_relabellings_give_the_result_of_one_chunk(name):
    from decode_tonal_langauge_amd.channel_selection import permutation_runs
    from decode_tonal_langauge_amd.channel_selection.utils import permutation_exceedances
    c = pr.case(name)
    arrays = _arrays(c)
    P = c["table"].shape[0]
    assert P > 16 and P % 16 != 0                                          # several chunks, the last one short
    one = permutation_runs(arrays, c["table"], c["counts"], c["alpha_cell"], perm_chunk=P)[0]
    for chunk in (16, 1000):
        assert torch.equal(one, permutation_runs(arrays, c["table"], c["counts"], c["alpha_cell"], perm_chunk=chunk)[0])
    assert torch.equal(permutation_exceedances(arrays, c["table"], c["counts"], c["alpha_cell"], perm_chunk=P),
                       permutation_exceedances(arrays, c["table"], c["counts"], c["alpha_cell"], perm_chunk=16))
    assert np.array_equal(one.cpu().numpy(), pr.expected(name)[1])


def test_a_label_outside_the_groups_contributes_to_no_group():
    """With samples that belong to no group the group sums no longer add up to the total, so the statistic depends on the
    frame the sums are taken in: the expectation is formed in the kernel's frame, x - sample 0, as the header defines it."""
    from decode_tonal_langauge_amd.channel_selection.utils import permutation_exceedances
    c = pr.case("three_groups_loose")
    table = c["table"].copy()
    table[3, ::5] = 200                                                    # dropped samples in one relabelling
    table[7, 2] = 3                                                        # the first value that names no group
    N, Cn, T = c["x64"].shape
    d = (c["x64"] - c["x64"][0]).reshape(N, Cn * T)
    total = d.sum(axis=0)
    tau = c["theta"] * ((d * d).sum(axis=0) - total * total / N) + total * total / N
    stat = sum(((table == g).astype(np.float64) @ d) ** 2 / n_g for g, n_g in enumerate(c["counts"]))
    assert np.min(np.abs(stat - tau) / np.abs(tau)[None, :]) >= pr.MARGIN_FLOOR
    want = (stat > tau).reshape(-1, Cn, T)
    untouched = [r for r in range(table.shape[0]) if r not in (3, 7)]
    assert np.array_equal(want[untouched], pr.expected("three_groups_loose")[0][untouched])
    assert not np.array_equal(want[[3, 7]], pr.expected("three_groups_loose")[0][[3, 7]])
    got = permutation_exceedances(_arrays(c), table, c["counts"], c["alpha_cell"])
    assert np.array_equal(got.cpu().numpy(), want)


def test_perm_runs_on_masks_of_every_row_length():
    from decode_tonal_langauge_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(21)
    for rows, T, density in ((5, 1, 0.5), (9, 63, 0.9), (9, 64, 0.9), (9, 65, 0.9), (7, 128, 0.97), (6, 257, 0.8),
                             (130, 600, 0.95), (3, 4097, 0.995)):
        m = (rng.random((rows, T)) < density).astype(np.uint8)
        m[0, :] = 1                                                        # one run through every 64-cell step
        if rows > 2:
            m[1, :] = 0
            m[2, :T // 3] = 0
            m[2, T // 3:] = 7                                              # any non-zero byte is set; a run to the row's end
        d = torch.from_numpy(m).cuda()
        out = torch.full((rows,), -1, dtype=torch.int32, device="cuda")
        _lib.check(lib.tl_perm_runs(d.data_ptr(), rows, T, out.data_ptr(), _lib.stream_ptr()), "tl_perm_runs")
        assert np.array_equal(out.cpu().numpy(), pr.runs_ref(m[None] != 0)[0]), (rows, T)


def test_the_entry_point_on_a_column_count_that_is_no_multiple_of_the_tile():
    """cols = 5 * 37 = 185 of the first case: the mask's buffer is followed by a canary the launch must leave alone."""
    from decode_tonal_langauge_amd import _lib
    lib = _lib.load()
    c = pr.case("three_groups_loose")
    x = _arrays(c)[0]
    N, Cn, T = x.shape
    cols, P, k = Cn * T, c["table"].shape[0], c["k"]
    d = x.double().reshape(N, cols)
    shift = x[0].reshape(cols).contiguous()
    S = (d - shift).sum(dim=0)
    sst = ((d - shift) ** 2).sum(dim=0) - S * S / N
    tau = (c["theta"] * sst + S * S / N).contiguous()
    labels = torch.tensor(c["table"]).cuda()
    buf = torch.full((P * cols + 256,), 77, dtype=torch.uint8, device="cuda")
    cnt = (C.c_int32 * k)(*c["counts"])
    _lib.check(lib.tl_perm_exceed(x.data_ptr(), N, None, 0, 1, cols, shift.data_ptr(), labels.data_ptr(), P, cnt, k,
                                  tau.data_ptr(), buf.data_ptr(), _lib.stream_ptr()), "tl_perm_exceed")
    buf = buf.cpu().numpy()
    assert (buf[P * cols:] == 77).all()
    assert np.array_equal(buf[:P * cols].reshape(P, Cn, T), pr.expected("three_groups_loose")[0].astype(np.uint8))


# ---------------------------------------------------------------------------------------------- the selector
@pytest.mark.parametrize("correction", ["max", "channel"])
def test_selector_equals_the_oracle_selection_in_both_forms(correction):
    from decode_tonal_langauge_amd.channel_selection import permutation
    # labelled form
    c = pr.case("four_groups_f64")
    spec = pr.CASES["four_groups_f64"]
    n_perm, seed = spec["P"] - 1, 100 + spec["seed"]
    labels = c["group_index"] * 3 + 5                                      # class values need not be 0..k-1
    res = permutation.run({"ecog": c["x"].copy(), "ecog_sf": np.array(100), "tone": labels[:, None]},
                          {"target": "tone", "p_threshold": spec["p_threshold"], "n_permutations": n_perm, "seed": seed,
                           "alpha": 0.1, "correction": correction, "perm_chunk": 16})
    _, runs, _, _ = pr.expected("four_groups_f64")
    selected, p = pr.selection_ref(runs, 0.1, correction)
    assert set(res) == {"selected_channels", "max_lengths", "p_values", "null_max_lengths", "f_crit"}
    assert res["selected_channels"] == selected and all(isinstance(ch, int) for ch in res["selected_channels"])
    assert res["max_lengths"] == [int(runs[0, ch]) for ch in selected]
    assert np.array_equal(res["p_values"], p) and res["p_values"].dtype == np.float64
    assert np.array_equal(res["null_max_lengths"], runs[1:].max(axis=1)) and res["null_max_lengths"].shape == (n_perm,)
    assert res["f_crit"] == c["f_crit"]
    assert {0, 1} <= set(selected) and len(selected) < c["x"].shape[1]    # the planted channels, and not every channel
    # rest against ERP: two arrays, no concatenated copy
    c = pr.case("rest_erp_offset_1e4")
    spec = pr.CASES["rest_erp_offset_1e4"]
    res = permutation.run({"ecog_rest": c["x"][:c["n0"]].copy(), "ecog": c["x"][c["n0"]:].copy(), "ecog_sf": np.array(100)},
                          {"p_threshold": spec["p_threshold"], "n_permutations": spec["P"] - 1, "seed": 100 + spec["seed"],
                           "alpha": 0.1, "correction": correction})
    _, runs, _, _ = pr.expected("rest_erp_offset_1e4")
    selected, p = pr.selection_ref(runs, 0.1, correction)
    assert res["selected_channels"] == selected and np.array_equal(res["p_values"], p)
    assert res["max_lengths"] == [int(runs[0, ch]) for ch in selected]
    assert {0, 1} <= set(selected)


def test_cpu_tensors_are_refused():
    from decode_tonal_langauge_amd.channel_selection import permutation_runs
    c = pr.case("three_groups_loose")
    with pytest.raises(RuntimeError, match="no CPU"):
        permutation_runs([torch.tensor(c["x64"])], c["table"], c["counts"], c["alpha_cell"])


# ---------------------------------------------------------------------------------------------- the stage
def test_stage_writes_the_oracles_selection_for_both_forms(tmp_path):
    from decode_tonal_langauge_amd import channel_selection_main
    from decode_tonal_langauge_amd.data_loading import synthetic
    written = synthetic.write_dataset(str(tmp_path / "data"))
    sample_dir = written["sample_dir"]
    path = os.path.join(sample_dir, "subject_1.npz")
    with np.load(path) as f:
        d = {key: f[key] for key in f.files}
    # the synthetic subject responds in every channel; the upper half becomes noise so that there is something to reject
    planted = list(range(d["ecog"].shape[1] // 2))
    rng = np.random.default_rng(77)
    d["ecog"][:, len(planted):, :] = rng.standard_normal(d["ecog"][:, len(planted):, :].shape).astype(d["ecog"].dtype)
    np.savez(path, **d)
    prm = {"p_threshold": 0.05, "n_permutations": 40, "seed": 11, "alpha": 0.05}
    selections = [
        {"module": "channel_selection.permutation", "selection_name": "tone_permutation",
         "params": dict(prm, target="tone", recording_name="ecog", correction="max")},
        {"module": "channel_selection.permutation", "selection_name": "active_permutation",
         "params": dict(prm, correction="channel", perm_chunk=16)}]
    out = channel_selection_main.run({"channel_selection": {"module": "channel_selection_main", "params": {
        "io": {"sample_dir": sample_dir, "output_dir": str(tmp_path / "channels")}, "selections": selections}}})
    with open(os.path.join(out, "subject_1.json")) as f:
        got = json.load(f)
    ecog, rest = d["ecog"].astype(np.float64), d["ecog_rest"].astype(np.float64)
    T = ecog.shape[2]
    want = {}
    for name, x, group_index, correction in (
            ("tone_permutation", ecog, np.unique(d["tone"], return_inverse=True)[1], "max"),
            ("active_permutation", np.concatenate([rest, ecog]), np.repeat([0, 1], [len(rest), len(ecog)]), "channel")):
        counts = np.bincount(group_index).tolist()
        table = pr.table_ref(group_index, 40, seed=11)
        _, theta = pr.theta_of(0.05 / T, len(counts), len(group_index))
        assert pr.margin(x, table, counts, theta) >= pr.MARGIN_FLOOR
        want[name] = pr.selection_ref(pr.runs_ref(pr.exceed_ref(x, table, counts, theta)), 0.05, correction)[0]
    print(f"[stage] {want}")
    assert got == want
    assert set(planted) <= set(got["tone_permutation"]) and set(planted) <= set(got["active_permutation"])
    assert len(got["tone_permutation"]) < ecog.shape[1]
    assert os.path.isdir(os.path.join(out, "figures", "tone_permutation", "subject_1"))
