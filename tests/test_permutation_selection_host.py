"""CPU: the host side of the label-permutation selector - the two entry points' wiring and argument checks, the YAML name, the
relabelling table, the p-value helper, the selector's parameter errors - and the oracle of the GPU tests held against
``scipy.stats.f_oneway`` on every input those tests use, with the margin that lets them demand equality."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import permutation_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"tl_perm_exceed": 14, "tl_perm_runs": 5}


def test_entry_points_are_declared_bound_and_exported():
    from decode_tonal_langauge_amd import _lib
    lib = _lib.load()
    with open(os.path.join(ROOT, "include", "tonal_hip.h")) as f:
        header = f.read()
    for name, nargs in NEW.items():
        assert re.search(rf"\bint\s+{name}\s*\(", header), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
    with open(os.path.join(ROOT, "README.md")) as f:
        count = int(re.search(r"(\d+) entry points", f.read()).group(1))
    assert count == len(re.findall(r"^int\s+tl_\w+\s*\(", header, flags=re.M)) + \
        len(re.findall(r"^const char\*\s+tl_\w+\s*\(", header, flags=re.M))


def test_entry_points_refuse_null_pointers_and_bad_sizes_without_gpu():
    from decode_tonal_langauge_amd import _lib
    lib = _lib.load()
    err = lib.tl_last_error
    cnt = (C.c_int32 * 3)(7, 8, 9)

    # tl_perm_exceed(x0, n0, x1, n1, is_f64, cols, shift, labels, P, counts, k, tau, exceed, stream)
    def exceed(x0=16, n0=24, x1=None, n1=0, cols=8, shift=16, labels=16, P=4, counts=cnt, k=3, tau=16, out=16):
        return lib.tl_perm_exceed(x0, n0, x1, n1, 1, cols, shift, labels, P, counts, k, tau, out, None)
    for kw in ({"x0": None}, {"shift": None}, {"labels": None}, {"counts": None}, {"tau": None}, {"out": None}):
        assert exceed(**kw) == -1 and b"null" in err(), kw
    assert exceed(n0=0) == -1 and b"n0" in err()
    assert exceed(n0=20, n1=4) == -1 and b"x1" in err()                   # a second array's rows without the array
    assert exceed(n1=-1) == -1
    assert exceed(cols=0) == -1 and b"cols" in err()
    assert exceed(P=0) == -1 and b"P" in err()
    assert exceed(k=1) == -1 and b"[2, 64]" in err()
    assert exceed(k=65) == -1 and b"[2, 64]" in err()
    assert exceed(n0=25) == -1 and b"add up" in err()                     # 7 + 8 + 9 != 25
    assert exceed(n0=20, x1=16, n1=5) == -1 and b"add up" in err()
    assert exceed(counts=(C.c_int32 * 3)(24, 0, 0)) == -1 and b"at least one sample" in err()
    assert exceed(cols=1 << 40, P=1 << 30) == -1 and b"too many blocks" in err()
    # tl_perm_runs(mask, rows, T, maxrun, stream)
    assert lib.tl_perm_runs(None, 4, 8, 16, None) == -1 and b"null" in err()
    assert lib.tl_perm_runs(16, 4, 8, None, None) == -1 and b"null" in err()
    assert lib.tl_perm_runs(16, 0, 8, 16, None) == -1 and b"at least 1" in err()
    assert lib.tl_perm_runs(16, 4, 0, 16, None) == -1 and b"at least 1" in err()
    assert lib.tl_perm_runs(16, 4, 1 << 31, 16, None) == -1
    assert lib.tl_perm_runs(16, 1 << 34, 8, 16, None) == -1 and b"too many rows" in err()


def test_yaml_name_resolves_and_helpers_are_exported():
    from decode_tonal_langauge_amd import channel_selection, channel_selection_main
    mod = channel_selection_main.resolve_selection_module("channel_selection.permutation")
    assert mod.__name__ == "decode_tonal_langauge_amd.channel_selection.permutation"
    assert callable(mod.run) and callable(mod.generate_figures)
    for name in ("permutation_table", "permutation_runs", "permutation_p_values"):
        assert callable(getattr(channel_selection, name))
    from decode_tonal_langauge_amd.channel_selection import utils
    assert utils.PERM_SAMPLE_CHUNK == pr.SAMPLE_CHUNK                     # the tests' N = chunk + 1 is the kernel's
    with open(os.path.join(ROOT, "decode_tonal_langauge_amd", "csrc", "tonal_anova.hip")) as f:
        assert re.search(rf"#define PX_KC {pr.SAMPLE_CHUNK}\b", f.read())


def test_permutation_table():
    from decode_tonal_langauge_amd.channel_selection import permutation_table
    g = np.array([2, 0, 1, 1, 0, 2, 2, 1, 0, 2, 1])
    t = permutation_table(g, 25, seed=3)
    assert t.dtype == np.uint8 and t.shape == (26, 11)
    assert np.array_equal(t[0], g)                                         # row 0 is the labelling
    for row in t:
        assert np.array_equal(np.bincount(row, minlength=3), np.bincount(g, minlength=3))    # every row keeps the class counts
    assert np.array_equal(t, permutation_table(g, 25, seed=3))            # deterministic
    assert np.array_equal(t, pr.table_ref(g, 25, seed=3))                 # default_rng(seed).permutation drawn in order
    assert not np.array_equal(t[1:], permutation_table(g, 25, seed=4)[1:])
    assert np.array_equal(t[:6], permutation_table(g, 5, seed=3))         # a longer table continues a shorter one
    assert permutation_table(g, 0).shape == (1, 11)
    with pytest.raises(ValueError):
        permutation_table(np.array([0, 64]), 3)
    with pytest.raises(ValueError):
        permutation_table(np.array([0.0, 1.0]), 3)


@pytest.mark.parametrize("name", list(pr.CASES))
def test_oracle_equals_f_oneway_cell_for_cell(name):
    from decode_tonal_langauge_amd.channel_selection import permutation_table
    c = pr.case(name)
    # the relabellings are the ones the package draws for this labelling
    assert np.array_equal(c["table"], permutation_table(c["group_index"], pr.CASES[name]["P"] - 1, 100 + pr.CASES[name]["seed"]))
    mask = pr.expected(name)[0]
    assert mask.shape == (pr.CASES[name]["P"],) + pr.CASES[name]["shape"][1:]
    assert np.array_equal(mask, pr.scipy_exceed(c["x64"], c["table"], c["k"], c["alpha_cell"]))
    if "nan_channel" not in pr.CASES[name]:
        assert mask[0, :min(2, mask.shape[1])].any() and not mask.all()   # both outcomes occur
    for row in c["table"]:
        assert np.array_equal(np.bincount(row, minlength=c["k"]), c["counts"])


@pytest.mark.parametrize("name", list(pr.CASES))
def test_inputs_keep_the_margin_of_the_equality_tests(name):
    from decode_tonal_langauge_amd.channel_selection.utils import critical_values
    c = pr.case(name)
    # the margin is taken at the threshold the package itself forms
    assert critical_values(c["alpha_cell"], c["k"], c["x"].shape[0]) == (c["f_crit"], c["theta"])
    m = pr.margin(c["x64"], c["table"], c["counts"], c["theta"])
    print(f"[{name}] margin {m:.3e}")
    assert m >= pr.MARGIN_FLOOR


def test_cases_have_the_properties_they_are_named_for():
    from decode_tonal_langauge_amd.channel_selection import utils
    assert utils.PERM_SAMPLE_CHUNK == pr.SAMPLE_CHUNK
    _, runs, _, _ = pr.expected("four_groups_f64")
    mask = pr.expected("four_groups_f64")[0]
    assert (mask[0, :2, 63] & mask[0, :2, 64]).any() and runs[0, :2].max() > 2      # an observed run crosses timepoint 64
    mask32 = pr.expected("four_groups_f32")[0]
    assert (mask32[0, :2, 63] & mask32[0, :2, 64]).any()
    c = pr.case("two_groups_ragged_rows")
    assert (c["table"].shape[0] * c["k"]) % 16 != 0                       # (relabelling, group) rows: no multiple of 16
    for name in ("chunk_plus_one_T257", "chunk_plus_one_T33"):
        c = pr.case(name)
        assert c["x"].shape[0] == pr.SAMPLE_CHUNK + 1 and min(c["counts"]) == 1 and c["k"] == 5
    mask, runs, p_channel, p_max = pr.expected("nan_and_constant_channels")
    assert not mask[:, 2:].any() and (runs[:, 2:] == 0).all()
    assert (p_channel[2:] == 1.0).all() and (p_max[2:] == 1.0).all()
    assert pr.case("rest_erp_offset_1e4")["x64"].mean() > 9e3


def test_permutation_p_values_on_a_hand_written_table():
    from decode_tonal_langauge_amd.channel_selection import permutation_p_values
    runs = np.array([[5, 2, 0, 9],          # observed
                     [1, 2, 0, 3],
                     [6, 0, 0, 1],
                     [0, 3, 0, 5],
                     [2, 1, 0, 0]], dtype=np.int32)
    p_channel, p_max = permutation_p_values(runs)
    assert p_channel.dtype == p_max.dtype == np.float64 and p_channel.shape == p_max.shape == (4,)
    # per channel: relabellings with a run >= the observed one; channel 2 (observed 0) is reached by every one
    assert p_channel.tolist() == [(1 + 1) / 5, (1 + 2) / 5, (1 + 4) / 5, (1 + 0) / 5]
    # the null maxima are 3, 6, 5, 2
    assert p_max.tolist() == [(1 + 2) / 5, (1 + 4) / 5, (1 + 4) / 5, (1 + 0) / 5]
    for got, want in zip(permutation_p_values(torch.from_numpy(runs)), pr.p_values_ref(runs)):
        assert np.array_equal(got, want)
    only = permutation_p_values(runs[:1])                                  # no relabelling: p = 1
    assert only[0].tolist() == [1.0] * 4 and only[1].tolist() == [1.0] * 4


def test_selector_parameter_errors_before_touching_the_gpu():
    from decode_tonal_langauge_amd.channel_selection import permutation
    x = np.zeros((6, 2, 5))
    lab = np.arange(6) % 2
    labelled = {"ecog": x, "ecog_sf": 100, "tone": lab}
    pair = {"ecog": x, "ecog_rest": x, "ecog_sf": 100}
    for data, base in ((labelled, {"target": "tone"}), (pair, {})):
        with pytest.raises(ValueError, match="n_permutations"):
            permutation.run(data, dict(base, n_permutations=0))
        with pytest.raises(ValueError, match="alpha"):
            permutation.run(data, dict(base, alpha=0.0))
        with pytest.raises(ValueError, match="alpha"):
            permutation.run(data, dict(base, alpha=1.5))
        with pytest.raises(ValueError, match="correction"):
            permutation.run(data, dict(base, correction="fdr"))
        with pytest.raises(ValueError, match="p_threshold"):
            permutation.run(data, dict(base, p_threshold=5.0))             # 5.0 / 5 timepoints = 1
    # the labelled form raises what `discriminative` raises
    with pytest.raises(ValueError, match="sampling frequency"):
        permutation.run({"ecog": x, "tone": lab}, {"target": "tone"})
    with pytest.raises(KeyError, match="Recording 'hga' not found"):
        permutation.run({"ecog": x, "hga_sf": 100}, {"target": "tone", "recording_name": "hga"})
    with pytest.raises(ValueError, match="must be a 3D array"):
        permutation.run({"ecog": x[0], "ecog_sf": 100}, {"target": "tone"})
    with pytest.raises(KeyError, match="Labels 'tone' not found"):
        permutation.run({"ecog": x, "ecog_sf": 100}, {"target": "tone"})
    with pytest.raises(ValueError, match="must be a 1D array"):
        permutation.run({"ecog": x, "ecog_sf": 100, "tone": np.zeros((2, 3), dtype=int)}, {"target": "tone"})
    with pytest.raises(ValueError, match=r"\(5\) does not match"):
        permutation.run({"ecog": x, "ecog_sf": 100, "tone": np.arange(5)}, {"target": "tone"})
    with pytest.raises(ValueError, match="must be integers"):
        permutation.run({"ecog": x, "ecog_sf": 100, "tone": np.arange(6) / 2}, {"target": "tone"})
    # the form without a target raises what `active` raises
    with pytest.raises(ValueError, match="sampling frequency"):
        permutation.run({"ecog": x, "ecog_rest": x}, {})
    with pytest.raises(KeyError, match="Recording 'ecog_rest' not found"):
        permutation.run({"ecog": x, "ecog_sf": 100}, {})
    with pytest.raises(KeyError, match="Recording 'erp' not found"):
        permutation.run({"ecog_rest": x, "ecog_sf": 100}, {"erp_name": "erp"})
    with pytest.raises(ValueError, match="Shape mismatch"):
        permutation.run({"ecog": x, "ecog_rest": np.zeros((4, 3, 5)), "ecog_sf": 100}, {})
    with pytest.raises(ValueError, match="same number of timepoints"):
        permutation.run({"ecog": x, "ecog_rest": np.zeros((4, 2, 6)), "ecog_sf": 100}, {})
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            permutation.run(labelled, {"target": "tone", "n_permutations": 3})
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            permutation.run(pair, {"n_permutations": 3})
