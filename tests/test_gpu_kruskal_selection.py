"""GPU: the rank form of channel selection (tl_rank_columns, tl_kruskal_finalize, ``kruskal_oneway``, the ``test`` key of the
selectors, ``statistic="kruskal"`` of the permutation helpers) against the references of tests/kruskal_ref.py, which the host
tests hold against ``scipy.stats.kruskal`` on the same inputs.

Ranks are compared for EQUALITY: a midrank is a multiple of 0.5 and exact in float32.

How the numeric bounds of H and p are formed - the rule of tests/test_gpu_channel_selection.py, for its reason.  The floor is
the yardstick's own error on the input: the largest relative distance of ``scipy.stats.kruskal`` from H evaluated in
rational arithmetic on the doubled ranks, and from p = Q((k - 1)/2, H/2) of that H at 50 digits (over p > 1e-290).  The
GPU is allowed 100 times that floor (another summation order, and the device's log / exp / lgamma at a few ulp each), never
more than the hard cap 1e-9 on which the exclusion rule of the decision tests rests; a floor of exactly zero is replaced by
2^-52.  The GPU's distance is taken from the same exact values."""
import numpy as np
import pytest
import torch

from tests import kruskal_ref as kr
from tests import parity_record

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------- ranks
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
@pytest.mark.parametrize("N", kr.RANK_N + (8192,))
def test_ranks_equal_rankdata(N, dtype):
    from decode_tonal_langauge_amd.channel_selection import rank_columns
    from decode_tonal_langauge_amd.channel_selection.utils import RANK_MAX_SAMPLES, rank_tile_columns
    assert max(kr.RANK_N + (8192,)) == RANK_MAX_SAMPLES                    # the limit is among the sizes
    tile = rank_tile_columns(N, dtype == np.float64)
    for Cn, T in kr.rank_shapes(tile):
        x = kr.rank_input(N, Cn, T, dtype)
        want = kr.midranks(x)
        got = rank_columns(x.copy())                                   # the shared input is read-only
        assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == (N, Cn, T)
        wrong = int((~((got == want) | (np.isnan(got) & np.isnan(want)))).sum())
        print(f"[N {N} {np.dtype(dtype).name} tile {tile}] {Cn} x {T}: wrong {wrong} of {got.size}")
        assert np.array_equal(got, want, equal_nan=True), (N, Cn, T)
        if Cn * T > 8:
            flat = got.reshape(N, -1)
            assert np.isnan(flat[:, 6]).all() and not np.isnan(flat[:, [5, 7]]).any()
    # the two-array form ranks both arrays as one sample; CUDA tensors stay on the device
    n0 = max(1, N // 3)
    xd = torch.tensor(x).cuda()
    both = rank_columns(xd[:n0], xd[n0:])
    assert both.is_cuda and both.dtype == torch.float32 and both.shape == (N, Cn, T)
    assert np.array_equal(both.cpu().numpy(), want, equal_nan=True)
    assert np.array_equal(both.cpu().numpy(), kr.midranks(x[:n0], x[n0:]), equal_nan=True)


def test_float64_keys_are_not_rounded_to_float32():
    from decode_tonal_langauge_amd.channel_selection import rank_columns
    N = 300
    x = (1.0 + np.random.default_rng(1).permutation(N) * 2.0 ** -40).reshape(N, 1, 1)
    assert len(np.unique(x.astype(np.float32))) == 1
    assert np.array_equal(rank_columns(x), kr.midranks(x))
    assert np.array_equal(np.sort(rank_columns(x).ravel()), np.arange(1, N + 1))
    assert (rank_columns(x.astype(np.float32)) == (N + 1) / 2).all()


def test_the_entry_point_leaves_the_bytes_after_the_ranks_alone():
    """65 samples, 35 columns (two tiles and three columns): a canary follows the ranks."""
    from decode_tonal_langauge_amd import _lib
    lib = _lib.load()
    N, cols = 65, 35
    x = kr.rank_input(N, 5, 7, np.float32)
    xd = torch.tensor(x).cuda()
    buf = torch.full((N * cols + 256,), -7.0, dtype=torch.float32, device="cuda")
    _lib.check(lib.tl_rank_columns(xd.data_ptr(), 20, xd[20:].data_ptr(), N - 20, 0, cols, buf.data_ptr(), _lib.stream_ptr()),
               "tl_rank_columns")
    buf = buf.cpu().numpy()
    assert (buf[N * cols:] == -7.0).all()
    assert np.array_equal(buf[:N * cols].reshape(N, 5, 7), kr.midranks(x), equal_nan=True)


# ---------------------------------------------------------------------------------------------- H and p
@pytest.mark.parametrize("variant", kr.HP_VARIANTS)
def test_h_and_p_within_100_floors_of_the_exact_values(variant):
    from decode_tonal_langauge_amd.channel_selection import kruskal_oneway
    x, lab = kr.hp_input(variant)
    (Hs, ps), (He, pe) = kr.hp_refs(variant)
    assert pe.min() < 1e-60 and pe.max() > 0.99                            # the p-values span 1e-60 .. 1
    H, p = kruskal_oneway(x.copy(), lab)
    assert isinstance(H, np.ndarray) and H.shape == p.shape == x.shape[1:] and H.dtype == p.dtype == np.float64
    mask_H, mask_p = np.isfinite(He), np.isfinite(pe) & (pe > 1e-290)
    floor_H = max(kr.rel(Hs, He, mask_H), kr.ULP)
    floor_p = max(kr.rel(ps, pe, mask_p), kr.ULP)
    dev_H, dev_p = kr.rel(H, He, mask_H), kr.rel(p, pe, mask_p)
    print(f"[{variant}] points {int(mask_p.sum())}  H: floor {floor_H:.3e} gpu {dev_H:.3e}   p: floor {floor_p:.3e} gpu {dev_p:.3e}"
          f"   min exact p {float(pe[mask_p].min()):.3e}")
    parity_record.record(f"kruskal_selection_{variant}", {"H_floor": floor_H, "H_gpu": dev_H, "p_floor": floor_p, "p_gpu": dev_p,
                                                         "points": int(mask_p.sum())})
    assert np.array_equal(np.isnan(H), np.isnan(Hs)) and np.array_equal(np.isnan(p), np.isnan(ps))
    assert dev_H <= 100 * floor_H and dev_H < kr.HARD_CAP, (variant, dev_H, floor_H)
    assert dev_p <= 100 * floor_p and dev_p < kr.HARD_CAP, (variant, dev_p, floor_p)


def test_calling_forms_and_degenerate_columns():
    from decode_tonal_langauge_amd.channel_selection import kruskal_oneway
    rng = np.random.default_rng(9)
    x = np.round(rng.standard_normal((60, 6, 30)) * 3) / 3
    lab = rng.integers(0, 3, 60) * 2 + 1
    x[lab == 5] += 0.7
    x[7, 0, 4] = np.nan                                                # a NaN in one sample
    x[:, 1, 3] = 3.5                                                   # constant everywhere: scipy raises, NaN here
    H_np, p_np = kruskal_oneway(x, lab)
    keep = np.ones(x.shape[1:], dtype=bool)
    keep[1, 3] = False
    Hs = np.full(x.shape[1:], np.nan)
    ps = np.full(x.shape[1:], np.nan)
    flat = x.reshape(60, -1)[:, keep.ravel()]
    Hs[keep], ps[keep] = kr.scipy_kruskal(flat, lab)
    assert np.isnan(H_np[0, 4]) and np.isnan(p_np[0, 4]) and np.isnan(H_np[1, 3]) and np.isnan(p_np[1, 3])
    assert np.array_equal(np.isnan(H_np), np.isnan(Hs)) and np.array_equal(np.isnan(p_np), np.isnan(ps))
    ok = np.isfinite(Hs)
    assert kr.rel(H_np, Hs, ok) < kr.HARD_CAP and kr.rel(p_np, ps, ok) < kr.HARD_CAP
    # CUDA tensors in, CUDA tensors out, the same bits
    xd = torch.from_numpy(x).cuda()
    H, p = kruskal_oneway(xd, torch.from_numpy(lab).cuda())
    assert H.is_cuda and p.is_cuda and H.dtype == torch.float64 and H.shape == (6, 30)
    assert np.array_equal(H.cpu().numpy(), H_np, equal_nan=True) and np.array_equal(p.cpu().numpy(), p_np, equal_nan=True)
    # one tensor per group (unequal sizes): three groups are pooled, two are ranked as two arrays
    groups = [xd[lab == v] for v in (1, 3, 5)]
    Hg, pg = kruskal_oneway(groups)
    assert Hg.is_cuda and kr.rel(Hg.cpu().numpy(), Hs, ok) < kr.HARD_CAP and kr.rel(pg.cpu().numpy(), ps, ok) < kr.HARD_CAP
    H2, p2 = kruskal_oneway([x[lab == 1][:, 2:], x[lab == 5][:, 2:]])
    Hs2, ps2 = kr.scipy_kruskal([x[lab == 1][:, 2:], x[lab == 5][:, 2:]])
    assert isinstance(H2, np.ndarray) and kr.rel(H2, Hs2, np.isfinite(Hs2)) < kr.HARD_CAP
    assert kr.rel(p2, ps2, np.isfinite(ps2)) < kr.HARD_CAP
    with pytest.raises(RuntimeError, match="no CPU"):
        kruskal_oneway(torch.from_numpy(x), lab)


# ---------------------------------------------------------------------------------------------- decisions
def _compare_cells(p_gpu, p_ref, thr, tag):
    """The cells whose reference p lies within 1e-9 of the threshold are left out; their share is capped at 1e-4."""
    _, _, near = kr.selection(p_ref, thr, 0)
    share = near.sum() / near.size
    wrong = int(((p_gpu < thr) != (p_ref < thr))[~near].sum())
    print(f"[{tag}] cells {near.size} left out {int(near.sum())} wrong {wrong}")
    assert share <= kr.SHARE_CAP and wrong == 0, tag


def test_discriminative_decisions_equal_the_reference_and_the_anova_is_unchanged():
    from decode_tonal_langauge_amd.channel_selection import discriminative
    x, lab = kr.heavy_tail_input()
    data = {"ecog": x.copy(), "ecog_sf": np.array(100), "tone": lab[:, None]}
    base = {"target": "tone", "p_threshold": 0.05, "active_time_threshold": 0.1}
    _, ps = kr.scipy_kruskal(x, lab)
    for att in (0.1, 0.25, 0.3, 0.5):                                  # lengths 10 and 25 below, 30 and 50 not below the planted run of 30
        res = discriminative.run(data, dict(base, active_time_threshold=att, test="kruskal"))
        selected, runs, _ = kr.selection(ps, 0.05 / 60, int(att * 100))
        assert res["selected_channels"] == selected and res["max_lengths"] == [] and res["p_values"].shape == (8, 60)
        _compare_cells(res["p_values"], ps, 0.05 / 60, f"heavy_tail att {att}")
    assert kr.selection(ps, 0.05 / 60, 29)[0] == [0, 1, 2, 3] and kr.selection(ps, 0.05 / 60, 30)[0] == []
    out = discriminative.test_discriminative_power(data, dict(base, test="kruskal"))
    assert set(out) == {"h_stat", "p_value"} and np.array_equal(out["p_value"], res["p_values"])
    assert kr.rel(out["h_stat"], kr.scipy_kruskal(x, lab)[0], np.ones((8, 60), dtype=bool)) < kr.HARD_CAP
    # the ANOVA, by name or by default, selects nothing on this input and returns what it returned
    plain = discriminative.run(data, base)
    named = discriminative.run(data, dict(base, test="anova"))
    assert plain["selected_channels"] == named["selected_channels"] == []
    assert np.array_equal(plain["p_values"], named["p_values"])
    assert set(discriminative.test_discriminative_power(data, base)) == {"f_stat", "p_value"}
    # ragged: 50 samples, 3 x 77 columns, tied values, labels -1, 2, 5
    x, lab = kr.ragged_labelled()
    _, ps = kr.scipy_kruskal(x, lab)
    res = discriminative.run({"ecog": x.copy(), "ecog_sf": 100, "tone": lab},
                             dict(base, active_time_threshold=0.05, test="kruskal"))
    assert res["selected_channels"] == kr.selection(ps, 0.05 / 77, 5)[0] == [0, 1]
    _compare_cells(res["p_values"], ps, 0.05 / 77, "ragged")


def test_active_decisions_equal_the_reference_and_the_anova_is_unchanged():
    from decode_tonal_langauge_amd.channel_selection import active
    rest, erp = kr.heavy_tail_rest_erp()
    data = {"ecog": erp.copy(), "ecog_rest": rest.copy(), "ecog_sf": np.array(100)}
    base = {"p_threshold": 0.05, "active_time_threshold": 0.1}
    _, ps = kr.scipy_kruskal([rest, erp])
    res = active.run(data, dict(base, test="kruskal"))
    selected, runs, _ = kr.selection(ps, 0.05 / 60, 10)
    assert res["selected_channels"] == selected == [0, 1, 2, 3] and res["max_lengths"] == [runs[c] for c in selected]
    assert res["p_values"].shape == (60,)                              # the last channel only, as with the ANOVA
    _compare_cells(res["p_values"][None], ps[-1:], 0.05 / 60, "heavy_tail rest / ERP, last channel")
    plain, named = active.run(data, base), active.run(data, dict(base, test="anova"))
    assert plain["selected_channels"] == named["selected_channels"] == [] and np.array_equal(plain["p_values"], named["p_values"])
    # ragged float32: 31 and 23 samples, 5 x 65 columns
    rest, erp = kr.ragged_rest_erp()
    _, ps = kr.scipy_kruskal([rest, erp])
    res = active.run({"ecog": erp.copy(), "ecog_rest": rest.copy(), "ecog_sf": 100},
                     dict(base, active_time_threshold=0.2, test="kruskal"))
    selected, runs, _ = kr.selection(ps, 0.05 / 65, 20)
    assert res["selected_channels"] == selected == [1, 2] and res["max_lengths"] == [runs[c] for c in selected]
    # mixed dtypes on the same pair: the rest float32, the ERP the same values as float64.  Widening float32 is exact, so
    # every result equals, bit for bit, that of both given as float64 - in this selector and in the permutation test
    from decode_tonal_langauge_amd.channel_selection import permutation
    mixed = {"ecog": erp.astype(np.float64), "ecog_rest": rest.copy(), "ecog_sf": 100}
    wide = dict(mixed, ecog_rest=rest.astype(np.float64))
    for test in ("anova", "kruskal"):
        for selector, prm in ((permutation, {"p_threshold": 0.05, "n_permutations": 40, "test": test}),
                              (active, dict(base, active_time_threshold=0.2, test=test))):
            got, want = selector.run(mixed, prm), selector.run(wide, prm)
            assert got["selected_channels"] == want["selected_channels"] and got["max_lengths"] == want["max_lengths"]
            assert np.array_equal(got["p_values"], want["p_values"])
    assert want["selected_channels"] == selected                        # active, rank form: the float32 pair's channels


# ---------------------------------------------------------------------------------------------- permutation test
@pytest.mark.parametrize("name", list(kr.PERM_CASES))
def test_permutation_on_the_ranks_equals_the_rational_oracle(name):
    from decode_tonal_langauge_amd.channel_selection import kruskal_oneway, max_run_below, permutation_runs
    from decode_tonal_langauge_amd.channel_selection.utils import permutation_exceedances
    c = kr.perm_case(name)
    want, excluded = kr.perm_expected(name)
    arrays = [torch.tensor(c["x"]).cuda()]
    P = c["table"].shape[0]
    mask = permutation_exceedances(arrays, c["table"], c["counts"], c["cell"], statistic="kruskal")
    assert mask.is_cuda and mask.dtype == torch.bool and mask.shape == want.shape
    mask = mask.cpu().numpy()
    wrong = int((mask != want)[~excluded].sum())
    print(f"[{name}] cells {mask.size} set {int(want.sum())} left out {int(excluded.sum())} wrong {wrong}")
    parity_record.record(f"kruskal_permutation_{name}", {"cells": mask.size, "cells_set": int(want.sum()),
                                                         "cells_left_out": int(excluded.sum()), "cells_wrong": wrong})
    assert excluded.sum() <= kr.SHARE_CAP * mask.size and wrong == 0
    runs, chi2_crit, theta = permutation_runs(arrays, c["table"], c["counts"], c["cell"], statistic="kruskal")
    assert (chi2_crit, theta) == (c["chi2_crit"], c["theta"]) and runs.shape == (P, c["x"].shape[1])
    if not excluded.any():
        assert runs.cpu().numpy().tolist() == [kr.longest_runs(m) for m in want]
    # row 0 is the run of the p-values of kruskal_oneway at the same cell level
    _, p = kruskal_oneway(arrays[0], c["table"][0])
    assert torch.equal(runs[0], max_run_below(p, c["cell"])[1])
    # the chunking of the relabellings does not matter
    for chunk in (16, 1000):
        assert torch.equal(runs, permutation_runs(arrays, c["table"], c["counts"], c["cell"], perm_chunk=chunk,
                                                  statistic="kruskal")[0])


def test_permutation_selector_with_the_rank_statistic():
    from decode_tonal_langauge_amd.channel_selection import permutation, permutation_p_values
    c = kr.perm_case("n97_k3")
    spec = kr.PERM_CASES["n97_k3"]
    T = c["x"].shape[2]
    params = {"target": "tone", "p_threshold": spec["cell"] * T, "n_permutations": spec["P"] - 1, "seed": 100 + spec["seed"],
              "alpha": 0.1, "correction": "channel"}
    data = {"ecog": c["x"].copy(), "ecog_sf": np.array(100), "tone": c["group_index"] * 2 + 3}
    res = permutation.run(data, dict(params, test="kruskal"))
    assert set(res) == {"selected_channels", "max_lengths", "p_values", "null_max_lengths", "f_crit", "chi2_crit"}
    assert res["f_crit"] is None and res["chi2_crit"] == c["chi2_crit"]
    want, excluded = kr.perm_expected("n97_k3")
    assert not excluded.any()
    runs = np.array([kr.longest_runs(m) for m in want], dtype=np.int32)
    p_channel, _ = permutation_p_values(runs)
    assert res["selected_channels"] == [int(ch) for ch in np.flatnonzero((runs[0] > 0) & (p_channel <= 0.1))]
    assert {0, 1} <= set(res["selected_channels"]) and np.array_equal(res["p_values"], p_channel)
    assert res["max_lengths"] == [int(runs[0, ch]) for ch in res["selected_channels"]]
    plain = permutation.run(data, params)
    assert set(plain) == {"selected_channels", "max_lengths", "p_values", "null_max_lengths", "f_crit"}
    assert plain["f_crit"] == permutation.run(data, dict(params, test="anova"))["f_crit"] > 0
