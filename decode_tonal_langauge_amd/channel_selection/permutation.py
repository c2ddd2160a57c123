"""Channels by a label-permutation test of the selectors' own statistic: the longest run of Bonferroni-significant timepoints.

``active`` and ``discriminative`` keep a channel when that run exceeds a hand-set length.  This selector asks the data
instead: the samples are relabelled ``n_permutations`` times, the ANOVA is redone at every (channel, timepoint) under each
relabelling, and a channel is kept when its observed run is rarely reached by chance - per channel (``correction:
channel``) or against the relabelling's maximum over all channels (``correction: max``, family-wise, the default).

With ``target`` in the parameters it is the labelled form and takes the keys of ``discriminative`` (``recording_name``,
``target``, ``p_threshold``); without, it is rest against ERP with the keys of ``active`` (``erp_name``, ``rest_name``,
``p_threshold``).  Both run the input checks of their counterpart (``utils.labelled_inputs``, ``utils.rest_erp_inputs``) and
raise its errors.  New keys: ``n_permutations`` (1000),
``seed`` (0), ``alpha`` (0.05), ``correction`` (``max`` | ``channel``) and ``perm_chunk`` (relabellings per launch; the
default bounds the mask) and ``test`` (``anova`` | ``kruskal``: the statistic at every cell; the rank form ranks the samples once,
``tl_rank_columns``, and relabels the ranks).  ``active_time_threshold`` is not used.  All relabellings are one float64 product on the device
(``tl_perm_exceed``) and one run search (``tl_perm_runs``); no p-value is evaluated per relabelling.  No CPU fallback."""
from __future__ import annotations

import os
import warnings

import numpy as np

from .utils import (check_statistic, device_recording, labelled_inputs, permutation_p_values, permutation_runs, permutation_table,
                    promote, rest_erp_inputs)

_CORRECTIONS = ("max", "channel")


def _new_keys(params: dict, n_timepoints: int):
    """The permutation keys, validated: ``(n_permutations, seed, alpha, correction, perm_chunk, cell level)``."""
    n_perm = params.get('n_permutations', 1000)
    alpha = params.get('alpha', 0.05)
    correction = params.get('correction', 'max')
    if int(n_perm) != n_perm or n_perm < 1:
        raise ValueError(f"n_permutations must be an integer of at least 1, got {n_perm}.")
    if not 0.0 < alpha <= 1.0:
        raise ValueError(f"alpha must lie in (0, 1], got {alpha}.")
    if correction not in _CORRECTIONS:
        raise ValueError(f"Unknown correction '{correction}': expected one of {list(_CORRECTIONS)}.")
    cell = params.get('p_threshold', 0.05) / n_timepoints                # Bonferroni, as the other selectors
    if not 0.0 < cell < 1.0:
        raise ValueError(f"p_threshold / n_timepoints must lie in (0, 1), got {cell}.")
    return int(n_perm), int(params.get('seed', 0)), float(alpha), correction, params.get('perm_chunk'), float(cell)


def run(data: dict, params: dict) -> dict:
    """``{'selected_channels', 'max_lengths', 'p_values', 'null_max_lengths', 'f_crit'}``.  A channel is kept when its
    observed run of ``p < p_threshold / n_timepoints`` is longer than 0 and its permutation p-value is at most ``alpha``.
    ``max_lengths`` holds the observed run of every kept channel, ``p_values`` (n_channels,) the permutation p-value that
    decided (per channel, or against the maximum over channels), ``null_max_lengths`` (n_permutations,) the maximum over
    channels of every relabelling and ``f_crit`` the F value of the cell level.  With ``test: kruskal`` the cells are those
    of the Kruskal-Wallis test: ``chi2_crit`` holds its critical value next to ``f_crit``, which is None."""
    what = "channel_selection.permutation"
    test = check_statistic(params.get('test', 'anova'), "test")
    if 'target' in params:
        name, series, labels = labelled_inputs(data, params)
        classes, group_index = np.unique(labels, return_inverse=True)
        if not 2 <= len(classes) <= 64:
            raise ValueError(f"Labels '{params['target']}' must hold between 2 and 64 classes, got {len(classes)}.")
        n_perm, seed, alpha, correction, perm_chunk, cell = _new_keys(params, series.shape[2])
        arrays = [device_recording(data, name, what)]
    else:
        rest_name, erp_name, rest, erp = rest_erp_inputs(data, params)
        n_perm, seed, alpha, correction, perm_chunk, cell = _new_keys(params, rest.shape[2])
        arrays = promote([device_recording(data, rest_name, what), device_recording(data, erp_name, what)])
        group_index = np.repeat(np.arange(2), [rest.shape[0], erp.shape[0]])
    counts = np.bincount(group_index).tolist()
    table = permutation_table(group_index, n_perm, seed)
    runs, crit, _ = permutation_runs(arrays, table, counts, cell, perm_chunk, statistic=test)
    runs = runs.cpu().numpy()
    p_channel, p_max = permutation_p_values(runs)
    p_used = p_max if correction == "max" else p_channel
    selected = [int(ch) for ch in np.flatnonzero((runs[0] > 0) & (p_used <= alpha))]
    print(f"Found {len(selected)} channels by the permutation test ({n_perm} relabellings, correction '{correction}').")
    result = {"selected_channels": selected, "max_lengths": [int(runs[0, ch]) for ch in selected], "p_values": p_used,
              "null_max_lengths": runs[1:].max(axis=1), "f_crit": crit}
    if test == "kruskal":
        result.update(f_crit=None, chi2_crit=crit)
    return result


def generate_figures(data: dict, results: dict, params: dict, figure_dir: str) -> None:
    """Histogram of the null maxima with the observed runs marked (host matplotlib; outside the tested contract)."""
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except ImportError:
        warnings.warn("matplotlib is not importable: no permutation-test figures")
        return
    os.makedirs(figure_dir, exist_ok=True)
    plt.figure(figsize=(10, 6))
    plt.hist(np.asarray(results["null_max_lengths"]), bins=30, alpha=0.7, color="grey", label="maximum over channels, relabelled")
    for ch, length in zip(results["selected_channels"], results["max_lengths"]):
        plt.axvline(length, color="red", alpha=0.5)
    plt.title("Longest significant run: null distribution and the kept channels", fontsize=16)
    plt.xlabel("Longest run (timepoints)", fontsize=14)
    plt.ylabel("Relabellings", fontsize=14)
    plt.legend()
    figure_path = os.path.join(figure_dir, "permutation_null.png")
    plt.savefig(figure_path, dpi=200)
    plt.close()
    print(f"Saved the permutation null distribution to {figure_path}")
