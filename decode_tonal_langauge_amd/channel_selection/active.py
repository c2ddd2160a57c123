"""Active channels: a one-way ANOVA of the event-related samples against the rest samples at every (channel, timepoint),
then the channels whose longest Bonferroni-significant run exceeds a length (mirror of reference
channel_selection/active.py:15-84).

Same keys (``erp_name``, ``rest_name``, ``ecog_sf``, ``p_threshold``, ``active_time_threshold``), same errors and the same
result dict as the reference.  Rest and ERP are two arrays with their own sample counts: one ``tl_group_moments`` launch
each, ``tl_anova_finalize``, ``tl_max_run_below``.  One key beyond the reference: ``test``, ``anova`` (the default) or
``kruskal`` - the Kruskal-Wallis test on the midranks of rest and ERP taken together (``tl_rank_columns``,
``tl_kruskal_finalize``), for amplitudes with heavy tails.  No CPU fallback."""
from __future__ import annotations

import os
import random
import warnings
from typing import Optional

import numpy as np

from .utils import channels_by_run, check_statistic, device_recording, group_test, promote, rest_erp_inputs


def run(data: dict, params: dict) -> dict:
    """``{'selected_channels', 'max_lengths', 'p_values'}``.  A channel is kept when its longest run of
    ``p < p_threshold / rest.shape[2]`` is strictly longer than ``int(active_time_threshold * ecog_sf)`` samples;
    ``max_lengths`` holds the run of every kept channel.

    ``p_values`` is the reference's quirk kept on purpose: it holds the p-values (n_timepoints,) of the LAST channel
    only, not of every channel - ``generate_figures`` downstream relies on that shape.

    One check goes beyond the reference: rest and ERP recordings with different numbers of timepoints raise a
    ``ValueError`` here (the reference fails later, inside scipy, on such a pair).  ``test: kruskal`` takes the p-values
    from the Kruskal-Wallis test; any value but ``anova`` / ``kruskal`` raises a ``ValueError``."""
    what = "channel_selection.active"
    test = check_statistic(params.get('test', 'anova'), "test")
    rest_name, erp_name, rest_samples, _ = rest_erp_inputs(data, params)
    length_threshold = int(params['active_time_threshold'] * data["ecog_sf"])
    corrected_p_threshold = params['p_threshold'] / rest_samples.shape[2]          # Bonferroni
    _, p = group_test(test, promote([device_recording(data, rest_name, what), device_recording(data, erp_name, what)]))
    active_channels, max_lengths = channels_by_run(p, corrected_p_threshold, length_threshold)
    print(f"Found {len(active_channels)} active channels.")
    return {"selected_channels": active_channels, "max_lengths": max_lengths, "p_values": p[-1].cpu().numpy()}


def generate_figures(data: dict, results: dict, params: dict, figure_dir: str) -> None:
    """Histogram of the active lengths and rest-against-ERP plots of up to ten kept channels (host matplotlib; outside
    the tested contract)."""
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except ImportError:
        warnings.warn("matplotlib is not importable: no active-channel figures")
        return
    ecog_sf = float(data["ecog_sf"])
    channels = results["selected_channels"]
    plt.figure(figsize=(10, 6))
    plt.hist(np.array(results["max_lengths"]) / ecog_sf, bins=30, alpha=0.7, color="blue")
    plt.title("Distribution of Active Length of Significant Channels", fontsize=18)
    plt.xlabel("Active length (s)", fontsize=16)
    plt.ylabel("Frequency", fontsize=16)
    figure_path = os.path.join(figure_dir, "active_lengths.png")
    plt.savefig(figure_path, dpi=200)
    plt.close()
    print(f"Saved distribution of lengths of significant channels to {figure_path}")
    rest_name, erp_name = params.get('rest_name', 'ecog_rest'), params.get('erp_name', 'ecog')
    chosen = random.sample(channels, min(10, len(channels)))
    for ch in chosen:
        plot_rest_erp(np.asarray(data[rest_name])[:, ch, :], np.asarray(data[erp_name])[:, ch, :], p_vals=results["p_values"],
                      p_val_threshold=params["p_threshold"], sampling_rate=ecog_sf,
                      figure_path=os.path.join(figure_dir, f"channel_{ch}_erp_rest.png"))
    print(f"Saved ERP vs Rest plots for {len(chosen)} channels to {figure_dir}")


def plot_rest_erp(rest_data: np.ndarray, erp_data: np.ndarray, p_vals, p_val_threshold: float = 0.05, sampling_rate: float = 400,
                  figure_path: Optional[str] = None) -> None:
    """Left: mean +- SEM of the rest and ERP samples (n_samples, n_timepoints) of one channel; right: the p-values."""
    import matplotlib.pyplot as plt
    if rest_data.shape[1] != erp_data.shape[1]:
        raise ValueError("Rest and ERP data must have the same number of timepoints.")
    n = rest_data.shape[1]
    t = np.linspace(0, n / sampling_rate, n)
    _, axes = plt.subplots(1, 2, figsize=(16, 6))
    for rows, name, colour in ((rest_data, 'Rest', 'blue'), (erp_data, 'ERP', 'orange')):
        mean, sem = rows.mean(axis=0), rows.std(axis=0) / np.sqrt(rows.shape[0])
        axes[0].plot(t, mean, label=f'{name} Mean ± SEM', color=colour)
        axes[0].fill_between(t, mean - sem, mean + sem, color=colour, alpha=0.2)
    axes[0].set_title('Comparison of Rest and ERP Activity', fontsize=16)
    axes[0].set_xlabel('Time (s)', fontsize=14)
    axes[0].set_ylabel('Amplitude', fontsize=14)
    axes[0].legend()
    axes[0].grid(True)
    axes[1].plot(t, p_vals, label='P-values', color='red')
    axes[1].axhline(y=p_val_threshold, color='black', linestyle='--', label='Significance Threshold')
    axes[1].set_title('P-values Over Time', fontsize=16)
    axes[1].set_xlabel('Time (s)', fontsize=14)
    axes[1].set_ylabel('P-value', fontsize=14)
    axes[1].legend()
    axes[1].grid(True)
    if figure_path:
        plt.savefig(figure_path, dpi=200, bbox_inches='tight')
        plt.close()
    else:
        plt.show()
