"""Discriminative channels: a one-way ANOVA of the recording against an integer label at every (channel, timepoint), then
the channels whose longest Bonferroni-significant run exceeds a length (mirror of reference
channel_selection/discriminative.py:16-182).

Same keys (``recording_name``, ``target``, ``p_threshold``, ``active_time_threshold``, ``<recording>_sf``), same errors and
the same result dict as the reference.  The per-channel ``scipy.stats.f_oneway`` loop is one launch of ``tl_group_moments``
per class plus ``tl_anova_finalize``; the per-channel run search is ``tl_max_run_below``.  One key beyond the reference:
``test``, ``anova`` (the default) or ``kruskal`` - the Kruskal-Wallis test on the midranks (``tl_rank_columns``,
``tl_kruskal_finalize``), for amplitudes with heavy tails.  No CPU fallback."""
from __future__ import annotations

import os
import random
import warnings
from typing import Dict, Mapping, Optional

import numpy as np

from .utils import channels_by_run, check_statistic, device_recording, group_test, labelled_inputs


def _test_on_device(data: Mapping, params: dict, need_sf: bool):
    """The reference's input checks and the test itself; returns (F, p) as (C, T) float64 CUDA tensors - (H, p) with
    ``test: kruskal``."""
    test = check_statistic(params.get('test', 'anova'), "test")
    name, _, labels = labelled_inputs(data, params, need_sf)
    x = device_recording(data, name, "channel_selection.discriminative")
    return group_test(test, [x], [np.flatnonzero(labels == v).astype(np.int32) for v in np.unique(labels)])


def test_discriminative_power(data: Mapping[str, np.ndarray], params: dict) -> Dict[str, np.ndarray]:
    """``{'f_stat', 'p_value'}``, both (n_channels, n_timepoints) float64 NumPy: the ANOVA of ``data[recording_name]``
    (n_samples, n_channels, n_timepoints) grouped by the integer labels ``data[target]``.  With ``test: kruskal`` the keys
    are ``{'h_stat', 'p_value'}``."""
    F, p = _test_on_device(data, params, need_sf=False)
    stat_key = 'h_stat' if params.get('test', 'anova') == "kruskal" else 'f_stat'
    return {stat_key: F.cpu().numpy(), 'p_value': p.cpu().numpy()}


test_discriminative_power.__test__ = False          # a mirrored name, not a pytest case


def run(data: dict, params: dict) -> dict:
    """``{'selected_channels', 'max_lengths', 'p_values'}``: the channels whose longest run of
    ``p < p_threshold / n_timepoints`` is strictly longer than ``int(active_time_threshold * <recording>_sf)`` samples,
    an empty ``max_lengths`` list (as the reference returns it) and the p-values (n_channels, n_timepoints)."""
    p_threshold = params.get('p_threshold', 0.05)
    target = params['target']
    _, p = _test_on_device(data, params, need_sf=True)
    length_threshold = int(params["active_time_threshold"] * data[f"{params.get('recording_name', 'ecog')}_sf"])
    significant_channels, _ = channels_by_run(p, p_threshold / p.shape[1], length_threshold)       # Bonferroni
    print(f'Found {len(significant_channels)} discriminative channels'
          f' for target "{target}"')
    return {'selected_channels': significant_channels, 'max_lengths': [], 'p_values': p.cpu().numpy()}


def generate_figures(data: dict, results: dict, params: dict, figure_dir: str):
    """Class means and p-values over time for up to ten selected channels (host matplotlib; outside the tested contract)."""
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt  # noqa: F401
    except ImportError:
        warnings.warn("matplotlib is not importable: no discriminative-channel figures")
        return
    os.makedirs(figure_dir, exist_ok=True)
    label_name = params['target']
    for file in os.listdir(figure_dir):
        if file.endswith('.png'):
            os.remove(os.path.join(figure_dir, file))
    recording_name = params.get('recording_name', 'ecog')
    channels = random.sample(results['selected_channels'], min(10, len(results['selected_channels'])))
    for ch in channels:
        plot_discriminative_channel(
            data, ch, sampling_rate=data[f"{recording_name}_sf"], p_vals=results['p_values'][ch, :],
            label_name=label_name, p_threshold=params.get('p_threshold', 0.05), recording_name=recording_name,
            onset_time=params.get('onset_time'), figure_path=os.path.join(figure_dir, f'{label_name}_channel_{ch}.png'))
    print(f"Saved discriminative channel figures to {figure_dir}")


def plot_discriminative_channel(data: dict, channel_idx: int, sampling_rate: int, p_vals: np.ndarray, p_threshold: float = 0.05,
                                label_name: str = 'syllable', recording_name: str = 'ecog', onset_time: Optional[int] = None,
                                figure_path: Optional[str] = None) -> None:
    """Left: mean +- SEM of the channel per class; right: its p-values against the threshold."""
    import matplotlib.pyplot as plt
    series = np.asarray(data[recording_name])
    labels = np.asarray(data[label_name]).squeeze()
    t = np.arange(series.shape[2]) / float(sampling_rate) - (onset_time or 0)
    _, axes = plt.subplots(1, 2, figsize=(12, 6))
    for label in np.unique(labels):
        rows = series[labels == label, channel_idx, :]
        mean, sem = rows.mean(axis=0), rows.std(axis=0) / np.sqrt(rows.shape[0])
        axes[0].plot(t, mean, label=f'{label_name} {label}')
        axes[0].fill_between(t, mean - sem, mean + sem, alpha=0.2)
    if onset_time is not None:
        axes[0].axvline(x=0, color='k', linestyle='--', label='Onset')
    axes[0].set_xlabel('Time (s)')
    axes[0].set_ylabel('Amplitude')
    axes[0].legend()
    axes[1].plot(t, p_vals, color='r', label='P-values')
    axes[1].axhline(y=p_threshold, color='k', linestyle='--', label='Significance Threshold')
    axes[1].set_xlabel('Time (s)')
    axes[1].set_ylabel('p-value')
    axes[1].legend()
    plt.suptitle(f'Discriminative Power for Channel {channel_idx} in distinguishing {label_name}', fontsize=18)
    if figure_path:
        plt.savefig(figure_path, dpi=200)
        plt.close()
    else:
        plt.show()
