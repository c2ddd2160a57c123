"""Plot helpers needed by the synthesis entry point.

``plot_training_losses`` is imported by the reference's ``train_synthesizer.py:21`` but does not
exist in its ``utils/visualise.py`` (the script raises ImportError as shipped, SURVEY.md section 0
finding 5); it is provided here, together with ``plot_confusion_matrix`` used by the classifier
pipeline.

``plot_psd`` and ``plot_channel_mean_std`` draw what ``utils/diagnostics.py`` computes on the GPU (a NumPy recording is uploaded,
a CUDA tensor is read where it is; only the spectrum / the moments come back), ``compare_confusion_matrices`` is host only.
The reference's Venn and metric plots need seaborn and matplotlib_venn and stay out."""
import os
from typing import List, Optional, Sequence

import numpy as np


def plot_training_losses(losses: Sequence[Sequence[float]], figure_path: Optional[str] = None,
                         labels: Optional[List[str]] = None):
    """One curve of per-epoch training loss per repeat; saves to ``figure_path`` if given."""
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    fig, ax = plt.subplots(figsize=(8, 5))
    for i, curve in enumerate(losses):
        ax.plot(range(1, len(curve) + 1), curve, label=(labels[i] if labels else f"run {i + 1}"))
    ax.set_xlabel("Epoch")
    ax.set_ylabel("Training loss (L1)")
    ax.set_title("Synthesizer training loss")
    if len(losses) <= 10:
        ax.legend()
    fig.tight_layout()
    if figure_path:
        fig.savefig(figure_path, dpi=150)
    plt.close(fig)
    return figure_path


def plot_confusion_matrix(confusion_matrix: np.ndarray, add_numbers: bool = False,
                          label_names: Optional[Sequence[str]] = None, figure_path: Optional[str] = None,
                          cmap: str = "Blues", title: str = "Confusion Matrix",
                          imshow_kwargs: Optional[dict] = None) -> None:
    """Heat map of a confusion matrix, rows = true label (reference utils/visualise.py:12-90)."""
    import matplotlib
    if figure_path is not None:
        matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    cm = np.asarray(confusion_matrix)
    fig, ax = plt.subplots(figsize=(8, 6))
    im = ax.imshow(cm, interpolation="nearest", cmap=cmap, **(imshow_kwargs or {}))
    ax.set_title(title, fontsize=20)
    fig.colorbar(im, ax=ax)
    ax.set_xlabel("Predicted Label", fontsize=18)
    ax.set_ylabel("True Label", fontsize=18)
    ticks_x, ticks_y = np.arange(cm.shape[1]), np.arange(cm.shape[0])
    if label_names is not None:
        ax.set_xticks(np.arange(len(label_names)), labels=list(label_names), rotation=45, fontsize=14)
        ax.set_yticks(np.arange(len(label_names)), labels=list(label_names), fontsize=14)
    else:
        ax.set_xticks(ticks_x)
        ax.set_yticks(ticks_y)
    if add_numbers:
        half = cm.max() / 2.0 if cm.size else 0.0
        for i in ticks_y:
            for j in ticks_x:
                v = cm[i, j]
                ax.text(j, i, f"{v:.0f}" if float(v).is_integer() else f"{v:.2f}", ha="center", va="center",
                        color="white" if v > half else "black")
    fig.tight_layout()
    if figure_path is not None:
        os.makedirs(os.path.dirname(figure_path) or ".", exist_ok=True)
        fig.savefig(figure_path)
        plt.close(fig)
    else:
        plt.show()


def compare_confusion_matrices(confusion_matrix: np.ndarray, baseline_matrix: np.ndarray,
                               title: str = "Confusion Matrix Difference", label_names: Optional[List[str]] = None,
                               figure_path: Optional[str] = None) -> None:
    """``confusion_matrix - baseline_matrix`` as a heat map on a colour scale symmetric about zero (reference
    utils/visualise.py:92-134)."""
    diff = np.asarray(confusion_matrix) - np.asarray(baseline_matrix)
    bound = float(np.max(np.abs(diff))) if diff.size else 0.0
    plot_confusion_matrix(diff, add_numbers=True, label_names=label_names, figure_path=figure_path, cmap="coolwarm", title=title,
                          imshow_kwargs={"vmin": -bound, "vmax": bound})


def _finish(fig, plt, figure_path: Optional[str], **save_kwargs) -> None:
    if figure_path:
        os.makedirs(os.path.dirname(figure_path) or ".", exist_ok=True)
        fig.savefig(figure_path, **save_kwargs)
        plt.close(fig)
    else:
        plt.show()


def plot_psd(data, figure_path: Optional[str] = None) -> None:
    """Welch spectrum of every channel of ``data (n_channels, n_timepoints)`` on one axis, the DC bin not drawn, at the
    reference's fixed settings (utils/visualise.py:137-173: ``plt.psd(NFFT=256, Fs=1000, noverlap=128)`` per channel, i.e.
    ``np.hanning(256)``, no detrend, density scaling).  The spectra are one ``diagnostics.welch_psd`` call for all channels;
    matplotlib only draws, on the dB scale ``plt.psd`` uses."""
    import matplotlib
    if figure_path is not None:
        matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    from . import diagnostics
    freqs, psd = diagnostics.welch_psd(data, fs=1000, window=np.hanning(256), nperseg=256, noverlap=128, nfft=256, detrend=False)
    if not isinstance(psd, np.ndarray):
        freqs, psd = freqs.cpu().numpy(), psd.cpu().numpy()
    n_channels = psd.shape[0]
    colours = plt.get_cmap("viridis")(np.linspace(0.0, 1.0, max(n_channels, 1)))
    fig, ax = plt.subplots(figsize=(12, 6))
    with np.errstate(divide="ignore"):
        for c in range(n_channels):
            ax.plot(freqs[1:], 10.0 * np.log10(psd[c, 1:]), color=colours[c])
    ax.set_title("Power Spectrum Density (PSD)", fontsize=18)
    ax.set_xlabel("Frequency (Hz)", fontsize=16)
    ax.set_ylabel("Power Spectral Density (dB/Hz)", fontsize=16)
    ax.grid(True)
    if not figure_path:
        fig.tight_layout()
    _finish(fig, plt, figure_path, dpi=300, bbox_inches="tight")


def plot_channel_mean_std(data, sampling_rate: int, start: float = 0.0, end: float = 30.0,
                          figure_path: Optional[str] = None) -> None:
    """Mean and standard deviation of every channel per one-second segment between ``start`` and ``end`` (seconds) as two
    channel x time images (reference utils/visualise.py:176-243); the numbers are ``diagnostics.segment_mean_std``, whose
    docstring says how the segments are defined."""
    import matplotlib
    if figure_path is not None:
        matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    from . import diagnostics
    means, stds = diagnostics.segment_mean_std(data, sampling_rate, start=start, end=end)
    if not isinstance(means, np.ndarray):
        means, stds = means.cpu().numpy(), stds.cpu().numpy()
    extent = (start, start + means.shape[1], -0.5, means.shape[0] - 0.5)
    fig, axes = plt.subplots(2, 1, figsize=(12, 8), sharex=True)
    for ax, values, cmap, name in ((axes[0], means, "viridis", "Mean"), (axes[1], stds, "plasma", "Standard Deviation")):
        image = ax.imshow(values, aspect="auto", cmap=cmap, origin="lower", extent=extent)
        ax.set_title(f"{name} Over Time", fontsize=14)
        ax.set_xlabel("Time (seconds)", fontsize=12)
        ax.set_ylabel("Channels", fontsize=12)
        fig.colorbar(image, ax=ax, orientation="vertical", label=name)
    fig.tight_layout()
    _finish(fig, plt, figure_path, dpi=300, bbox_inches="tight")
