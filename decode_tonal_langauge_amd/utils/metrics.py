"""Classification metrics on label arrays (counterpart of reference utils/metrics.py:5-139).

Same names, arguments and results: metrics are looked up in a fixed table first
(accuracy, weighted f1_score / precision / recall, cohen_kappa, confusion_matrix) and then by name in
``sklearn.metrics`` (``average='weighted'`` when the function takes it); joint metrics over several
targets flatten the per-target labels into one mixed-radix label, first target most significant
(reference :117-137)."""
from __future__ import annotations

from typing import Dict, List

import numpy as np
from sklearn import metrics as _sk

_WEIGHTED = ("f1_score", "precision", "recall")
_TABLE = {
    "accuracy": _sk.accuracy_score,
    "f1_score": _sk.f1_score,
    "precision": _sk.precision_score,
    "recall": _sk.recall_score,
    "cohen_kappa": _sk.cohen_kappa_score,
    "confusion_matrix": _sk.confusion_matrix,
}


def compute_classification_metrics(true: np.ndarray, preds: np.ndarray, metrics: List[str] = ["accuracy"],
                                   verbose: bool = False) -> Dict[str, object]:
    if verbose:
        print("Unique labels in true: {}".format(set(true)))
        print("Unique predictions in preds: {}".format(set(preds)))
    out = {}
    for name in metrics:
        fn = _TABLE.get(name)
        if fn is not None:
            out[name] = fn(true, preds, average="weighted") if name in _WEIGHTED else fn(true, preds)
            continue
        fn = getattr(_sk, name, None)
        if fn is None:
            raise ValueError(f"Metric '{name}' is not recognized in sklearn.metrics, and "
                             f"not part of the supported metrics: {list(_TABLE.keys())}.")
        takes_average = "average" in getattr(getattr(fn, "__code__", None), "co_varnames", ())
        out[name] = fn(true, preds, average="weighted") if takes_average else fn(true, preds)
    return out


def compute_classification_metrics_joint(all_true: Dict[str, np.ndarray], all_preds: Dict[str, np.ndarray],
                                         metrics: List[str] = ["accuracy"], verbose: bool = False) -> Dict[str, object]:
    if set(all_true.keys()) != set(all_preds.keys()):
        raise ValueError("Keys in all_true and all_preds must match.")
    targets = list(all_true.keys())
    if verbose:
        for t in targets:
            print("Unique labels in {}: {}".format(t, set(all_true[t])))
            print("Unique predictions in {}: {}".format(t, set(all_preds[t])))
    true = [np.asarray(all_true[t]).astype(int) for t in targets]
    pred = [np.asarray(all_preds[t]).astype(int) for t in targets]
    radix = [len(np.unique(t)) for t in true]
    joint_true = np.zeros_like(true[0])
    joint_pred = np.zeros_like(pred[0])
    for i in range(len(targets)):
        weight = int(np.prod(radix[i + 1:]))
        joint_true = joint_true + true[i] * weight
        joint_pred = joint_pred + pred[i] * weight
    return compute_classification_metrics(joint_true, joint_pred, metrics)


# ------------------------------------------------------------------------------------------ F0 contours
#: a both-voiced frame further than this from the reference F0 (relative) is a gross pitch error (Rabiner et al. 1976)
GROSS_PITCH_TOLERANCE = 0.2


def f0_voicing(track, voicing_threshold: float = 0.1, silence_db: float = 40.0) -> np.ndarray:
    """Which frames of an F0 track (``utils.audio.F0Track``: f0, aperiodicity, period_index, rms, each (n_frames,) or
    (clips, n_frames)) are voiced: ``aperiodicity < voicing_threshold`` and an ``rms`` within ``silence_db`` of the loudest
    frame of the same clip.  A clip of silence has no voiced frame."""
    aper, rms = np.asarray(track[1], dtype=np.float64), np.asarray(track[3], dtype=np.float64)
    peak = rms.max(axis=-1, keepdims=True)
    return (aper < voicing_threshold) & (rms > 0) & (rms >= peak * 10.0 ** (-silence_db / 20.0))


def compute_f0_metrics(ref, est, voicing_threshold: float = 0.1, silence_db: float = 40.0) -> Dict[str, float]:
    """How well the F0 contour ``est`` follows ``ref`` (two ``utils.audio.F0Track`` of equal shape, e.g. of original and
    synthesised waveforms): ``f0_rmse_cents`` (root mean square of ``1200 log2(est / ref)``) and ``f0_corr`` (Pearson
    correlation of ``log2 f0``) over the frames voiced in both, ``gross_pitch_error`` (share of those frames more than 20 %
    off), ``voicing_error`` (share of all frames voiced in one track only) and ``n_voiced`` (frames voiced in both).  With
    fewer than two such frames the three F0 figures are NaN; the correlation is also NaN where a contour is constant."""
    f_ref, f_est = np.asarray(ref[0], dtype=np.float64), np.asarray(est[0], dtype=np.float64)
    if f_ref.shape != f_est.shape:
        raise ValueError(f"the two tracks differ in shape: {f_ref.shape} and {f_est.shape}")
    v_ref = f0_voicing(ref, voicing_threshold, silence_db)
    v_est = f0_voicing(est, voicing_threshold, silence_db)
    both = v_ref & v_est
    n = int(both.sum())
    out = {"f0_rmse_cents": float("nan"), "f0_corr": float("nan"), "gross_pitch_error": float("nan"),
           "voicing_error": float(np.mean(v_ref != v_est)) if v_ref.size else float("nan"), "n_voiced": n}
    if n < 2:
        return out
    l_ref, l_est = np.log2(f_ref[both]), np.log2(f_est[both])
    out["f0_rmse_cents"] = float(np.sqrt(np.mean((1200.0 * (l_est - l_ref)) ** 2)))
    d_ref, d_est = l_ref - l_ref.mean(), l_est - l_est.mean()
    norm = np.sqrt(np.sum(d_ref ** 2) * np.sum(d_est ** 2))
    if np.ptp(l_ref) > 0 and np.ptp(l_est) > 0 and norm > 0:
        out["f0_corr"] = float(np.sum(d_ref * d_est) / norm)
    out["gross_pitch_error"] = float(np.mean(np.abs(f_est[both] / f_ref[both] - 1.0) > GROSS_PITCH_TOLERANCE))
    return out
