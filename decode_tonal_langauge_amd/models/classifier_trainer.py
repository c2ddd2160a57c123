"""Training loop for ``ClassifierModel``s (counterpart of reference models/classifier_trainer.py:22-177
plus the ``pl.Trainer`` / ``EarlyStopping`` / ``CSVLogger`` it is driven by in
training/classifier_pipeline.py:131-160).

pytorch_lightning and torchmetrics are not part of the MI355X image, so the same behaviour is written
out as a plain loop:
  * loss ``nn.CrossEntropyLoss`` on ``labels.long()``; optimiser ``NAdam`` with two groups - parameters
    with ndim >= 2 get ``weight_decay``, the rest 0 (reference :63-74);
  * one optimiser step per batch, one validation pass per epoch; the epoch's ``val/loss`` is the
    sample-weighted mean over batches;
  * early stopping on ``val/loss``: stop after ``patience`` consecutive epochs without a new minimum;
  * test: macro accuracy and macro F1 over the classes that occur (torchmetrics' macro average
    ignores classes with no true and no predicted sample), confusion matrix rows = true class;
  * ``metrics.csv`` per run with Lightning's column names, ``confusion_matrix_test.csv`` after test.

``fused=True`` runs the same loop on the HIP path (``_simple_classifier_engine`` for the linear and shallow classifiers,
``_cnn_classifier_train_engine`` for ``CNNClassifier``, ``_cnnrnn_classifier_train_engine`` for ``CNNRNNClassifier``: fused
cross-entropy step, ``FusedNAdam``);
loss and confusion matrix then stay on the device and are read once per epoch.

Under a multi-rank process group (``parallel.init_from_env``; ``fused=True`` only) every rank iterates the same global batches,
the engine works on its rows and exchanges gradients, ``epoch_stats`` returns the global statistics on every rank - so early
stopping decides alike everywhere - and rank 0 alone writes ``metrics.csv`` / ``confusion_matrix_test.csv``.
"""
from __future__ import annotations

import csv
import os
from typing import Dict, List, Optional

import numpy as np
import torch
import torch.nn as nn
from torch.optim import NAdam

from .. import parallel
from .classifier import ClassifierModel
from .utils import split_decay_groups


def _confusion(true: torch.Tensor, pred: torch.Tensor, n: int) -> torch.Tensor:
    idx = true.long() * n + pred.long()
    return torch.bincount(idx, minlength=n * n).reshape(n, n)


def macro_scores(cm: torch.Tensor) -> Dict[str, float]:
    """Macro accuracy (= mean per-class recall) and macro F1 from a confusion matrix."""
    cm = cm.double()
    tp = cm.diag()
    fn = cm.sum(1) - tp
    fp = cm.sum(0) - tp
    present = (tp + fp + fn) > 0
    recall = torch.where(tp + fn > 0, tp / (tp + fn).clamp(min=1), torch.zeros_like(tp))
    f1 = torch.where(2 * tp + fp + fn > 0, 2 * tp / (2 * tp + fp + fn).clamp(min=1), torch.zeros_like(tp))
    k = max(int(present.sum()), 1)
    return {"accuracy": float(recall[present].sum() / k), "f1": float(f1[present].sum() / k)}


# ---------------------------------------------------------------------- shared with ``ClassifierEnsembleTrainer``
def epoch_row(epoch: int, step: int, tr: Dict[str, float], va: Dict[str, float], model: nn.Module) -> Dict[str, float]:
    """The ``metrics.csv`` row of one epoch (Lightning's column names); ``step``: optimiser steps taken so far."""
    return {"epoch": epoch, "step": step - 1, "train/loss_epoch": tr["loss"], "train/accuracy": tr["accuracy"],
            "val/loss": va["loss"], "val/accuracy": va["accuracy"], "train/weight_norm": weight_norm(model)}


def epoch_line(row: Dict[str, float]) -> str:
    return (f"epoch {row['epoch']}: train/loss {row['train/loss_epoch']:.4f}  val/loss {row['val/loss']:.4f}  "
            f"val/accuracy {row['val/accuracy']:.3f}")


class EarlyStopping:
    """Early stopping of one model on ``val/loss``: ``patience`` consecutive epochs without a new minimum."""

    def __init__(self, patience: int) -> None:
        self.patience, self.best, self.wait = patience, float("inf"), 0

    def stops(self, val_loss: float) -> bool:
        """Record an epoch's ``val/loss``; true when training stops after it."""
        if val_loss < self.best:
            self.best, self.wait = val_loss, 0
            return False
        self.wait += 1
        return self.wait >= self.patience


def weight_norm(model: nn.Module) -> float:
    return float(sum(float(p.detach().norm(2)) ** 2 for p in model.parameters() if p.requires_grad) ** 0.5)


def write_metrics(log_dir: Optional[str], history: List[Dict[str, float]]) -> None:
    """``metrics.csv`` of one run (the writing rank only)."""
    if log_dir is None or not history or not parallel.is_writer():
        return
    os.makedirs(log_dir, exist_ok=True)
    with open(os.path.join(log_dir, "metrics.csv"), "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=list(history[0].keys()))
        w.writeheader()
        w.writerows(history)


def write_confusion(log_dir: Optional[str], cm: torch.Tensor) -> None:
    """``confusion_matrix_test.csv`` of one run (the writing rank only)."""
    if log_dir is None or not parallel.is_writer():
        return
    os.makedirs(log_dir, exist_ok=True)
    np.savetxt(os.path.join(log_dir, "confusion_matrix_test.csv"), cm.numpy(), fmt="%d", delimiter=",")


class ClassifierTrainer:
    def __init__(self, model: ClassifierModel, learning_rate: float = 0.0005, weight_decay: float = 0.0,
                 log_dir: Optional[str] = None, verbose: bool = False, fused: bool = False) -> None:
        self.model = model
        self.learning_rate = float(learning_rate)
        self.weight_decay = float(weight_decay)
        self.criterion = nn.CrossEntropyLoss()
        self.log_dir = log_dir
        self.verbose = verbose
        self.fused = bool(fused)
        self.engine = None
        if not self.fused and parallel.world()[1] > 1:
            raise ValueError(f"ClassifierTrainer(fused=False) under a process group of {parallel.world()[1]} ranks: data-parallel "
                             "classifier training runs on the HIP engines only (fused=True); the autograd loop is single-process")
        if self.fused:         # an explicit request: a model / device pair the engine does not take raises (ValueError)
            from .deep_classifiers import CNNClassifier, CNNRNNClassifier
            if isinstance(model, CNNClassifier):
                from .._cnn_classifier_train_engine import CnnClassifierTrainEngine as Engine
            elif isinstance(model, CNNRNNClassifier):
                from .._cnnrnn_classifier_train_engine import CnnRnnClassifierTrainEngine as Engine
            else:
                from .._simple_classifier_engine import SimpleClassifierEngine as Engine
            self.engine = Engine(model, self.learning_rate, self.weight_decay)
            self.optimizer = self.engine.optimizer
        else:
            self.optimizer = self.configure_optimizers()
        self.history: List[Dict[str, float]] = []
        self.confusion_matrix: Optional[torch.Tensor] = None
        self.test_accuracy: Optional[float] = None
        self.test_f1: Optional[float] = None
        self.stopped_epoch: Optional[int] = None

    # ------------------------------------------------------------------ optimiser
    def configure_optimizers(self) -> NAdam:
        decay, no_decay = split_decay_groups(self.model.named_parameters())
        return NAdam([{"params": decay, "weight_decay": self.weight_decay},
                      {"params": no_decay, "weight_decay": 0.0}], lr=self.learning_rate)

    # ------------------------------------------------------------------ epochs
    def _run_epoch(self, loader, train: bool) -> Dict[str, float]:
        if self.engine is not None:
            return self._run_epoch_fused(loader, train)
        n_cls = self.model.n_classes
        loss_sum, n_seen = 0.0, 0
        cm = torch.zeros(n_cls, n_cls, dtype=torch.long)
        self.model.train(train)
        for x, y in loader:
            y = y.long()
            with torch.set_grad_enabled(train):
                logits = self.model(x)
                loss = self.criterion(logits, y)
            if train:
                self.optimizer.zero_grad()
                loss.backward()
                self.optimizer.step()
            loss_sum += float(loss.detach()) * len(y)
            n_seen += len(y)
            cm += _confusion(y.cpu(), logits.detach().argmax(1).cpu(), n_cls)
        return {"loss": loss_sum / max(n_seen, 1), "accuracy": macro_scores(cm)["accuracy"]}

    def _run_epoch_fused(self, loader, train: bool) -> Dict[str, float]:
        """The same epoch on the engine: the per-sample losses and the confusion matrix accumulate on the device, one read."""
        self.model.train(train)
        step = self.engine.train_batch if train else self.engine.eval_batch
        for x, y in loader:
            step(x, y)
        loss_sum, n_seen, cm = self.engine.epoch_stats()
        return {"loss": loss_sum / max(n_seen, 1), "accuracy": macro_scores(cm)["accuracy"]}

    def fit(self, train_loader, val_loader, max_epochs: int, patience: int) -> List[Dict[str, float]]:
        stopping, step = EarlyStopping(patience), 0
        for epoch in range(max_epochs):
            tr = self._run_epoch(train_loader, True)
            step += len(train_loader)
            va = self._run_epoch(val_loader, False)
            row = epoch_row(epoch, step, tr, va, self.model)
            self.history.append(row)
            if self.verbose:
                print(epoch_line(row))
            if stopping.stops(va["loss"]):
                self.stopped_epoch = epoch
                break
        self._write_metrics()
        return self.history

    def _write_metrics(self) -> None:
        write_metrics(self.log_dir, self.history)

    # ------------------------------------------------------------------ evaluation
    @torch.no_grad()
    def test(self, loader) -> Dict[str, object]:
        n_cls = self.model.n_classes
        cm = torch.zeros(n_cls, n_cls, dtype=torch.long)
        self.model.eval()
        if self.engine is not None:
            for x, y in loader:
                self.engine.eval_batch(x, y)
            cm = self.engine.epoch_stats()[2]
        else:
            for x, y in loader:
                cm += _confusion(y.long().cpu(), self.model(x).argmax(1).cpu(), n_cls)
        scores = macro_scores(cm)
        self.test_accuracy, self.test_f1, self.confusion_matrix = scores["accuracy"], scores["f1"], cm
        write_confusion(self.log_dir, cm)
        return {"accuracy": self.test_accuracy, "f1": self.test_f1, "confusion_matrix": cm}

    @torch.no_grad()
    def predict(self, loader) -> torch.Tensor:
        self.model.eval()
        if self.engine is not None:
            return torch.cat([self.engine.predict_batch(x) for x, _ in loader])
        return torch.cat([self.model(x).argmax(dim=1) for x, _ in loader])

    # ------------------------------------------------------------------ helpers
    def get_nparams(self) -> int:
        return self.model.get_nparams()

    def get_layer_nparams(self) -> Dict[str, int]:
        return self.model.get_layer_nparams()
