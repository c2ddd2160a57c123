"""Training of ``LogisticRegressionClassifier`` and ``ShallowNNClassifier`` on the HIP path (the loop of reference
models/classifier_trainer.py:22-177: ``nn.CrossEntropyLoss``, ``loss.backward()``, ``NAdam`` with two decay groups, a
confusion matrix per epoch).

One train step of a batch (B, K):
  forward   ``tl_linear_rows`` (and, for the hidden layer, the NT GEMM with bias and ReLU / LeakyReLU in its epilogue) - the
            launches inference uses; the hidden activations are kept for the backward;
  loss      ``tl_ce_loss``: dlogits, the output bias gradient, and loss sum / sample count / confusion matrix ADDED to device
            words that are read once per epoch (``epoch_stats``) - no per-batch host read;
  backward  ``tl_head_bwd``: one pass over the head's input gives its input gradient (activation derivative applied), the
            hidden bias gradient and, when wanted, the head's weight gradient;
  update    one ``FusedNAdam``.  With B <= ``FusedNAdam.LOWRANK_MAX`` a weight gradient is the rank-B product
            ``dout^T . input`` and is applied by ``tl_nadam_lowrank`` without ever being stored; above that it is written by
            ``tl_head_bwd`` (head) or the TN GEMM (hidden layer) and applied by ``tl_nadam``.

Under a process group (``parallel.active()``) every public step takes the GLOBAL batch and works on this rank's rows
(``_classifier_train_engine``, ``_classifier_dp``): ``grad_scale`` is 1 / B_global, the bias gradients (and dense weight gradients) are summed by one bucketed
all-reduce, and at B_global <= ``LOWRANK_MAX`` the weights travel as the gathered factor rows - every rank applies the same
rank-B_global update.  Without one the step is the same launches on the whole batch.

There is no CPU fallback and no fallback to autograd: a model outside the supported set is refused."""
from __future__ import annotations

from typing import Dict, Tuple

import torch
import torch.nn as nn

from . import _lib
from ._classifier_train_engine import SUPPORTED  # noqa: F401  (re-exported: it was defined here)
from ._classifier_train_engine import ClassifierTrainEngine, parameter_unmet, refuse
from ._launch import launch_nt, launch_tn, r4
from ._lib import EPI_LRELU, LOAD_DIRECT, ptr


def activation_code(model) -> Tuple[int, float]:
    """(act code of ``tl_head_bwd``, slope) of a ``ShallowNNClassifier``'s activation; (0, 0.0) without a hidden layer."""
    if not hasattr(model, "hidden"):
        return 0, 0.0
    act = model.activation
    return (1, 0.0) if isinstance(act, nn.ReLU) else (2, float(act.negative_slope))


def unmet(model) -> Dict[str, str]:
    """What a simple classifier misses of the conditions the HIP step sets per model: {condition: the reason to refuse it
    with}.  The keys - "activation", "hidden_dim", "input_dim", "n_classes", "bias", "parameters" - come in the order in
    which the refusals are reported."""
    out, shallow = {}, hasattr(model, "hidden")
    layers = (model.hidden, model.output) if shallow else (model.linear,)
    if shallow:
        if not isinstance(model.activation, (nn.ReLU, nn.LeakyReLU)):
            out["activation"] = f"activation {type(model.activation).__name__}"
        if model.hidden.out_features % 4 != 0:
            out["hidden_dim"] = f"hidden_dim {model.hidden.out_features}"
    if model.input_dim % 4 != 0:
        out["input_dim"] = f"input_dim {model.input_dim}"
    if model.n_classes > 64:
        out["n_classes"] = f"n_classes {model.n_classes}"
    if any(layer.bias is None for layer in layers):
        out["bias"] = "a layer without bias"
    whys = [why for why in map(parameter_unmet, model.parameters()) if why]
    if whys:
        out["parameters"] = whys[0]
    return out


def check_supported(model) -> None:
    """Raise ``ValueError`` (stating the supported set) unless ``model`` can be trained by ``SimpleClassifierEngine``."""
    from .models.simple_classifiers import LogisticRegressionClassifier, ShallowNNClassifier
    if not isinstance(model, (LogisticRegressionClassifier, ShallowNNClassifier)):
        refuse(f"model {type(model).__name__}")
    for why in unmet(model).values():
        refuse(why)


class _Workspace:
    """Buffers of one batch size (a loader has two: the full batch and the ragged last one)."""

    def __init__(self, B: int, N: int, H: int, dev):
        f32 = dict(dtype=torch.float32, device=dev)
        self.x = None                                   # the input rows of the last forward pass
        self.logits = torch.empty(B, N, **f32)
        self.dlogits = torch.zeros(B, r4(N), **f32)
        self.pred = torch.empty(B, dtype=torch.int64, device=dev)
        self.h = torch.empty(B, H, **f32) if H else None
        self.dh = torch.empty(B, H, **f32) if H else None


class SimpleClassifierEngine(ClassifierTrainEngine):
    CE = "tl_ce_loss"
    CE_BUFFERS = ("logits", "dlogits")
    INPUT_ERROR = "Expected input dimension {}, got {got}."

    def __init__(self, model, learning_rate: float = 0.0005, weight_decay: float = 0.0):
        check_supported(model)
        self.lib = _lib.load()
        self.K = int(model.input_dim)
        self.input_shape = (self.K,)
        self.shallow = hasattr(model, "hidden")
        self.act, self.slope = activation_code(model)
        if self.shallow:
            self.H = int(model.hidden.out_features)
            self.head_name, weights = "output", ("output.weight", "hidden.weight")
        else:
            self.H = 0
            self.head_name, weights = "linear", ("linear.weight",)
        self.head_bias = self.head_name + ".bias"
        # the biases are always dense; a weight gets its buffer on demand (dense path only)
        self._setup_training(model, learning_rate, weight_decay, lowrank_names=weights)

    # ------------------------------------------------------------------ plumbing
    def _make_workspace(self, B: int, dev) -> _Workspace:
        return _Workspace(B, self.N, self.H, dev)

    def _input(self, x: torch.Tensor) -> torch.Tensor:
        x = super()._input(x.reshape(x.size(0), -1) if x.ndim > 2 else x)
        return x if x.data_ptr() % 16 == 0 else x.clone()

    def _forward(self, x: torch.Tensor, dropout: bool) -> _Workspace:
        B, prm = x.shape[0], self.params
        ws = self._workspace(B, x.device)
        ws.x = x
        feat, kf = x, self.K
        if self.shallow:
            launch_nt(self.lib, A=ptr(x), Bw=ptr(prm["hidden.weight"]), bias=ptr(prm["hidden.bias"]), out=ptr(ws.h), M=B, A_rows=B,
                      N=self.H, K=self.K, lda=self.K, ldb=self.K, ldo=self.H, Tvalid=1, loader=LOAD_DIRECT, epilogue=EPI_LRELU,
                      slope=self.slope)
            feat, kf = ws.h, self.H
        self._call(None, "tl_linear_rows", ptr(feat), ptr(prm[self.head_name + ".weight"]), ptr(prm[self.head_bias]),
                   ptr(ws.logits), B, kf, self.N, kf, 0)
        return ws

    def _backward(self, ws: _Workspace, B: int, dense: bool) -> None:
        """Every gradient of the step from ``ws.dlogits``: the biases (and, when ``dense``, the weights) into ``self.grads``,
        otherwise the weights as factors in ``self.last_lowrank``."""
        x, ldd = ws.x, ws.dlogits.shape[1]
        hw = self.head_name + ".weight"
        dout = ws.dlogits[:, :self.N]
        self.last_lowrank = {}
        if self.shallow:
            self._call(None, "tl_head_bwd", ptr(ws.dlogits), ptr(ws.h), ptr(self.params[hw]), ptr(ws.dh),
                       ptr(self.grads["hidden.bias"]), ptr(self._dense(hw)) if dense else None, B, self.H, self.N, ldd, self.act,
                       self.slope)
            if dense:
                launch_tn(self.lib, A=ptr(ws.dh), B=ptr(x), slab=ptr(self._dense("hidden.weight")), Krows=B, A_rows=B, B_rows=B,
                          Mdim=self.H, Ndim=self.K, lda=self.H, ldb=self.K, ldc=self.K, loader=LOAD_DIRECT)
            else:
                self.last_lowrank = {hw: (dout, ws.h), "hidden.weight": (ws.dh, x)}
        elif dense:
            self._call(None, "tl_head_bwd", ptr(ws.dlogits), ptr(x), ptr(self.params[hw]), None, None, ptr(self._dense(hw)), B,
                       self.K, self.N, ldd, 0, 0.0)
        else:
            self.last_lowrank = {hw: (dout, x)}

    def _lowrank_wire(self, ws: _Workspace):
        return {self.head_name + ".weight": ws.dlogits}       # dlogits travels at its stored width (the factor is its first N columns)
