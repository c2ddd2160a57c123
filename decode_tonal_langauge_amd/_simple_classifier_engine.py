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
(``_classifier_dp``): ``grad_scale`` is 1 / B_global, the bias gradients (and dense weight gradients) are summed by one bucketed
all-reduce, and at B_global <= ``LOWRANK_MAX`` the weights travel as the gathered factor rows - every rank applies the same
rank-B_global update.  Without one nothing changes.

There is no CPU fallback and no fallback to autograd: a model outside the supported set is refused."""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch
import torch.nn as nn

from . import _lib
from ._classifier_dp import ClassifierDP
from ._launch import launch_nt, launch_tn, r4
from ._lib import EPI_LRELU, LOAD_DIRECT, check, ptr
from .models.utils import split_decay_groups
from .optim import FusedNAdam

SUPPORTED = ("the fused classifier step supports LogisticRegressionClassifier and ShallowNNClassifier with fp32 parameters on "
             "a CUDA device, input_dim % 4 == 0, hidden_dim % 4 == 0, n_classes <= 64 and a ReLU or LeakyReLU activation; "
             "CNNClassifier (_cnn_classifier_train_engine) with fp32 parameters on a CUDA device, negative_slope >= 0, "
             "n_classes <= 64 and dropout < 1; CNNRNNClassifier (_cnnrnn_classifier_train_engine) under the same conditions with "
             "at least one row left behind its (3,1) pool")


def check_supported(model) -> None:
    """Raise ``ValueError`` (stating the supported set) unless ``model`` can be trained by ``SimpleClassifierEngine``."""
    from .models.simple_classifiers import LogisticRegressionClassifier, ShallowNNClassifier

    def refuse(why: str):
        raise ValueError(f"{why}: {SUPPORTED}")
    if isinstance(model, LogisticRegressionClassifier):
        layers = [model.linear]
    elif isinstance(model, ShallowNNClassifier):
        layers = [model.hidden, model.output]
        if not isinstance(model.activation, (nn.ReLU, nn.LeakyReLU)):
            refuse(f"activation {type(model.activation).__name__}")
        if model.hidden.out_features % 4 != 0:
            refuse(f"hidden_dim {model.hidden.out_features}")
    else:
        refuse(f"model {type(model).__name__}")
    if model.input_dim % 4 != 0:
        refuse(f"input_dim {model.input_dim}")
    if model.n_classes > 64:
        refuse(f"n_classes {model.n_classes}")
    for layer in layers:
        if layer.bias is None:
            refuse("a layer without bias")
        for p in (layer.weight, layer.bias):
            if not p.is_cuda or p.dtype != torch.float32:
                refuse(f"parameters on '{p.device}' in {p.dtype}")


class _Workspace:
    """Buffers of one batch size (a loader has two: the full batch and the ragged last one)."""

    def __init__(self, B: int, N: int, H: int, dev):
        f32 = dict(dtype=torch.float32, device=dev)
        self.logits = torch.empty(B, N, **f32)
        self.dlogits = torch.zeros(B, r4(N), **f32)
        self.pred = torch.empty(B, dtype=torch.int64, device=dev)
        self.h = torch.empty(B, H, **f32) if H else None
        self.dh = torch.empty(B, H, **f32) if H else None


class SimpleClassifierEngine(ClassifierDP):
    def __init__(self, model, learning_rate: float = 0.0005, weight_decay: float = 0.0):
        check_supported(model)
        self.lib = _lib.load()
        self.model = model
        self.N = int(model.n_classes)
        self.K = int(model.input_dim)
        self.shallow = hasattr(model, "hidden")
        if self.shallow:
            self.H = int(model.hidden.out_features)
            act = model.activation
            self.act, self.slope = (1, 0.0) if isinstance(act, nn.ReLU) else (2, float(act.negative_slope))
            self.head = model.output
        else:
            self.H, self.act, self.slope = 0, 0, 0.0
            self.head = model.linear
        self.device = self.head.weight.device
        decay, no_decay = split_decay_groups(model.named_parameters())
        self.optimizer = FusedNAdam([{"params": decay, "weight_decay": float(weight_decay)},
                                     {"params": no_decay, "weight_decay": 0.0}], lr=float(learning_rate), stored_beta2=True)
        self.force_dense = False           # tests / the benchmark: materialise dW at a batch the low-rank update would take
        # loss sum (the bits of a double), sample count, label-range flag, confusion matrix: one buffer, one read per epoch
        self.stats = torch.zeros(3 + self.N * self.N, dtype=torch.int64, device=self.device)
        self._dp_setup()
        if self.dp:            # the always-dense gradients (the biases) as views of one arena: one all-reduce, no staging copy
            named = {k: p for k, p in model.named_parameters() if any(p is q for q in no_decay)}
            views = self._make_arena({k: p.shape for k, p in named.items()})
            self.grads: Dict[nn.Parameter, torch.Tensor] = {named[k]: v for k, v in views.items()}
        else:
            self.grads = {p: torch.zeros_like(p) for p in no_decay}
        self._ws: Dict[int, _Workspace] = {}
        self.last_lowrank: Dict[nn.Parameter, Tuple[torch.Tensor, torch.Tensor]] = {}   # the factors of the last train step

    # ------------------------------------------------------------------ plumbing
    def _workspace(self, B: int) -> _Workspace:
        ws = self._ws.get(B)
        if ws is None:
            if len(self._ws) > 4:
                self._ws.clear()
            ws = self._ws[B] = _Workspace(B, self.N, self.H, self.device)
        return ws

    def _input(self, x: torch.Tensor) -> torch.Tensor:
        _lib.require_gpu(x, "SimpleClassifierEngine")
        if x.ndim > 2:
            x = x.reshape(x.size(0), -1)
        if x.ndim != 2 or x.shape[1] != self.K:
            raise ValueError(f"Expected input dimension {self.K}, got {tuple(x.shape)}.")
        if x.shape[0] < 1:
            raise ValueError("empty batch")
        x = x.float().contiguous()
        return x if x.data_ptr() % 16 == 0 else x.clone()

    def _labels(self, y: torch.Tensor, B: int) -> torch.Tensor:
        _lib.require_gpu(y, "SimpleClassifierEngine")
        if y.shape != (B,):
            raise ValueError(f"expected {B} labels, got {tuple(y.shape)}")
        return y.long().contiguous()

    def _stream(self) -> int:
        return torch.cuda.current_stream().cuda_stream

    def _forward(self, x: torch.Tensor, ws: _Workspace) -> None:
        B, st = x.shape[0], self._stream()
        feat, kf = x, self.K
        if self.shallow:
            hid = self.model.hidden
            launch_nt(self.lib, A=ptr(x), Bw=ptr(hid.weight), bias=ptr(hid.bias), out=ptr(ws.h), M=B, A_rows=B, N=self.H,
                      K=self.K, lda=self.K, ldb=self.K, ldo=self.H, Tvalid=1, loader=LOAD_DIRECT, epilogue=EPI_LRELU,
                      slope=self.slope)
            feat, kf = ws.h, self.H
        check(self.lib.tl_linear_rows(ptr(feat), ptr(self.head.weight), ptr(self.head.bias), ptr(ws.logits), B, kf, self.N, kf,
                                      0, st), "tl_linear_rows")

    def _ce(self, ws: _Workspace, y: Optional[torch.Tensor], B: int, grad: bool, pred: bool) -> None:
        base = self._stats_base()
        check(self.lib.tl_ce_loss(ptr(ws.logits), ptr(y), ptr(ws.dlogits) if grad else None,
                                  ptr(self.grads[self.head.bias]) if grad else None, ptr(ws.pred) if pred else None,
                                  base, base + 8, base + 24, base + 16, B, self.N, self.N, ws.dlogits.shape[1],
                                  self._grad_scale(), self._stream()), "tl_ce_loss")

    def _dense(self, p: nn.Parameter) -> torch.Tensor:
        g = self.grads.get(p)
        if g is None:
            g = self.grads[p] = torch.empty_like(p)
        return g

    # ------------------------------------------------------------------ the public steps
    @torch.no_grad()
    def train_batch(self, x: torch.Tensor, y: torch.Tensor) -> None:
        """Forward, loss, backward and update for one batch; everything stays on the stream (no host read)."""
        x = self._input(x)
        y = self._labels(y, x.shape[0])
        dense = self.force_dense or x.shape[0] > FusedNAdam.LOWRANK_MAX      # (from the GLOBAL batch: the same on every rank)
        x, y = self._take(x, y)
        B = x.shape[0]
        ws = self._workspace(B)
        st = self._stream()
        self._forward(x, ws)
        self._ce(ws, y, B, grad=True, pred=False)
        ldd = ws.dlogits.shape[1]
        hw = self.head.weight
        grads = {p: g for p, g in self.grads.items() if p.ndim < 2}
        lowrank: Dict[nn.Parameter, Tuple[torch.Tensor, torch.Tensor]] = {}
        dout = ws.dlogits[:, :self.N]
        if self.shallow:
            hid = self.model.hidden
            check(self.lib.tl_head_bwd(ptr(ws.dlogits), ptr(ws.h), ptr(hw), ptr(ws.dh), ptr(self.grads[hid.bias]),
                                       ptr(self._dense(hw)) if dense else None, B, self.H, self.N, ldd, self.act, self.slope, st),
                  "tl_head_bwd")
            if dense:
                launch_tn(self.lib, A=ptr(ws.dh), B=ptr(x), slab=ptr(self._dense(hid.weight)), Krows=B, A_rows=B, B_rows=B,
                          Mdim=self.H, Ndim=self.K, lda=self.H, ldb=self.K, ldc=self.K, loader=LOAD_DIRECT)
                grads[hw], grads[hid.weight] = self.grads[hw], self.grads[hid.weight]
            else:
                lowrank[hw], lowrank[hid.weight] = (dout, ws.h), (ws.dh, x)
        elif dense:
            check(self.lib.tl_head_bwd(ptr(ws.dlogits), ptr(x), ptr(hw), None, None, ptr(self._dense(hw)), B, self.K, self.N, ldd,
                                       0, 0.0, st), "tl_head_bwd")
            grads[hw] = self.grads[hw]
        else:
            lowrank[hw] = (dout, x)
        if self.dp:
            # dlogits travels at its stored width (the factor is its first N columns)
            sent = {p: (ws.dlogits if fa is dout else fa, fb) for p, (fa, fb) in lowrank.items()}
            got = self._exchange(extra=[g for p, g in grads.items() if p.ndim >= 2], lowrank=sent)
            lowrank = {p: (fa[:, :self.N] if sent[p][0] is ws.dlogits else fa, fb) for p, (fa, fb) in got.items()}
        self.last_lowrank = lowrank
        self.optimizer.step(grads=grads, lowrank=lowrank or None)

    @torch.no_grad()
    def eval_batch(self, x: torch.Tensor, y: torch.Tensor) -> None:
        """Forward and loss statistics of one batch (no gradients, no update)."""
        x = self._input(x)
        x, y = self._take(x, self._labels(y, x.shape[0]))
        ws = self._workspace(x.shape[0])
        self._forward(x, ws)
        self._ce(ws, y, x.shape[0], grad=False, pred=False)

    @torch.no_grad()
    def predict_batch(self, x: torch.Tensor) -> torch.Tensor:
        """Arg-max class of every row (int64, on the device)."""
        x, _ = self._take(self._input(x))
        ws = self._workspace(x.shape[0])
        self._forward(x, ws)
        self._ce(ws, None, x.shape[0], grad=False, pred=True)
        return self._gather_pred(ws.pred) if self.dp else ws.pred.clone()

    epoch_stats = ClassifierDP.epoch_stats
