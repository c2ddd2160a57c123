"""All seeds of a classifier experiment in one pass: M ``LogisticRegressionClassifier``s or M ``ShallowNNClassifier``s of equal
shape ("members") trained side by side by the launches that train one (``_simple_classifier_engine``).

A step of the single engine is a handful of launches that occupy a few of the 256 CUs for a few microseconds each; the group
kernels (``tl_*_group``, include/tonal_hip.h) are the same kernels with a member dimension on the grid, so the step of M
members costs the same number of launches.  They are the SAME kernels - the single entry points launch them with M = 1 - and
every member therefore gets the bits ``SimpleClassifierEngine`` would give it on the same batches.

Storage is stacked, per Linear layer: the weight (M, out, in), the bias (M, r4(out)) (a row of N floats is not 16-byte aligned,
which the update kernels want), moments and the bias gradient likewise; logits, dlogits, pred, the hidden activations and their
gradient (M, B, ...) and the statistics words (M, 3 + N^2).  Each module's parameters become views of the stacks, so
``state_dict()``, ``torch.save`` and inference through the module keep working.

The shallow step mirrors the single engine's low-rank route launch for launch: the hidden layer on the NT GEMM's group form
(bias and ReLU / LeakyReLU in its epilogue), the output layer on ``tl_linear_rows_group``, ``tl_ce_loss_group``,
``tl_head_bwd_act_group`` (dh with the activation derivative, the hidden bias gradient - it reads the output weight BEFORE its
update), then the two weights as rank-B updates and the two biases.  Its training batches hold at most
``FusedNAdam.LOWRANK_MAX`` rows: above that the single engine forms the hidden weight gradient on TN GEMM kernels that have no
member dimension.  Evaluation and prediction take any batch size.  The logistic group keeps its dense route.

``set_active(mask)``: the workgroups of a member whose mask word is 0 return before their first load - a member that stopped
early stays frozen, to the bit, while the others go on.  The NAdam schedule is one counter shared by the active members: they
advance in lockstep from step 0, and a member never resumes, so its step count freezes with its parameters.

Out of scope (refused with the supported set): every other model class, a group mixing the two classes, members of differing
shape or activation, a multi-rank process group.  There is no CPU fallback."""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import torch
import torch.nn as nn

from . import _lib, parallel
from ._classifier_train_engine import parameter_unmet
from ._launch import launch_nt_group, r4
from ._lib import EPI_LRELU, LOAD_DIRECT, check, ptr
from ._simple_classifier_engine import activation_code, unmet
from .models.utils import split_decay_groups
from .optim import FusedNAdam

SUPPORTED = ("the classifier ensemble supports one or more LogisticRegressionClassifier of equal input_dim and n_classes, or one or "
             "more ShallowNNClassifier of equal input_dim, hidden_dim and n_classes with the same ReLU or LeakyReLU activation "
             "(equal negative_slope), hidden_dim % 4 == 0 and training batches of at most 64 rows - never a mix of the two "
             "classes - with biases and fp32 parameters on one CUDA device, input_dim % 4 == 0 and n_classes <= 64, in a single "
             "process (no multi-rank process group); the deep classifiers train one model at a time (ClassifierTrainer)")


def refuse(why: str):
    raise ValueError(f"{why}: {SUPPORTED}")


def _shape(m) -> tuple:
    hidden = getattr(m, "hidden", None)
    return (int(m.input_dim),) + ((int(hidden.out_features),) if hidden is not None else ()) + (int(m.n_classes),)


def _arrow(shape: tuple) -> str:
    return "(" + " -> ".join(str(s) for s in shape) + ")"


def check_supported(models: Sequence) -> None:
    """Raise ``ValueError`` (stating the supported set) unless ``models`` can be trained by ``ClassifierEnsembleEngine``: the
    conditions of the single engine on every member (``_simple_classifier_engine.unmet``) and, between them, the group's."""
    from .models.simple_classifiers import LogisticRegressionClassifier, ShallowNNClassifier
    models = list(models)
    if not models:
        refuse("no models")
    first = models[0]
    for m in models:
        if not isinstance(m, (LogisticRegressionClassifier, ShallowNNClassifier)):
            refuse(f"model {type(m).__name__}")
        if type(m) is not type(first):
            refuse(f"model {type(m).__name__} in a group of {type(first).__name__}")
    for i, m in enumerate(models):
        if _shape(m) != _shape(first):
            refuse(f"member {i} has shape {_arrow(_shape(m))}, member 0 {_arrow(_shape(first))}")
    misses = [unmet(m) for m in models]
    if hasattr(first, "hidden"):
        for i, m in enumerate(models):
            if "activation" in misses[i]:
                refuse(misses[i]["activation"])
            if type(m.activation) is not type(first.activation):
                refuse(f"member {i} has activation {type(m.activation).__name__}, member 0 {type(first.activation).__name__}")
            if activation_code(m) != activation_code(first):
                refuse(f"member {i} has negative_slope {activation_code(m)[1]}, member 0 {activation_code(first)[1]}")
        if activation_code(first)[1] < 0:
            refuse(f"negative_slope {activation_code(first)[1]}")
    for condition in ("hidden_dim", "input_dim", "n_classes", "bias"):
        for miss in misses:
            if condition in miss:
                refuse(miss[condition])
    if parallel.world()[1] > 1:
        refuse(f"a process group of {parallel.world()[1]} ranks")
    dev = None
    for m in models:
        for p in m.parameters():
            if parameter_unmet(p):
                refuse(parameter_unmet(p))
            if dev is not None and p.device != dev:
                refuse(f"parameters on '{p.device}' and '{dev}'")
            dev = p.device


def check_train_batch(shallow: bool, B: int) -> None:
    """Raise ``ValueError`` for a training batch size the group cannot take (shallow members: the low-rank route only)."""
    if shallow and B > FusedNAdam.LOWRANK_MAX:
        raise ValueError(f"a training batch of {B} rows: the ShallowNNClassifier ensemble trains batches of at most "
                         f"{FusedNAdam.LOWRANK_MAX} rows (above that the hidden layer's weight gradient needs the TN GEMM "
                         "kernels, which have no member dimension); evaluation and prediction take any batch size")


def _member_stride(t: torch.Tensor, *same) -> int:
    """The member stride of a stacked buffer, read off the tensor whose pointer a group launch is given - once, where the
    buffer is made.  Every member must be one dense block (the launches take the leading dimensions from the sizes), and the
    buffers in ``same`` - moments, a gradient - are passed with the same stride."""
    if not t[0].is_contiguous() or any(u.stride() != t.stride() for u in same):
        raise RuntimeError(f"a stacked buffer {tuple(t.shape)} with strides {t.stride()}: members not dense, or not laid out "
                           "like the buffers that share its member stride")
    return t.stride(0)


class _Layer:
    """One Linear layer of all members: weight (M, rows, cols), bias (M, r4(rows)), their moments, the bias gradient."""

    def __init__(self, name: str, layers: Sequence[nn.Linear], dev):
        self.name = name
        M, (rows, cols) = len(layers), layers[0].weight.shape
        self.rows, self.cols = int(rows), int(cols)
        f32 = dict(dtype=torch.float32, device=dev)
        self.W = torch.empty(M, rows, cols, **f32)
        self.b = torch.zeros(M, r4(self.rows), **f32)
        with torch.no_grad():
            for m, layer in enumerate(layers):
                # parameters move into the stacks; the modules keep views of them
                self.W[m].copy_(layer.weight.detach())
                self.b[m, :rows].copy_(layer.bias.detach())
                layer.weight.data = self.W[m]
                layer.bias.data = self.b[m, :rows]
        self.mW, self.vW = torch.zeros_like(self.W), torch.zeros_like(self.W)
        self.mb, self.vb = torch.zeros_like(self.b), torch.zeros_like(self.b)
        self.db = torch.zeros_like(self.b)
        self.s_W = _member_stride(self.W, self.mW, self.vW)
        self.s_b = _member_stride(self.b, self.mb, self.vb, self.db)

    def moments(self, m: int):
        return {self.name + ".weight": (self.mW[m], self.vW[m]),
                self.name + ".bias": (self.mb[m, :self.rows], self.vb[m, :self.rows])}


class _Workspace:
    """Buffers of one batch size (a loader has two: the full batch and the ragged last one)."""

    def __init__(self, M: int, B: int, N: int, H: int, dev):
        f32 = dict(dtype=torch.float32, device=dev)
        self.logits = torch.empty(M, B, N, **f32)
        self.dlogits = torch.zeros(M, B, r4(N), **f32)
        self.pred = torch.zeros(M, B, dtype=torch.int64, device=dev)
        self.h = torch.zeros(M, B, H, **f32) if H else None          # the hidden activations, kept for the backward
        self.dh = torch.zeros(M, B, H, **f32) if H else None
        self.s_logits, self.s_dlogits, self.s_pred = (_member_stride(t) for t in (self.logits, self.dlogits, self.pred))
        self.s_h = _member_stride(self.h, self.dh) if H else 0


class ClassifierEnsembleEngine:
    def __init__(self, models: Sequence, learning_rate: float = 0.0005, weight_decay: float = 0.0):
        check_supported(models)
        self.models = list(models)
        self.lib = _lib.load()
        M = self.M = len(self.models)
        first = self.models[0]
        self.shallow = hasattr(first, "hidden")
        K, N = self.K, self.N = int(first.input_dim), int(first.n_classes)
        dev = self.device = next(first.parameters()).device
        self.act, self.slope = activation_code(first)
        if self.shallow:
            self.H = int(first.hidden.out_features)
            self.hidden = _Layer("hidden", [m.hidden for m in self.models], dev)
            self.head = _Layer("output", [m.output for m in self.models], dev)
            self.layers = [self.hidden, self.head]
        else:
            self.H = 0
            self.hidden = None
            self.head = _Layer("linear", [m.linear for m in self.models], dev)
            self.layers = [self.head]
        self._dW: Optional[torch.Tensor] = None          # on demand (the logistic dense path only), with its member stride
        self._s_dW = 0
        # loss sum (the bits of a double), sample count, label-range flag, confusion matrix per member: one read per epoch
        self.stats = torch.zeros(M, 3 + N * N, dtype=torch.int64, device=dev)
        self.s_stats = _member_stride(self.stats)        # in 8-byte words
        # the schedule and the hyper-parameters are the single engine's: the two decay groups of ``_setup_training`` (the
        # weights decay, the biases do not), ``stored_beta2`` scalars; member 0's parameters stand for the group
        decay, no_decay = split_decay_groups(first.named_parameters())
        self.optimizer = FusedNAdam([{"params": decay, "weight_decay": float(weight_decay)},
                                     {"params": no_decay, "weight_decay": 0.0}], lr=float(learning_rate), stored_beta2=True)
        self.step_no, self.mu_product = 0, 1.0
        # tests / the benchmark: materialise dW at a batch the low-rank update would take (logistic members only)
        self.force_dense = False
        self._mask = [1] * M
        self._active: Optional[torch.Tensor] = None      # device words; None while every member is active
        self._workspaces = {}

    # ------------------------------------------------------------------ plumbing
    def _stream(self) -> int:
        return torch.cuda.current_stream().cuda_stream

    def _call(self, name: str, *args) -> None:
        check(getattr(self.lib, name)(*args, ptr(self._active), self._stream()), name)

    def _workspace(self, B: int) -> _Workspace:
        ws = self._workspaces.get(B)
        if ws is None:
            if len(self._workspaces) > 4:
                self._workspaces.clear()
            ws = self._workspaces[B] = _Workspace(self.M, B, self.N, self.H, self.device)
        return ws

    def set_active(self, mask: Sequence) -> None:
        """``mask[m]`` false: member m is frozen from now on.  Uploaded only when it changes."""
        mask = [1 if a else 0 for a in mask]
        if len(mask) != self.M:
            raise ValueError(f"expected a mask of {self.M} members, got {len(mask)}")
        if mask == self._mask:
            return
        self._mask = mask
        self._active = None if all(mask) else torch.tensor(mask, dtype=torch.int32).to(self.device)

    @property
    def active(self) -> List[bool]:
        return [bool(a) for a in self._mask]

    def _input(self, x: torch.Tensor) -> torch.Tensor:
        _lib.require_gpu(x, type(self).__name__)
        if x.ndim > 3:
            x = x.reshape(x.size(0), x.size(1), -1)
        if x.ndim != 3 or x.shape[0] != self.M or x.shape[2] != self.K:
            raise ValueError(f"expected input ({self.M}, B, {self.K}), got {tuple(x.shape)}")
        if x.shape[1] < 1:
            raise ValueError("empty batch")
        x = x.float().contiguous()
        return x if x.data_ptr() % 16 == 0 else x.clone()

    def _labels(self, y: torch.Tensor, B: int) -> torch.Tensor:
        _lib.require_gpu(y, type(self).__name__)
        if y.shape != (self.M, B):
            raise ValueError(f"expected ({self.M}, {B}) labels, got {tuple(y.shape)}")
        return y.long().contiguous()

    def _input_stride(self, t: torch.Tensor) -> int:
        """The member stride of a batch ``_input`` / ``_labels`` made dense.  A group of one has none: the leading stride of a
        dense (1, ...) tensor is arbitrary, and the kernels multiply it by member 0."""
        return t.stride(0) if self.M > 1 else 0

    def _forward(self, x: torch.Tensor) -> _Workspace:
        B = x.shape[1]
        ws = self._workspace(B)
        s_x = self._input_stride(x)
        feat, s_feat, kf = x, s_x, self.K
        if self.shallow:
            hid, H = self.hidden, self.H
            # the launch of ``SimpleClassifierEngine._forward`` with the member on grid.z
            launch_nt_group(self.lib, self.M, s_x, hid.s_W, hid.s_b, ws.s_h, self._active, A=ptr(x), Bw=ptr(hid.W),
                            bias=ptr(hid.b), out=ptr(ws.h), M=B, A_rows=B, N=H, K=self.K, lda=self.K, ldb=self.K, ldo=H, Tvalid=1,
                            loader=LOAD_DIRECT, epilogue=EPI_LRELU, slope=self.slope)
            feat, s_feat, kf = ws.h, ws.s_h, H
        head = self.head
        self._call("tl_linear_rows_group", ptr(feat), ptr(head.W), ptr(head.b), ptr(ws.logits), self.M, B, kf, self.N, kf, 0,
                   s_feat, head.s_W, head.s_b, ws.s_logits)
        return ws

    def _ce(self, ws: _Workspace, y: Optional[torch.Tensor], B: int, grad: bool, pred: bool) -> None:
        base, ldd = self.stats.data_ptr(), ws.dlogits.shape[2]
        self._call("tl_ce_loss_group", ptr(ws.logits), ptr(y), ptr(ws.dlogits) if grad else None,
                   ptr(self.head.db) if grad else None, ptr(ws.pred) if pred else None, base, base + 8, base + 24, base + 16, self.M,
                   B, self.N, self.N, ldd, 1.0 / B, ws.s_logits, 0 if y is None else self._input_stride(y), ws.s_dlogits, self.head.s_b,
                   ws.s_pred, self.s_stats)

    def _scalars(self):
        """The step's (coef_grad, coef_mom, bias_corr2): ``FusedNAdam._scalars``, as the single path computes them (both groups
        share lr, betas and momentum_decay, so one set serves weights and biases)."""
        self.step_no += 1
        cg, cm, bc2, self.mu_product = self.optimizer._scalars(self.step_no, self.mu_product, self.optimizer.param_groups[0])
        return cg, cm, bc2

    def _update_lowrank(self, layer: _Layer, fa: torch.Tensor, s_fa: int, fb: torch.Tensor, s_fb: int, B: int, scalars) -> None:
        """``layer``'s weights by the rank-B gradient fa^T . fb, fa (M, B, ld >= rows), fb (M, B, cols), at their member
        strides."""
        gw = self.optimizer.param_groups[0]
        b1, b2 = gw["betas"]
        cg, cm, bc2 = scalars
        self._call("tl_nadam_lowrank_group", ptr(layer.W), ptr(layer.mW), ptr(layer.vW), ptr(fa), ptr(fb), self.M, B, layer.rows,
                   layer.cols, fa.shape[2], layer.cols, layer.s_W, s_fa, s_fb, cg, cm, b1, b2, bc2, gw["eps"],
                   gw["weight_decay"], 1.0)

    def _update_bias(self, layer: _Layer, scalars) -> None:
        gb = self.optimizer.param_groups[1]
        b1, b2 = gb["betas"]
        cg, cm, bc2 = scalars
        self._call("tl_nadam_group", ptr(layer.b), ptr(layer.db), ptr(layer.mb), ptr(layer.vb), self.M, layer.rows, layer.s_b,
                   layer.s_b, cg, cm, b1, b2, bc2, gb["eps"], gb["weight_decay"], 1.0)

    # ------------------------------------------------------------------ the public steps
    @torch.no_grad()
    def train_batch(self, x: torch.Tensor, y: torch.Tensor) -> None:
        """Forward, loss, backward and update of every active member for the stacked batch x (M, B, ...), y (M, B);
        everything stays on the stream (no host read)."""
        x = self._input(x)
        B = x.shape[1]
        y = self._labels(y, B)
        check_train_batch(self.shallow, B)
        if self.shallow and self.force_dense:
            raise ValueError(f"force_dense: the ShallowNNClassifier ensemble has no dense route (training batches of at most "
                             f"{FusedNAdam.LOWRANK_MAX} rows, always as rank-B updates)")
        dense = self.force_dense or B > FusedNAdam.LOWRANK_MAX          # the single engine's decision: B alone
        ws = self._forward(x)
        self._ce(ws, y, B, grad=True, pred=False)
        ldd, s_x = ws.dlogits.shape[2], self._input_stride(x)
        scalars = self._scalars()
        head = self.head
        if self.shallow:
            # dh (activation derivative applied) and the hidden bias gradient, off the output weight as it is BEFORE its update
            self._call("tl_head_bwd_act_group", ptr(ws.dlogits), ptr(ws.h), ptr(head.W), ptr(ws.dh), ptr(self.hidden.db), None,
                       self.M, B, self.H, self.N, ldd, self.act, self.slope, ws.s_dlogits, ws.s_h, head.s_W, ws.s_h,
                       self.hidden.s_b, 0)
            self._update_lowrank(self.hidden, ws.dh, ws.s_h, x, s_x, B, scalars)
            self._update_lowrank(head, ws.dlogits, ws.s_dlogits, ws.h, ws.s_h, B, scalars)
            self._update_bias(self.hidden, scalars)
        elif dense:
            gw = self.optimizer.param_groups[0]
            b1, b2 = gw["betas"]
            cg, cm, bc2 = scalars
            if self._dW is None:
                self._dW = torch.empty_like(head.W)
                self._s_dW = _member_stride(self._dW)
            dW = self._dW
            # the weight gradient alone: the arguments ``SimpleClassifierEngine._backward`` gives ``tl_head_bwd`` on this route
            self._call("tl_head_bwd_group", ptr(ws.dlogits), ptr(x), ptr(head.W), ptr(dW), self.M, B, self.K, self.N, ldd,
                       ws.s_dlogits, s_x, head.s_W, self._s_dW)
            self._call("tl_nadam_group", ptr(head.W), ptr(dW), ptr(head.mW), ptr(head.vW), self.M, self.N * self.K, head.s_W,
                       self._s_dW, cg, cm, b1, b2, bc2, gw["eps"], gw["weight_decay"], 1.0)
        else:
            self._update_lowrank(head, ws.dlogits, ws.s_dlogits, x, s_x, B, scalars)
        self._update_bias(head, scalars)

    @torch.no_grad()
    def eval_batch(self, x: torch.Tensor, y: torch.Tensor) -> None:
        """Forward and loss statistics of every active member for the stacked batch (no gradients, no update)."""
        x = self._input(x)
        ws = self._forward(x)
        self._ce(ws, self._labels(y, x.shape[1]), x.shape[1], grad=False, pred=False)

    @torch.no_grad()
    def predict_batch(self, x: torch.Tensor) -> torch.Tensor:
        """Arg-max class of every row, (M, B) int64 on the device (the rows of an inactive member are not written)."""
        x = self._input(x)
        ws = self._forward(x)
        self._ce(ws, None, x.shape[1], grad=False, pred=True)
        return ws.pred.clone()

    def logits(self, B: int) -> torch.Tensor:
        """The float32 logits (M, B, n_classes) of the last forward pass at batch ``B``."""
        return self._workspaces[B].logits

    def moments(self, m: int):
        """Member m's NAdam moments {parameter name: (exp_avg, exp_avg_sq)} (views of the stacks)."""
        out = {}
        for layer in self.layers:
            out.update(layer.moments(m))
        return out

    def epoch_stats(self) -> List[Tuple[float, int, torch.Tensor]]:
        """Per member (loss sum, samples counted, confusion matrix (N, N) int64 on the host) since the last call - ONE
        device-to-host read for the group - and zero them.  Raises ``ValueError`` if a label was outside [0, n_classes)."""
        host = self.stats.cpu()
        self.stats.zero_()
        for m in range(self.M):
            if int(host[m, 2]) != 0:
                raise ValueError(f"labels must lie in [0, {self.N}) for a model with {self.N} classes (member {m})")
        return [(float(host[m, 0:1].view(torch.float64)[0]), int(host[m, 1]), host[m, 3:].reshape(self.N, self.N).clone())
                for m in range(self.M)]
