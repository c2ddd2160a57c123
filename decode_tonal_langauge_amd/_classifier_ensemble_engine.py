"""All seeds of a classifier experiment in one pass: M ``LogisticRegressionClassifier``s of equal shape ("members") trained
side by side by the launches that train one (``_simple_classifier_engine``).

A step of the single engine is a handful of launches that occupy a few of the 256 CUs for a few microseconds each; the group
kernels (``tl_*_group``, include/tonal_hip.h) are the same kernels with a member dimension on the grid, so the step of M
members costs the same number of launches.  They are the SAME kernels - the single entry points launch them with M = 1 - and
every member therefore gets the bits ``SimpleClassifierEngine`` would give it on the same batches.

Storage is stacked: W (M, N, K), the biases (M, r4(N)) (a row of N floats is not 16-byte aligned, which the update kernels
want), moments, gradients, logits, dlogits, pred and the statistics words (M, 3 + N^2) likewise.  Each module's parameters
become views of the stacks, so ``state_dict()``, ``torch.save`` and inference through the module keep working.

``set_active(mask)``: the workgroups of a member whose mask word is 0 return before their first load - a member that stopped
early stays frozen, to the bit, while the others go on.  The NAdam schedule is one counter shared by the active members: they
advance in lockstep from step 0, and a member never resumes, so its step count freezes with its parameters.

Out of scope (refused with the supported set): every other model class, members of differing shape, a multi-rank process
group.  There is no CPU fallback."""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import torch

from . import _lib, parallel
from ._launch import r4
from ._lib import check, ptr
from .models.utils import split_decay_groups
from .optim import FusedNAdam

SUPPORTED = ("the classifier ensemble supports one or more LogisticRegressionClassifier of equal input_dim and n_classes with "
             "fp32 parameters on one CUDA device, input_dim % 4 == 0 and n_classes <= 64, in a single process (no multi-rank "
             "process group); ShallowNNClassifier and the deep classifiers train one model at a time (ClassifierTrainer)")


def refuse(why: str):
    raise ValueError(f"{why}: {SUPPORTED}")


def check_supported(models: Sequence) -> None:
    """Raise ``ValueError`` (stating the supported set) unless ``models`` can be trained by ``ClassifierEnsembleEngine``."""
    from .models.simple_classifiers import LogisticRegressionClassifier
    models = list(models)
    if not models:
        refuse("no models")
    for m in models:
        if not isinstance(m, LogisticRegressionClassifier):
            refuse(f"model {type(m).__name__}")
    first = models[0]
    for i, m in enumerate(models):
        if (int(m.input_dim), int(m.n_classes)) != (int(first.input_dim), int(first.n_classes)):
            refuse(f"member {i} has shape ({m.input_dim} -> {m.n_classes}), member 0 ({first.input_dim} -> {first.n_classes})")
    if first.input_dim % 4 != 0:
        refuse(f"input_dim {first.input_dim}")
    if first.n_classes > 64:
        refuse(f"n_classes {first.n_classes}")
    for m in models:
        if m.linear.bias is None:
            refuse("a layer without bias")
    if parallel.world()[1] > 1:
        refuse(f"a process group of {parallel.world()[1]} ranks")
    dev = None
    for m in models:
        for p in m.parameters():
            if not p.is_cuda or p.dtype != torch.float32:
                refuse(f"parameters on '{p.device}' in {p.dtype}")
            if dev is not None and p.device != dev:
                refuse(f"parameters on '{p.device}' and '{dev}'")
            dev = p.device


class _Workspace:
    """Buffers of one batch size (a loader has two: the full batch and the ragged last one)."""

    def __init__(self, M: int, B: int, N: int, dev):
        f32 = dict(dtype=torch.float32, device=dev)
        self.logits = torch.empty(M, B, N, **f32)
        self.dlogits = torch.zeros(M, B, r4(N), **f32)
        self.pred = torch.zeros(M, B, dtype=torch.int64, device=dev)


class ClassifierEnsembleEngine:
    def __init__(self, models: Sequence, learning_rate: float = 0.0005, weight_decay: float = 0.0):
        check_supported(models)
        self.models = list(models)
        self.lib = _lib.load()
        M = self.M = len(self.models)
        first = self.models[0]
        K, N = self.K, self.N = int(first.input_dim), int(first.n_classes)
        self.ldb = r4(N)
        dev = self.device = first.linear.weight.device
        f32 = dict(dtype=torch.float32, device=dev)
        # parameters move into the stacks; the modules keep views of them
        self.W = torch.empty(M, N, K, **f32)
        self.b = torch.zeros(M, self.ldb, **f32)
        with torch.no_grad():
            for m, model in enumerate(self.models):
                self.W[m].copy_(model.linear.weight.detach())
                self.b[m, :N].copy_(model.linear.bias.detach())
                model.linear.weight.data = self.W[m]
                model.linear.bias.data = self.b[m, :N]
        self.mW, self.vW = torch.zeros_like(self.W), torch.zeros_like(self.W)
        self.mb, self.vb = torch.zeros_like(self.b), torch.zeros_like(self.b)
        self.db = torch.zeros_like(self.b)
        self._dW: Optional[torch.Tensor] = None          # on demand (dense path only)
        # loss sum (the bits of a double), sample count, label-range flag, confusion matrix per member: one read per epoch
        self.words = 3 + N * N
        self.stats = torch.zeros(M, self.words, dtype=torch.int64, device=dev)
        # the schedule and the hyper-parameters are the single engine's: the two decay groups of ``_setup_training`` (the
        # weight decays, the bias does not), ``stored_beta2`` scalars; member 0's parameters stand for the group
        decay, no_decay = split_decay_groups(first.named_parameters())
        self.optimizer = FusedNAdam([{"params": decay, "weight_decay": float(weight_decay)},
                                     {"params": no_decay, "weight_decay": 0.0}], lr=float(learning_rate), stored_beta2=True)
        self.step_no, self.mu_product = 0, 1.0
        self.force_dense = False           # tests / the benchmark: materialise dW at a batch the low-rank update would take
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
            ws = self._workspaces[B] = _Workspace(self.M, B, self.N, self.device)
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

    def _forward(self, x: torch.Tensor) -> _Workspace:
        B = x.shape[1]
        ws = self._workspace(B)
        self._call("tl_linear_rows_group", ptr(x), ptr(self.W), ptr(self.b), ptr(ws.logits), self.M, B, self.K, self.N, self.K, 0,
                   B * self.K, self.N * self.K, self.ldb, B * self.N)
        return ws

    def _ce(self, ws: _Workspace, y: Optional[torch.Tensor], B: int, grad: bool, pred: bool) -> None:
        base, ldd = self.stats.data_ptr(), ws.dlogits.shape[2]
        self._call("tl_ce_loss_group", ptr(ws.logits), ptr(y), ptr(ws.dlogits) if grad else None, ptr(self.db) if grad else None,
                   ptr(ws.pred) if pred else None, base, base + 8, base + 24, base + 16, self.M, B, self.N, self.N, ldd, 1.0 / B,
                   B * self.N, B, B * ldd, self.ldb, B, self.words)

    def _scalars(self):
        """The step's (coef_grad, coef_mom, bias_corr2): ``FusedNAdam._scalars``, as the single path computes them (both groups
        share lr, betas and momentum_decay, so one set serves weight and bias)."""
        self.step_no += 1
        cg, cm, bc2, self.mu_product = self.optimizer._scalars(self.step_no, self.mu_product, self.optimizer.param_groups[0])
        return cg, cm, bc2

    # ------------------------------------------------------------------ the public steps
    @torch.no_grad()
    def train_batch(self, x: torch.Tensor, y: torch.Tensor) -> None:
        """Forward, loss, backward and update of every active member for the stacked batch x (M, B, ...), y (M, B);
        everything stays on the stream (no host read)."""
        x = self._input(x)
        B = x.shape[1]
        y = self._labels(y, B)
        dense = self.force_dense or B > FusedNAdam.LOWRANK_MAX          # the single engine's decision: B alone
        ws = self._forward(x)
        self._ce(ws, y, B, grad=True, pred=False)
        ldd = ws.dlogits.shape[2]
        gw, gb = self.optimizer.param_groups
        b1, b2 = gw["betas"]
        cg, cm, bc2 = self._scalars()
        NK = self.N * self.K
        if dense:
            if self._dW is None:
                self._dW = torch.empty_like(self.W)
            self._call("tl_head_bwd_group", ptr(ws.dlogits), ptr(x), ptr(self.W), ptr(self._dW), self.M, B, self.K, self.N, ldd,
                       B * ldd, B * self.K, NK, NK)
            self._call("tl_nadam_group", ptr(self.W), ptr(self._dW), ptr(self.mW), ptr(self.vW), self.M, NK, NK, NK, cg, cm, b1, b2,
                       bc2, gw["eps"], gw["weight_decay"], 1.0)
        else:
            self._call("tl_nadam_lowrank_group", ptr(self.W), ptr(self.mW), ptr(self.vW), ptr(ws.dlogits), ptr(x), self.M, B, self.N,
                       self.K, ldd, self.K, NK, B * ldd, B * self.K, cg, cm, b1, b2, bc2, gw["eps"], gw["weight_decay"], 1.0)
        b1, b2 = gb["betas"]
        self._call("tl_nadam_group", ptr(self.b), ptr(self.db), ptr(self.mb), ptr(self.vb), self.M, self.N, self.ldb, self.ldb, cg,
                   cm, b1, b2, bc2, gb["eps"], gb["weight_decay"], 1.0)
        for model in self.models:
            # the update wrote through data_ptr: an inference engine of the module keys its packed weights on ``_version``
            hip = getattr(model, "_hip", None)
            if hip is not None:
                hip._packed.clear()

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
        return {"linear.weight": (self.mW[m], self.vW[m]), "linear.bias": (self.mb[m, :self.N], self.vb[m, :self.N])}

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
