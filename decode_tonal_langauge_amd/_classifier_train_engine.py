"""What the three classifier train engines (``_simple_classifier_engine``, ``_cnn_classifier_train_engine``,
``_cnnrnn_classifier_train_engine``) share: ``ClassifierTrainEngine``, the base class that owns construction (optimiser, epoch
statistics, gradient buffers), input / label validation, the workspace cache, the loss launch, the public steps and the
data-parallel side of them (``_classifier_dp`` keeps the free-standing parts of that).

An engine supplies ``_make_workspace``, ``_forward``, ``_backward`` and, where it has one, ``_lowrank_wire``; it names its loss kernel (``CE``), the buffers of its workspace that kernel reads and writes (``CE_BUFFERS``) and its head bias
(``head_bias``), and says in ``_setup_training`` which Linear weights take the low-rank update.

Under a process group (``parallel.active()``) every public step takes the GLOBAL batch and works on this rank's rows; without
one the plan of a step is the whole batch (``ShardPlan(B, 0, B, 1.0)``), so the same launches run either way."""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch
import torch.distributed as dist
import torch.nn as nn

from . import _lib, parallel
from ._classifier_dp import RowGather, ShardPlan, reduce_stats_words, shard_plan
from ._launch import LaunchTimers
from ._lib import check, ptr
from .models.utils import split_decay_groups
from .optim import FusedNAdam

SUPPORTED = ("the fused classifier step supports LogisticRegressionClassifier and ShallowNNClassifier with fp32 parameters on "
             "a CUDA device, input_dim % 4 == 0, hidden_dim % 4 == 0, n_classes <= 64 and a ReLU or LeakyReLU activation; "
             "CNNClassifier (_cnn_classifier_train_engine) with fp32 parameters on a CUDA device, negative_slope >= 0, "
             "n_classes <= 64 and dropout < 1; CNNRNNClassifier (_cnnrnn_classifier_train_engine) under the same conditions with "
             "at least one row left behind its (3,1) pool")


def refuse(why: str):
    raise ValueError(f"{why}: {SUPPORTED}")


def parameter_unmet(p) -> Optional[str]:
    """The reason to refuse a parameter that is not fp32 on a CUDA device (None: it is)."""
    return None if p.is_cuda and p.dtype == torch.float32 else f"parameters on '{p.device}' in {p.dtype}"


def check_common(model, slopes=(), dropout: float = 0.0, also=()) -> None:
    """The conditions every engine sets, in the order the refusals are reported: ``negative_slope >= 0``, ``n_classes <= 64``,
    ``dropout < 1``, then the engine's own ``also`` [(refused, why)], last fp32 parameters on a CUDA device."""
    for slope in slopes:
        if slope < 0:
            refuse(f"negative_slope {slope}")
    if model.n_classes > 64:
        refuse(f"n_classes {model.n_classes}")
    if not dropout < 1.0:
        refuse(f"dropout {dropout}")
    for refused, why in also:
        if refused:
            refuse(why)
    for p in model.parameters():
        if parameter_unmet(p):
            refuse(parameter_unmet(p))


class ClassifierTrainEngine(LaunchTimers):
    CE = "tl_ce_scores_loss"               # the loss kernel: on sigmoid scores, or ``tl_ce_loss`` on logits
    CE_BUFFERS = ("scores", "dz")          # the workspace's input of that kernel and its gradient buffer (B, r4(N))
    INPUT_ERROR = "expected input (B, {}, {}), got {got}"
    UPDATE_TAG = None                      # timer tag around the optimiser step
    dp = False

    # ------------------------------------------------------------------ construction
    def _setup_training(self, model, learning_rate: float, weight_decay: float, lowrank_names=(), arena_order=()) -> None:
        """Optimiser, epoch statistics and gradient buffers.  ``lowrank_names``: the Linear weights that go as rank-B factors at
        B <= ``FusedNAdam.LOWRANK_MAX`` and get a dense buffer on demand; every other gradient is always dense.
        ``arena_order``: the order in which the backward finishes the dense ones."""
        self.model = model
        self.N = int(model.n_classes)
        self.params: Dict[str, nn.Parameter] = dict(model.named_parameters())
        self.device = next(iter(self.params.values())).device
        decay, no_decay = split_decay_groups(model.named_parameters())
        self.optimizer = FusedNAdam([{"params": decay, "weight_decay": float(weight_decay)},
                                     {"params": no_decay, "weight_decay": 0.0}], lr=float(learning_rate), stored_beta2=True)
        # loss sum (the bits of a double), sample count, label-range flag, confusion matrix: one buffer, one read per epoch
        self.stats = torch.zeros(3 + self.N * self.N, dtype=torch.int64, device=self.device)
        self.lowrank_names = tuple(lowrank_names)
        self.force_dense = False           # tests / the benchmark: materialise dW at a batch the low-rank update would take
        self.last_lowrank: Dict[str, Tuple[torch.Tensor, torch.Tensor]] = {}      # the factors of the last train step
        self.last_seed = 0                 # dropout seed of the last forward pass (0: no dropout applied)
        self._workspaces: Dict[tuple, object] = {}
        self.dp = parallel.active()
        self.rank, self.world = parallel.world()
        self._plan: Optional[ShardPlan] = None
        self._seed_fix = 0
        self._arena: Optional[parallel.FlatGrads] = None
        self._gathers: Dict[int, RowGather] = {}
        self.exchange_events: Optional[list] = None      # a list: (start, end) HIP event pairs around every exchange
        # dense gradient buffers (kept: the optimiser caches its pointer table)
        shapes = {k: p.shape for k, p in self.params.items() if k not in self.lowrank_names}
        if not self.dp:
            self.grads: Dict[str, torch.Tensor] = {k: torch.zeros_like(self.params[k]) for k in shapes}
            return
        parallel.broadcast_parameters_(model)
        if self.world > 1:
            # the dropout seed of a step is rank 0's: its torch seed and its count of draws so far, broadcast once
            box = [(int(torch.initial_seed()), int(getattr(model, "_drop_calls", 0)))]
            dist.broadcast_object_list(box, src=0)
            seed0, calls0 = box[0]
            self._seed_fix = ((seed0 - int(torch.initial_seed())) * 0x9E3779B1) & 0xFFFFFFFFFFFFFFFF
            if hasattr(model, "_drop_calls"):
                model._drop_calls = calls0
        self._void = torch.zeros_like(self.stats)        # where a weight-0 rank's duplicated row is counted
        # ... as views of one flat arena (16-byte aligned: the optimiser's pointer table takes them): one all-reduce
        self._arena = parallel.FlatGrads(shapes, list(arena_order), self.device)
        self.grads = dict(self._arena.views)

    # ------------------------------------------------------------------ plumbing
    def _stream(self) -> int:
        return torch.cuda.current_stream().cuda_stream

    def _call(self, tag: Optional[str], name: str, *args) -> None:
        ev = self._tick(tag)
        check(getattr(self.lib, name)(*args, self._stream()), name)
        if ev:
            ev[1].record()

    def _input(self, x: torch.Tensor) -> torch.Tensor:
        _lib.require_gpu(x, type(self).__name__)
        if tuple(x.shape[1:]) != self.input_shape:
            raise ValueError(self.INPUT_ERROR.format(*self.input_shape, got=tuple(x.shape)))
        if x.shape[0] < 1:
            raise ValueError("empty batch")
        return x.float().contiguous()

    def _labels(self, y: torch.Tensor, B: int) -> torch.Tensor:
        _lib.require_gpu(y, type(self).__name__)
        if y.shape != (B,):
            raise ValueError(f"expected {B} labels, got {tuple(y.shape)}")
        return y.long().contiguous()

    def _workspace(self, B: int, device=None):
        """The engine's buffers of one batch size (a loader has two: the full batch and the ragged last one)."""
        key = (B, self.device if device is None else device)
        ws = self._workspaces.get(key)
        if ws is None:
            if len(self._workspaces) > 4:
                self._workspaces.clear()
            ws = self._workspaces[key] = self._make_workspace(*key)
        return ws

    def _dense(self, name: str) -> torch.Tensor:
        g = self.grads.get(name)
        if g is None:
            g = self.grads[name] = torch.empty_like(self.params[name])
        return g

    def _ce(self, ws, y: Optional[torch.Tensor], B: int, grad: bool, pred: bool) -> None:
        scores, dz = (getattr(ws, name) for name in self.CE_BUFFERS)
        base = (self.stats if self._plan.live else self._void).data_ptr()
        self._call(None, self.CE, ptr(scores), ptr(y), ptr(dz) if grad else None,
                   ptr(self.grads[self.head_bias]) if grad else None, ptr(ws.pred) if pred else None, base, base + 8, base + 24,
                   base + 16, B, self.N, self.N, dz.shape[1], 1.0 / self._plan.B if self._plan.live else 0.0)

    # ------------------------------------------------------------------ the engine's hook
    def _lowrank_wire(self, ws) -> Dict[str, torch.Tensor]:
        """{name: buffer}: a low-rank weight whose first factor is the leading columns of a wider stored buffer, which is what
        travels between the ranks."""
        return {}

    # ------------------------------------------------------------------ data parallel, per step
    def _take(self, x: torch.Tensor, y: Optional[torch.Tensor] = None):
        """This rank's rows of the global batch (the whole batch without a process group) and the plan of the step."""
        B = x.shape[0]
        if not self.dp:
            self._plan = ShardPlan(B, 0, B, 1.0)
            return x, y
        plan = self._plan = shard_plan(B, self.rank, self.world)
        x = x[plan.slice]
        if x.data_ptr() % 16:
            x = x.clone()
        return x, (None if y is None else y[plan.slice])

    def _step_seed(self) -> int:
        return (int(self.model._next_seed()) + self._seed_fix) & 0xFFFFFFFFFFFFFFFF

    def _gather(self, t: torch.Tensor) -> torch.Tensor:
        plan = self._plan
        g = self._gathers.get(plan.B)
        if g is None:
            if len(self._gathers) > 4:
                self._gathers.clear()
            g = self._gathers[plan.B] = RowGather(plan.B, self.world, self.device)
        return g(t, plan.rows_sent)

    def _exchange(self, extra=(), lowrank: Optional[Dict[str, Tuple[torch.Tensor, torch.Tensor]]] = None):
        """Sum the arena (and ``extra``: dense buffers allocated on demand) over the ranks - one bucketed all-reduce - and
        gather the low-rank factor rows in global row order.  Returns the gathered ``lowrank``."""
        ev = None
        if self.exchange_events is not None:
            ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            ev[0].record()
        parallel.allreduce_bucketed([self._arena.flat] + list(extra))
        out = {k: (self._gather(fa), self._gather(fb)) for k, (fa, fb) in (lowrank or {}).items()}
        if ev is not None:
            ev[1].record()
            self.exchange_events.append(ev)
        return out

    # ------------------------------------------------------------------ the public steps
    def _step(self, x: torch.Tensor, y: torch.Tensor, update: bool) -> None:
        x = self._input(x)
        x, y = self._take(x, self._labels(y, x.shape[0]))
        # dense or low-rank from the GLOBAL batch: the same on every rank
        dense = not self.lowrank_names or self.force_dense or self._plan.B > FusedNAdam.LOWRANK_MAX
        B = x.shape[0]
        ws = self._forward(x, dropout=self.model.training)
        self._ce(ws, y, B, grad=True, pred=False)
        self._backward(ws, B, dense)
        if self.dp:
            low = self.last_lowrank
            wire = self._lowrank_wire(ws)
            got = self._exchange(extra=[self.grads[k] for k in self.lowrank_names] if dense else (),
                                 lowrank={k: (wire.get(k, fa), fb) for k, (fa, fb) in low.items()})
            self.last_lowrank = {k: (fa[:, :low[k][0].shape[1]], fb) for k, (fa, fb) in got.items()}
        if update:
            ev = self._tick(self.UPDATE_TAG)
            grads = {self.params[k]: g for k, g in self.grads.items() if dense or k not in self.lowrank_names}
            self.optimizer.step(grads=grads, lowrank={self.params[k]: f for k, f in self.last_lowrank.items()} or None)
            if ev:
                ev[1].record()

    @torch.no_grad()
    def train_batch(self, x: torch.Tensor, y: torch.Tensor) -> None:
        """Forward, loss, backward and update for one batch; everything stays on the stream (no host read)."""
        self._step(x, y, update=True)

    @torch.no_grad()
    def backward_only(self, x: torch.Tensor, y: torch.Tensor) -> Dict[str, object]:
        """Debug hook: forward, loss and backward of one batch WITHOUT the update.  {parameter name: gradient}, a Linear weight
        on the low-rank path as its factors ``(fa (B, rows), fb (B, cols))`` with gradient ``fa^T . fb``.  The tensors are the
        engine's buffers: valid until the next step.  The batch is counted in the epoch statistics like any other."""
        self._step(x, y, update=False)
        return self.step_gradients()

    def step_gradients(self) -> Dict[str, object]:
        """The gradients of the last ``train_batch`` / ``backward_only`` (see there)."""
        out: Dict[str, object] = {k: g for k, g in self.grads.items() if k not in self.last_lowrank}
        out.update(self.last_lowrank)
        return out

    @torch.no_grad()
    def eval_batch(self, x: torch.Tensor, y: torch.Tensor) -> None:
        """Forward (no dropout) and loss statistics of one batch (no gradients, no update)."""
        x = self._input(x)
        x, y = self._take(x, self._labels(y, x.shape[0]))
        ws = self._forward(x, dropout=False)
        self._ce(ws, y, x.shape[0], grad=False, pred=False)

    @torch.no_grad()
    def predict_batch(self, x: torch.Tensor) -> torch.Tensor:
        """Arg-max class of every row (int64, on the device)."""
        x, _ = self._take(self._input(x))
        ws = self._forward(x, dropout=False)
        self._ce(ws, None, x.shape[0], grad=False, pred=True)
        return self._gather(ws.pred.view(-1, 1)).view(-1) if self.dp else ws.pred.clone()

    def scores(self, B: int) -> torch.Tensor:
        """The float32 scores (B, n_classes) of the last forward pass at batch ``B``."""
        return getattr(self._workspaces[B, self.device], self.CE_BUFFERS[0])

    def epoch_stats(self):
        """(loss sum, samples counted, confusion matrix (N, N) int64 on the host) since the last call - ONE device-to-host
        read - and zero them.  Under a process group the words of all ranks are summed first (one small collective), so every
        rank returns the same values.  Raises ``ValueError`` if a label was outside [0, n_classes)."""
        if self.dp:
            host = reduce_stats_words(self.stats)
            self._void.zero_()
        else:
            host = self.stats.cpu()
        self.stats.zero_()
        if int(host[2]) != 0:
            raise ValueError(f"labels must lie in [0, {self.N}) for a model with {self.N} classes")
        return float(host[0:1].view(torch.float64)[0]), int(host[1]), host[3:].reshape(self.N, self.N).clone()
