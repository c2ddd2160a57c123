"""All repeats of a SynthesisLite experiment in one pass: M ``SynthesisLite`` models of equal shape ("members") trained side by
side by the launches that train one.

The Lite step is ~55 launches of 4-20 us that occupy a few of the 256 CUs each: it is bound by launches, not by the GPU.  The
group kernels (``tl_lite_*_group`` and their neighbours, include/tonal_hip.h) are the same kernels with a member dimension on
the grid - the single entries launch them with M = 1 - so a step of M members is the same number of launches.  The plan of the
step exists once, in ``_lite_engine.LiteEngine``, written for M members: ``LiteEnsembleEngine`` is that class with M > 1 allowed,
the members' storage, and the member forms of the two GEMM launches.  Every split-K factor, every ``bm`` and every
direct-vs-slab choice is therefore the single engine's, taken from one member's sizes, and every member gets the bits
``LiteEngine`` gives it on the same inputs.

Storage is stacked: every parameter, BatchNorm buffer, gradient and (in the optimiser) NAdam moment is (M, ...), and each
member's module holds views of the stacks, so ``state_dict()``, ``torch.save``, ``model(x, labels)`` and
``SynthesisTrainer.evaluate`` on a member keep working through the single path.

Where ``tl_permute_reduce`` is used the member rides a free dimension of its 4-d view.  The kernel it picks depends on the last
dimension, on the number of slabs nz and - its wave-parallel form, nz >= 64 and at most 16384 outputs - on the number of outputs,
which grows with M: the pad, the transposes and the split-K sums have nz <= 16 and so take the single launch's kernel for any
M; the ``_colsum`` fallback (up to 256 slabs) cuts the members into launches that stay inside the bound, so only there can the
launch count depend on M (M > 32 with out_dim >= 512).  fc.3's split-K reduction adds a per-member bias row and therefore runs
on ``tl_splitk_bias_lrelu_group`` with slope 1 (the identity: the same sum in the same order) - the one launch that is another
kernel than the single engine's.

Out of scope (refused with the supported set): other model classes, members of unequal constructor arguments, parameters that
are not fp32 on one CUDA device, a multi-rank process group, and what takes one of the three weight-gradient GEMMs off the
short-reduction kernel, the only TN kernel with a member dimension: training batches with B > 512 or B L - 1 > 512, and
models with 512 * r4(conv_channels * (n_timepoints // 4) + lstm_hidden) > 2^20 or r4(output_dim) * 512 > 2^20 (the fc.1 / fc.3
weight gradient; the default model from 252 time points on).  No CPU fallback."""
from __future__ import annotations

from typing import Dict, Sequence

import torch

from . import parallel
from ._launch import launch_nt_group_fc, launch_tn_group
from ._lib import check, ptr
from ._lite_engine import MAX_OUT, MAX_ROWS, LiteEngine

SUPPORTED = ("the synthesis ensemble supports one or more SynthesisLite models of equal constructor arguments (output_dim, "
             "n_channels, n_timepoints, label_dim, conv_channels, lstm_hidden, dropout, negative_slope) with fp32 parameters on "
             "one CUDA device, in a single process (no multi-rank process group), fc.1 of at most 2048 padded inputs "
             "(r4(conv_channels * (n_timepoints // 4) + lstm_hidden) <= 2048) and output_dim <= 2048 (the weight gradients of "
             "wider layers run on GEMM kernels without a member dimension), and training batches of B <= 512 rows with "
             "B * L - 1 <= 512 (L = length of the label sequence)")


def refuse(why: str):
    raise ValueError(f"{why}: {SUPPORTED}")


def _signature(m) -> tuple:
    e = m._engine
    return (e.out_dim, e.C, e.T, e.in_dim, e.CC, e.H, e.p_drop, e.slope)


def check_supported(models: Sequence) -> None:
    """Raise ``ValueError`` (stating the supported set) unless ``models`` can be trained by ``LiteEnsembleEngine``."""
    from .models.synthesis_models import SynthesisLite
    models = list(models)
    if not models:
        refuse("no models")
    for m in models:
        if not isinstance(m, SynthesisLite):
            refuse(f"model {type(m).__name__}")
    first = _signature(models[0])
    for i, m in enumerate(models):
        if _signature(m) != first:
            refuse(f"member {i} was built with {_signature(m)}, member 0 with {first}")
    e = models[0]._engine
    if e.hid * e.ldf > MAX_OUT:
        refuse(f"fc.1 with {e.ldf} padded inputs (conv_channels {e.CC} * (n_timepoints {e.T} // 4) + lstm_hidden {e.H})")
    if e.ldd * e.hid > MAX_OUT:
        refuse(f"output_dim {e.out_dim}")
    if parallel.world()[1] > 1:
        refuse(f"a process group of {parallel.world()[1]} ranks")
    dev = None
    for m in models:
        for name, t in list(m.named_parameters()) + list(m.named_buffers()):
            if t.is_floating_point() and t.dtype != torch.float32:
                refuse(f"'{name}' of dtype {t.dtype}")
            if t.device.type != "cuda":
                refuse(f"'{name}' on '{t.device}'")
            if dev is not None and t.device != dev:
                refuse(f"parameters on '{t.device}' and '{dev}'")
            dev = t.device


def check_train_batch(B: int, L: int) -> None:
    """Raise ``ValueError`` for a training batch the group cannot take: B <= 512 and B L - 1 <= 512."""
    if B > MAX_ROWS or B * L - 1 > MAX_ROWS:
        refuse(f"a training batch of B = {B} rows with label length L = {L} (B * L - 1 = {B * L - 1})")


class LiteEnsembleEngine(LiteEngine):
    NAME = "SynthesisLite ensemble"

    def __init__(self, models: Sequence):
        check_supported(models)
        self.models = list(models)
        M = len(self.models)
        first = self.models[0]
        super().__init__(*_signature(first), M=M)
        self.device = next(first.parameters()).device
        self.names = list(first._pnames)
        # parameters and buffers move into the stacks; the modules keep views of them
        self.params: Dict[str, torch.Tensor] = {}
        self.buffers: Dict[str, torch.Tensor] = {}
        with torch.no_grad():
            for name in self.names:
                ps = [dict(m.named_parameters())[name] for m in self.models]
                stack = torch.stack([p.detach() for p in ps]).contiguous()
                for m, p in enumerate(ps):
                    p.data = stack[m]
                self.params[name] = stack
            for name, _ in first.named_buffers():
                bs = [dict(m.named_buffers())[name] for m in self.models]
                stack = torch.stack([b.detach() for b in bs]).contiguous()
                for m, b in enumerate(bs):
                    b.data = stack[m]
                self.buffers[name] = stack
        self.grads = {k: torch.zeros_like(v) for k, v in self.params.items()}
        # the plan's member strides are products of sizes: every stack is dense (checked here, once, not per launch)
        for k, v in [*self.params.items(), *self.buffers.items(), *self.grads.items()]:
            if not v.is_contiguous():
                raise RuntimeError(f"the stack of '{k}' is not dense")
        # the dropout seed table, one word per member
        self.seeds = self.seed_dev = torch.zeros(M, dtype=torch.int64, device=self.device)

    # ------------------------------------------------------------------ the member forms of the plan's launches
    def _nt(self, s_A, s_Bw, s_bias, s_aux, s_out, **fields) -> None:
        launch_nt_group_fc(self.lib, self.M, s_A, s_Bw, s_bias, s_aux, s_out, self.active, stream=self._tail[1], **fields)

    def _tn(self, s_A, s_B, s_slab, s_colsum, **fields) -> None:
        launch_tn_group(self.lib, self.M, s_A, s_B, s_slab, s_colsum, self.active, stream=self._tail[1], **fields)

    def _fc3_sum(self, slab3, bias, out, sk3, B) -> None:
        # sum of the slabs + the member's bias row: the reduction of the single step (tl_permute_reduce with a bias) as
        # tl_splitk_bias_lrelu with slope 1 - the same additions in the same order, and v * 1 = v
        D = self.out_dim
        check(self.lib.tl_splitk_bias_lrelu_group(ptr(slab3), ptr(bias), ptr(out), sk3, B * D, D, 1.0, self.M, B * D, sk3 * B * D,
                                                  D, B * D, *self._tail), "tl_splitk_bias_lrelu_group")

    # ------------------------------------------------------------------ stacked tensors in, the engine's own stacks
    def forward(self, x: torch.Tensor, labels: torch.Tensor, training: bool, save: bool = True) -> torch.Tensor:
        """x (M, B, C, T), labels (M, B, label_dim, L) -> (M, B, out_dim).  The dropout seeds are read from ``self.seeds``."""
        M = self.M
        if x.dim() != 4 or x.shape[0] != M or x.shape[2] != self.C or x.shape[3] != self.T:
            raise ValueError(f"expected ECoG input ({M}, B, {self.C}, {self.T}), got {tuple(x.shape)}")
        B = x.shape[1]
        if labels.dim() != 4 or tuple(labels.shape[:3]) != (M, B, self.in_dim):
            raise ValueError(f"expected labels ({M}, B, {self.in_dim}, L), got {tuple(labels.shape)}")
        if training:
            check_train_batch(B, labels.shape[3])
        return self._forward({**self.params, **self.buffers}, x, labels, B, training, save)

    def backward(self, dout: torch.Tensor) -> None:
        """dout (M, B, ldd) -> ``self.grads`` (every entry (M, ...))."""
        self._backward({**self.params, **self.buffers}, dout, self.grads)
