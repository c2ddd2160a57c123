"""HIP-graph capture and replay of a launch-bound train step, for ``SynthesisTrainer`` and ``SynthesisEnsembleTrainer``.

The step of a small model (SynthesisLite: ~58 launches of 4-20 us) is bound by launch overhead, not by the GPU: after three
eager steps at a batch shape it is captured once into a HIP graph and replayed.  What changes from step to step lives in device
memory - the NAdam coefficients (``tl_nadam_multi_dev``) and the dropout seed (``tl_lite_cat_group`` / ``tl_lite_uncat_group``) -
and is refreshed, together with the batch in the graph's static input buffers, by one small launch before each replay.

A trainer keeps what is its own: whether a step may be captured at all, the captured step and its engine's fingerprint row."""
from __future__ import annotations

import ctypes as C
import warnings
from typing import Callable, Dict, Iterable, Optional, Sequence

import torch

from . import _kernels
from ._lib import check, ptr

WARM_UP = 3          # eager steps at a batch shape before it is captured
MAX_SHAPES = 2       # captured shapes held at a time


def frozen_rows(optimizer, grad_of: Callable, classifiers: Iterable) -> list:
    """What every captured step has frozen into its kernel arguments besides the batch: the optimiser's hyper-parameters (launch
    scalars), the storage of every parameter, of its gradient (``grad_of(p)``, a tensor or None) and of its NAdam moments, and
    the classifiers' weights (their packed copies are rebuilt when a weight's version changes - and ``FusedNAdam`` moves
    ``_version`` like torch's own in-place writes, so a classifier trained on the fused path between two steps is seen here).
    A replay is only valid while these rows, and the row the trainer appends for its engine, are what they were at capture:
    ``optimizer.load_state_dict`` (new moment tensors), an edited ``param_groups`` entry, a re-loaded classifier or a re-assigned
    ``.data`` would otherwise leave the graph reading freed or stale buffers."""
    fp = []
    for group in optimizer.param_groups:
        fp.append((tuple(group["betas"]), group["eps"], group["weight_decay"], group["momentum_decay"]))
        for p in group["params"]:
            st = optimizer.state.get(p) or {}
            g = grad_of(p)
            fp.append((p.data_ptr(), None if g is None else g.data_ptr(),
                       None if "exp_avg" not in st else st["exp_avg"].data_ptr(),
                       None if "exp_avg_sq" not in st else st["exp_avg_sq"].data_ptr()))
    for clf in classifiers:
        fp.append(tuple((q.data_ptr(), q._version) for q in clf.parameters()) + (clf.training,))
    return fp


class StepGraphs:
    """The per-shape graphs of one trainer.  ``states`` maps a batch shape to ``{"warm", "graph", "in", "params", "keep",
    "fingerprint"}``; ``scalars`` (4 x f32: what ``FusedNAdam.step_graph`` reads) and ``seed`` (1 x int64: the dropout seed word
    of a single model) are allocated with the first capture."""

    def __init__(self, owner: str, lib, optimizer, device) -> None:
        self.owner, self.lib, self.optimizer, self.device = owner, lib, optimizer, device
        self.enabled = _kernels.get("graph") != "0"
        self.states: Dict[tuple, dict] = {}
        self.scalars = self.seed = None

    def _capture(self, st: dict, batch, params, fingerprint, capture) -> bool:
        st["in"] = tuple(torch.empty_like(t) for t in batch)
        if self.scalars is None:
            self.scalars = torch.zeros(4, dtype=torch.float32, device=self.device)
            self.seed = torch.zeros(1, dtype=torch.int64, device=self.device)
        for d, t in zip(st["in"], batch):
            d.copy_(t)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        try:
            capture(torch.cuda.graph(g), st["in"])
        except Exception as e:      # noqa: BLE001 - capture refused (e.g. an op that synchronises): stay eager for good
            warnings.warn(f"{self.owner}: HIP-graph capture of the train step failed ({e!r}); continuing eagerly")
            self.enabled = False
            return False            # nothing was executed during the failed capture: the caller runs this step eagerly
        # the graph holds raw pointers into the optimiser's entry tables: keep those tensors alive with it (the optimiser's own
        # cache is cleared when it grows), and remember what the capture froze
        st.update(graph=g, params=set(params), keep=list(self.optimizer._tables.values()), fingerprint=fingerprint())
        return True

    def step(self, batch: Sequence[torch.Tensor], params: Iterable, fingerprint: Callable[[], tuple],
             capture: Callable, seed: Optional[Callable[[], int]] = None) -> bool:
        """One train step on ``batch`` (at most four tensors) through the graph of its shape.  False: the caller runs the step
        eagerly (warm-up, a third shape, a failed capture, graphs switched off).  ``params``: what ``advance_scalars`` advances,
        read at capture; ``fingerprint()``: the tuple a replay stays valid for; ``capture(recording, static_inputs)`` enqueues
        the step on the static inputs inside ``with recording:`` (``FusedNAdam.step_graph`` on ``self.scalars``); ``seed()``:
        the dropout seed word, called once per step the graph runs (the capture step included), never for an eager one."""
        if not self.enabled:
            return False
        key = tuple(tuple(t.shape) for t in batch) + tuple(t.dtype for t in batch)
        st = self.states.get(key)
        if st is None:
            st = self.states[key] = {"warm": 0, "graph": None}
        if st["graph"] is not None and st["fingerprint"] != fingerprint():
            # something the capture had frozen was replaced: drop the graph (and the NAdam entry table it pinned), warm up
            # eagerly again and recapture - never replay onto freed or stale buffers
            st.update(graph=None, warm=0, params=None, keep=None, fingerprint=None)
        staged = ()
        if st["graph"] is None:
            if st["warm"] < WARM_UP or sum(v["graph"] is not None for v in self.states.values()) >= MAX_SHAPES:
                st["warm"] += 1
                return False
            if not self._capture(st, batch, params, fingerprint, capture):
                return False
        else:
            staged = tuple(zip(st["in"], batch))
        cg, cm, bc2 = self.optimizer.advance_scalars(st["params"])
        word = 0 if seed is None else seed()
        stream = torch.cuda.current_stream().cuda_stream
        # the values travel as launch arguments (a pinned host buffer would be overwritten by the next step before an
        # asynchronous copy of this one has read it: the host runs ahead of the stream); the batch goes into the graph's
        # static input buffers by the same launch
        if all(t.is_cuda and t.is_contiguous() and t.dtype == d.dtype and t.shape == d.shape for d, t in staged):
            src = (C.c_void_p * 4)(*[t.data_ptr() for _, t in staged])
            dst = (C.c_void_p * 4)(*[d.data_ptr() for d, _ in staged])
            nby = (C.c_int64 * 4)(*[t.numel() * t.element_size() for _, t in staged])
            check(self.lib.tl_stage_step(ptr(self.scalars), ptr(self.seed), cg, cm, bc2, word, src, dst, nby, len(staged),
                                         stream), "tl_stage_step")
        else:
            for d, t in staged:
                d.copy_(t, non_blocking=True)
            check(self.lib.tl_set_step_scalars(ptr(self.scalars), ptr(self.seed), cg, cm, bc2, word, stream),
                  "tl_set_step_scalars")
        st["graph"].replay()
        return True
