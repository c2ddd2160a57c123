"""The data-parallel side of the three classifier train engines (``_classifier_train_engine.ClassifierTrainEngine`` and its
subclasses): one process per GPU, every rank is handed the GLOBAL batch and works on its rows.  The free-standing parts live
here, the per-step side (``_take`` / ``_exchange`` / ``epoch_stats``) in the base class.

  shard      ``parallel.shard_plan``, as ``SynthesisTrainer._shard`` - contiguous ``parallel.shard_rows``; a ragged batch gives unequal shards, each weighted by its share of the rows; a batch with fewer rows than ranks leaves some ranks
             recomputing row ``rank % B`` with weight 0 so that every rank still takes part in every collective;
  loss       ``grad_scale`` of the CE kernel is 1 / B_global on a live rank (so the SUM over ranks is the global mean's gradient:
             no 1 / N anywhere else) and 0 on a weight-0 rank, whose statistics go to a scratch buffer that nobody reads;
  exchange   the dense gradients live in one ``parallel.FlatGrads`` arena and are summed by ``parallel.allreduce_bucketed``;
             a Linear weight on the low-rank path travels as its factor ROWS - ``gather_rows`` puts the ranks' rows in global row
             order, and every rank runs the same ``tl_nadam_lowrank`` on the same B_global rows;
  statistics ``reduce_stats_words``: one small collective per epoch over the process group on the raw int64 words.

No collective here runs without an active process group (``parallel.active()``); a single-process step is the plan
``ShardPlan(B, 0, B, 1.0)`` on the same launches."""
from __future__ import annotations

from typing import List

import torch
import torch.distributed as dist

from . import parallel
from .parallel import ShardPlan, shard_plan          # noqa: F401 - the shard rule lives beside shard_rows


def _group_device(like: torch.Tensor) -> torch.device:
    """Where a tensor must lie for the process group to move it: the host under gloo, the GPU under RCCL."""
    return torch.device("cpu") if dist.get_backend() == "gloo" else like.device


def reduce_stats_words(words: torch.Tensor) -> torch.Tensor:
    """The epoch statistics of all ranks from one rank's int64 words [loss sum (the bits of a double), count, label flag,
    confusion matrix...]: ONE all-gather of the raw words over the process group, then the loss is summed as fp64 in rank
    order and the rest as int64 - exact, and the same bits on every rank.  ``words`` on any device; the result is on the host."""
    n = dist.get_world_size()
    src = words.detach().to(_group_device(words)).contiguous()
    out = torch.empty(n * src.numel(), dtype=torch.int64, device=src.device)
    dist.all_gather_into_tensor(out, src)
    allw = out.view(n, -1).cpu()
    total = allw.sum(0)
    loss = torch.zeros((), dtype=torch.float64)
    for r in range(n):
        loss = loss + allw[r, 0:1].view(torch.float64)[0]
    total[0:1] = loss.reshape(1).view(torch.int64)
    return total


class RowGather:
    """All-gather of per-row tensors of one global batch size in global row order.  Every rank sends ``kmax`` rows (its own, zero
    padded); the rows that belong to the batch are picked out of the (world * kmax) gathered ones by one index."""

    def __init__(self, B: int, world: int, device):
        plans = [shard_plan(B, r, world) for r in range(world)]
        self.kmax = max(p.rows for p in plans)
        self.world = world
        pick: List[int] = []
        for r, p in enumerate(plans):
            pick += [r * self.kmax + i for i in range(p.rows_sent)]
        assert len(pick) == B
        self.identity = pick == list(range(B)) and world * self.kmax == B
        self.pick = torch.tensor(pick, dtype=torch.int64, device=device)

    def __call__(self, t: torch.Tensor, rows_sent: int) -> torch.Tensor:
        """(B_global, cols) from this rank's (rows, cols) ``t``, of which the first ``rows_sent`` count."""
        cols = t.shape[1]
        if t.shape[0] == self.kmax and rows_sent == self.kmax and t.is_contiguous():
            mine = t
        else:
            mine = torch.zeros(self.kmax, cols, dtype=t.dtype, device=t.device)
            mine[:rows_sent] = t[:rows_sent]
        out = torch.empty(self.world * self.kmax, cols, dtype=t.dtype, device=t.device)
        if t.dtype == torch.float32:
            parallel._all_gather_rows(out, mine)
        else:                                    # (int64 predictions: the process group, never the fp32 C-ABI handle)
            dev = _group_device(t)
            ho = torch.empty(out.shape, dtype=t.dtype, device=dev)
            dist.all_gather_into_tensor(ho, mine.to(dev))
            out.copy_(ho)
        return out if self.identity else out.index_select(0, self.pick)
