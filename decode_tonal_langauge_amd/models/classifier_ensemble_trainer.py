"""``ClassifierTrainer(fused=True)``'s loop for M ``LogisticRegressionClassifier``s or M ``ShallowNNClassifier``s at once (the
seeds of one experiment): every step of the group is the launches of one model's step (``_classifier_ensemble_engine``), every
batch of the group one gather launch (``tl_gather_rows_group``) over the ONE ``ResidentDataset`` the members' splits index.
Shallow members train batches of at most ``FusedNAdam.LOWRANK_MAX`` (64) rows: ``fit`` refuses larger training loaders before
the first epoch; validation, test and predict loaders may have any batch size.

Member m's result is what a sequential ``ClassifierTrainer(fused=True)`` run of that member over its ``ResidentLoader``s gives:
the same kernels on the same batches, early stopping per member (own ``best``, own ``wait``; a member that stops is masked out
and stays frozen while the group runs on), the same ``metrics.csv`` / ``confusion_matrix_test.csv`` per member.

Random streams.  A sequential run draws from torch's global CPU generator: one ``DataLoader`` base seed plus the
``RandomSampler`` seed per training epoch, one base seed per validation, test and predict pass.  Here every member keeps its
own generator state (``MemberStreams``); it is installed around that member's draws - which ``ResidentLoader.iter_indices()``
performs on the host exactly as the loader does - and captured again after.  ``rng_states[m]`` is the state at which member
m's ``fit`` would have been entered (default: a copy of the current state for each member).  On return from every public
method the global generator holds the LAST member's state, as a sequential loop over the members would leave it.

The order drawing (``MemberStreams``, ``draw_orders``, ``check_loaders``) is host only and needs no GPU."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import torch

from ..data_loading.resident import ResidentLoader
from .classifier_trainer import EarlyStopping, epoch_line, epoch_row, macro_scores, write_confusion, write_metrics

LOADERS = ("the classifier ensemble takes one ResidentLoader per member, all over the SAME ResidentDataset object, with equal "
           "subset sizes and equal batch size")


class MemberStreams:
    """One state of torch's global CPU generator per member."""

    def __init__(self, n_members: int, states: Optional[Sequence[torch.Tensor]] = None) -> None:
        if states is None:
            now = torch.get_rng_state()
            states = [now.clone() for _ in range(n_members)]
        if len(states) != n_members:
            raise ValueError(f"expected {n_members} generator states, got {len(states)}")
        self.states: List[torch.Tensor] = [s.clone() for s in states]

    def run(self, m: int, fn):
        """``fn()`` with member m's state installed; the state it leaves is the member's new one."""
        torch.set_rng_state(self.states[m])
        out = fn()
        self.states[m] = torch.get_rng_state()
        return out

    def leave(self) -> None:
        """What a sequential loop over the members leaves in the global generator: the last member's state."""
        torch.set_rng_state(self.states[-1])


def check_loaders(loaders: Sequence, n_members: int) -> None:
    """Raise ``ValueError`` (stating what is supported) unless ``loaders`` can feed one group."""
    loaders = list(loaders)
    if len(loaders) != n_members:
        raise ValueError(f"{len(loaders)} loaders for {n_members} members: {LOADERS}")
    for m, lo in enumerate(loaders):
        if not isinstance(lo, ResidentLoader):
            raise ValueError(f"loader {m} is a {type(lo).__name__}: {LOADERS}")
    first = loaders[0]
    for m, lo in enumerate(loaders):
        if lo.dataset is not first.dataset:
            raise ValueError(f"loader {m} reads another dataset than loader 0: {LOADERS}")
        if len(lo.sampler.indices) != len(first.sampler.indices):
            raise ValueError(f"loader {m} has {len(lo.sampler.indices)} samples, loader 0 {len(first.sampler.indices)}: {LOADERS}")
        if lo.batch_size != first.batch_size:
            raise ValueError(f"loader {m} has batch size {lo.batch_size}, loader 0 {first.batch_size}: {LOADERS}")
    if len(first.sampler.indices) == 0:
        raise ValueError(f"empty subset: {LOADERS}")


def draw_orders(loaders: Sequence[ResidentLoader], streams: MemberStreams, members: Sequence[int]) -> Dict[int, torch.Tensor]:
    """One epoch's draws of every member in ``members`` from its own stream: {m: the epoch's order as global sample numbers
    (int64, host)}.  An epoch's draws are made when its iterator is built (the ``DataLoader``'s base seed) and at its first
    batch (the ``RandomSampler``'s seed and permutation); nothing is drawn after that, so the first batch is all that is
    taken."""
    def one(lo: ResidentLoader) -> torch.Tensor:
        next(lo.iter_indices())
        return lo.sampler.order.clone()
    return {m: streams.run(m, lambda lo=loaders[m]: one(lo)) for m in members}


class ClassifierEnsembleTrainer:
    def __init__(self, models: Sequence, learning_rate: float = 0.0005, weight_decay: float = 0.0,
                 log_dirs: Optional[Sequence[Optional[str]]] = None, verbose: bool = False,
                 rng_states: Optional[Sequence[torch.Tensor]] = None) -> None:
        from .._classifier_ensemble_engine import ClassifierEnsembleEngine
        self.models = list(models)
        self.engine = ClassifierEnsembleEngine(self.models, float(learning_rate), float(weight_decay))
        M = self.M = len(self.models)
        self.log_dirs = list(log_dirs) if log_dirs is not None else [None] * M
        if len(self.log_dirs) != M:
            raise ValueError(f"expected {M} log directories, got {len(self.log_dirs)}")
        self.verbose = verbose
        self.streams = MemberStreams(M, rng_states)
        self.history: List[List[Dict[str, float]]] = [[] for _ in range(M)]
        self.stopped_epoch: List[Optional[int]] = [None] * M
        self.test_accuracy: List[Optional[float]] = [None] * M
        self.test_f1: List[Optional[float]] = [None] * M
        self.confusion_matrix: List[Optional[torch.Tensor]] = [None] * M
        self._err = torch.zeros(1, dtype=torch.int32, device=self.engine.device)
        self._fitted = False

    def rng_state(self, m: int) -> torch.Tensor:
        """Member m's current generator state."""
        return self.streams.states[m].clone()

    # ------------------------------------------------------------------ epochs
    def _batches(self, loaders: Sequence[ResidentLoader], members: Sequence[int]):
        """The stacked batches (x (M, B, ...), y (M, B)) of one epoch: the M orders are drawn, go to the device as one (M, n)
        table, and every batch is one gather launch."""
        check_loaders(loaders, self.M)
        orders = draw_orders(loaders, self.streams, members)
        n, bs, ds = len(loaders[0].sampler.indices), loaders[0].batch_size, loaders[0].dataset
        table = torch.zeros(self.M, n, dtype=torch.int64)
        for m, order in orders.items():
            table[m] = order
        table = table.to(ds.device)                          # once per epoch
        for start in range(0, n, bs):
            yield ds.gather_group(table, start, min(start + bs, n), self._err, self.engine._active)

    def _check_gather(self) -> None:
        bits = int(self._err.item())                         # (the epoch's statistics were just read: the stream is idle)
        if bits:
            self._err.zero_()
            what = " and ".join(w for b, w in ((1, "a sample index"), (2, "a channel number")) if bits & b)
            raise IndexError(f"ClassifierEnsembleTrainer: {what} was out of range during the epoch; those rows were not written")

    def _run_epoch(self, loaders, train: bool, members: Sequence[int]) -> Dict[int, Dict[str, float]]:
        for m in members:
            self.models[m].train(train)
        step = self.engine.train_batch if train else self.engine.eval_batch
        for x, y in self._batches(loaders, members):
            step(x, y)
        stats = self.engine.epoch_stats()
        self._check_gather()
        return {m: {"loss": stats[m][0] / max(stats[m][1], 1), "accuracy": macro_scores(stats[m][2])["accuracy"],
                    "confusion_matrix": stats[m][2]} for m in members}

    def fit(self, train_loaders, val_loaders, max_epochs: int, patience: int) -> List[List[Dict[str, float]]]:
        from .._classifier_ensemble_engine import check_train_batch
        if self._fitted:
            raise RuntimeError("ClassifierEnsembleTrainer.fit runs once: the members share one NAdam schedule from step 0 and a "
                               "stopped member does not resume")
        self._fitted = True
        M = self.M
        check_loaders(train_loaders, M)
        check_loaders(val_loaders, M)
        # shallow members train batches of at most FusedNAdam.LOWRANK_MAX rows: refused here, before the first epoch
        check_train_batch(self.engine.shallow, int(train_loaders[0].batch_size))
        stopping, step = [EarlyStopping(patience) for _ in range(M)], 0
        active = [True] * M
        try:
            for epoch in range(max_epochs):
                members = [m for m in range(M) if active[m]]
                if not members:
                    break
                self.engine.set_active(active)
                tr = self._run_epoch(train_loaders, True, members)
                step += len(train_loaders[0])
                va = self._run_epoch(val_loaders, False, members)
                for m in members:
                    row = epoch_row(epoch, step, tr[m], va[m], self.models[m])
                    self.history[m].append(row)
                    if self.verbose:
                        print(f"member {m} {epoch_line(row)}")
                    if stopping[m].stops(va[m]["loss"]):
                        self.stopped_epoch[m] = epoch
                        active[m] = False
            for m in range(M):
                write_metrics(self.log_dirs[m], self.history[m])
        finally:
            self.engine.set_active([True] * M)               # evaluation takes every member; nothing updates from here on
            self.streams.leave()
        return self.history

    # ------------------------------------------------------------------ evaluation
    @torch.no_grad()
    def test(self, loaders) -> List[Dict[str, object]]:
        members = list(range(self.M))
        try:
            got = self._run_epoch(loaders, False, members)
        finally:
            self.streams.leave()
        out = []
        for m in members:
            cm = got[m]["confusion_matrix"]
            scores = macro_scores(cm)
            self.test_accuracy[m], self.test_f1[m], self.confusion_matrix[m] = scores["accuracy"], scores["f1"], cm
            write_confusion(self.log_dirs[m], cm)
            out.append({"accuracy": scores["accuracy"], "f1": scores["f1"], "confusion_matrix": cm})
        return out

    @torch.no_grad()
    def predict(self, loaders) -> List[torch.Tensor]:
        members = list(range(self.M))
        for model in self.models:
            model.eval()
        try:
            preds = torch.cat([self.engine.predict_batch(x) for x, _ in self._batches(loaders, members)], dim=1)
            self._check_gather()
        finally:
            self.streams.leave()
        return [preds[m].clone() for m in members]
