"""``SynthesisTrainer``'s loop for the M ``SynthesisLite`` models of one ``--repeat M`` experiment at once: every step of the
group is the launches of one model's step (``_lite_ensemble_engine``), every batch of the group one gather launch
(``tl_gather_rows_group``) over the ONE ``ResidentDataset`` the members' splits index.

Member m ends with the bits a sequential ``SynthesisTrainer`` run of that member gives it - parameters, BatchNorm buffers,
per-epoch loss / MCD, evaluation output: the same kernels on the same batches, the same labels (the classifiers are in eval mode,
so a row's label does not depend on the batch it sits in: one label pass over the M B rows), the dropout mask of the member's own
seed and call counter (``SynthesisLite._next_seed``'s rule, formed on the device into the seed table the group kernels read), one
``FusedNAdam`` over the stacked tensors (the update is element-wise; the members advance in lockstep from step 0).

After three eager steps at a batch shape the group step is captured into a HIP graph and replayed, as ``SynthesisTrainer`` does
for one model: single stream, static input buffers, the NAdam scalars and the seeds in device memory, a fingerprint of what the
capture froze; ``TONAL_GRAPH=0`` turns it off, a failed capture falls back to eager with a warning.

Random streams: every member keeps its own state of torch's global CPU generator (``MemberStreams``), from which its epoch
orders are drawn exactly as its ``ResidentLoader`` would draw them (``epoch_tables``).

Refused (``ValueError``): ``train_classifiers=True`` (classifier dropout makes the labels member-dependent), a CPU device, data
parallelism, and what ``LiteEnsembleEngine`` refuses.  Evaluation runs member by member through the single path."""
from __future__ import annotations

from typing import Dict, Iterable, Iterator, List, Optional, Sequence, Tuple

import torch

from .. import _lib, parallel
from .._lib import check, ptr
from .._step_graph import StepGraphs, frozen_rows
from ..data_loading.resident import ResidentDataset, ResidentLoader
from ..optim import FusedNAdam
from .classifier_ensemble_trainer import MemberStreams, check_loaders, draw_orders
from .synthesis_trainer import SynthesisTrainer

_MASK64 = 0xFFFFFFFFFFFFFFFF


def _i64(v: int) -> int:
    """The 64-bit word ``v`` as the signed integer an int64 tensor holds."""
    v &= _MASK64
    return v - (1 << 64) if v >= (1 << 63) else v


class SynthesisEnsembleTrainer:
    def __init__(self, models: Sequence, tone_model, syllable_model, tone_dynamic_mapping: Dict[str, List[int]],
                 seeds: Sequence[int], device: torch.device = torch.device("cpu"), learning_rate: float = 0.0005,
                 beta_1: float = 0.9, beta_2: float = 0.999, epsilon: float = 1e-08, schedule_decay: float = 0.004,
                 verbose: bool = True, train_classifiers: bool = False,
                 rng_states: Optional[Sequence[torch.Tensor]] = None) -> None:
        from .._lite_ensemble_engine import LiteEnsembleEngine, check_supported
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError(f"SynthesisEnsembleTrainer needs a CUDA device (got '{self.device}'): the synthesis ensemble runs "
                             "hand-written HIP kernels and has no CPU fallback")
        if train_classifiers:
            raise ValueError("SynthesisEnsembleTrainer: train_classifiers=True is not supported - classifiers in train mode draw "
                             "dropout masks, which makes a row's label depend on the member; give both classifier checkpoints")
        if parallel.active():
            raise ValueError("SynthesisEnsembleTrainer: data parallelism is not supported - the synthesis ensemble runs in a "
                             "single process (no process group)")
        models = list(models)
        if len(seeds) != len(models):
            raise ValueError(f"expected {len(models)} seeds, got {len(seeds)}")
        models = [m.to(self.device) for m in models]
        check_supported(models)
        self.lib = _lib.load()
        M = self.M = len(models)
        self.models = models
        # ONE single-model trainer: its label pass serves the group, and evaluation runs through it member by member (its model
        # swapped; it never steps, so its optimiser holds no state)
        self.single = SynthesisTrainer(models[0], tone_model, syllable_model, tone_dynamic_mapping, device=self.device,
                                       learning_rate=learning_rate, beta_1=beta_1, beta_2=beta_2, epsilon=epsilon,
                                       schedule_decay=schedule_decay, verbose=verbose, train_classifiers=False)
        self.tone_model, self.syllable_model = self.single.tone_model, self.single.syllable_model
        self.engine = LiteEnsembleEngine(models)
        self._stacks = [self.engine.params[k] for k in self.engine.names]
        self._grads = {self.engine.params[k]: self.engine.grads[k] for k in self.engine.names}
        self.optimizer = FusedNAdam(self._stacks, lr=learning_rate, betas=(beta_1, beta_2), eps=epsilon,
                                    weight_decay=schedule_decay)
        self.seeds = [int(s) for s in seeds]
        # SynthesisLite._next_seed: (torch.initial_seed() * 0x9E3779B1 + calls) mod 2^64, the member's own seed and counter
        self._seed_base = torch.tensor([_i64(s * 0x9E3779B1) for s in self.seeds], dtype=torch.int64, device=self.device)
        self._calls_host = [int(m._drop_calls) for m in models]          # what the device counters hold
        self._calls = torch.tensor(self._calls_host, dtype=torch.int64, device=self.device)
        self._stats = torch.zeros(M, 4, dtype=torch.float32, device=self.device)
        self._err = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.streams = MemberStreams(M, rng_states)
        self._replay = StepGraphs("SynthesisEnsembleTrainer", self.lib, self.optimizer, self.device)
        self._graphs = self._replay.states

    # ------------------------------------------------------------------ one step
    def _labels(self, inputs_tone: torch.Tensor, inputs_syllable: torch.Tensor) -> torch.Tensor:
        """The label pass over the M B rows: (M, B, ...) inputs -> (M, B, 2, L)."""
        M, B = inputs_tone.shape[:2]
        lab = self.single._labels(inputs_tone.flatten(0, 1), inputs_syllable.flatten(0, 1))
        return lab.view(M, B, *lab.shape[1:])

    def _step(self, inputs_non, inputs_label, targets, graph: bool = False) -> None:
        eng = self.engine
        # the members' dropout seeds of this step, formed where the kernels read them
        self._calls.add_(1)
        torch.add(self._seed_base, self._calls, out=eng.seeds)
        out = eng.forward(inputs_non, inputs_label, training=True, save=True)
        M, B, D = out.shape
        self._last_out = out
        dout = (torch.empty if eng.ldd == D else torch.zeros)(M, B, eng.ldd, dtype=torch.float32, device=out.device)
        check(self.lib.tl_l1_mcd_group(ptr(out), ptr(targets), ptr(dout), ptr(self._stats), M, B, D, eng.ldd, 1, 1.0, B * D,
                                       targets.stride(0), B * eng.ldd, ptr(eng.active),
                                       torch.cuda.current_stream().cuda_stream), "tl_l1_mcd_group")
        eng.backward(dout)
        if graph:
            self.optimizer.step_graph(self._grads, self._replay.scalars, grad_scale=1.0)
        else:
            self.optimizer.step(grads=self._grads, grad_scale=1.0)

    def _check_batch(self, inputs_non, inputs_syllable, inputs_tone, targets):
        M = self.M
        for t in (inputs_non, inputs_syllable, inputs_tone, targets):
            if t.dim() < 2 or t.shape[0] != M or t.shape[1] != inputs_non.shape[1]:
                raise ValueError(f"expected stacked batches ({M}, B, ...), got {tuple(t.shape)}")
        if targets.dim() != 3 or targets.shape[2] != self.engine.out_dim:
            raise ValueError(f"expected targets ({M}, B, {self.engine.out_dim}), got {tuple(targets.shape)}")

    def train_step(self, inputs_non, inputs_syllable, inputs_tone, targets) -> None:
        """One step of every member on its own batch: stacked (M, B, ...) tensors.  Loss / MCD go to ``self._stats`` (M, 4)."""
        from .._lite_ensemble_engine import check_train_batch
        dev = self.device
        inputs_non = inputs_non.to(dev).float().contiguous()
        inputs_syllable, inputs_tone = inputs_syllable.to(dev).contiguous(), inputs_tone.to(dev).contiguous()
        targets = targets.to(dev).float().contiguous()
        self._check_batch(inputs_non, inputs_syllable, inputs_tone, targets)
        check_train_batch(int(inputs_non.shape[1]), self.single._L)        # refused before any launch
        # a member's forward through its module (evaluation, inference) advances its call counter on the host only: bring the
        # device counters up to date before they are used (a host comparison per step, a copy only when something moved)
        now = [int(m._drop_calls) for m in self.models]
        if now != self._calls_host:
            self._calls.copy_(torch.tensor(now, dtype=torch.int64))
        for m in self.models:
            m.train()
            m._drop_calls += 1                       # the host's mirror of the device counters
        self._calls_host = [c + 1 for c in now]
        self.tone_model.eval()
        self.syllable_model.eval()
        if self._graph_ok() and self._replay.step((inputs_non, inputs_syllable, inputs_tone, targets), self._stacks,
                                                  self._graph_fingerprint, self._graph_capture):
            return
        with torch.no_grad():
            inputs_label = self._labels(inputs_tone, inputs_syllable)
        self._step(inputs_non, inputs_label, targets)

    # ------------------------------------------------------------------ HIP-graph replay (_step_graph.StepGraphs)
    def _graph_ok(self) -> bool:
        return not self.single._need_check

    def _graph_fingerprint(self) -> tuple:
        """What a captured step has frozen into its kernel arguments besides the batch (``_step_graph.frozen_rows``)."""
        eng = self.engine
        return tuple(frozen_rows(self.optimizer, self._grads.get, (self.tone_model, self.syllable_model))
                     + [(eng.p_drop, tuple(b.data_ptr() for b in eng.buffers.values()),
                         None if eng.active is None else eng.active.data_ptr())])

    def _graph_capture(self, recording, static) -> None:
        calls = self._calls.clone()
        try:
            with recording:
                with torch.no_grad():
                    lab = self._labels(static[2], static[1])
                self._step(static[0], lab, static[3], graph=True)
        except Exception:
            self._calls.copy_(calls)
            raise

    # ------------------------------------------------------------------ public API
    def epoch_tables(self, loaders: Sequence[ResidentLoader]) -> Iterator[torch.Tensor]:
        """One (M, n) int64 table of global sample numbers per epoch, for ever: member m's row is the order its loader draws from
        the member's own random stream - what a sequential run of that member iterates."""
        check_loaders(loaders, self.M)
        members = list(range(self.M))
        while True:
            orders = draw_orders(loaders, self.streams, members)
            yield torch.stack([orders[m] for m in members])

    def train(self, resident_dataset: ResidentDataset, index_tables: Iterable[torch.Tensor], epochs: int, batch_size: int = 8,
              verbose: bool = False) -> List[List[Tuple[float, float]]]:
        """``epochs`` epochs over ``resident_dataset``: ``index_tables`` yields one (M, n) int64 table per epoch (member m trains on
        samples ``table[m]`` in that order, ``batch_size`` per step, the last batch ragged).  Returns one [(loss, mcd), ...] per
        member.  One host synchronisation per epoch."""
        M = self.M
        history: List[List[Tuple[float, float]]] = [[] for _ in range(M)]
        tables = iter(index_tables)
        try:
            for epoch in range(epochs):
                table = next(tables)
                if table.dim() != 2 or table.shape[0] != M or table.dtype != torch.int64:
                    raise ValueError(f"expected an ({M}, n) int64 index table, got {tuple(table.shape)} {table.dtype}")
                table = table.to(resident_dataset.device).contiguous()           # once per epoch
                n = table.shape[1]
                self._stats.zero_()
                nb = 0
                for start in range(0, n, batch_size):
                    batch = resident_dataset.gather_group(table, start, min(start + batch_size, n), self._err, self.engine.active)
                    self.train_step(*batch)
                    nb += 1
                stats = self._stats.tolist()                                     # the one host sync of the epoch
                bits = int(self._err.item())
                if bits:
                    self._err.zero_()
                    raise IndexError("SynthesisEnsembleTrainer: a sample index or channel number was out of range during the epoch")
                for m in range(M):
                    history[m].append((stats[m][0] / max(nb, 1), stats[m][1] / max(nb, 1)))
                    if verbose:
                        print(f"member {m} Epoch {epoch+1}/{epochs}, Loss: {history[m][-1][0]:.4f}, Mean MCD: {history[m][-1][1]:.4f}")
        finally:
            self.streams.leave()
        return history

    def train_loaders(self, loaders: Sequence[ResidentLoader], epochs: int, verbose: bool = False):
        """``train`` on the members' own ``ResidentLoader``s (one per member, over one ``ResidentDataset``)."""
        check_loaders(loaders, self.M)
        return self.train(loaders[0].dataset, self.epoch_tables(loaders), epochs, batch_size=loaders[0].batch_size, verbose=verbose)

    def evaluate(self, loaders: Sequence) -> List[tuple]:
        """One ``(mcd, recon, origin)`` per member, each through ``SynthesisTrainer.evaluate`` on the member's module."""
        if len(loaders) != self.M:
            raise ValueError(f"{len(loaders)} loaders for {self.M} members")
        out = []
        try:
            for model, lo in zip(self.models, loaders):
                self.single.model = model
                out.append(self.single.evaluate(lo))
        finally:
            self.single.model = self.models[0]
        return out
