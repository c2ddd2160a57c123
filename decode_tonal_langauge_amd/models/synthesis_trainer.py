"""``SynthesisTrainer`` on MI355X (mirror of reference models/synthesis_trainer.py:46-302).

Same constructor keywords, ``train(loader, epochs, verbose) -> [(loss, mcd)]`` and
``evaluate(loader) -> (mcd, recon, origin)``.  What changes is where the work happens:

* the label dynamics are gathered on the device (``tl_tone_dynamics``) instead of the
  ``.cpu().numpy()`` -> Python loop -> ``torch.Tensor`` round trip (:212-218);
* for the models of this package the step is fused: forward, L1 (+ MCD statistics), backward and
  NAdam run as HIP kernels on one stream with no autograd graph and no host sync per step
  (the reference syncs three times per step, :214-215,228,229); loss / MCD are accumulated on
  the device and read once per epoch;
* under ``torch.distributed`` (one process per GPU) every rank takes its row shard of each
  global batch and gradients are reduced over RCCL (parallel.py).

Reference quirks kept on purpose: training targets are truncated to integers (:222), evaluation
targets are not (:290); the classifiers are never updated (their parameters are not in the
optimizer, :131-137) - ``train_classifiers`` only toggles ``.train()``.
"""
from __future__ import annotations

from typing import Dict, List, Tuple

import torch
import torch.nn as nn
from torch.utils.data import DataLoader

from .. import _kernels, _lib, parallel
from .._lib import check, ptr
from .._step_graph import StepGraphs, frozen_rows
from ..optim import FusedNAdam
from .classifier import ClassifierModel
from .synthesis_models import SynthesisModel


def compute_mcd(true_mcc: torch.Tensor, pred_mcc: torch.Tensor) -> float:
    """Mean over the batch of 10/ln10 * sqrt(2 * sum_k (t - p)^2) (reference :14-43), computed by
    the ``tl_l1_mcd`` kernel."""
    t = true_mcc.float().contiguous()
    p = pred_mcc.detach().float().contiguous()
    _lib.require_gpu(p, "compute_mcd")
    stats = torch.zeros(4, dtype=torch.float32, device=p.device)
    B, D = p.shape
    check(_lib.load().tl_l1_mcd(ptr(p), ptr(t.to(p.device)), None, ptr(stats), B, D, D, 0, 1.0,
                                torch.cuda.current_stream().cuda_stream), "tl_l1_mcd")
    return float(stats[3].item())


# with the row-sharded LSTM its dgates - hence the W_ih / bias gradients - already belong to the global batch on every rank:
# they stay out of the all-reduce
_LSTM_LOCAL = ("label_lstm.weight_ih_l0", "label_lstm.bias_ih_l0", "label_lstm.bias_hh_l0")
_EARLY = ("output_layer.weight", "output_layer.bias")       # final before the convolution backward starts (on_grad_ready)


def tone_dynamics_table(tone_dynamic_mapping: Dict[str, List[float]]):
    """(table, L, n_rows): row t of the float32 host table is ``mapping[str(t)]``, NaN where a tone below the largest key has
    no entry.  Every entry must have the same length L."""
    keys = sorted(int(k) for k in tone_dynamic_mapping)
    lens = {len(v) for v in tone_dynamic_mapping.values()}
    if len(lens) != 1:
        raise ValueError("every entry of tone_dynamic_mapping must have the same length")
    L = lens.pop()
    n_rows = (max(keys) + 1) if keys else 0
    table = torch.full((max(n_rows, 1), L), float("nan"))
    for k in keys:
        if k >= 0:
            table[k] = torch.tensor(tone_dynamic_mapping[str(k)], dtype=torch.float32)
    return table, L, n_rows


class SynthesisTrainer:
    def __init__(self, synthesize_model: SynthesisModel, tone_model: ClassifierModel, syllable_model: ClassifierModel,
                 tone_dynamic_mapping: Dict[str, List[int]], device: torch.device = torch.device("cpu"),
                 learning_rate: float = 0.0005, beta_1: float = 0.9, beta_2: float = 0.999, epsilon: float = 1e-08,
                 schedule_decay: float = 0.004, verbose: bool = True, train_classifiers: bool = False) -> None:
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("SynthesisTrainer (MI355X build) needs a 'cuda' device: the synthesis path runs "
                               "hand-written HIP kernels and has no CPU fallback")
        self.lib = _lib.load()
        self.train_classifiers = train_classifiers
        self.tone_dynamic_mapping = tone_dynamic_mapping
        self.model = synthesize_model.to(self.device)
        if verbose:
            print(f"Number of trainable parameters in the synthesis model: {self.model.get_nparams():,}")
        self.optimizer = FusedNAdam(self.model.parameters(), lr=learning_rate, betas=(beta_1, beta_2), eps=epsilon,
                                    weight_decay=schedule_decay)
        self.criterion = nn.L1Loss()          # generic (autograd) path only
        self.tone_model = tone_model.to(self.device)
        self.syllable_model = syllable_model.to(self.device)
        if not train_classifiers:
            self.tone_model.eval()
            self.syllable_model.eval()
        elif verbose:
            for nm, m in (("tone", self.tone_model), ("syllable", self.syllable_model)):
                n = sum(p.numel() for p in m.parameters() if p.requires_grad)
                print(f"Number of trainable parameters in the {nm} model: {n:,}")
        table, self._L, self._n_rows = tone_dynamics_table(tone_dynamic_mapping)
        self._table_host = table
        n_cls = getattr(self.tone_model, "n_classes", None)
        self._need_check = n_cls is None or any(str(t) not in tone_dynamic_mapping for t in range(n_cls))
        self._table = table.to(self.device)
        # every (tone, syllable) class pair as a label sequence: the synthesis model's LSTM runs on these rows and
        # the batch gathers from them by id = tone * n_syllables + syllable (no torch.unique, no host sync per step)
        n_syl = getattr(self.syllable_model, "n_classes", None)
        self._pair_table = None
        # Only the tone classes the classifier can predict (rows 0 .. n_classes - 1, all present when _need_check is
        # False) enter the table: a mapping with extra keys above them (say "5" beside a 4-class model) would otherwise
        # contribute NaN rows for the keys in between - no batch element gathers them, but the LSTM unrolls over every
        # table row and 0 * NaN in its backward pass would poison all of W_hh, W_ih and the biases.
        if not self._need_check and n_syl is not None and n_syl >= 1 and n_cls * n_syl <= 16:
            syl_col = torch.arange(n_syl, dtype=torch.float32).view(1, n_syl, 1).expand(n_cls, n_syl, self._L)
            dyn = table[:n_cls].view(n_cls, 1, self._L).expand(n_cls, n_syl, self._L)
            assert not torch.isnan(dyn).any()
            self._pair_table = torch.stack([syl_col, dyn], dim=2).reshape(n_cls * n_syl, 2, self._L).contiguous() \
                .to(self.device)
            self._n_syl = int(n_syl)
        self._pair_ids = None                 # (pair id per row, the label tensor they belong to) of the last label pass
        self._err = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._stats = torch.zeros(4, dtype=torch.float32, device=self.device)
        self._grads, self._flat, self._last_out = None, None, None
        self.rank, self.world = parallel.world()
        self.dp = parallel.active()
        self._row0, self._weight = 0, 1.0     # this rank's shard of the current batch (_shard)
        self._whh_dirty = False
        self._guard_hooked = False
        self.exchange_events = self.exchange_wait_events = None          # lists: HIP events around the exchange (bench.py)
        self._replay = StepGraphs("SynthesisTrainer", self.lib, self.optimizer, self.device)
        self._graphs = self._replay.states
        eng = getattr(self.model, "_engine", None)    # None: a plug-in SynthesisModel on torch autograd (_generic_step)
        if (self.dp and eng is not None and eng.lowrank_param is not None and self._pair_table is not None
                and _kernels.get("lstm_shard") != "0"):
            eng.lstm_shard = (self.rank, self.world)        # row-sharded label LSTM (parallel.py docstring)
            # Between steps each rank holds current values only for its own rows of weight_hh_l0.  `train` / `evaluate`
            # re-assemble it, but `train_step` is public: anything that reads the whole model (state_dict -> checkpoints)
            # first runs the collective, on every rank (a collective: all ranks must call state_dict together).  The
            # NAdam moments of that parameter stay per-rank shards: optimizer state under data parallelism is per rank.
            self.model.register_state_dict_pre_hook(self._state_dict_guard)
            self._guard_hooked = True

    def _state_dict_guard(self, module, prefix, keep_vars) -> None:
        """``state_dict()`` of the model while its label LSTM is row-sharded and out of date.  Re-assembling the weight is a
        collective: hidden inside ``state_dict`` it would deadlock the usual ``if rank == 0: torch.save(model.state_dict())``
        (and fire again for every nested / partial call).  So this raises; ``train`` / ``evaluate`` synchronise themselves,
        after a bare ``train_step`` call ``sync_parameters()`` (or ``model_state_dict()``) on EVERY rank first."""
        if self._whh_dirty:
            raise RuntimeError(
                "SynthesisTrainer: label_lstm.weight_hh_l0 is row-sharded over the data-parallel ranks and this rank only "
                "holds current values for its own rows.  Call trainer.sync_parameters() (or trainer.model_state_dict()) on "
                "every rank before model.state_dict() - it is a collective and is therefore not run implicitly here.")

    # ------------------------------------------------------------------ helpers
    def _labels(self, inputs_tone, inputs_syllable) -> torch.Tensor:
        """argmax of both classifiers + device gather of the dynamics (reference :207-218)."""
        st, ss = self.tone_model(inputs_tone), self.syllable_model(inputs_syllable)
        B = st.shape[0]
        labels = torch.empty(B, 2, self._L, dtype=torch.float32, device=self.device)
        self._pair_ids = None
        if st.dim() == 2 and ss.dim() == 2 and st.dtype == torch.float32 and ss.dtype == torch.float32 and st.is_cuda and ss.is_cuda:
            # arg-max of both score matrices, the dynamics gather and the pair id in one launch
            st, ss = st.detach().contiguous(), ss.detach().contiguous()
            tone = torch.empty(B, dtype=torch.int64, device=self.device)
            syl = torch.empty(B, dtype=torch.int64, device=self.device)
            pair = torch.empty(B, dtype=torch.int32, device=self.device) if self._pair_table is not None else None
            check(self.lib.tl_labels_from_scores(ptr(st), ptr(ss), ptr(self._table), ptr(labels), ptr(tone), ptr(syl),
                                                 ptr(pair) if pair is not None else None, ptr(self._err), B, st.shape[1],
                                                 ss.shape[1], self._n_rows, self._n_syl if pair is not None else 1, self._L,
                                                 torch.cuda.current_stream().cuda_stream), "tl_labels_from_scores")
            if pair is not None:                  # ids are valid for exactly this label tensor
                self._pair_ids = (pair, labels)
        else:
            tone = torch.argmax(st, dim=1).contiguous()
            syl = torch.argmax(ss, dim=1).contiguous()
            if self._pair_table is not None:          # ids are valid for exactly this label tensor
                self._pair_ids = ((tone * self._n_syl + syl).to(torch.int32), labels)
            check(self.lib.tl_tone_dynamics(ptr(tone), ptr(syl), ptr(self._table), ptr(labels), ptr(self._err), B,
                                            self._n_rows, self._L, torch.cuda.current_stream().cuda_stream),
                  "tl_tone_dynamics")
        if self._need_check:
            # a predicted tone may be absent from the mapping: keep the reference's immediate error.  Under
            # data parallelism the decision is taken by all ranks together (a rank that raised alone would
            # leave its peers blocked in the next collective).
            bad = [int(t) for t in tone.tolist() if str(int(t)) not in self.tone_dynamic_mapping]
            flag = torch.tensor([bad[0] + 1 if bad else 0], dtype=torch.int64, device=self.device)
            if self.dp:
                parallel.all_reduce_(flag, op=torch.distributed.ReduceOp.MAX)
            worst = int(flag.item())
            if worst:
                raise ValueError(f"Tone {worst - 1} not found in tone_dynamic_mapping."
                                 f"Available tones in mapping: {list(self.tone_dynamic_mapping.keys())}")
        return labels

    def _shard(self, *tensors):
        """Row shard of a global batch for this rank (``parallel.shard_plan``).  Sets ``self._row0`` (first global row of the
        shard) and ``self._weight``, the share of the global mean loss this rank's rows carry."""
        if self.world == 1:
            self._row0, self._weight = 0, 1.0
            return tensors
        plan = parallel.shard_plan(tensors[0].shape[0], self.rank, self.world)
        self._row0, self._weight = plan.row0, plan.weight
        return tuple(t[plan.slice] for t in tensors)

    def _loss_stats(self, out, targets, dout, ldd, trunc: int, stats=None) -> None:
        """``tl_l1_mcd``: loss gradient (scaled by this rank's weight in the global mean) and the
        L1 / MCD statistics.  Under data parallelism the per-rank statistics are accumulated with the
        same weight so that their sum over ranks is the statistic of the global batch."""
        stats = self._stats if stats is None else stats
        B, D = out.shape
        w = self._weight
        if not self.dp:
            check(self.lib.tl_l1_mcd(ptr(out), ptr(targets), ptr(dout), ptr(stats), B, D, ldd, trunc, 1.0,
                                     torch.cuda.current_stream().cuda_stream), "tl_l1_mcd")
            return
        tmp = torch.zeros(4, dtype=torch.float32, device=out.device)
        check(self.lib.tl_l1_mcd(ptr(out), ptr(targets), ptr(dout), ptr(tmp), B, D, ldd, trunc, float(w),
                                 torch.cuda.current_stream().cuda_stream), "tl_l1_mcd")
        stats[:2] += w * tmp[:2]
        stats[2:] = w * tmp[2:]

    def _timed(self, fn):
        """Wrap an exchange-step call with HIP events when ``self.exchange_events`` is a list (bench.py)."""
        events = self.exchange_events
        if events is None:
            return fn

        def run(*a, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = fn(*a, **k)
            e1.record()
            events.append((e0, e1))
            return r
        return run

    def _fused_step(self, inputs_non, inputs_label, targets, graph: bool = False) -> None:
        model = self.model
        eng = model._engine
        names = model._pnames
        params = dict(model.named_parameters())
        prm = {k: params[k].detach() for k in names}
        skip = eng.lowrank_param
        if self._grads is None:
            # the low-rank parameter's gradient (5.4 GB at the north-star shape) is only materialised
            # if its rank exceeds what the fused optimiser kernel takes (the engine then allocates it)
            if self.dp and eng.grad_order is not None:
                # data parallel: ONE flat buffer in the order the backward pass finishes the gradients - a bucket of the
                # exchange step is a contiguous slice (no torch.cat in front of the collective, no copy back behind it)
                sharded = eng.lstm_shard is not None and self._pair_table is not None
                local_only = _LSTM_LOCAL if sharded else ()
                self._flat = parallel.FlatGrads({k: v.shape for k, v in prm.items() if k != skip}, eng.grad_order(),
                                                prm[names[0]].device, local=local_only)
                self._grads = self._flat.views
            else:
                self._grads = {k: torch.empty_like(v) for k, v in prm.items() if k != skip}
        prm.update(model._engine_buffers())
        kw = {}
        ids = self._pair_ids
        if ids is not None and ids[1] is inputs_label and skip is not None:
            kw = dict(label_ids=ids[0], label_table=self._pair_table)             # CNN engine: skip torch.unique
        # (HIP-graph capture: the engine reads the dropout seed from device memory, the host seed counter is advanced by
        # the caller once per replay)
        out = eng.forward(prm, inputs_non, inputs_label, training=model.training, save=True,
                          seed=0 if graph else model._next_seed(), row0=self._row0, **kw)
        B, D = out.shape
        self._last_out = out             # the step's outputs (pre-update), for callers that track them (tests)
        # (tl_l1_mcd writes all D columns of a row: the zero fill is only for padding columns)
        dout = (torch.empty if eng.ldd == D else torch.zeros)(B, eng.ldd, dtype=torch.float32, device=out.device)
        self._loss_stats(out, targets, dout, eng.ldd, 1)
        gather = self._timed(parallel.gather_lowrank) if self.dp else None
        reduce_rows = self._timed(parallel.all_reduce_) if self.dp else None
        scale = 1.0          # the 1/N of the global mean is already in dout (weight of this rank's rows)
        early = []

        def on_factors(dh=None):
            # single process: the W_hh update (33 GB of HBM traffic) is issued as soon as its gradient factors exist, on the
            # stream the LSTM backward runs on - beside the convolution backward instead of behind it.  ``dh``: the engine
            # asks for the last BPTT product out of the same pass (they exist one step early: h_0 = 0)
            factors = eng.whh_factors
            if factors is not None and not self.dp:
                self.optimizer.step_lowrank({params[skip]: factors}, grad_scale=scale, dh=dh)
                early.append(params[skip])
        on_factors.fuse_dh = not self.dp
        flat = self._flat if self.dp else None
        pending = []

        def on_grad_ready(group):
            # Data parallel: the gradients of the output layer (63 MB of the 72 MB that are exchanged at the north-star
            # shape) are final before the convolution backward starts - their all-reduce is started here and runs beside
            # that backward pass ("launched as soon as each grad is final"); the optimiser waits for it below
            if flat is not None and group == "output_layer":
                pending.append(self._timed(parallel.all_reduce_async)(flat.span(_EARLY)))
        bkw = dict(on_grad_ready=on_grad_ready) if flat is not None else {}
        eng.backward(prm, dout, self._grads, gather_whh=gather, whh_factors=skip is not None, reduce_rows=reduce_rows,
                     on_factors=on_factors if skip is not None else None, **bkw)
        if self.dp:
            self._exchange(eng, flat, pending, skip)
        factors = eng.whh_factors
        if graph:            # scalars of the step from device memory (advanced by the caller per replay)
            self.optimizer.step_graph({params[k]: self._grads[k] for k in names}, self._replay.scalars, grad_scale=scale)
        elif early:            # W_hh is already updated
            self.optimizer.step(grads={params[k]: self._grads[k] for k in names if k != skip}, grad_scale=scale, skip=set(early))
        elif factors is not None:          # the optimiser forms that gradient from its factors on the fly
            self.optimizer.step(grads={params[k]: self._grads[k] for k in names if k != skip}, grad_scale=scale,
                                lowrank={params[skip]: factors})
        else:
            self.optimizer.step(grads={params[k]: self._grads[k] for k in names}, grad_scale=scale)

    def _exchange(self, eng, flat, pending, skip) -> None:
        """The data-parallel gradient exchange behind the backward pass: ``pending`` holds the all-reduce of the early bucket
        when ``on_grad_ready`` started one, ``skip`` names the low-rank parameter (exchanged as factors, inside the backward)."""
        sharded = eng.ran_sharded
        local_only = _LSTM_LOCAL if sharded else ()
        wait_events = self.exchange_wait_events
        if flat is not None and local_only == tuple(flat.local):
            rest = [k for k in flat.offsets if k not in _EARLY and k not in local_only]
            if not pending:                              # (an engine that never reported the early group)
                rest = [k for k in flat.offsets if k not in local_only]
            if rest:
                pending.append(self._timed(parallel.all_reduce_async)(flat.span(rest)))
            for h in pending:
                h.wait(wait_events)
        else:
            # The row-sharded LSTM fell back for this step (its shard decision is per forward: (L - 1) U > 64, a gate-row
            # count the world size does not divide, no label table) or started to shard after the flat layout was fixed:
            # the flat span no longer matches what must be reduced.  The early bucket (output layer) is already in
            # flight: wait for it and reduce every OTHER gradient exactly once.
            reduced = set()
            for h in pending:
                h.wait(wait_events)
                reduced.update(_EARLY)
            self._timed(parallel.allreduce_bucketed)([g for k, g in self._grads.items()
                                                      if k != skip and k not in local_only and k not in reduced])
        self._whh_dirty = self._whh_dirty or sharded

    def _generic_step(self, inputs_non, inputs_label, targets) -> None:
        """Any other ``SynthesisModel`` subclass: torch autograd for the model, fused NAdam."""
        self.optimizer.zero_grad()
        outputs = self.model(inputs_non, inputs_label)
        tgt = targets.long()
        loss = self.criterion(outputs, tgt)
        if self.dp:
            (loss * self._weight).backward()
            for p in self.model.parameters():
                if p.grad is None:
                    p.grad = torch.zeros_like(p)
            self._timed(parallel.allreduce_bucketed)([p.grad for p in self.model.parameters()])
        else:
            loss.backward()
        self.optimizer.step(grad_scale=1.0)
        out = outputs.detach().float().contiguous()
        self._loss_stats(out, targets.float().contiguous(), None, out.shape[1], 1)

    def sync_parameters(self) -> None:
        """Re-assemble parameters that data-parallel ranks update shard-wise (the row-sharded ``weight_hh_l0``):
        afterwards every rank holds the full, current model (``state_dict``, ``evaluate``)."""
        if not self._whh_dirty:
            return
        eng = self.model._engine
        p = dict(self.model.named_parameters())[eng.lowrank_param]
        rows = p.shape[0] // self.world
        parallel.all_gather_param_rows_(p.data, self.rank * rows, rows)
        self._whh_dirty = False

    def set_lstm_shard(self, on: bool) -> bool:
        """Switch the gate-row sharding of the label LSTM on or off BETWEEN steps (data parallel only; a collective: every
        rank must call it with the same value).  The weight is re-assembled first; the NAdam state of ``weight_hh_l0``
        follows the mode - its moments are cut to this rank's rows (whole -> shard: every rank holds the same full
        moments) or all-gathered (shard -> whole), its step count and mu product stay - so the parameter keeps the
        single-process trajectory across a switch (bench.py ``--lstm-shard auto`` switches during warm-up).  The flat gradient
        layout is rebuilt.  Returns whether the LSTM will run sharded (False where the model / label table does not allow it)."""
        eng = getattr(self.model, "_engine", None)
        if not self.dp or eng is None or eng.lowrank_param is None:
            return False
        self.sync_parameters()
        want = (self.rank, self.world) if (on and self._pair_table is not None and self.world > 1) else None
        if want != eng.lstm_shard:
            eng.lstm_shard = want
            p = dict(self.model.named_parameters())[eng.lowrank_param]
            st = self.optimizer.state.get(p)
            if st:
                rows = p.shape[0] // self.world
                r0 = self.rank * rows
                for key in ("exp_avg", "exp_avg_sq"):
                    if p.is_cuda:
                        torch.cuda.empty_cache()              # (a fresh allocation per moment tensor: optim.FusedNAdam._state_for)
                    if want is not None:                      # whole -> this rank's rows
                        st[key] = st[key][r0:r0 + rows].clone()
                    else:                                     # row shards -> the whole matrix on every rank
                        full = torch.zeros_like(p, memory_format=torch.preserve_format)
                        full[r0:r0 + rows].copy_(st[key])
                        st[key] = parallel.all_gather_param_rows_(full, r0, rows)
                st["shard_rows"] = (r0, rows) if want is not None else None
            self._grads, self._flat = None, None
            if want is not None and not self._guard_hooked:
                self.model.register_state_dict_pre_hook(self._state_dict_guard)
                self._guard_hooked = True
        return eng.lstm_shard is not None

    def model_state_dict(self):
        """``model.state_dict()`` with the shard-wise updated parameters re-assembled first.  Collective under data
        parallelism (every rank must call it).  The NAdam moments of a row-sharded parameter stay per rank and
        shard-shaped: an optimizer checkpoint is only resumable with the same world size."""
        self.sync_parameters()
        return self.model.state_dict()

    def train_step(self, inputs_non, inputs_syllable, inputs_tone, targets) -> None:
        """One body of the batch loop (reference :201-229).  Loss / MCD go to ``self._stats``.

        Under data parallelism with the row-sharded label LSTM a rank holds current values only for its own gate rows of
        ``label_lstm.weight_hh_l0`` between steps: ``train`` and ``evaluate`` re-assemble them (``sync_parameters``); a caller
        that drives ``train_step`` itself must call ``sync_parameters()`` (or ``model_state_dict()``) on every rank before it
        reads, evaluates or saves the model."""
        dev = self.device
        inputs_non = inputs_non.to(dev, non_blocking=True)
        inputs_syllable = inputs_syllable.to(dev, non_blocking=True)
        inputs_tone = inputs_tone.to(dev, non_blocking=True)
        targets = targets.to(dev, non_blocking=True).float().contiguous()
        inputs_non, inputs_syllable, inputs_tone, targets = self._shard(inputs_non, inputs_syllable, inputs_tone,
                                                                        targets)
        eng = getattr(self.model, "_engine", None)    # None: a plug-in SynthesisModel on torch autograd
        if self._graph_ok(eng) and self._replay.step((inputs_non, inputs_syllable, inputs_tone, targets), self.model.parameters(),
                                                     self._graph_fingerprint, self._graph_capture, self.model._next_seed):
            return
        with torch.no_grad():
            inputs_label = self._labels(inputs_tone, inputs_syllable)
        if eng is not None:
            self._fused_step(inputs_non.float().contiguous(), inputs_label, targets.contiguous())
        else:
            self._generic_step(inputs_non, inputs_label, targets)

    # ------------------------------------------------------------------ HIP-graph replay (_step_graph.StepGraphs)
    def _graph_ok(self, eng) -> bool:
        """Whether this step may go through a HIP graph.  Not under data parallelism (collectives), not with classifiers in
        train mode (their dropout seed is a launch argument), not for the big model (GPU-bound; its W_hh update takes
        launch-argument scalars).  TONAL_GRAPH=0 turns it off."""
        return (eng is not None and eng.graph_capable and not self.dp and not self.train_classifiers and not self._need_check
                and self.model.training)

    def _graph_fingerprint(self) -> tuple:
        """What a captured step has frozen into its kernel arguments besides the batch (``_step_graph.frozen_rows``)."""
        name_of = {id(p): k for k, p in self.model.named_parameters()}       # gradient storage is keyed by parameter NAME
        grads = self._grads or {}
        return tuple(frozen_rows(self.optimizer, lambda p: grads.get(name_of.get(id(p))), (self.tone_model, self.syllable_model))
                     + [(self.model._engine.p_drop, self.model.training)])

    def _graph_capture(self, recording, static) -> None:
        eng = self.model._engine
        eng.seed_dev = self._replay.seed         # the captured step reads its dropout seed from device memory
        try:
            with recording:
                with torch.no_grad():
                    lab = self._labels(static[2], static[1])
                self._fused_step(static[0].float().contiguous(), lab, static[3].contiguous(), graph=True)
        finally:
            eng.seed_dev = None                  # eager steps (other shapes) keep passing the seed by value

    # ------------------------------------------------------------------ public API
    def train(self, train_loader: DataLoader, epochs: int, verbose: bool = True) -> List[Tuple[float, float]]:
        self.model.train()
        if self.train_classifiers:
            self.tone_model.train()
            self.syllable_model.train()
        history = []
        for epoch in range(epochs):
            self._stats.zero_()
            nb = 0
            for inputs_non, inputs_syllable, inputs_tone, targets in train_loader:
                self.train_step(inputs_non, inputs_syllable, inputs_tone, targets)
                nb += 1
            self.sync_parameters()
            stats = self._stats.clone()
            if self.dp:
                parallel.all_reduce_(stats)          # per-rank statistics carry their weight in the global mean
            s = stats.tolist()                                  # the one host sync of the epoch
            epoch_loss, mcd = s[0] / max(nb, 1), s[1] / max(nb, 1)
            history.append((epoch_loss, mcd))
            if verbose:
                print(f"Epoch {epoch+1}/{epochs}, Loss: {epoch_loss:.4f}, Mean MCD: {mcd:.4f}")
        return history

    def evaluate(self, test_loader: DataLoader):
        self.sync_parameters()
        self.model.eval()
        self.tone_model.eval()
        self.syllable_model.eval()
        recon, origin = [], []
        stats = torch.zeros(4, dtype=torch.float32, device=self.device)
        nb = 0
        with torch.no_grad():
            for inputs_non, inputs_syllable, inputs_tone, targets in test_loader:
                inputs_non = inputs_non.to(self.device)
                inputs_syllable = inputs_syllable.to(self.device)
                inputs_tone = inputs_tone.to(self.device)
                targets = targets.to(self.device).float().contiguous()
                inputs_label = self._labels(inputs_tone, inputs_syllable)
                outputs = self.model(inputs_non, inputs_label).float().contiguous()
                B, D = outputs.shape
                check(self.lib.tl_l1_mcd(ptr(outputs), ptr(targets), None, ptr(stats), B, D, D, 0, 1.0,
                                         torch.cuda.current_stream().cuda_stream), "tl_l1_mcd")
                recon.append(outputs.cpu())
                origin.append(targets.cpu())
                nb += 1
        mcd = float(stats[1].item()) / max(nb, 1)
        return mcd, torch.cat(recon, dim=0).numpy(), torch.cat(origin, dim=0).numpy()
