"""Training of ``CNNClassifier`` on the HIP path (the loop of reference models/classifier_trainer.py:22-177 around the model
of models/deep_classifiers.py:17-155: ``nn.CrossEntropyLoss`` on the model's SIGMOID outputs, ``loss.backward()``, ``NAdam``
with two decay groups, a confusion matrix per epoch).

One train step of a batch (B, C, T):
  trunk     the six conv stages on ``ConvStack`` - the kernels, the layout and the three passes per stage of the synthesis
            model's ECoG block (F(6,3) / F(4,3) V form / direct MFMA by ``TONAL_KERNELS`` wino), with the arg-max and sign
            planes (or V) the backward needs; ``tl_dropout_scale_at`` on the last pooled feature map in train mode;
  fc1       the feature map is gathered into torch's flatten order (B, K) by ``tl_permute_reduce`` and the NT GEMM runs on
            ``classifier[1].weight`` WHERE IT LIES (1.2 GB at 128 x 400: a re-packed copy is right for frozen weights only),
            split-K, bias and LeakyReLU behind it; the activations a1 are kept;
  loss      ``tl_linear_rows(act=1)`` then ``tl_ce_scores_loss``: dz with respect to the pre-sigmoid output, the fc2 bias
            gradient, loss sum / count / confusion matrix ADDED to device words read once per epoch;
  head      ``tl_head_bwd`` (LeakyReLU' off the stored a1) gives da1, db1 (and dW2 when dense); dfeat = da1 . W1 is ONE read of
            W1 by the TN GEMM (A = da1^T); it is permuted back into the last stage's gradient rows (pad rows / columns zero) and
            ``tl_dropout_scale_at`` with the forward's seed is dropout's backward;
  trunk     per stage, last to first, ``stage_wgrad`` then ``stage_dgrad``; then the first stage's weight gradient;
  update    one ``FusedNAdam``; at B <= ``FusedNAdam.LOWRANK_MAX`` the two Linear weights go as rank-B factors (fc1's 1.2 GB
            gradient is never written), above that dW1 comes from the TN GEMM and dW2 from ``tl_head_bwd``.

Under a process group (``parallel.active()``) every public step takes the GLOBAL batch and works on this rank's rows
(``_classifier_train_engine``, ``_classifier_dp``): the dropout mask is indexed by the element's position in the global batch
(``tl_dropout_scale_at`` - without a process group the shard starts at row 0 and the mask is ``tl_dropout_scale``'s, bit for bit; same
masks for 1 or N ranks), ``grad_scale`` is 1 / B_global, the conv and bias gradients are views of one arena summed by one bucketed
all-reduce, and at B_global <= ``LOWRANK_MAX`` the two Linear weights travel as the gathered factor rows (da1, flat) and
(dz, a1) - fc1's gradient is never reduced and never written.

No host read happens in ``train_batch`` / ``eval_batch``.  There is no CPU fallback and no fallback to autograd."""
from __future__ import annotations

import torch
import torch.nn as nn

from ._classifier_train_engine import SUPPORTED, ClassifierTrainEngine, check_common, refuse
from ._conv_stack import ConvStack
from ._launch import r4
from ._lib import EPI_LRELU, EPI_MASK, EPI_STORE, LOAD_DIRECT, ptr


def _stage_defs(model):
    """([(C_out, taps, pooled)], [index of each Conv2d in ``feature_extractor``])"""
    defs, at = [], []
    for i, m in enumerate(model.feature_extractor):
        if isinstance(m, nn.Conv2d):
            defs.append([m.out_channels, m.kernel_size[0], False])
            at.append(i)
        elif isinstance(m, nn.MaxPool2d):
            defs[-1][2] = True
    return [tuple(d) for d in defs], at


def check_supported(model) -> None:
    """Raise ``ValueError`` (stating the supported set) unless ``model`` can be trained by ``CnnClassifierTrainEngine``."""
    from .models.deep_classifiers import CNNClassifier
    if not isinstance(model, CNNClassifier):
        refuse(f"model {type(model).__name__}")
    hidden = model.classifier[1].out_features
    check_common(model, [m.negative_slope for m in list(model.feature_extractor) + list(model.classifier)
                         if isinstance(m, nn.LeakyReLU)], float(model.feature_extractor[-1].p),
                 also=[(hidden % 4 != 0, f"hidden width {hidden}")])


class _Head:
    """Buffers of the two Linear layers for one batch size."""

    def __init__(self, B: int, N: int, H: int, K: int, dev):
        f32 = dict(dtype=torch.float32, device=dev)
        self.flat = torch.empty(B, K, **f32)            # the feature map in torch's flatten order
        self.a1 = torch.empty(B, H, **f32)
        self.da1 = torch.empty(B, H, **f32)
        self.ldt = (B + 31) // 32 * 32
        self.da1t = torch.empty(H, self.ldt, **f32)     # da1^T, columns B .. ldt - 1 zero: the A operand of dfeat = da1 . W1
        self.scores = torch.empty(B, N, **f32)
        self.dz = torch.zeros(B, r4(N), **f32)
        self.pred = torch.empty(B, dtype=torch.int64, device=dev)


class CnnClassifierTrainEngine(ClassifierTrainEngine, ConvStack):
    head_bias = "classifier.3.bias"

    def __init__(self, model, learning_rate: float = 0.0005, weight_decay: float = 0.0):
        check_supported(model)
        stage_defs, conv_at = _stage_defs(model)
        n_electrodes, n_timepoints, slope = model._hip_cfg
        # an un-pooled stage keeps the row stride r4(C_out) (ConvStack: ld5); this stack has one, mid-stack
        flat_widths = {r4(d[0]) for d in stage_defs[1:] if not d[2]}
        if len(flat_widths) > 1:
            raise ValueError(f"un-pooled conv stages of different widths {sorted(flat_widths)}: {SUPPORTED}")
        super().__init__(n_electrodes, n_timepoints, stage_defs, slope, flat_widths.pop() if flat_widths else stage_defs[-1][0])
        self.STAGE_NAMES = {st.idx: f"feature_extractor.{conv_at[st.idx - 1]}" for st in self.stages}
        self.name1 = f"feature_extractor.{conv_at[0]}"
        self.fc1, self.fc2 = model.classifier[1], model.classifier[3]
        self.hidden = int(self.fc1.out_features)
        last = self.stages[-1]
        self.c_last, self.tp_last = last.cout, last.tp_out
        self.ld_last = last.cout if last.pool else self.ld5
        self.K = self.c_last * self.C * self.lat
        if self.K != self.fc1.in_features:
            raise ValueError(f"classifier[1] takes {self.fc1.in_features} features, the conv stack gives {self.K}")
        self.p_drop = float(model.feature_extractor[-1].p)
        self.input_shape = (self.C, self.T)
        # the two Linear weights get a dense buffer on demand; the backward finishes the others last layer first
        self._setup_training(model, learning_rate, weight_decay, lowrank_names=("classifier.1.weight", "classifier.3.weight"),
                             arena_order=[k for k, _ in model.named_parameters()][::-1])
        self._eye = None

    # ------------------------------------------------------------------ stack shape
    def _v43(self, st) -> bool:
        # the V-form input gradient reads LeakyReLU' of the stage's input from 1-bit sign planes, which only a pooling epilogue
        # writes: a stage behind an un-pooled one runs on the direct kernels (which read the mask off the stored rows)
        return super()._v43(st) and (st.idx == 2 or self.stages[st.idx - 3].pool)

    # ------------------------------------------------------------------ plumbing
    def _make_workspace(self, B: int, dev) -> _Head:
        return _Head(B, self.N, self.hidden, self.K, dev)

    @property
    def _heads(self):
        """{B: the head buffers of batch ``B`` on the engine's device}: a read-only view of the workspace cache (the test
        helpers read the kept fc1 activations ``_heads[B].a1`` of the last step)."""
        return {B: ws for (B, dev), ws in self._workspaces.items() if dev == self.device}

    # ------------------------------------------------------------------ forward
    def _forward(self, x: torch.Tensor, dropout: bool) -> _Head:
        B = x.shape[0]
        self._alloc(B, x.device)
        ws = self._workspace(B, x.device)
        prm = self.params
        self.generation += 1
        self.conv1_forward(x, prm[self.name1 + ".weight"].data, prm[self.name1 + ".bias"].data)
        for st in self.stages:
            name = self.STAGE_NAMES[st.idx]
            self.stage_forward(st, prm[name + ".weight"].data, prm[name + ".bias"].data)
        feat = self.P[self.stages[-1].idx]                       # [S * tp_last][ld_last]
        self.last_seed = 0
        if dropout and self.p_drop > 0.0:
            self.last_seed = self._step_seed()
            self._drop(feat)
        # torch's flatten of (B, ch, t, c): column ch * lat * C + t * C + c  <-  row (b * C + c) * tp + t, column ch
        lat, Cn, tp, ld = self.lat, self.C, self.tp_last, self.ld_last
        self._permute(feat, ws.flat, (B, self.c_last, lat, Cn), (Cn * tp * ld, 1, ld, tp * ld))
        H, K = self.hidden, self.K
        w1, b1 = self.fc1.weight.data, self.fc1.bias.data
        tiles = ((B + 127) // 128) * ((H + 127) // 128)
        sk = self._splitk(tiles, (K + 31) // 32, 1024)
        kw = dict(A=ptr(ws.flat), Bw=ptr(w1), M=B, A_rows=B, N=H, K=K, lda=K, ldb=K, ldo=H, loader=LOAD_DIRECT)
        if sk > 1:
            slab = torch.empty(sk, B, H, dtype=torch.float32, device=x.device)
            self._nt(tag="fc1_fwd", out=ptr(slab), epilogue=EPI_STORE, splitk=sk, slab_stride=B * H, **kw)
            self._call(None, "tl_splitk_bias_lrelu", ptr(slab), ptr(b1), ptr(ws.a1), sk, B * H, H, self.slope)
        else:
            self._nt(tag="fc1_fwd", bias=ptr(b1), out=ptr(ws.a1), epilogue=EPI_LRELU, slope=self.slope, **kw)
        self._call(None, "tl_linear_rows", ptr(ws.a1), ptr(self.fc2.weight.data), ptr(self.fc2.bias.data), ptr(ws.scores), B, H,
                   self.N, H, 1)
        return ws

    def _drop(self, rows: torch.Tensor) -> None:
        """Dropout (forward and backward alike) on the last stage's rows [(b * C + c) * tp + t][ld] with ``last_seed``; a shard
        that starts at global row b0 draws its rows of the single-process mask (b0 = 0: ``tl_dropout_scale``'s, bit for bit)."""
        index0 = self._plan.row0 * self.C * self.tp_last * self.ld_last
        self._call(None, "tl_dropout_scale_at", ptr(rows), rows.numel(), self.p_drop, self.last_seed, index0)

    # ------------------------------------------------------------------ backward
    def _backward(self, ws: _Head, B: int, dense: bool) -> None:
        """Every gradient of the step from ``ws.dz``: dense ones into ``self.grads``, the two Linear weights as factors in
        ``self.last_lowrank`` unless ``dense``."""
        self._alloc_bwd()
        prm = self.params
        H, K, N = self.hidden, self.K, self.N
        f32 = dict(dtype=torch.float32, device=self._dev)
        w1, w2 = self.fc1.weight.data, self.fc2.weight.data
        self._call(None, "tl_head_bwd", ptr(ws.dz), ptr(ws.a1), ptr(w2), ptr(ws.da1), ptr(self.grads["classifier.1.bias"]),
                   ptr(self._dense("classifier.3.weight")) if dense else None, B, H, N, ws.dz.shape[1], 2, self.slope)
        self.last_lowrank = {}
        if dense:
            self._tn(tag="fc1_wgrad", A=ptr(ws.da1), B=ptr(ws.flat), slab=ptr(self._dense("classifier.1.weight")), Krows=B,
                     A_rows=B, B_rows=B, Mdim=H, Ndim=K, lda=H, ldb=K, ldc=K, loader=LOAD_DIRECT)
        else:
            self.last_lowrank = {"classifier.1.weight": (ws.da1, ws.flat), "classifier.3.weight": (ws.dz[:, :N], ws.a1)}
        # dfeat (B, K) = da1 . W1: the TN GEMM reduces over the 1024 rows of W1 as stored, A = da1^T (pad columns zero)
        ldt = ws.ldt
        self._permute(ws.da1, ws.da1t, (1, 1, H, ldt), (0, 0, 1, H), (1, 1, H, B))
        slab, sk = self._tn_stored("fc1_dgrad", ws.da1t, ldt, w1, H, K)
        # ... summed over the splits and scattered into the last stage's gradient rows [(b * C + c) * tp + t][ch]; the source
        # limits leave the pad rows (t >= lat) and pad columns zero
        last = self.stages[-1]
        G = self.G[last.idx]
        lat, Cn, tp, ld = self.lat, self.C, self.tp_last, self.ld_last
        dfeat = torch.empty_like(G)
        self._permute(slab, dfeat, (B, Cn, tp, ld), (K, 1, Cn, lat * Cn), (B, Cn, lat, self.c_last), nz=sk, zs=ldt * K)
        # G[idx] is the gradient at the stage's pre-activation (the stage above applies LeakyReLU' in its MASK epilogue); the last
        # stage has no stage above, so the MASK epilogue runs here on the one-tap NT GEMM against the identity (exact: x * 1 + 0;
        # 2 * rows * 256^2 FLOPs, 1e-3 of the trunk) with the stored feature map as the sign source - a kept element keeps its
        # sign through dropout, a dropped one is zeroed below whatever its mask
        if self._eye is None or self._eye.device != G.device:
            self._eye = torch.eye(ld, dtype=torch.float32, device=G.device)
        feat = self.P[last.idx]
        self._nt(tag="feat_mask", A=ptr(dfeat), Bw=ptr(self._eye), aux=ptr(feat), out=ptr(G), M=G.shape[0], A_rows=G.shape[0],
                 N=ld, K=ld, lda=ld, ldb=ld, ldo=ld, ldaux=ld, loader=LOAD_DIRECT, epilogue=EPI_MASK, slope=self.slope)
        if self.last_seed:           # dropout's backward: same index, same keep decision, same 1 / (1 - p)
            self._drop(G)
        part = None
        for st in reversed(self.stages):
            name = self.STAGE_NAMES[st.idx]
            self.stage_wgrad(st, self.grads[name + ".weight"], self.grads[name + ".bias"])
            part = self.stage_dgrad(st, prm[name + ".weight"].data)
        if part is None:
            S = self.S
            nblk = int(min(2048, S))
            part = torch.empty(nblk, (self.k1 + 1) * self.c1, **f32)
            self._call(None, "tl_conv1_wgrad", ptr(self._x), ptr(self.G[1]), ptr(self.bits[1]), ptr(part), nblk, S, self.T,
                       self.k1, self.c1, self.tp1, self.tout1)
        self._reduce_c1_partials(part, self.grads[self.name1 + ".weight"], self.grads[self.name1 + ".bias"])

    def _lowrank_wire(self, ws: _Head):
        return {"classifier.3.weight": ws.dz}                # dz travels at its stored width (the factor is its first N columns)
