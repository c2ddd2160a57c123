"""Training of ``CNNRNNClassifier`` on the HIP path (the loop of reference models/classifier_trainer.py:22-177 around the model
of models/deep_classifiers.py:158-343: ``nn.CrossEntropyLoss`` on the model's SIGMOID outputs, ``loss.backward()``, ``NAdam``
with two decay groups, a confusion matrix per epoch).

One train step of a batch (B, C, T); t1 = (T - 6) // 2, ta = t1 - 6, tb = ta - 6, t' = tb // 3, w1 = lstm_dim / T, W = w1 + C:
  lstm1     input projection of all T steps by one NT GEMM, then ``tl_lstm_train_seq`` (one fused launch per step) keeping
            hs / cs / the activated gates of every step, rows time-major (t * B + b); h1 = hs[T - 1];
  trunk     two ``tl_conv1_fwd`` launches (7 taps) write one branch-major row matrix - the B * w1 sequences cut from h1, then
            the B * C electrode sequences - the two 7-tap stages run in the form ``TONAL_KERNELS conv7=`` selects (``wino63``:
            ``tl_conv7_wino63v_nt``, or ``direct``), ``tl_pool3_fwd_shard`` pools (3,1), applies the dropout mask and writes lstm2's
            input matrix in the reference's raw-view order, rows time-major;
  lstm2     as lstm1 over the t' steps; ``tl_linear_rows(act=1)`` on its last hidden state gives the sigmoid scores;
  loss      ``tl_ce_scores_loss``: dz with respect to the pre-sigmoid output, the output bias gradient, loss sum / count /
            confusion matrix ADDED to device words read once per epoch;
  backward  ``tl_head_bwd`` -> dh2; ``tl_lstm_bptt_seq`` (one fused launch per step) -> dgates and their transposed copy;
            dW_hh, dW_ih, db and dX2 = dgates . W_ih (ONE read of the weight, A = dgates^T) on the TN GEMM; ``tl_pool3_bwd_shard``;
            ``ConvStack.stage_wgrad`` / ``stage_dgrad`` for the two 7-tap stages (direct kernels, J = 7; under ``TONAL_KERNELS
            conv7=wino63bwd`` both passes on F(6,3): ``_wgrad7`` / ``_dgrad7``); ``tl_conv1_wgrad`` per branch; ``tl_conv1_dgrad``
            on the LSTM branch -> dh1; lstm1's BPTT and GEMMs;
  update    one ``FusedNAdam`` over dense gradients (an LSTM weight gradient has rank T * B: no low-rank form).

Under a process group (``parallel.active()``) every public step takes the GLOBAL batch and works on this rank's rows
(``_classifier_train_engine``, ``_classifier_dp``): the dropout mask of the (3,1) pool is indexed by the sequence's number in the
global batch's branch-major order (``tl_pool3_fwd_shard`` / ``tl_pool3_bwd_shard`` - without a process group the shard is the whole
batch and they are ``tl_pool3_fwd`` / ``tl_pool3_bwd``, bit for bit; same masks for 1 or N ranks), ``grad_scale`` is 1 / B_global, and all
gradients - views of one arena - are summed by one bucketed all-reduce (an LSTM weight gradient has no low-rank form, and
``output.weight`` is 4 KB).

No host read happens in ``train_batch`` / ``eval_batch``.  There is no CPU fallback and no fallback to autograd."""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn

from . import _kernels
from ._classifier_engine import C_A, C_B, C_FIRST, K7, Conv7Trunk, geometry, lstm_pack, lstm_pack_buffers
from ._classifier_train_engine import SUPPORTED, ClassifierTrainEngine, check_common, refuse
from ._conv_stack import ConvStack
from ._launch import r4
from ._lib import EPI_MASK, EPI_STORE, LOAD_DIRECT, LOAD_V, LOAD_Y, check, ptr

def lstm2_input_index(b: int, ch: int, s: int, w: int, B: int, tq: int, W: int, channels: int = C_B):
    """(row, column) of element (b, ch, s, w) of the contiguous (B, channels, tq, W) activation in lstm2's input matrix as this
    engine keeps it: the reference's raw ``view(B, tq, -1)`` (:315) with rows time-major, row = step * B + b."""
    f = (ch * tq + s) * W + w
    return (f // (channels * W)) * B + b, f % (channels * W)


def check_supported(model) -> None:
    """Raise ``ValueError`` (stating the supported set) unless ``model`` can be trained by ``CnnRnnClassifierTrainEngine``."""
    from .models.deep_classifiers import CNNRNNClassifier
    if not isinstance(model, CNNRNNClassifier):
        refuse(f"model {type(model).__name__}")
    tq = geometry(model.input_channels, model.input_length, model.lstm1.hidden_size)["tq"]
    check_common(model, [m.negative_slope for m in model.modules() if isinstance(m, nn.LeakyReLU)], float(model.conv_block3[5].p),
                 also=[(tq < 1, f"input_length {model.input_length} (no row is left behind the (3,1) pool)")])


class _Lstm:
    """The kept state of one ``nn.LSTM`` for one batch size, rows time-major (t * B + b), and the packs of its weights the last
    forward ran on (``_lstm_pack``)."""

    def __init__(self, name: str, mod: nn.LSTM, T: int, B: int, dev, want_dx: bool):
        f32 = dict(dtype=torch.float32, device=dev)
        self.name, self.T, self.B = name, T, B
        self.in_dim, self.H = mod.input_size, mod.hidden_size
        self.Kp, self.Hp = r4(self.in_dim), (self.H + 7) // 8 * 8
        H4, rows = 4 * self.Hp, T * B
        self.wi = self.bs = self.whp = self.whT = None
        self.xp = torch.empty(rows, H4, **f32)
        self.hs = torch.empty(rows, self.Hp, **f32)
        self.cs = torch.empty(rows, self.Hp, **f32)
        self.act = torch.empty(rows, H4, **f32)
        self.dgates = torch.empty(rows, H4, **f32)
        self.dc = torch.empty(B, self.Hp, **f32)
        self.dh_last = torch.zeros(B, self.Hp, **f32)                            # pad columns stay zero
        self.ldt = (rows + 31) // 32 * 32
        self.dgT = torch.zeros(H4, self.ldt, **f32) if want_dx else None         # pad columns stay zero
        self.colsum = torch.empty(H4, **f32)

    def h_last(self) -> torch.Tensor:
        return self.hs[(self.T - 1) * self.B:]


class _Ws:
    """Buffers outside the conv stack for one batch size."""

    def __init__(self, eng, B: int, dev):
        f32 = dict(dtype=torch.float32, device=dev)
        m = eng.model
        self.l1 = _Lstm("lstm1", m.lstm1, eng.T, B, dev, False)
        self.l2 = _Lstm("lstm2", m.lstm2, eng.tq, B, dev, True)
        self.x1 = torch.zeros(eng.T * B, self.l1.Kp, **f32)                      # lstm1's input rows (t * B + b, electrode)
        self.xb = torch.empty(B * eng.w1, eng.T, **f32)                          # block 2's sequences cut from h1
        self.X2 = torch.empty(eng.tq * B, C_B * eng.W, **f32)                    # lstm2's input rows
        self.dX2 = torch.empty(eng.tq * B, C_B * eng.W, **f32)
        self.scores = torch.empty(B, eng.N, **f32)
        self.dz = torch.zeros(B, r4(eng.N), **f32)
        self.pred = torch.empty(B, dtype=torch.int64, device=dev)


class CnnRnnClassifierTrainEngine(ClassifierTrainEngine, Conv7Trunk, ConvStack):
    F63_CAPABLE = False        # (the 3-tap F(6,3) stack does not apply: every stage here has 7 taps)
    UPDATE_TAG = "update"
    head_bias = "output.bias"

    def __init__(self, model, learning_rate: float = 0.0005, weight_decay: float = 0.0):
        check_supported(model)
        Cn, T = int(model.input_channels), int(model.input_length)
        slope = float(model.conv_pool_block1[1].negative_slope)
        self._trunk_geometry(Cn, T, model.lstm1.hidden_size)
        self.Cn = Cn
        # the conv stack sees W sequences per batch element (branch-major: see _forward); three 7-tap stages, the first pooled
        super().__init__(self.W, T, [(C_FIRST, K7, True), (C_A, K7, False), (C_B, K7, False)], slope, C_B)
        assert self.t1 == self.tout1 and self.stages[1].tout == self.tb
        # conv7=wino63bwd: the weight and input gradients of the two wide stages on F(6,3) too (_wgrad7 / _dgrad7; needs whole
        # 256-channel tiles of C_in for the transform-free weight-gradient kernel - the model's widths have them)
        self.conv7_bwd = _kernels.get("conv7") == "wino63bwd"
        self.tp1 = self.Tp
        for st in self.stages:
            st.tp_in = st.tp_out = self.Tp
        self.fuse_c1 = False
        self.STAGE_NAMES = {2: "conv_block3.0", 3: "conv_block3.2"}
        self.p_drop = float(model.conv_block3[5].p)
        self.input_shape = (Cn, T)
        if model.lstm2.hidden_size % 8 != 0 or model.lstm2.input_size != C_B * self.W:
            raise ValueError(f"lstm2 ({model.lstm2.input_size} -> {model.lstm2.hidden_size}): {SUPPORTED}")
        # every gradient is dense (an LSTM weight gradient has rank T * B); the order the backward finishes them in
        names = [k for k, _ in model.named_parameters()]
        self._setup_training(model, learning_rate, weight_decay, arena_order=(
            ["output.bias", "output.weight"] + [k for k in names if k.startswith("lstm2.")]
            + [k for k in names if k.startswith("conv_block3.")][::-1]
            + [k for k in names if k.startswith("conv_pool_block")] + [k for k in names if k.startswith("lstm1.")]))

    # ------------------------------------------------------------------ buffers
    def _alloc_rows(self):
        S, dev, Tp = self.S, self._dev, self.Tp
        z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
        zi = lambda *s: torch.zeros(*s, dtype=torch.int32, device=dev)
        rows = S * Tp
        # + 8 rows: a 7-tap window reads up to 6 rows past the last row it is asked about
        self.P = {1: z(rows + 8, C_FIRST), 2: z(rows + 8, C_A), 3: z(rows, C_B)}
        self.bits = {1: zi(rows, C_FIRST // 32)}
        self.sbits = {1: zi(rows, C_FIRST // 32)}
        self.V7 = self._alloc_v7(rows, 6 if self.conv7_bwd else 2, dev)
        self._v7_of = None                 # (generation, tag) of the transform V7 holds
        self.Y7 = self.D7 = None           # conv7=wino63bwd: Y = A dz, and V0 / V1 of the moved dz (allocated with G)

    def _alloc_bwd(self) -> bool:
        if self.G is not None:
            return False
        z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=self._dev)
        rows = self.S * self.Tp
        self.G = {1: z(rows, C_FIRST), 2: z(rows, C_A), 3: z(rows, C_B)}
        if self.conv7_bwd:
            # three hex arrays of the wider gradient (C_A channels; stage 3 re-views them): 32 x rows x C_A / 6 bytes each
            nh_pad = self.V7[0].shape[0]
            self.Y7 = z(nh_pad, 8, C_A)
            self.D7 = (z(nh_pad, 8, C_A), z(nh_pad, 8, C_A))
        return True

    def _make_workspace(self, B: int, dev) -> _Ws:
        return _Ws(self, B, dev)

    # ------------------------------------------------------------------ LSTM
    def _lstm_pack(self, l: _Lstm) -> None:
        """The packs of the CURRENT weights: once per weight version (a train step moves it, ``eval_batch`` does not)."""
        w = tuple(self.params[f"{l.name}.{n}"].detach() for n in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0"))
        l.wi, l.bs, l.whp, l.whT = self.packs.get(l.name, w, lambda: lstm_pack_buffers(l.in_dim, l.H, w[0].device, train=True),
                                                  into=lambda packs: lstm_pack(self.lib, packs, *w))

    def _w_ih(self, l: _Lstm) -> torch.Tensor:
        return l.wi if l.wi is not None else self.params[f"{l.name}.weight_ih_l0"].data      # (lstm2: used where it lies)

    def _lstm_forward(self, l: _Lstm, x_rows: torch.Tensor) -> None:
        self._lstm_pack(l)
        rows, H4 = l.T * l.B, 4 * l.Hp
        self._nt(tag=f"{l.name}_xproj", A=ptr(x_rows), Bw=ptr(self._w_ih(l)), bias=ptr(l.bs), out=ptr(l.xp), M=rows, A_rows=rows,
                 N=H4, K=l.Kp, lda=l.Kp, ldb=l.Kp, ldo=H4, Tvalid=1, loader=LOAD_DIRECT, epilogue=EPI_STORE)
        self._call(f"{l.name}_fwd_seq", "tl_lstm_train_seq", ptr(l.xp), H4, l.B * H4, ptr(l.whp), ptr(l.hs), ptr(l.cs),
                   ptr(l.act), l.B, l.Hp, l.T)

    def _colsum_wide(self, M: torch.Tensor, rows: int, ncols: int, dst: torch.Tensor) -> None:
        flat = M.view(-1)
        for c0 in range(0, ncols, 1024):
            nc = min(1024, ncols - c0)
            self._colsum(flat[c0:], rows, nc, ncols, 1, 1, dst[c0:c0 + nc])

    def _tn_reduced(self, tag, A, a_off, Bm, Krows, Mdim, Ndim, lda, ldb, dst, dst_dims, dst_strides) -> None:
        """dst (a 4-d contiguous view given by ``dst_dims``) = the (Mdim, Ndim) product A^T . B read through ``dst_strides``,
        split-K slabs summed on the way; written in place when no split and no re-indexing is needed."""
        f32 = dict(dtype=torch.float32, device=self._dev)
        tiles = ((Mdim + 127) // 128) * ((Ndim + 127) // 128)
        sk = self._splitk(tiles, (Krows + 31) // 32, 1024)
        direct = sk == 1 and dst.numel() == Mdim * Ndim
        slab = dst if direct else torch.empty(sk, Mdim, Ndim, **f32)
        self._tn(tag=tag, A=A.data_ptr() + 4 * a_off, B=ptr(Bm), slab=ptr(slab), Krows=Krows, A_rows=Krows, B_rows=Krows,
                 Mdim=Mdim, Ndim=Ndim, lda=lda, ldb=ldb, ldc=Ndim, loader=LOAD_DIRECT, splitk=sk, slab_stride=Mdim * Ndim)
        if not direct:
            self._permute(slab, dst, dst_dims, dst_strides, nz=sk, zs=Mdim * Ndim)

    def _lstm_backward(self, l: _Lstm, x_rows: torch.Tensor, dx: Optional[torch.Tensor]) -> None:
        """BPTT from ``l.dh_last``; dW_ih, dW_hh, both bias gradients into ``self.grads``; ``dx`` (rows, in_dim) on request."""
        rows, B, T, H, Hp, H4 = l.T * l.B, l.B, l.T, l.H, l.Hp, 4 * l.Hp
        g = self.grads
        self._call(f"{l.name}_bptt_seq", "tl_lstm_bptt_seq", ptr(l.whT), ptr(l.dh_last), ptr(l.act), ptr(l.cs), ptr(l.dc),
                   ptr(l.dgates), ptr(l.dgT), l.ldt, B, Hp, T)
        ghh = g[f"{l.name}.weight_hh_l0"]
        if T > 1:          # dW_hh = dgates[1:]^T . hs[:-1]: a row offset of B between the operands
            self._tn_reduced(f"{l.name}_whh_grad", l.dgates, B * H4, l.hs, (T - 1) * B, H4, Hp, H4, Hp, ghh, (1, 4, H, H),
                             (0, Hp * Hp, Hp, 1))
        else:
            ghh.zero_()
        self._tn_reduced(f"{l.name}_wih_grad", l.dgates, 0, x_rows, rows, H4, l.Kp, H4, l.Kp, g[f"{l.name}.weight_ih_l0"],
                         (1, 4, H, l.in_dim), (0, Hp * l.Kp, l.Kp, 1))
        self._colsum_wide(l.dgates, rows, H4, l.colsum)
        for which in ("bias_ih_l0", "bias_hh_l0"):
            self._permute(l.colsum, g[f"{l.name}.{which}"], (1, 1, 4, H), (0, 0, Hp, 1))
        if dx is None:
            return
        # dx (rows, in) = dgates . W_ih: the TN GEMM reduces over the 4 H rows of the weight as stored, A = dgates^T (pad
        # columns zero) - one read of the weight, no transposed copy
        ldt, K = l.ldt, l.Kp
        slab, sk = self._tn_stored(f"{l.name}_dx", l.dgT, ldt, self._w_ih(l), H4, K)
        self._permute(slab, dx, (1, 1, rows, l.in_dim), (0, 0, K, 1), nz=sk, zs=ldt * K)

    # ------------------------------------------------------------------ the 7-tap stages, forward
    def _conv7(self, tag, src, name, dst, cin, cout, tvalid) -> None:
        """``Conv7Trunk._conv7`` over every row of the stack, timed under ``tag``; V7 then holds this stage's transform."""
        prm = self.params
        super()._conv7(tag, src, prm[name + ".weight"].detach(), prm[name + ".bias"].data, dst, cin, cout, tvalid,
                       self.S * self.Tp, tag=tag)
        self._v7_of = (self.generation, tag)

    # ------------------------------------------------------------------ the 7-tap stages, backward on F(6,3) (conv7=wino63bwd)
    def _wgrad7(self, st, gw: torch.Tensor, gb: torch.Tensor) -> None:
        """dW_j = sum_R dz[R] (x) x[R + j] as three 3-tap F(6,3) weight gradients: taps 3 s .. 3 s + 2 see x shifted by 3 s rows =
        V0(x), V1(x) and V0(x) one hex on (``a_hex``), all against Y = A dz (``tl_wino63_ydz`` of G[idx]); the transform-free
        kernel of the synthesis stack runs them.  V0 / V1 of the stage input are the forward's where V7 still holds them
        (stage 3: the last transform of the forward), else recomputed (stage 2: V7 is one buffer pair for both stages - keeping
        its transform would cost two more arrays of rows x C_FIRST / 6 x 32 bytes; the recompute is timed in ``_wgrad_xform``, the
        split-K sums, the three finalize passes and the scatter into the seven taps in ``_wgrad_reduce``)."""
        S, Tp = self.S, self.Tp
        rows, nhex, cin, cout = S * Tp, S * Tp // 6, st.cin, st.cout
        f32 = dict(dtype=torch.float32, device=self._dev)
        src, Gs = self.P[st.idx - 1], self.G[st.idx]
        tag = f"conv{st.idx}_wgrad"
        fwd_tag = "conv3a_fwd" if st.idx == 2 else "conv3b_fwd"
        kept = self._v7_of == (self.generation, fwd_tag)
        V0, V1 = (self._hex_view(v, cin, nhex) for v in self.V7)
        ev = self._tick(tag + "_xform")
        if not kept:
            check(self.lib.tl_wino63_xform2(ptr(src), ptr(V0), ptr(V1), rows, Tp, st.tin, cin, src.shape[1], cin, self._stream()),
                  "tl_wino63_xform2")
            self._v7_of = (self.generation, fwd_tag)
        Y = self._hex_view(self.Y7, cout, nhex)
        check(self.lib.tl_wino63_ydz(ptr(Gs), ptr(Y), rows, Tp, st.tout, cout, Gs.shape[1], cout, self._stream()), "tl_wino63_ydz")
        if ev:
            ev[1].record()
        sk = self._splitk((cin // 64) * (cout // 64), (rows + 35) // 36, 4096)
        slab = torch.empty(3, sk, 8 * cin, cout, **f32)
        bias_part = torch.empty(sk, cout, **f32)
        ev = self._tick(tag)
        for s, (V, a_hex) in enumerate(((V0, 0), (V1, 0), (V0, 1))):
            self._tn(fn="tl_conv3_wino63v_tn", A=ptr(V), B=ptr(Y), slab=ptr(slab[s]), Krows=rows, A_rows=V.shape[0],
                     B_rows=Y.shape[0], Mdim=cin, Ndim=cout, lda=cin, ldb=cout, ldc=cout, J=3, Tp=Tp, splitk=sk,
                     slab_stride=8 * cin * cout, loader=LOAD_Y, Tvalid=st.tout, a_hex=a_hex,
                     colsum=ptr(bias_part) if s == 0 else None)
        if ev:
            ev[1].record()
        # (slab: 3 sk x 32 cin cout bytes, 1.6 GB at the wider stage of 128 x 400, batch 64 - transient, back in torch's caching
        # allocator behind the step; the direct form's slabs are sk x 28 cin cout bytes, 73 MB there)
        n = 8 * cin * cout
        ev = self._tick(tag + "_reduce")
        red = torch.empty(8 * cin, cout, **f32) if sk > 1 else None
        g3 = torch.empty(cout, cin, 3, **f32)
        gw7 = gw.view(cout, cin, K7)
        for s in range(3):
            if sk > 1:
                self._permute(slab[s], red, (1, 1, 1, n), (0, 0, 0, 1), nz=sk, zs=n)
            check(self.lib.tl_wino63_wgrad_finalize(ptr(red if sk > 1 else slab[s]), ptr(g3), cout, cin, cout, self._stream()),
                  "tl_wino63_wgrad_finalize")
            nt = min(3, K7 - 3 * s)                    # (segment 2: tap 6 alone - its taps 7, 8 do not exist)
            gw7[:, :, 3 * s:3 * s + nt].copy_(g3[:, :, :nt])
        self._permute(bias_part, gb, (1, 1, 1, cout), (0, 0, 0, 1), nz=sk, zs=cout)
        if ev:
            ev[1].record()

    def _dgrad7(self, st, w: torch.Tensor) -> None:
        """G[idx - 1][t] = (sum_j W_j^T dz[t - j]) * LeakyReLU'(input): the forward kernel on dz moved down six rows inside its
        sequence (``tl_wino63_xform2s``: t_out + 6 <= Tp, so no window leaves the sequence) with the taps of the flipped,
        transposed weight; the mask from the sign words under stage 2 (its input came out of a pool), from P[2] under stage 3."""
        S, Tp = self.S, self.Tp
        rows, nhex, cin, cout = S * Tp, S * Tp // 6, st.cin, st.cout
        Gs, out = self.G[st.idx], self.G[st.idx - 1]
        tag = f"conv{st.idx}_dgrad"
        name = self.STAGE_NAMES[st.idx] + ".weight"
        D0, D1 = (self._hex_view(v, cout, nhex) for v in self.D7)
        ev = self._tick(tag + "_xform")
        check(self.lib.tl_wino63_xform2s(ptr(Gs), ptr(D0), ptr(D1), rows, Tp, st.tout, K7 - 1, cout, Gs.shape[1], cout,
                                         self._stream()), "tl_wino63_xform2s")
        def flipped(wp):
            wf = w.reshape(cout, cin, K7).flip(2).permute(1, 0, 2).contiguous()        # (I, O, 7): wf[i][o][j] = w[o][i][6 - j]
            check(self.lib.tl_wino63_weights7(ptr(wf), ptr(wp), cin, cout, K7, self._stream()), "tl_wino63_weights7")
        wp = self.packs.get(tag, self.params[name], into=flipped,
                            build=lambda: torch.empty(3 * cout // 8, 8, cin, 8, dtype=torch.float32, device=w.device))
        if ev:
            ev[1].record()
        kw = dict(auxbits=ptr(self.sbits[1]), ld_auxbits=self.sbits[1].shape[1]) if st.idx == 2 else \
            dict(mask=ptr(self.P[2]), ld_mask=self.P[2].shape[1])
        self._nt(tag=tag, fn="tl_conv7_wino63v_dgrad_nt", A=ptr(D0), aux=ptr(D1), A_rows=D0.shape[0], lda=cout, Bw=ptr(wp),
                 out=ptr(out), M=rows, N=cin, K=cout, ldb=3 * cout, ldo=out.shape[1], J=K7, row_shift=0, Tp=Tp, Tvalid=Tp,
                 slope=self.slope, loader=LOAD_V, epilogue=EPI_MASK, **kw)

    def stage_wgrad(self, st, gw, gb) -> None:
        if self.conv7_bwd:
            return self._wgrad7(st, gw, gb)
        return super().stage_wgrad(st, gw, gb)

    def stage_dgrad(self, st, w):
        if self.conv7_bwd:
            return self._dgrad7(st, w)
        return super().stage_dgrad(st, w)

    # ------------------------------------------------------------------ forward
    def _branches(self, ws: _Ws, B: int):
        """(sequences, count, first row of the stack, parameter prefix) of the two first-stage branches, in storage order:
        the LSTM branch (block 2), then the electrodes (block 1) - the width order of ``torch.cat((x1, x), dim=3)``."""
        nb = B * self.w1
        return ((ws.xb, nb, 0, "conv_pool_block2.0"), (self._x, B * self.Cn, nb * self.Tp, "conv_pool_block1.0"))

    def _forward(self, x: torch.Tensor, dropout: bool) -> _Ws:
        B = x.shape[0]
        self._alloc(B, x.device)
        ws = self._workspace(B, x.device)
        prm = self.params
        self.generation += 1
        self._x = x
        Cn, T, w1, Tp = self.Cn, self.T, self.w1, self.Tp
        # lstm1 over the electrodes: rows (t * B + b), columns the electrodes (pad columns stay zero)
        l1, l2 = ws.l1, ws.l2
        self._permute(x, ws.x1, (1, T, B, l1.Kp), (0, 1, Cn * T, T), (1, T, B, Cn))
        self._lstm_forward(l1, ws.x1)
        # block 2 reads h1 as (B, 1, T, w1): sequence (b, j) holds h1[b][t * w1 + j]
        self._permute(l1.hs, ws.xb, (1, B, w1, T), (0, l1.Hp, 1, w1), src_off=(T - 1) * B * l1.Hp)
        ev = self._tick("conv1_fwd")
        for seqs, n, row0, name in self._branches(ws, B):
            w = prm[name + ".weight"].data.reshape(C_FIRST, K7)
            check(self.lib.tl_conv1_fwd(ptr(seqs), ptr(w), ptr(prm[name + ".bias"].data), ptr(self.P[1][row0:]),
                                        ptr(self.bits[1][row0:]), ptr(self.sbits[1][row0:]), n, T, K7, C_FIRST, Tp, self.t1,
                                        self.slope, self._stream()), "tl_conv1_fwd")
        if ev:
            ev[1].record()
        self._conv7("conv3a_fwd", self.P[1], "conv_block3.0", self.P[2], C_FIRST, C_A, self.t1)
        self._conv7("conv3b_fwd", self.P[2], "conv_block3.2", self.P[3], C_A, C_B, self.ta)
        self.last_seed = 0
        if dropout and self.p_drop > 0.0:
            self.last_seed = self._step_seed()
        self._call("pool3_fwd", "tl_pool3_fwd_shard", ptr(self.P[3]), ptr(ws.X2), B, w1, Cn, C_B, Tp, self.tq, C_B, 1, B,
                   self.p_drop if self.last_seed else 0.0, self.last_seed, self._plan.row0, self._plan.B)
        self._lstm_forward(l2, ws.X2)
        out = self.model.output
        self._call(None, "tl_linear_rows", ptr(l2.h_last()), ptr(out.weight.data), ptr(out.bias.data), ptr(ws.scores), B, l2.Hp,
                   self.N, l2.Hp, 1)
        return ws

    # ------------------------------------------------------------------ backward
    def _backward(self, ws: _Ws, B: int, dense: bool) -> None:
        """Every gradient of the step from ``ws.dz`` into ``self.grads``."""
        self._alloc_bwd()
        prm, g = self.params, self.grads
        l1, l2 = ws.l1, ws.l2
        Cn, T, w1, Tp = self.Cn, self.T, self.w1, self.Tp
        self._call(None, "tl_head_bwd", ptr(ws.dz), ptr(l2.h_last()), ptr(self.model.output.weight.data), ptr(l2.dh_last), None,
                   ptr(g["output.weight"]), B, l2.Hp, self.N, ws.dz.shape[1], 0, self.slope)
        self._lstm_backward(l2, ws.X2, ws.dX2)
        self._call("pool3_bwd", "tl_pool3_bwd_shard", ptr(self.P[3]), ptr(ws.dX2), ptr(self.G[3]), B, w1, Cn, C_B, Tp, self.tq, C_B,
                   C_B, 1, B, self.p_drop if self.last_seed else 0.0, self.last_seed, self.slope, self._plan.row0, self._plan.B)
        for st in reversed(self.stages):
            name = self.STAGE_NAMES[st.idx]
            self.stage_wgrad(st, g[name + ".weight"], g[name + ".bias"])
            self.stage_dgrad(st, prm[name + ".weight"].data)
        f32 = dict(dtype=torch.float32, device=self._dev)
        ev = self._tick("conv1_wgrad")
        for seqs, n, row0, name in self._branches(ws, B):
            nblk = int(min(2048, n))
            part = torch.empty(nblk, (K7 + 1) * C_FIRST, **f32)
            check(self.lib.tl_conv1_wgrad(ptr(seqs), ptr(self.G[1][row0:]), ptr(self.bits[1][row0:]), ptr(part), nblk, n, T, K7,
                                          C_FIRST, Tp, self.t1, self._stream()), "tl_conv1_wgrad")
            self._reduce_c1_partials(part, g[name + ".weight"], g[name + ".bias"])
        if ev:
            ev[1].record()
        # dh1[b][t * w1 + j] = dx of sequence (b, j) at sample t: straight into lstm1's dh_last (pad columns stay zero)
        w2 = prm["conv_pool_block2.0.weight"].data.reshape(C_FIRST, K7)
        self._call("conv1_dgrad", "tl_conv1_dgrad", ptr(self.G[1]), ptr(self.bits[1]), ptr(w2), ptr(l1.dh_last), B * w1, T, K7,
                   C_FIRST, Tp, self.t1, w1, l1.Hp, w1, 1)
        self._lstm_backward(l1, ws.x1, None)
