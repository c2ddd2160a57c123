"""Forward-only HIP path of ``CNNClassifier`` (reference models/deep_classifiers.py:62-99,115-119).

The feature extractor is the same shared-weight (3,1) conv + LeakyReLU (+ (2,1) max-pool) pattern as
the synthesis model's ECoG block, so it runs on the same kernels (``tl_conv1_fwd`` and the fp32-MFMA
``tl_gemm_nt_window``) in the same channels-last, sequence-major layout; the two Linear layers are NT
GEMMs on re-packed weights.  Used when the classifier is called without autograd on CUDA tensors -
which is how the synthesis trainer uses it (reference models/synthesis_trainer.py:207-210: the
outputs are arg-maxed and the classifiers are never updated)."""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Tuple

import torch

from . import _kernels, _lib
from ._conv_stack import ConvStack
from ._launch import launch_nt, r4
from ._lib import EPI_LRELU, EPI_POOL, EPI_POOLV, EPI_STORE, LOAD_DIRECT, LOAD_V, check, ptr


def _cached(packed: dict, key: str, param: torch.Tensor, build):
    """Packed copies of the (usually frozen) classifier weights in ``packed``, rebuilt when the parameter changes."""
    ver = (param._version, param.data_ptr())
    hit = packed.get(key)
    if hit is None or hit[0] != ver:
        hit = packed[key] = (ver, build())
    return hit[1]


class CnnClassifierEngine(ConvStack):
    F63_CAPABLE = False        # this engine enqueues its stages itself (F(6,3) prefix, then F(4,3) V form / direct kernels)

    def __init__(self, n_electrodes: int, n_timepoints: int, stage_defs, hidden: int, n_classes: int,
                 negative_slope: float):
        super().__init__(n_electrodes, n_timepoints, stage_defs, negative_slope, stage_defs[-1][0])
        self.fuse_c1 = False       # forward only: no first-stage weight gradient, conv1 writes raw rows (tl_conv1_fwd)
        self.hidden = hidden
        self.n_classes = n_classes
        last = self.stages[-1]
        self.c_last = last.cout
        self.tp_last = last.tp_out
        self.ld_last = last.cout if last.pool else self.ld5
        self.kflat_cls = n_electrodes * self.tp_last * self.ld_last
        self._packed: Dict[str, Tuple[int, torch.Tensor]] = {}
        # Round 5: the leading pooled 3-tap stages on the F(6,3) V-form kernels of the synthesis stack (tonal_wino63.hip: conv1
        # writes V1 in hex form, every stage but the last writes the next stage's V from its forward epilogue, the last one
        # pooled rows in this engine's own row geometry through out_tp) - forward only.  n63 = how many stages after the first
        # run that way (0: none - TONAL_KERNELS wino != 6, or a shape the kernels do not take).
        self.n63, self.tp63 = self._plan63(stage_defs, n_timepoints)

    def _plan63(self, stage_defs, T):
        if _kernels.get("wino") != "6":
            return 0, []
        c1, k1, p1 = stage_defs[0]
        if not (p1 and 1 <= k1 <= 3 and c1 in (128, 256, 512, 1024) and T >= 2 * self.tout1 + 2 and T * 4 <= 64 * 1024):
            return 0, []
        n, cin = 0, c1
        for st in self.stages:
            if not (st.k == 3 and st.pool and cin % 128 == 0 and st.cout % 64 == 0 and cin >= 40 and st.tout >= 1):
                break
            n, cin = n + 1, st.cout
        n = min(n, 3)
        if n == 0:
            return 0, []
        unit = 6 << (n - 1)                                  # every stage but the last: Tp % 12 == 0, halved by its pool
        tp = (self.tout1 + unit - 1) // unit * unit
        tps = []
        for _ in range(n):
            tps.append(tp)
            tp //= 2
        return n, tps

    def _forward63(self, convs, x, S, T):
        """Stages 1 .. 1 + n63 on the F(6,3) kernels; leaves the pooled rows of stage 1 + n63 in self.P (row geometry of this
        engine) and returns the number of conv layers consumed."""
        lib, st_ = self.lib, self._stream()
        zi = lambda *sh: torch.zeros(*sh, dtype=torch.int32, device=x.device)
        buf = self._bits63
        w1, b1 = convs[0]
        tp1 = self.tp63[0]
        V = self._v_hex_buffer(self.V, 1, S * tp1, self.c1)
        if 1 not in buf:
            buf[1] = zi(S * tp1, self.c1 // 32)
        check(lib.tl_conv1_fwd_v6(ptr(x), ptr(w1.reshape(self.c1, self.k1).contiguous()), ptr(b1), None, ptr(V),
                                  ptr(buf[1]), None, S, T, self.k1, self.c1, tp1, self.tout1, self.slope, st_), "tl_conv1_fwd_v6")
        tile_rows = self._nt63_rows()
        for i in range(self.n63):
            st, (w, b) = self.stages[i], convs[1 + i]
            tp_in = self.tp63[i]
            last = i == self.n63 - 1
            wp = self._cached(f"conv{st.idx}w63", w, lambda w=w: self._pack_wino63(w, True))
            rows_in = S * tp_in
            if st.idx not in buf:
                buf[st.idx] = zi(S * (st.tp_out if last else tp_in // 2), st.cout // 32)
            kw = dict(A=ptr(V), A_rows=V.shape[0], lda=V.shape[2], loader=LOAD_V, Bw=ptr(wp), bias=ptr(b), M=rows_in, N=st.cout,
                      K=st.cin, ldb=st.cin, J=3, row_shift=0, Tp=tp_in, slope=self.slope, obits=ptr(buf[st.idx]),
                      ld_obits=st.cout // 32, Tvalid=2 * st.tout)
            if last:
                dst = self.P[st.idx]
                self._nt(fn="tl_conv3_wino63v_nt", out=ptr(dst), ldo=dst.shape[1], epilogue=EPI_POOL, out_tp=st.tp_out, **kw)
            else:
                rows_out = S * (tp_in // 2)
                ntm = -(-rows_in // tile_rows)
                Vn = self._v_hex_buffer(self.V, st.idx, rows_out, st.cout)
                halo = self._halo_buffer(st.idx, ntm, st.cout)
                self._nt(fn="tl_conv3_wino63v_nt", out=None, ldo=st.cout, epilogue=EPI_POOLV, vout=ptr(Vn), vhalo=ptr(halo),
                         vout_quads=Vn.shape[0], ld_vout=Vn.shape[2], **kw)
                check(lib.tl_wino63_v_fixup(ptr(Vn), ptr(halo), rows_out // 6, ntm, tp_in // 2, st.cout, Vn.shape[2], st_),
                      "tl_wino63_v_fixup")
                V = Vn
        return 1 + self.n63

    def _alloc_rows(self):
        # forward only: every stage keeps its raw rows (each transforms its own input), no sign bits
        S, dev = self.S, self._dev
        z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
        zi = lambda *s: torch.zeros(*s, dtype=torch.int32, device=dev)
        self.P = {1: z(S * self.tp1, self.c1)}
        self.bits = {1: zi(S * self.tp1, self.c1 // 32)}
        self.sbits = {}
        self._bits63 = {}          # arg-max bits of the F(6,3) prefix (its own row geometry, tp63)
        for st in self.stages:
            rows = S * st.tp_out
            self.P[st.idx] = z(rows, st.cout if st.pool else r4(st.cout))
            if st.pool:
                self.bits[st.idx] = zi(rows, st.cout // 32)

    def _cached(self, key, param, build):
        return _cached(self._packed, key, param, build)

    def forward_scores(self, convs: List[Tuple[torch.Tensor, torch.Tensor]], fc1, fc2, x: torch.Tensor,
                       p_drop: float = 0.0, seed: int = 0) -> torch.Tensor:
        """``p_drop`` > 0: the module's ``nn.Dropout`` after the last pool (reference :81) is active - applied in place on
        the feature map by ``tl_dropout_scale`` (counter-hash stream, ``seed``), so train-mode classifiers stay on HIP."""
        B, Cn, T = x.shape
        if Cn != self.C or T != self.T:
            raise ValueError(f"expected input (B, {self.C}, {self.T}), got {tuple(x.shape)}")
        x = x.contiguous().float()
        dev = x.device
        self._alloc(B, dev)
        lib, st_ = self.lib, self._stream()
        S = self.S
        done = 1
        if self.n63:
            done = self._forward63(convs, x, S, T)
        else:
            self.conv1_forward(x, *convs[0])
        for st, (w, b) in list(zip(self.stages, convs[1:]))[done - 1:]:
            # pooled 3-tap stages the F(4,3) V form covers: one transform pass over the stage's input, then the transform-free
            # kernel of the synthesis engine (half the direct form's MFMA work); everything else on the direct MFMA kernel
            v43 = self._v43(st)
            if v43:
                wp = self._cached(f"conv{st.idx}w43", w, lambda w=w: self._pack_wino43(w, True))
            else:
                wp = self._cached(f"conv{st.idx}", w, lambda w=w, st=st: self._pack_conv(w, st.cin, False))
            src, dst = self.P[st.idx - 1], self.P[st.idx]
            kw = dict(A=ptr(src), Bw=ptr(wp), bias=ptr(b), out=ptr(dst), M=S * st.tp_in, A_rows=src.shape[0],
                      N=st.cout, K=st.cin, lda=src.shape[1], ldb=st.cin, ldo=dst.shape[1], J=st.k, row_shift=0,
                      Tp=st.tp_in, slope=self.slope, loader=LOAD_DIRECT)
            if st.pool:
                kw.update(epilogue=EPI_POOL, obits=ptr(self.bits[st.idx]), ld_obits=st.cout // 32, Tvalid=2 * st.tout)
            else:
                kw.update(epilogue=EPI_LRELU, Tvalid=st.tout)
            if v43:
                V = self._input_transform(st)
                kw.update(A=ptr(V), A_rows=V.shape[0], lda=V.shape[2], loader=LOAD_V)
            self._nt(fn="tl_conv3_wino43v_nt" if v43 else "tl_gemm_nt_window", **kw)
        feat = self.P[self.stages[-1].idx]                       # [S*tp_last][ld_last] == [B][kflat_cls]
        if p_drop > 0.0:
            check(lib.tl_dropout_scale(ptr(feat), feat.numel(), float(p_drop), int(seed), st_), "tl_dropout_scale")
        w_fc1, b_fc1 = fc1
        lat, latC = self.lat, self.lat * self.C

        def pack_fc1():
            dst = torch.empty(self.hidden, self.kflat_cls, dtype=torch.float32, device=dev)
            # torch flatten of (B, ch, t, c): index ch*lat*C + t*C + c  ->  ours (c*Tp + t)*ld + ch
            self._permute(w_fc1, dst, (self.hidden, self.C, self.tp_last, self.ld_last),
                          (self.c_last * latC, 1, self.C, latC), (self.hidden, self.C, lat, self.c_last))
            return dst
        wp1 = self._cached("fc1", w_fc1, pack_fc1)
        f32 = dict(dtype=torch.float32, device=dev)
        nkc = (self.kflat_cls + 31) // 32
        tiles = ((B + 127) // 128) * ((self.hidden + 127) // 128)
        sk = self._splitk(tiles, nkc, 1024)
        if sk > 1:
            slab = torch.empty(sk, B, self.hidden, **f32)
            self._nt(A=ptr(feat), Bw=ptr(wp1), out=ptr(slab), M=B, A_rows=B, N=self.hidden, K=self.kflat_cls,
                     lda=self.kflat_cls, ldb=self.kflat_cls, ldo=self.hidden, loader=LOAD_DIRECT, epilogue=EPI_STORE,
                     splitk=sk, slab_stride=B * self.hidden)
            a1 = torch.empty(B, self.hidden, **f32)             # split-K sum + bias + LeakyReLU in one launch
            check(lib.tl_splitk_bias_lrelu(ptr(slab), ptr(b_fc1), ptr(a1), sk, B * self.hidden, self.hidden, float(self.slope), st_),
                  "tl_splitk_bias_lrelu")
        else:
            a1 = torch.empty(B, self.hidden, **f32)
            self._nt(A=ptr(feat), Bw=ptr(wp1), bias=ptr(b_fc1), out=ptr(a1), M=B, A_rows=B, N=self.hidden,
                     K=self.kflat_cls, lda=self.kflat_cls, ldb=self.kflat_cls, ldo=self.hidden, loader=LOAD_DIRECT,
                     epilogue=EPI_LRELU, slope=self.slope)
        w_fc2, b_fc2 = fc2
        out = torch.empty(B, self.n_classes, **f32)
        if self.n_classes <= 64 and self.hidden % 4 == 0:          # output layer + sigmoid in one launch
            check(lib.tl_linear_rows(ptr(a1), ptr(w_fc2.contiguous()), ptr(b_fc2), ptr(out), B, self.hidden, self.n_classes,
                                     self.hidden, 1, st_), "tl_linear_rows")
            return out
        self._nt(A=ptr(a1), Bw=ptr(w_fc2.contiguous()), bias=ptr(b_fc2), out=ptr(out), M=B, A_rows=B,
                 N=self.n_classes, K=self.hidden, lda=self.hidden, ldb=self.hidden, ldo=self.n_classes,
                 loader=LOAD_DIRECT, epilogue=EPI_STORE)
        return torch.sigmoid(out)


class LstmInferEngine:
    """Last hidden state of a one-layer ``nn.LSTM(batch_first=True)`` with zero initial state, forward only -
    the two LSTMs of ``CNNRNNClassifier`` (reference models/deep_classifiers.py:230-233, 263-264, 294-296,
    316-318), which the synthesis trainer runs once per train step without gradients.

    Two phases:
      1. the input projection of EVERY time step in one fp32-MFMA GEMM:  Xp = X W_ih^T + (b_ih + b_hh)   (B*T rows);
      2. per time step ONE fused launch - h_{t-1} W_hh^T on the matrix cores (W_hh, 10 MB for hidden 800, streams from L2)
         and the cell update in its epilogue - all T steps enqueued by one C call (``tl_lstm_infer_seq_fused``).
    The sequence is latency bound (T dependent steps); one launch per step.  Hidden and input widths
    that are not multiples of 4 are zero-padded in the packed weights (a padded unit has i = f = o = 1/2,
    g = 0, so its c and h stay exactly 0 and feed nothing)."""

    def __init__(self, in_dim: int, hidden: int):
        self.lib = _lib.load()
        self.in_dim, self.H = in_dim, hidden
        self.Kp, self.Hp = r4(in_dim), (hidden + 7) // 8 * 8
        self._packed = None

    def _weights(self, w_ih, w_hh, b_ih, b_hh):
        ver = tuple((t._version, t.data_ptr()) for t in (w_ih, w_hh, b_ih, b_hh))
        if self._packed is None or self._packed[0] != ver:
            H, Hp, Kp, dev = self.H, self.Hp, self.Kp, w_hh.device
            wi = torch.zeros(4, Hp, Kp, dtype=torch.float32, device=dev)
            wi[:, :H, :self.in_dim] = w_ih.detach().float().view(4, H, self.in_dim)
            wh = torch.zeros(4, Hp, Hp, dtype=torch.float32, device=dev)
            wh[:, :H, :H] = w_hh.detach().float().view(4, H, H)
            bs = torch.zeros(4, Hp, dtype=torch.float32, device=dev)
            bs[:, :H] = (b_ih.detach().float() + b_hh.detach().float()).view(4, H)
            whp = wh.permute(1, 0, 2).contiguous().view(4 * Hp, Hp)      # unit-major: row 4 u + g
            self._packed = (ver, wi.view(4 * Hp, Kp), wh.view(4 * Hp, Hp), bs.view(4 * Hp), whp)
        return self._packed[1:]

    @torch.no_grad()
    def last_hidden(self, x_seq: torch.Tensor, w_ih, w_hh, b_ih, b_hh) -> torch.Tensor:
        """x_seq (B, T, in_dim) -> h_T (B, hidden)."""
        B, T, D = x_seq.shape
        if D != self.in_dim:
            raise ValueError(f"expected input width {self.in_dim}, got {D}")
        dev = x_seq.device
        wi, wh, bs, whp = self._weights(w_ih, w_hh, b_ih, b_hh)
        H, Hp, Kp = self.H, self.Hp, self.Kp
        f32 = dict(dtype=torch.float32, device=dev)
        x = x_seq.float()
        if Kp != D:
            xp_in = torch.zeros(B, T, Kp, **f32)
            xp_in[:, :, :D] = x
            x = xp_in
        x = x.contiguous()
        rows = B * T
        xp = torch.empty(rows, 4 * Hp, **f32)
        # phase 1: every step's input projection + both biases
        launch_nt(self.lib, A=ptr(x), Bw=ptr(wi), bias=ptr(bs), out=ptr(xp), M=rows, A_rows=rows, N=4 * Hp, K=Kp,
                  lda=Kp, ldb=Kp, ldo=4 * Hp, Tvalid=1, loader=LOAD_DIRECT, epilogue=EPI_STORE)
        h = torch.empty(B, Hp, **f32)
        c = torch.empty(B, Hp, **f32)
        h2 = torch.empty(B, Hp, **f32)
        in_b = C.c_int(0)
        check(self.lib.tl_lstm_infer_seq_fused(ptr(xp), T * 4 * Hp, ptr(whp), ptr(h), ptr(h2), ptr(c), B, Hp, T,
                                               C.byref(in_b), torch.cuda.current_stream().cuda_stream),
              "tl_lstm_infer_seq_fused")
        h = h2 if in_b.value else h
        return h[:, :H] if Hp != H else h


class CnnRnnConvEngine:
    """Convolutional trunk of ``CNNRNNClassifier`` (reference models/deep_classifiers.py:230-259, 294-312)
    on the HIP kernels, forward only: the two (7,1) conv + LeakyReLU + (2,1) max-pool branches
    (``tl_conv1_fwd``, C_in = 1), the width-wise concatenation, the two 7-tap convolutions
    1024 -> 512 -> 256 with LeakyReLU (``tl_gemm_nt_window``, J = 7) and the (3,1) max-pool.  The two
    LSTMs and the output layer stay library calls of the owning module.

    Layout as everywhere else: one *sequence* per (batch element, width column), rows = time,
    channels last; the LSTM branch comes first in the width order, as ``torch.cat((x1, x), dim=3)``."""

    K = 7

    def __init__(self, input_channels: int, input_length: int, lstm_dim: int, negative_slope: float):
        self.lib = _lib.load()
        self.C, self.T = input_channels, input_length
        self.w1 = lstm_dim // input_length
        self.W = self.w1 + input_channels
        self.slope = float(negative_slope)
        self.t1 = (input_length - self.K + 1) // 2           # after conv (7,1) + pool (2,1)
        self.ta = self.t1 - self.K + 1                        # after the 1024 -> 512 convolution
        self.tb = self.ta - self.K + 1                        # after the 512 -> 256 convolution
        self.tq = self.tb // 3                                # after pool (3,1)
        if self.tq < 1:
            raise ValueError("input_length too small for the CNN-RNN convolution stack")
        # 7-tap stack: "wino63" (default since round 5) three F(6,3) segments summed in the transform domain by ONE launch of
        # the V-form NT kernel of the synthesis stack (tl_conv7_wino63v_nt: segment 2 re-reads V0 one hex on, so only two
        # transformed arrays exist); "direct" the 7-tap window GEMM (72.8 ms for the CNN-RNN forward at C5, batch 64, against
        # 46 ms).  The segmented F(4,3) forms of rounds 2-4 were retired in round 6
        _kernels.validate()
        self.conv7_form = _kernels.conv7_forward()
        # rows per sequence: whole hexes for the F(6,3) form, whole quads for the others
        self.Tp = (self.t1 + 5) // 6 * 6 if self.conv7_form == "wino63" else (self.t1 + 3) // 4 * 4
        self._packed: Dict[str, Tuple[tuple, torch.Tensor]] = {}
        self._B = None

    def _cached(self, key, param, build):
        return _cached(self._packed, key, param, build)

    def _alloc(self, B: int, dev):
        if self._B == B and self._dev == dev:
            return
        self._B, self._dev = B, dev
        z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
        zi = lambda *s: torch.zeros(*s, dtype=torch.int32, device=dev)
        rows = B * self.W * self.Tp
        # + 8 rows: the segmented convolution reads up to 6 rows past the last row it is asked about
        self.P, self.Y1, self.Y2 = z(rows + 8, 1024), z(rows + 8, 512), z(rows, 256)
        # sequences are stored branch-major - all LSTM-branch columns of all batch elements, then all electrode
        # columns - so both first-stage convolutions write straight into P (the stack is per sequence; only the
        # final feature map needs the reference's (batch, width) order)
        nb = B * self.w1 * self.Tp
        self.Pb, self.Pa = self.P[:nb], self.P[nb:rows]
        self.bits_a, self.bits_b = zi(B * self.C * self.Tp, 32), zi(B * self.w1 * self.Tp, 32)
        self.V7 = None
        if self.conv7_form == "wino63":
            # V0 / V1 of a 7-tap layer's input (hex transforms of the rows and of the rows shifted by 3, pair layout, whole
            # 128-hex tiles + one pair: the third segment reads one hex past a tile); shared by the two layers (1024, then 512
            # channels: the second fits into the first's storage)
            nh_pad = (rows // 6 + 2 + 127) // 128 * 128
            self.V7 = (z(nh_pad, 8, 1024), z(nh_pad, 8, 1024))

    def _conv7(self, src, w, b, dst, cin, cout, key, rows):
        """dst[r] = lrelu(sum_j w[:, :, j] src[r + j] + b) for r < rows; src holds rows + 8 rows."""
        st_ = torch.cuda.current_stream().cuda_stream
        if self.conv7_form == "wino63" and cin % 8 == 0 and cout % 32 == 0:
            nhex = rows // 6
            V0 = self.V7[0].view(-1)[: self.V7[0].shape[0] * 8 * cin].view(-1, 8, cin)
            V1 = self.V7[1].view(-1)[: self.V7[1].shape[0] * 8 * cin].view(-1, 8, cin)
            # rows from the valid length of THIS layer's input on enter as zeros (they only feed rows nobody reads)
            tvalid = self.t1 if cin == 1024 else self.ta
            if V0.shape[2] != self.V7[0].shape[2]:
                # a narrower layer re-views the storage: its pad hexes (whole pairs behind the last hex, which the third
                # segment and the rows past M of the last tile read) overlay the wider layer's transform data - zero them, as
                # tl_conv7_wino63v_nt's contract says ("zero hexes appended"); ~2 MB per array
                h0 = (nhex + 1) // 2 * 2
                V0[h0:].zero_()
                V1[h0:].zero_()
            check(self.lib.tl_wino63_xform2(ptr(src), ptr(V0), ptr(V1), rows, self.Tp, tvalid, cin, src.shape[1], cin, st_),
                  "tl_wino63_xform2")

            def pack63():
                wp = torch.empty(3 * cin // 8, 8, cout, 8, dtype=torch.float32, device=w.device)
                check(self.lib.tl_wino63_weights7(ptr(w.detach().reshape(cout, cin, self.K).contiguous()), ptr(wp), cout, cin,
                                                  self.K, st_), "tl_wino63_weights7")
                return wp
            wp = self._cached(key + "wino63", w, pack63)
            launch_nt(self.lib, fn="tl_conv7_wino63v_nt", A=ptr(V0), aux=ptr(V1), A_rows=V0.shape[0], lda=cin, Bw=ptr(wp),
                      bias=ptr(b.detach()), out=ptr(dst), M=rows, N=cout, K=cin, ldb=3 * cin, ldo=dst.shape[1], J=self.K,
                      row_shift=0, Tp=self.Tp, Tvalid=self.Tp, slope=self.slope, loader=LOAD_V, epilogue=EPI_LRELU)
            return
        # "direct" (or a width the F(6,3) form does not take): the 7-tap window GEMM, which reads rows + 8 input rows
        if src.shape[0] < rows + 8:
            raise RuntimeError("conv7: the input buffer is shorter than the rows the 7-tap window reads")
        wp = self._cached(key + "direct", w, lambda: w.detach().reshape(cout, cin, self.K).permute(2, 0, 1).contiguous())   # [J][O][I]
        launch_nt(self.lib, A=ptr(src), Bw=ptr(wp), bias=ptr(b.detach()), out=ptr(dst), M=rows, A_rows=rows + 8, N=cout, K=cin,
                  lda=cin, ldb=cin, ldo=cout, J=self.K, row_shift=0, Tp=self.Tp, Tvalid=self.Tp, slope=self.slope,
                  loader=LOAD_DIRECT, epilogue=EPI_LRELU)

    @torch.no_grad()
    def linear(self, a: torch.Tensor, w: torch.Tensor, b: torch.Tensor, sigmoid: bool = False) -> torch.Tensor:
        """a (B, K) @ w (N, K)^T + b (the classifier's output layer; ``sigmoid``: the activation it ends with)."""
        a = a.contiguous().float()
        B, K = a.shape
        if K % 4 != 0:
            raise ValueError("linear: the feature width must be a multiple of 4")
        N = w.shape[0]
        out = torch.empty(B, N, dtype=torch.float32, device=a.device)
        if N <= 64:
            check(self.lib.tl_linear_rows(ptr(a), ptr(w.contiguous()), ptr(b), ptr(out), B, K, N, K, int(sigmoid),
                                          torch.cuda.current_stream().cuda_stream), "tl_linear_rows")
            return out
        launch_nt(self.lib, A=ptr(a), Bw=ptr(w.contiguous()), bias=ptr(b), out=ptr(out), M=B, A_rows=B, N=N, K=K, lda=K,
                  ldb=K, ldo=N, Tvalid=1, loader=LOAD_DIRECT, epilogue=EPI_STORE)
        return torch.sigmoid(out) if sigmoid else out

    @torch.no_grad()
    def features(self, x: torch.Tensor, h1: torch.Tensor, block1, block2, conv3a, conv3b, p_drop: float = 0.0,
                 seed: int = 0) -> torch.Tensor:
        """x (B, C, T), h1 (B, lstm_dim); blockN / conv3x = (weight, bias).  Returns the tensor the
        reference feeds to its second LSTM: (B, t', 256 * W) - a raw view of the contiguous
        (B, 256, t', W) activation (reference :315)."""
        B = x.shape[0]
        dev = x.device
        self._alloc(B, dev)
        lib, st_ = self.lib, torch.cuda.current_stream().cuda_stream
        xa = x.contiguous().float()                                                   # (B*C, T) sequences
        xb = h1.float().reshape(B, self.T, self.w1).permute(0, 2, 1).contiguous()     # column j: h1[b, t*w1 + j]
        for seqs, n, (w, b), P, bits in ((xa, B * self.C, block1, self.Pa, self.bits_a),
                                         (xb, B * self.w1, block2, self.Pb, self.bits_b)):
            check(lib.tl_conv1_fwd(ptr(seqs), ptr(w.detach().reshape(1024, self.K).contiguous()), ptr(b.detach()), ptr(P),
                                   ptr(bits), None, n, self.T, self.K, 1024, self.Tp, self.t1, self.slope, st_),
                  "tl_conv1_fwd")
        rows = B * self.W * self.Tp
        self._conv7(self.P, conv3a[0], conv3a[1], self.Y1, 1024, 512, "conv3a", rows)
        self._conv7(self.Y1, conv3b[0], conv3b[1], self.Y2, 512, 256, "conv3b", rows)
        y = self.Y2.view(B * self.W, self.Tp, 256)[:, :3 * self.tq]
        y = y.reshape(B * self.W, self.tq, 3, 256).amax(dim=2).contiguous()            # MaxPool (3,1), per sequence
        if p_drop > 0.0:                   # the block's nn.Dropout (reference :258), train mode: in place on (seq, t', 256)
            check(lib.tl_dropout_scale(ptr(y), y.numel(), float(p_drop), int(seed), st_), "tl_dropout_scale")
        nb = B * self.w1
        y = torch.cat((y[:nb].view(B, self.w1, self.tq, 256), y[nb:].view(B, self.C, self.tq, 256)), dim=1)
        f = y.permute(0, 3, 2, 1).contiguous()                                         # (B, 256, t', W)
        return f.view(B, self.tq, -1)
