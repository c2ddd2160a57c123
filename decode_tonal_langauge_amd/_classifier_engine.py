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
from ._launch import LaunchTimers, PackCache, launch_nt, permute_reduce, r4
from ._lib import EPI_LRELU, EPI_POOL, EPI_POOLV, EPI_STORE, LOAD_DIRECT, LOAD_V, check, ptr


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
        self.packs = PackCache()
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
            wp = self.packs.get(f"conv{st.idx}w63", w, lambda w=w: self._pack_wino63(w, True))
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
                wp = self.packs.get(f"conv{st.idx}w43", w, lambda w=w: self._pack_wino43(w, True))
            else:
                wp = self.packs.get(f"conv{st.idx}", w, lambda w=w, st=st: self._pack_conv(w, st.cin, False))
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
        wp1 = self.packs.get("fc1", w_fc1, pack_fc1)
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
        self.packs = PackCache()

    def _weights(self, *weights):
        """(W_ih as the projection GEMM reads it, b_ih + b_hh, W_hh unit-major) of (w_ih, w_hh, b_ih, b_hh)."""
        def build():
            w = [t.detach().float().contiguous() for t in weights]
            wi, bs, whp, _ = lstm_pack_buffers(self.in_dim, self.H, w[0].device)
            lstm_pack(self.lib, (wi, bs, whp, None), *w)
            return (w[0] if wi is None else wi), bs, whp
        return self.packs.get("lstm", weights, build)

    @torch.no_grad()
    def last_hidden(self, x_seq: torch.Tensor, w_ih, w_hh, b_ih, b_hh) -> torch.Tensor:
        """x_seq (B, T, in_dim) -> h_T (B, hidden)."""
        B, T, D = x_seq.shape
        if D != self.in_dim:
            raise ValueError(f"expected input width {self.in_dim}, got {D}")
        dev = x_seq.device
        wi, bs, whp = self._weights(w_ih, w_hh, b_ih, b_hh)
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


def lstm_pack_buffers(in_dim: int, hidden: int, dev, train: bool = False) -> tuple:
    """Zeroed (wi, bs, whp, whT) for ``lstm_pack``: hidden padded to 8, the input width to 4.  ``wi`` is None when nothing is
    padded (``weight_ih_l0`` is used where it lies); ``whT`` (W_hh^T: row u', column g Hp + u) only for training."""
    Kp, Hp = r4(in_dim), (hidden + 7) // 8 * 8
    z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
    padded = Kp != in_dim or Hp != hidden
    return z(4 * Hp, Kp) if padded else None, z(4 * Hp), z(4 * Hp, Hp), z(Hp, 4 * Hp) if train else None


def lstm_pack(lib, packs: tuple, w_ih, w_hh, b_ih, b_hh) -> None:
    """Fill ``packs`` from the (fp32, contiguous) weights of one ``nn.LSTM``: W_ih gate-major (row g Hp + u), the bias sum the
    same, W_hh unit-major (row 4 u + g); pad rows and columns stay zero."""
    wi, bs, whp, whT = packs
    H, D, Hp, Kp = w_hh.shape[1], w_ih.shape[1], whp.shape[1], r4(w_ih.shape[1])
    if wi is not None:
        permute_reduce(lib, w_ih, wi, (1, 4, Hp, Kp), (0, H * D, D, 1), (1, 4, H, D))
    permute_reduce(lib, w_hh, whp, (1, Hp, 4, Hp), (0, H, H * H, 1), (1, H, 4, H))
    if whT is not None:
        permute_reduce(lib, w_hh, whT, (1, Hp, 4, Hp), (0, 1, H * H, H), (1, H, 4, H))
    bs.view(4, Hp)[:, :H] = (b_ih + b_hh).view(4, H)


K7 = 7            # taps of every convolution of CNNRNNClassifier
C_FIRST, C_A, C_B = 1024, 512, 256


def geometry(n_channels: int, n_timepoints: int, lstm_dim: int) -> Dict[str, int]:
    """Row counts of the CNN-RNN trunk: after block 1 / 2 (t1), the two 7-tap stages (ta, tb), the (3,1) pool (tq)."""
    t1 = (n_timepoints - K7 + 1) // 2
    ta = t1 - K7 + 1
    tb = ta - K7 + 1
    w1 = lstm_dim // n_timepoints
    return dict(t1=t1, ta=ta, tb=tb, tq=tb // 3, w1=w1, W=w1 + n_channels)


class Conv7Trunk:
    """What the forward-only trunk of ``CNNRNNClassifier`` (below) and the training one (``_cnnrnn_classifier_train_engine``)
    share: the geometry, the rows per sequence, the transform buffers and the forward of a 7-tap stage.  The host class brings
    ``lib``, ``slope``, ``_nt(tag=, fn=, **fields)`` and ``_tick(tag)``."""

    def _trunk_geometry(self, n_channels: int, n_timepoints: int, lstm_dim: int) -> None:
        geo = geometry(n_channels, n_timepoints, lstm_dim)
        self.t1, self.ta, self.tb, self.tq, self.w1, self.W = (geo[k] for k in ("t1", "ta", "tb", "tq", "w1", "W"))
        # 7-tap stack: "wino63" (default since round 5) three F(6,3) segments summed in the transform domain by ONE launch of
        # the V-form NT kernel of the synthesis stack (tl_conv7_wino63v_nt: segment 2 re-reads V0 one hex on, so only two
        # transformed arrays exist); "direct" the 7-tap window GEMM (72.8 ms for the CNN-RNN forward at C5, batch 64, against
        # 46 ms).  The segmented F(4,3) forms of rounds 2-4 were retired in round 6
        _kernels.validate()
        self.conv7_form = _kernels.conv7_forward()
        # rows per sequence: whole hexes for the F(6,3) form, whole quads for the others
        self.Tp = (self.t1 + 5) // 6 * 6 if self.conv7_form == "wino63" else (self.t1 + 3) // 4 * 4
        self.packs = PackCache()

    def _alloc_v7(self, rows: int, extra_hexes: int, dev):
        """V0 / V1 of a 7-tap layer's input (hex transforms of the rows and of the rows shifted by 3, pair layout), shared by
        the two layers (1024, then 512 channels: the second fits into the first's storage): whole 128-hex tiles of the NT
        kernel behind ``extra_hexes`` - 2: its third segment reads one hex past a tile; 6 under conv7=wino63bwd: also whole
        6-hex K-steps of the weight-gradient kernel, which the rounding does not imply (253 hexes: 256 < 258)."""
        if self.conv7_form != "wino63":
            return None
        nh_pad = (rows // 6 + extra_hexes + 127) // 128 * 128
        return tuple(torch.zeros(nh_pad, 8, C_FIRST, dtype=torch.float32, device=dev) for _ in range(2))

    def _hex_view(self, buf: torch.Tensor, c: int, nhex: int) -> torch.Tensor:
        """``buf`` (hexes, 8, wider) re-viewed for ``c`` channels; the pad hexes of a narrower view (whole pairs behind the last
        hex, which the third segment and the rows past M of the last tile read) overlay the wider layer's data: zeroed, as
        tl_conv7_wino63v_nt's contract says ("zero hexes appended") - with an odd ``nhex`` the second hex of the last pair too,
        which no transform kernel writes (the weight-gradient kernel reads whole 6-hex K-steps of BOTH operands: a stale hex
        of Y against a stale hex of V is a term of the sum)."""
        if c == buf.shape[2]:
            return buf
        v = buf.view(-1)[: buf.shape[0] * 8 * c].view(-1, 8, c)
        v[(nhex + 1) // 2 * 2:].zero_()
        if nhex % 2:
            v.view(-1, c // 8, 8, 2, 8)[nhex // 2, :, :, 1].zero_()          # (pair layout: [hex / 2][c / 8][8][hex % 2][8])
        return v

    def _conv7(self, key, src, w, b, dst, cin, cout, tvalid, rows, tag=None) -> None:
        """dst[r] = lrelu(sum_j w[:, :, j] src[r + j] + b) for r < rows; src holds rows + 8 rows, of which ``tvalid`` per
        sequence are data (the rows behind them enter as zeros: they only feed rows nobody reads).  ``w`` carries the
        parameter's version counter (the parameter or its ``.detach()``): the weight pack ``key`` follows it."""
        st_ = torch.cuda.current_stream().cuda_stream
        w7 = w.reshape(cout, cin, K7)
        if self.conv7_form == "wino63":
            V0, V1 = (self._hex_view(v, cin, rows // 6) for v in self.V7)
            ev = self._tick(tag and tag + "_xform")
            check(self.lib.tl_wino63_xform2(ptr(src), ptr(V0), ptr(V1), rows, self.Tp, tvalid, cin, src.shape[1], cin, st_),
                  "tl_wino63_xform2")
            wp = self.packs.get(key, w, lambda: torch.empty(3 * cin // 8, 8, cout, 8, dtype=torch.float32, device=w.device),
                                into=lambda wp: check(self.lib.tl_wino63_weights7(ptr(w7), ptr(wp), cout, cin, K7, st_),
                                                      "tl_wino63_weights7"))
            if ev:
                ev[1].record()
            self._nt(tag=tag, fn="tl_conv7_wino63v_nt", A=ptr(V0), aux=ptr(V1), A_rows=V0.shape[0], lda=cin, Bw=ptr(wp),
                     bias=ptr(b), out=ptr(dst), M=rows, N=cout, K=cin, ldb=3 * cin, ldo=dst.shape[1], J=K7, row_shift=0,
                     Tp=self.Tp, Tvalid=self.Tp, slope=self.slope, loader=LOAD_V, epilogue=EPI_LRELU)
            return
        # "direct": the 7-tap window GEMM, which reads rows + 8 input rows
        if src.shape[0] < rows + 8:
            raise RuntimeError("conv7: the input buffer is shorter than the rows the 7-tap window reads")
        wp = self.packs.get(key, w, lambda: torch.empty(K7, cout, cin, dtype=torch.float32, device=w.device),     # [J][O][I]
                            into=lambda wp: permute_reduce(self.lib, w7, wp, (1, K7, cout, cin), (0, 1, cin * K7, K7)))
        self._nt(tag=tag, A=ptr(src), Bw=ptr(wp), bias=ptr(b), out=ptr(dst), M=rows, A_rows=rows + 8, N=cout, K=cin, lda=cin,
                 ldb=cin, ldo=cout, J=K7, row_shift=0, Tp=self.Tp, Tvalid=self.Tp, slope=self.slope, loader=LOAD_DIRECT,
                 epilogue=EPI_LRELU)


class CnnRnnConvEngine(Conv7Trunk, LaunchTimers):
    """Convolutional trunk of ``CNNRNNClassifier`` (reference models/deep_classifiers.py:230-259, 294-312)
    on the HIP kernels, forward only: the two (7,1) conv + LeakyReLU + (2,1) max-pool branches
    (``tl_conv1_fwd``, C_in = 1), the width-wise concatenation, the two 7-tap convolutions
    1024 -> 512 -> 256 with LeakyReLU (``Conv7Trunk._conv7``) and the (3,1) max-pool.  The two
    LSTMs and the output layer stay library calls of the owning module.

    Layout as everywhere else: one *sequence* per (batch element, width column), rows = time,
    channels last; the LSTM branch comes first in the width order, as ``torch.cat((x1, x), dim=3)``."""

    K = K7

    def __init__(self, input_channels: int, input_length: int, lstm_dim: int, negative_slope: float):
        self.lib = _lib.load()
        self.C, self.T = input_channels, input_length
        self.slope = float(negative_slope)
        self._trunk_geometry(input_channels, input_length, lstm_dim)
        if self.tq < 1:
            raise ValueError("input_length too small for the CNN-RNN convolution stack")
        self._B = None

    def _nt(self, tag=None, fn="tl_gemm_nt_window", **fields):
        launch_nt(self.lib, fn, **fields)

    def _alloc(self, B: int, dev):
        if self._B == B and self._dev == dev:
            return
        if self._B is not None and self._dev != dev:
            self.packs = PackCache()           # (a stale pack is refilled where it lies: on the device left behind)
        self._B, self._dev = B, dev
        z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
        zi = lambda *s: torch.zeros(*s, dtype=torch.int32, device=dev)
        rows = B * self.W * self.Tp
        # + 8 rows: the segmented convolution reads up to 6 rows past the last row it is asked about
        self.P, self.Y1, self.Y2 = z(rows + 8, C_FIRST), z(rows + 8, C_A), z(rows, C_B)
        # sequences are stored branch-major - all LSTM-branch columns of all batch elements, then all electrode
        # columns - so both first-stage convolutions write straight into P (the stack is per sequence; only the
        # final feature map needs the reference's (batch, width) order)
        nb = B * self.w1 * self.Tp
        self.Pb, self.Pa = self.P[:nb], self.P[nb:rows]
        self.bits_a, self.bits_b = zi(B * self.C * self.Tp, 32), zi(B * self.w1 * self.Tp, 32)
        self.V7 = self._alloc_v7(rows, 2, dev)

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
        self._conv7("conv3a", self.P, *conv3a, self.Y1, C_FIRST, C_A, self.t1, rows)
        self._conv7("conv3b", self.Y1, *conv3b, self.Y2, C_A, C_B, self.ta, rows)
        y = self.Y2.view(B * self.W, self.Tp, 256)[:, :3 * self.tq]
        y = y.reshape(B * self.W, self.tq, 3, 256).amax(dim=2).contiguous()            # MaxPool (3,1), per sequence
        if p_drop > 0.0:                   # the block's nn.Dropout (reference :258), train mode: in place on (seq, t', 256)
            check(lib.tl_dropout_scale(ptr(y), y.numel(), float(p_drop), int(seed), st_), "tl_dropout_scale")
        nb = B * self.w1
        y = torch.cat((y[:nb].view(B, self.w1, self.tq, 256), y[nb:].view(B, self.C, self.tq, 256)), dim=1)
        f = y.permute(0, 3, 2, 1).contiguous()                                         # (B, 256, t', W)
        return f.view(B, self.tq, -1)
