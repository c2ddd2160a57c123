"""The shared-weight ECoG convolution stack on MI355X: stage geometry (padded row strides per stage), the HBM workspaces
and the three passes of every stage on the three kernel families (Winograd F(6,3) / F(4,3) on pre-transformed operands,
direct-form MFMA).  ``CnnEngine`` (the synthesis model around it) and ``CnnClassifierEngine`` (forward only) build on it.

Data layout: activations are channels-last, sequence-major: one *sequence* is one
(batch element, ECoG channel) pair, ``seq = b*C + c``; a stage's tensor is a row-major matrix
``[seq*Tp + t][channel]`` with ``Tp`` (rows per sequence) padded so every max-pool pair is
row-aligned.  In that layout the (k,1) convolution of the reference
(models/synthesis_models.py:86-105) is a GEMM whose A rows are overlapping windows of the
activation matrix - no im2col copy exists anywhere.
"""
from __future__ import annotations

from typing import List

import torch

from . import _kernels, _lib
from ._launch import LaunchTimers, launch_nt, launch_tn, permute_reduce, r4
from ._lib import (EPI_C1WGRAD, EPI_GY, EPI_LRELU, EPI_MASK, EPI_MASKY, EPI_POOL, EPI_POOLV, LOAD_DIRECT, LOAD_UNPOOL, LOAD_V,
                   LOAD_Y, check, ptr)


class _Stage:
    """One ecog_conv_block stage (conv (k,1) + LeakyReLU [+ MaxPool (2,1)])."""

    def __init__(self, idx, cin, cout, k, pool, tin, tp_in):
        self.idx, self.cin, self.cout, self.k, self.pool = idx, cin, cout, k, pool
        self.tin, self.tp_in = tin, tp_in
        self.tc = tin - k + 1
        self.tout = self.tc // 2 if pool else self.tc
        self.tp_out = tp_in // 2 if pool else tp_in


class ConvStack(LaunchTimers):
    #: the forward-only classifier engine (which walks an F(6,3) prefix in a row geometry of its own) keeps the F(4,3) geometry
    F63_CAPABLE = True

    def __init__(self, n_channels: int, n_timepoints: int, stage_defs, negative_slope: float, conv_channels: int):
        if negative_slope < 0:
            raise ValueError("the MI355X path needs negative_slope >= 0 (max-pool / LeakyReLU are fused)")
        self.lib = _lib.load()
        self.C = n_channels
        self.T = n_timepoints
        self.slope = float(negative_slope)
        # ---- geometry ----
        k1 = stage_defs[0][1]
        npool_after = sum(1 for s in stage_defs[1:] if s[2])
        tc1 = n_timepoints - k1 + 1
        self.k1 = k1
        self.c1 = stage_defs[0][0]
        self.tout1 = tc1 // 2
        if not stage_defs[0][2]:
            raise ValueError("first stage must pool")
        align = 1 << npool_after
        self.tp1 = max(align, (self.tout1 + align - 1) // align * align)
        # wino 6: Winograd F(6,3) on pre-transformed operands for stages 2 and 3 (csrc/tonal_wino63.hip; 8 products per
        # 6 conv rows).  A sequence of stage 2 holds a multiple of 12 rows (hexes of 6 rows, pooled into hexes of stage 3);
        # the pooled output of stage 3 keeps the row stride of the default geometry (tl_nt_params.out_tp), so everything from
        # stage 4 on is unchanged.  Shapes the form does not cover fall back to wino 4 as a whole.
        _kernels.validate()                    # TONAL_KERNELS: unknown keys / values raise here, not on the hot path
        self.wino63 = (self.F63_CAPABLE and _kernels.get("wino") == "6"
                       and self._f63_covers(stage_defs, n_timepoints))
        tp1_default = self.tp1
        if self.wino63:
            self.tp1 = (self.tout1 + 11) // 12 * 12
        # the input gradient of stage 3 writes the operand of stage 2's backward - Y2 = A dz - instead of the gradient rows G2
        # (epilogue 6 of tl_conv3_wino63v_nt): the weight gradient of stage 2 then runs without a transform
        # (tl_conv3_wino63v_tn, loader 3; needs C_in of stage 2 % 256 == 0) and its input gradient on the same Y2 (epilogue 4
        # with row_shift 0, taps of tl_wino63_weights_y); Vd2 is written only under store_p1 (nothing reads it).
        # TONAL_F63_YPROD=0: off (G2 is stored, the weight-gradient kernel un-pools and transforms it itself and writes
        # Vd2, the operand of the input gradient, as stage 3's does)
        self.f63_yprod = (self.wino63 and _kernels.get("f63_yprod") != "0" and stage_defs[0][0] % 256 == 0
                          and self.tp1 >= 12)
        # ... and stage 3's (whose gradient rows no Winograd epilogue produces) from a kernel of its own, tl_wino63_unpool_yvd
        # (f63_yprod 0: its weight-gradient kernel un-pools and transforms G3 itself and writes Vd3)
        self.f63_yprod3 = (self.wino63 and _kernels.get("f63_yprod") != "0" and stage_defs[1][0] % 256 == 0)
        self.stages: List[_Stage] = []
        cin, tin, tp = self.c1, self.tout1, self.tp1
        for i, (cout, k, pool) in enumerate(stage_defs[1:], start=2):
            st = _Stage(i, cin, cout, k, pool, tin, tp)
            if st.tout < 1:
                raise ValueError("n_timepoints too small for the conv stack")
            if self.wino63 and i == 3:
                st.tp_out = tp1_default // 4               # the default geometry's rows per sequence behind stage 3
            self.stages.append(st)
            cin, tin, tp = cout, st.tout, st.tp_out
        self.gy4 = self._gy_applies()          # (fixed here: _alloc_bwd leaves out the gradient rows this path never stores)
        # stage 3 on whole-sequence tiles (f63_seq16; TONAL_KERNELS f63_yprod=vd3 switches it off alone): where its valid conv rows fit 16 hexes but a sequence stores
        # more (the reference shape: 96 rows, 17 hexes), its forward and input-gradient launches compute 16 hexes per sequence
        # (compact-M mode of tl_conv3_wino63v_nt: a lane owns one sequence) and the input gradient runs on Y3, as stage 2's does on
        # Y2 - Vd3 then has no reader: conv4's input gradient writes Y3 only, without halo rows or a fix-up pass.  The weight
        # gradient keeps the stored geometry.
        st3 = self.stages[1] if len(self.stages) >= 2 else None
        self.f63_seq16 = bool(self.wino63 and self.f63_yprod and self.f63_yprod3 and self.gy4
                              and _kernels.get("f63_yprod") == "1" and -(-st3.tc // 6) <= 16 < st3.tp_in // 6)
        self.lat = tin
        self.tp5 = tp
        self.ld5 = r4(conv_channels)
        # Kernels for the pooled 3-tap stages (TONAL_KERNELS wino):
        #   6  default: Winograd F(6,3) on pre-transformed operands for all three passes of stages 2 and 3 where the stack
        #      allows it (_f63_covers; 4/9 of the direct-form MFMA work); the F(4,3) V form below, stage by stage, elsewhere
        #   4  Winograd F(4,3) on pre-transformed operands (tonal_wino43v.hip; 1/2 of the MFMA work): the A/B partner
        #   0  direct-form MFMA kernels (the parity partner, and the fallback for every shape neither V form covers)
        # (the in-loop-transform F(2,3) / F(4,3) kernels of rounds 1-2 were retired in round 6)
        mode = _kernels.get("wino")
        self.wino43 = mode != "0"
        # with V written by the first stage the raw pooled rows P1 (13.4 GB at the north-star shape) have no reader
        # left (the LeakyReLU' mask of the backward pass comes from the 1-bit sign array); store_p1 keeps them anyway - and
        # with them the other operands the default path no longer writes (P2; Vd2 of the f63_yprod form)
        self.store_p1 = _kernels.get("store_p1") == "1"
        # fold the first stage's weight gradient into the stage-2 input-gradient epilogue (Winograd kernels)
        self.fuse_c1 = True                    # (tests clear it to reach the stand-alone tl_conv1_wgrad)
        # test hooks of the F(4,3) V form (no TONAL_KERNELS keys): wino_vout False - forward epilogues write raw rows, every
        # stage transforms its own input; tn_bm 64 / 127 / 128 - force a C_in tile of the weight-gradient kernel (0: auto)
        self.wino_vout = True
        self.tn_bm = 0
        self._gy_A = None      # per-batch / per-device scratch of the NT63 input-gradient paths (_alloc resets both)
        self._vhalo = {}
        self._B = None
        self.generation = 0

    # ------------------------------------------------------------------ buffers
    def _alloc(self, B: int, dev) -> bool:
        """Workspaces of the stack for batch ``B`` on ``dev``; False when they are there already."""
        if self._B == B and self._dev == dev:
            return False
        self._B, self._dev = B, dev
        self.S = B * self.C
        self._v_ready = {}     # V tensors already written by the producing kernel in this forward
        self._gy_A = None      # (per-batch / per-device scratch of the NT63 input-gradient paths: re-created on demand)
        self._vhalo = {}
        self._alloc_rows()
        self.Yt = {}           # F(6,3): Y = A dz of stage idx, written by the input gradient of the stage above (f63_yprod)
        self._y_ready = {}
        self.V = {}            # F(4,3) input transforms of P[idx] (quads, 6, channels) for the stages that read them
        self.Vd = {}           # ... and of the un-pooled dZ of stage idx (the operand of its input-gradient pass; stage 3 on
                               # whole-sequence tiles reads Y3 instead: Vd[3] is then that tensor, no Vd3 exists)
        self._vd_ready = {}
        self.G = None          # gradient workspaces are allocated lazily on the first backward
        return True

    def _alloc_rows(self):
        """Activation rows and pooling bits of every stage (the forward-only classifier keeps a set of its own)."""
        S, dev = self.S, self._dev
        z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
        zi = lambda *s: torch.zeros(*s, dtype=torch.int32, device=dev)
        self.P = {}
        if not (self.wino63 or self._conv1_writes_v()) or self.store_p1:
            self.P[1] = z(S * self.tp1, self.c1)
        self.bits = {1: zi(S * self.tp1, self.c1 // 32)}
        self.sbits = {1: zi(S * self.tp1, self.c1 // 32)}      # "pooled output > 0": the LeakyReLU' mask of backward
        for st in self.stages:
            rows = S * st.tp_out
            ld = st.cout if st.pool else self.ld5
            # raw rows are not stored where the forward epilogue hands the next stage V instead: F(6,3) stage 2 (POOLV), or
            # an F(4,3) stage whose successor reads V - but never F(6,3) stage 3, whose POOL epilogue always writes rows
            no_rows = (self.wino63 and st.idx == 2) or (self._writes_v(st) and not self._f63(st))
            if not no_rows or self.store_p1:
                self.P[st.idx] = z(rows, ld)
            if st.pool:
                self.bits[st.idx] = zi(rows, st.cout // 32)
                self.sbits[st.idx] = zi(rows, st.cout // 32)

    def _alloc_bwd(self) -> bool:
        if self.G is not None:
            return False
        z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=self._dev)
        S = self.S
        self.G = {}
        if not self.wino63 and not (self.fuse_c1 and self._c1_fusable() and self._v43(self.stages[0])):
            self.G[1] = z(S * self.tp1, self.c1)      # otherwise G1 never leaves the stage-2 epilogue
        for st in self.stages:
            # (with f63_yprod G2 is never stored; with the NT63 form of stage 4's input gradient neither is G3)
            if not (self.f63_yprod and st.idx == 2) and not (self.gy4 and st.idx == 3):
                self.G[st.idx] = z(S * st.tp_out, st.cout if st.pool else self.ld5)
        return True

    # ------------------------------------------------------------------ ABI helpers
    def _stream(self):
        return torch.cuda.current_stream().cuda_stream

    def _permute(self, src, dst, dims, strides, *args, **kw):
        permute_reduce(self.lib, src, dst, dims, strides, *args, **kw)

    def _nt(self, tag=None, fn="tl_gemm_nt_window", **kw):
        ev = self._tick(tag)
        launch_nt(self.lib, fn, **kw)
        if ev:
            ev[1].record()

    def _tn(self, tag=None, fn="tl_gemm_tn_window", **kw):
        ev = self._tick(tag)
        launch_tn(self.lib, fn, **kw)
        if ev:
            ev[1].record()

    @staticmethod
    def _splitk(tiles: int, ksteps: int, target: int = 2048) -> int:
        return int(max(1, min(ksteps, (target + tiles - 1) // tiles, 1024)))

    def _tn_stored(self, tag, At, ldt, W, rows, K):
        """A . W on a weight ``W`` (rows, K) as it lies - one read of it, no transposed copy: the TN GEMM reduces over the rows,
        its A operand is ``At`` = A^T (rows, ldt), pad columns zero.  Returns the split-K slabs ``(sk, ldt, K)`` and ``sk``."""
        if ldt <= 32:                # skinny streaming kernel: 512-column tiles, 16-deep K stages
            sk = self._splitk((K + 511) // 512, (rows + 15) // 16, 1024)
        else:
            sk = self._splitk(((ldt + 127) // 128) * ((K + 127) // 128), (rows + 31) // 32, 1024)
        slab = torch.empty(sk, ldt, K, dtype=torch.float32, device=self._dev)
        self._tn(tag=tag, A=ptr(At), B=ptr(W), slab=ptr(slab), Krows=rows, A_rows=rows, B_rows=rows, Mdim=ldt, Ndim=K, lda=ldt,
                 ldb=K, ldc=K, loader=LOAD_DIRECT, splitk=sk, slab_stride=ldt * K)
        return slab, sk

    # ------------------------------------------------------------------ weight packing
    def _pack_conv(self, w, cin_ld, flip_for_dgrad):
        """torch (O, I, J, 1) -> forward pack [J][O][cin_ld] or dgrad pack [J'][I_ld][O_ld] (J flipped)."""
        O, I, J, _ = w.shape
        if not flip_for_dgrad:
            dst = torch.empty(J, O, cin_ld, dtype=torch.float32, device=w.device)
            self._permute(w, dst, (1, J, O, cin_ld), (0, 1, I * J, J), (1, J, O, I))
            return dst
        old = r4(O)
        dst = torch.empty(J, cin_ld, old, dtype=torch.float32, device=w.device)
        # dst[j'][i][o] = w[o][i][J-1-j']
        self._permute(w, dst, (1, J, cin_ld, old), (0, -1, J, I * J), (1, J, I, O), src_off=J - 1)
        return dst

    @staticmethod
    def _f63_covers(stage_defs, T) -> bool:
        """The F(6,3) kernels cover the stack: stages 2 and 3 are pooled 3-tap convolutions with C_in % 128 == 0 and
        C_out % 64 == 0, the first stage has 1..3 taps, one input channel and a width tl_conv1_fwd_v6 takes, and the fused
        first-stage weight gradient can read its sample windows."""
        if len(stage_defs) < 4:
            return False
        (c1, k1, p1), (c2, k2, p2), (c3, k3, p3) = stage_defs[0], stage_defs[1], stage_defs[2]
        tout1 = (T - k1 + 1) // 2
        tout2 = (tout1 - 2) // 2
        tout3 = (tout2 - 2) // 2
        return (p1 and p2 and p3 and k2 == 3 and k3 == 3 and 1 <= k1 <= 3 and c1 in (128, 256, 512, 1024)
                and c2 % 128 == 0 and c3 % 64 == 0 and tout3 >= 1 and T >= 2 * tout1 + 2)

    def _f63(self, st) -> bool:
        return self.wino63 and st.idx in (2, 3)

    def _nt63_rows(self) -> int:
        """conv rows of a row tile of tl_conv3_wino63v_nt: its halo arrays and the fused conv1 gradient's partial sums hold one
        entry per row tile"""
        return int(self.lib.tl_wino63_nt_tile_rows())

    def _v_hex_buffer(self, store, idx, rows, cin):
        """V / Vd of a stage input in hex form: rows / 6 hexes, padded with zero hexes to whole 128-hex tiles (and by at
        least 24: the weight-gradient kernel prefetches three 6-hex K-steps past the last one it uses)."""
        nh = rows // 6
        nh_pad = (nh + 24 + 127) // 128 * 128
        if self.f63_seq16 and ((store is self.V and idx == 2) or (store is self.Yt and idx == 3)):
            # the operands of stage 3's whole-sequence launches: every row tile reads 8 stored sequences (a last tile that
            # holds fewer reads zero hexes); nothing more where the sequence count is a multiple of 8
            nh_pad = max(nh_pad, (-(-self.S // 8) * 8 * (self.stages[1].tp_in // 6) + 127) // 128 * 128)
        V = store.get(idx)
        if V is None or V.shape[0] != nh_pad or V.shape[1] != 8 or V.shape[2] != cin:
            V = store[idx] = torch.zeros(nh_pad, 8, cin, dtype=torch.float32, device=self._dev)
        return V

    def _vd3_buffer(self, rows, cin):
        """Vd3 as a buffer of its own.  On whole-sequence tiles ``Vd[3]`` names Y3 - the operand stage 3's input gradient reads -
        and no Vd3 is allocated; a producer that does write Vd3 (store_p1, the stand-alone tl_wino63_unpool_yvd) gets a real one."""
        if self.Vd.get(3) is not None and self.Vd[3] is self.Yt.get(3):
            del self.Vd[3]
        return self._v_hex_buffer(self.Vd, 3, rows, cin)

    def _halo_buffer(self, key, ntm, cout):
        """The halo rows a V / Vd-writing epilogue leaves for its fix-up kernel: two per row tile."""
        halo = self._vhalo.get(key)
        if halo is None or halo.shape[0] != ntm or halo.shape[2] != cout:
            halo = self._vhalo[key] = torch.zeros(ntm, 2, cout, dtype=torch.float32, device=self._dev)
        return halo

    def _pack_wino63(self, w, forward: bool):
        O, I = w.shape[0], w.shape[1]
        dst = torch.empty(8, O, I, dtype=torch.float32, device=w.device) if forward else \
            torch.empty(8, I, O, dtype=torch.float32, device=w.device)
        check(self.lib.tl_wino63_weights(ptr(w), ptr(dst) if forward else None, None if forward else ptr(dst), O, I, I, O,
                                         self._stream()), "tl_wino63_weights")
        return dst

    def _seq16(self, st) -> bool:
        """Stage ``st`` runs its forward and input gradient on whole-sequence tiles (f63_seq16; _v_hex_buffer sizes their operands)."""
        return self.f63_seq16 and st.idx == 3

    def f63_issue_factor(self, st, wgrad: bool = False) -> float:
        """MFMA FLOPs the F(6,3) kernels issue per direct-convolution FLOP of the stage (8 products per hex, hexes padded
        to whole sequences, against 3 MACs per valid conv row): of its forward / input-gradient launches, or (``wgrad``) of its
        weight gradient, which always runs over the stored hexes."""
        hexes = 16 if (not wgrad and self._seq16(st)) else st.tp_in // 6
        return hexes * 8.0 / (st.tc * 3.0)

    def _stage_forward63(self, st, w, bia) -> None:
        S = self.S
        wp = self._pack_wino63(w, True)
        V = self._v_ready[st.idx - 1]
        if st.idx == 2 and self.store_p1 and 2 not in self.P:       # (tests: the raw pooled rows of stage 2 as well)
            self.P[2] = torch.zeros(S * st.tp_out, st.cout, dtype=torch.float32, device=self._dev)
        Pout = self.P.get(st.idx) if (st.idx != 2 or self.store_p1) else None
        kw = dict(A=ptr(V), A_rows=V.shape[0], lda=V.shape[2], loader=LOAD_V, Bw=ptr(wp), bias=ptr(bia), out=ptr(Pout),
                  M=S * st.tp_in, N=st.cout, K=st.cin, ldb=st.cin, ldo=Pout.shape[1] if Pout is not None else st.cout, J=3,
                  row_shift=0, Tp=st.tp_in, slope=self.slope, obits=ptr(self.bits[st.idx]), osign=ptr(self.sbits[st.idx]),
                  ld_obits=st.cout // 32, Tvalid=2 * st.tout)
        if st.idx == 2:
            rows_out = S * st.tp_out
            Vn = self._v_hex_buffer(self.V, 2, rows_out, st.cout)
            ntm = -(-(S * st.tp_in) // self._nt63_rows())
            halo = self._halo_buffer(2, ntm, st.cout)
            kw.update(epilogue=EPI_POOLV, vout=ptr(Vn), vhalo=ptr(halo), vout_quads=Vn.shape[0], ld_vout=Vn.shape[2])
            self._nt(tag="conv2_fwd", fn="tl_conv3_wino63v_nt", **kw)
            check(self.lib.tl_wino63_v_fixup(ptr(Vn), ptr(halo), rows_out // 6, ntm, st.tp_out, st.cout, Vn.shape[2],
                                             self._stream()), "tl_wino63_v_fixup")
            self._v_ready[2] = Vn
        else:
            if Pout is None:
                raise RuntimeError("F(6,3) stage 3 writes pooled rows: its output buffer was not allocated")
            kw.update(epilogue=EPI_POOL, out_tp=st.tp_out)
            if self._seq16(st):
                # 16 computed hexes per sequence: the pad rows of the output and their words are never written (zero from allocation)
                kw.update(M=S * 96, Tp=96, a_hps_extra=st.tp_in // 6 - 16)
            self._nt(tag="conv3_fwd", fn="tl_conv3_wino63v_nt", **kw)

    def _stage_wgrad63(self, st, gw, gb) -> None:
        S = self.S
        f32 = dict(dtype=torch.float32, device=self._dev)
        rows_in = S * st.tp_in
        nd = st.cout
        ldg = nd
        V = self._v_ready[st.idx - 1]
        tiles = (st.cin // 64) * (nd // 64)
        sk = self._splitk(tiles, (rows_in + 35) // 36, 4096)
        slab = torch.empty(sk, 8 * st.cin, ldg, **f32)
        bias_part = torch.empty(sk, nd, **f32)
        if (st.idx == 3 and self.f63_yprod3 and self._y_ready.get(3) != self.generation):
            # stage 3's gradient rows come out of stage 4's one-tap GEMM: a kernel of its own un-pools and transforms them
            # (Y3, Vd3), and the weight gradient below runs without a transform like stage 2's
            Gs = self.G[3]
            Y3 = self._v_hex_buffer(self.Yt, 3, rows_in, nd)
            Vd3 = self._vd3_buffer(rows_in, nd)
            ev = self._tick("conv3_yvd")
            check(self.lib.tl_wino63_unpool_yvd(ptr(Gs), ptr(self.bits[3]), ptr(Y3), ptr(Vd3), rows_in, Gs.shape[0], st.tp_in,
                                                st.tp_out, 2 * st.tout, nd, Gs.shape[1], st.cout // 32, nd, self._stream()),
                  "tl_wino63_unpool_yvd")
            if ev:
                ev[1].record()
            self._y_ready[3] = self.generation
            self._vd_ready[3] = self.generation
        if self._y_ready.get(st.idx) == self.generation:
            # both operands pre-transformed: Y of this stage was written by the input gradient of the stage above.  (_y_ready
            # is this pass's flag alone: stage 2's input gradient reads the same Y2 after it, under _vd_ready)
            Y = self.Yt[st.idx]
            self._y_ready[st.idx] = -1
            self._tn(tag=f"conv{st.idx}_wgrad", fn="tl_conv3_wino63v_tn", A=ptr(V), B=ptr(Y), slab=ptr(slab), Krows=rows_in,
                     A_rows=V.shape[0], B_rows=Y.shape[0], Mdim=st.cin, Ndim=nd, lda=V.shape[2], ldb=Y.shape[2], ldc=ldg, J=3,
                     Tp=st.tp_in, splitk=sk, slab_stride=8 * st.cin * ldg, loader=LOAD_Y, Tvalid=2 * st.tout,
                     colsum=ptr(bias_part))
        else:
            Gs = self.G[st.idx]
            Vd = self._v_hex_buffer(self.Vd, st.idx, rows_in, nd)
            self._tn(tag=f"conv{st.idx}_wgrad", fn="tl_conv3_wino63v_tn", A=ptr(V), B=ptr(Gs), slab=ptr(slab), Krows=rows_in,
                     A_rows=V.shape[0], B_rows=Gs.shape[0], Mdim=st.cin, Ndim=nd, lda=V.shape[2], ldb=Gs.shape[1], ldc=ldg, J=3,
                     Tp=st.tp_in, splitk=sk, slab_stride=8 * st.cin * ldg, loader=LOAD_UNPOOL, bbits=ptr(self.bits[st.idx]),
                     ld_bbits=st.cout // 32, Tvalid=2 * st.tout, colsum=ptr(bias_part), vd=ptr(Vd), ld_vd=nd, g_tp=st.tp_out)
            self._vd_ready[st.idx] = self.generation
        self._wino_wgrad_tail(st, slab, bias_part, 8, "tl_wino63_wgrad_finalize", gw, gb)

    def _wino_wgrad_tail(self, st, slab, bias_part, taps, finalize, gw, gb) -> None:
        """Behind a Winograd weight-gradient launch: sum the split-K slabs ``[sk][taps * cin][ldg]``, turn the ``taps``
        transform-domain sums into torch's (O, I, 3, 1) and reduce the bias partials ``[sk][nd]``."""
        sk, rows, ldg = slab.shape
        if sk > 1:
            red = torch.empty(rows, ldg, dtype=torch.float32, device=self._dev)
            n = taps * st.cin * ldg
            self._permute(slab, red, (1, 1, 1, n), (0, 0, 0, 1), nz=sk, zs=n)
        else:
            red = slab
        check(getattr(self.lib, finalize)(ptr(red), ptr(gw), st.cout, st.cin, ldg, self._stream()), finalize)
        self._permute(bias_part, gb, (1, 1, 1, st.cout), (0, 0, 0, 1), nz=sk, zs=bias_part.shape[1])

    def _gy_stage(self, st) -> bool:
        """The one-tap pooled stage right behind F(6,3) stage 3 (conv4 of the reference stack) whose input gradient runs on the
        NT63 kernel and writes stage 3's backward operands Y3 / Vd3 itself (tl_conv1_wino63v_dgrad_nt; TONAL_KERNELS
        conv4_dgrad=gemm: the one-tap GEMM + tl_wino63_unpool_yvd of round 4)."""
        return self.gy4 and st.idx == 4

    def _gy_applies(self) -> bool:
        if not (self.wino63 and self.f63_yprod3 and len(self.stages) >= 3):
            return False
        below, st = self.stages[1], self.stages[2]
        return (_kernels.get("conv4_dgrad") == "nt63" and st.k == 1 and st.pool and self._f63(below)
                and st.cout % 32 == 0 and st.cout >= 40 and st.cin % 32 == 0 and (below.tp_in // 2) % 3 == 0)

    def _stage_dgrad_gy(self, st, w):
        S = self.S
        below = self.stages[1]                                   # the 3-tap stage whose pooled output this stage reads
        tpg = below.tp_in // 2                                   # gradient rows per sequence in ITS hex geometry (3 per hex)
        rows = S * tpg
        f32 = dict(dtype=torch.float32, device=self._dev)
        nh = -(-rows // 6)
        nh_pad = (nh + 127) // 128 * 128
        A = self._gy_A
        if A is None or A.shape[0] != nh_pad or A.shape[2] != st.cout:
            A = self._gy_A = torch.zeros(nh_pad, 8, st.cout, **f32)   # slots 6, 7 and the pad hexes stay zero
        Gs = self.G[st.idx]
        ev = self._tick(f"conv{st.idx}_dgrad")
        check(self.lib.tl_wino63_unpool_rows6(ptr(Gs), ptr(self.bits[st.idx]), ptr(A), rows, Gs.shape[0], tpg, st.tp_out,
                                              2 * st.tout, st.cout, Gs.shape[1], st.cout // 32, st.cout, 0, self._stream()),
              "tl_wino63_unpool_rows6")
        taps = torch.empty(st.cout // 8, 8, st.cin, 8, **f32)
        check(self.lib.tl_wino63_weights1(ptr(w), ptr(taps), st.cout, st.cin, st.cout, self._stream()), "tl_wino63_weights1")
        rows3 = S * below.tp_in                                  # conv rows of the stage below: six per hex of ITS geometry
        Y3 = self._v_hex_buffer(self.Yt, below.idx, rows3, below.cout)
        # with stage 3's input gradient on Y3 (f63_seq16) Vd3 has no reader: Y only, no halo rows, no fix-up pass
        # (store_p1 keeps it: Vd2 comes out of the Vd form of stage 3's input gradient alone)
        y_only = self._seq16(below) and not self.store_p1
        Vd3 = None if y_only else self._vd3_buffer(rows3, below.cout)
        if y_only:
            self.Vd[below.idx] = Y3                              # the operand of stage 3's input-gradient pass IS Y3 here
        ntm = -(-rows // self._nt63_rows())
        halo = None if y_only else self._halo_buffer("d3", ntm, below.cout)
        self._nt(tag=None, fn="tl_conv1_wino63v_dgrad_nt", A=ptr(A), A_rows=A.shape[0], lda=A.shape[2], loader=LOAD_V,
                 Bw=ptr(taps), M=rows, N=st.cin, K=st.cout, ldb=st.cout, ldo=st.cin, J=1, row_shift=0, Tp=tpg, slope=self.slope,
                 auxbits=ptr(self.sbits[below.idx]), ld_auxbits=self.sbits[below.idx].shape[1], abits=ptr(self.bits[below.idx]),
                 ld_abits=below.cout // 32, out_tp=below.tp_out, Tvalid_in=2 * below.tout, epilogue=EPI_GY, out=None,
                 vout=ptr(Y3), vout2=ptr(Vd3), vhalo=ptr(halo), vout_quads=Y3.shape[0], ld_vout=Y3.shape[2])
        if not y_only:
            check(self.lib.tl_wino63_vd_fixup(ptr(Vd3), ptr(halo), rows // 3, ntm, below.tp_in // 6, below.cout, Vd3.shape[2],
                                              self._stream()), "tl_wino63_vd_fixup")
        if ev:
            ev[1].record()
        self._y_ready[below.idx] = self.generation
        self._vd_ready[below.idx] = self.generation
        return None

    def _stage_dgrad63(self, st, w):
        S = self.S
        rows_in = S * st.tp_in
        # _vd_ready[idx]: the operand of this pass is there - Vd of the stage, or (stage 2 with f63_yprod; stage 3 with
        # f63_seq16) its Y
        if self._vd_ready.get(st.idx) != self.generation:
            raise RuntimeError("F(6,3) input gradient: its operand (Vd from the stage's weight-gradient pass, or Y2 from the "
                               "input gradient of stage 3) must be written first")
        self._vd_ready[st.idx] = -1
        seq16 = self._seq16(st)
        on_y = (st.idx == 2 and self.f63_yprod) or seq16   # hex H of Y yields rows 6 H .. 6 H + 7 (tonal_wino63_epi.h)
        Vd = self.Yt[st.idx] if on_y else self.Vd[st.idx]
        if on_y:
            wd = torch.empty(8, st.cin, st.cout, dtype=torch.float32, device=w.device)
            check(self.lib.tl_wino63_weights_y(ptr(w), ptr(wd), st.cout, st.cin, st.cout, self._stream()), "tl_wino63_weights_y")
        else:
            wd = self._pack_wino63(w, False)               # [8][cin][cout]
        kw = dict(A=ptr(Vd), A_rows=Vd.shape[0], lda=Vd.shape[2], loader=LOAD_V, Bw=ptr(wd), M=rows_in, N=st.cin,
                  K=st.cout, ldb=st.cout, ldo=st.cin, J=3, row_shift=0 if on_y else -2, Tp=st.tp_in, slope=self.slope,
                  auxbits=ptr(self.sbits[st.idx - 1]), ld_auxbits=self.sbits[st.idx - 1].shape[1])
        if seq16:
            # whole-sequence tiles on Y3: rows 0 .. 97 of a sequence's gradient from its 16 hexes, Y2 only (hexes 0 .. 32 of the 34)
            below = self.stages[0]
            Y2 = self._v_hex_buffer(self.Yt, 2, S * below.tp_in, below.cout)
            kw.update(M=S * 96, Tp=96, a_hps_extra=st.tp_in // 6 - 16)
            self._nt(tag="conv3_dgrad", fn="tl_conv3_wino63v_nt", epilogue=EPI_MASKY, out=None, vout=ptr(Y2), vout2=None, vhalo=None,
                     vout_quads=Y2.shape[0], ld_vout=Y2.shape[2], abits=ptr(self.bits[2]), ld_abits=below.cout // 32,
                     Tvalid_in=2 * below.tout, **kw)
            if self.store_p1:
                # (tests) Vd2 beside Y2: only the Vd form's epilogue writes it - that launch as well, its Y into a scratch buffer
                Vd3, Vd2 = self.Vd[3], self._v_hex_buffer(self.Vd, 2, S * below.tp_in, below.cout)
                ntm = -(-rows_in // self._nt63_rows())
                halo = self._halo_buffer("d2", ntm, below.cout)
                kw.update(A=ptr(Vd3), A_rows=Vd3.shape[0], lda=Vd3.shape[2], Bw=ptr(self._pack_wino63(w, False)), M=rows_in,
                          Tp=st.tp_in, a_hps_extra=0, row_shift=-2)
                self._nt(fn="tl_conv3_wino63v_nt", epilogue=EPI_MASKY, out=None, vout=ptr(torch.empty_like(Y2)), vout2=ptr(Vd2),
                         vhalo=ptr(halo), vout_quads=Y2.shape[0], ld_vout=Y2.shape[2], abits=ptr(self.bits[2]),
                         ld_abits=below.cout // 32, Tvalid_in=2 * below.tout, **kw)
                check(self.lib.tl_wino63_vd_fixup(ptr(Vd2), ptr(halo), rows_in // 3, ntm, below.tp_in // 6, below.cout,
                                                  Vd2.shape[2], self._stream()), "tl_wino63_vd_fixup")
            self._y_ready[2] = self.generation
            self._vd_ready[2] = self.generation
            return None
        if st.idx == 3 and self.f63_yprod:
            below = self.stages[0]
            rows2 = S * below.tp_in                              # conv rows of stage 2: six per hex = three of this GEMM's rows
            Y2 = self._v_hex_buffer(self.Yt, 2, rows2, below.cout)
            # Vd2 has no reader (stage 2's input gradient runs on Y2): written, with its fix-up pass, only under store_p1
            Vd2 = self._v_hex_buffer(self.Vd, 2, rows2, below.cout) if self.store_p1 else None
            ntm = -(-rows_in // self._nt63_rows())
            halo = self._halo_buffer("d2", ntm, below.cout) if self.store_p1 else None
            self._nt(tag="conv3_dgrad", fn="tl_conv3_wino63v_nt", epilogue=EPI_MASKY, out=None, vout=ptr(Y2), vout2=ptr(Vd2),
                     vhalo=ptr(halo), vout_quads=Y2.shape[0], ld_vout=Y2.shape[2], abits=ptr(self.bits[2]),
                     ld_abits=below.cout // 32, Tvalid_in=2 * below.tout, **kw)
            if Vd2 is not None:
                check(self.lib.tl_wino63_vd_fixup(ptr(Vd2), ptr(halo), rows_in // 3, ntm, below.tp_in // 6, below.cout,
                                                  Vd2.shape[2], self._stream()), "tl_wino63_vd_fixup")
            self._y_ready[2] = self.generation
            self._vd_ready[2] = self.generation
            return None
        if st.idx == 3:
            self._nt(tag="conv3_dgrad", fn="tl_conv3_wino63v_nt", epilogue=EPI_MASK, out=ptr(self.G[2]), **kw)
            return None
        ntm = -(-rows_in // self._nt63_rows())
        part = torch.empty(ntm, (self.k1 + 1) * self.c1, dtype=torch.float32, device=self._dev)
        self._nt(tag="conv2_dgrad", fn="tl_conv3_wino63v_nt", epilogue=EPI_C1WGRAD, out=None, c1x=ptr(self._x),
                 c1bits=ptr(self.bits[1]), c1partial=ptr(part), c1T=self.T, c1kt=self.k1, Tvalid=self.tout1, **kw)
        return part

    def _c1_fusable(self) -> bool:
        # the epilogue reads x[2t + a + j] for j < 3 unconditionally (4 floats from 2t)
        return self.k1 <= 3 and self.T >= 2 * self.tout1 + 2

    def _v43(self, st) -> bool:
        """The stage runs on the F(4,3) V-form kernels, all three passes: forward and weight gradient on V (the input transform
        its producer wrote), input gradient on Vd (the transformed un-pooled dZ its weight-gradient launch writes).  Every
        other shape runs on the direct MFMA kernels."""
        return (self.wino43 and st.k == 3 and st.pool and st.cin % 64 == 0 and st.cout % 32 == 0 and st.tp_in % 4 == 0
                and r4(st.cout) % 16 == 0)

    def _tn_bm(self, st) -> int:
        """C_in tile of the V-form weight-gradient kernel: 128 (8 waves, the Y side by LDS-DMA: C_in % 128 == 0,
        C_out % 64 == 0) where the shape allows it, else 64 (4 waves)."""
        wide = st.cin % 128 == 0
        dma8 = wide and r4(st.cout) % 64 == 0 and (st.cout // 32) % 2 == 0
        if self.tn_bm == 127:                  # (the 8-wave kernel that stages Y through registers: bit-identical A/B partner)
            return 127 if wide else 64
        if self.tn_bm in (0, 128):
            return 128 if dma8 else 64
        return 64

    def _conv1_writes_v(self) -> bool:
        """The first stage hands its output to stage 2 as V (tl_conv1_fwd_v) - nothing else reads P1 then."""
        return (self._v43(self.stages[0]) and self.tp1 % 4 == 0 and self.c1 in (128, 256, 512, 1024)
                and (self.fuse_c1 and self._c1_fusable()))

    def _writes_v(self, st) -> bool:
        """The forward pass of this stage writes V of its own output for the next stage (nothing else reads the raw rows:
        the next stage's forward and weight gradient read V, its input gradient's LeakyReLU' mask the 1-bit sign array)."""
        if not (self.wino_vout and st.pool and st.idx - 1 < len(self.stages)):
            return False
        nxt = self.stages[st.idx - 1]                      # stages[k] has idx k + 2
        return self._v43(st) and self._v43(nxt) and st.tp_in % 8 == 0 and nxt.cin == st.cout

    def _pin(self, st):
        """Input activation of a stage, or None when only its V form exists (stage 2 behind tl_conv1_fwd_v)."""
        return self.P.get(st.idx - 1)

    def _v_buffer(self, idx, rows, cin, store=None):
        """V of P[idx] (or, in ``store`` = Vd, of the un-pooled dZ of stage idx): rows / 4 quads, padded with zero quads to
        whole 128-quad tiles (the weight-gradient kernel reads whole 8-quad K-steps, the forward kernel 128-quad tiles)."""
        store = self.V if store is None else store
        nq = rows // 4
        nq_pad = (nq + 127) // 128 * 128
        V = store.get(idx)
        if V is None or V.shape[0] != nq_pad or V.shape[2] != cin:
            V = store[idx] = torch.zeros(nq_pad, 6, cin, dtype=torch.float32, device=self._dev)
        return V

    def _input_transform(self, st):
        """V of the stage's input P[idx-1] (stand-alone transform kernel; stage 2 gets it from tl_conv1_fwd)."""
        src = self.P[st.idx - 1]
        V = self._v_buffer(st.idx - 1, src.shape[0], st.cin)
        ev = self._tick(f"conv{st.idx}_xform")
        check(self.lib.tl_wino43_input_transform(ptr(src), ptr(V), src.shape[0], st.tp_in, st.cin, src.shape[1], st.cin,
                                                 self._stream()), "tl_wino43_input_transform")
        if ev:
            ev[1].record()
        return V

    def wgrad_issue_factor(self, st) -> float:
        """MFMA FLOPs the weight-gradient kernel of a stage issues per direct-convolution FLOP."""
        if self._f63(st):
            return self.f63_issue_factor(st, wgrad=True)
        return 0.5 if self._v43(st) else 1.0

    def kernel_families(self):
        """({rocprofv3 kernel family: [timer tags]}, {family: MFMA FLOPs issued per algorithmic FLOP})
        for the conv stages - bench.py prices the HIP-event timers of ``enable_timers`` with it."""
        if self.wino63:
            self._fam_share = {}
            st2, st3 = self.stages[0], self.stages[1]
            f6 = "Winograd F(6,3) on pre-transformed operands, LDS-DMA"
            seq16 = self._seq16(st3)
            s16 = f"; 16 of the {st3.tp_in // 6} stored hexes per sequence" if seq16 else ""
            tn = "wino63v_tn4_kernel<true>" if st3.cin % 256 == 0 and st3.tp_in >= 12 else "wino63v_tn_kernel<true>"
            tn2 = "wino63v_tn4_kernel<true>" if st2.cin % 256 == 0 else "wino63v_tn_kernel<true>"
            fams = {f"wino63v_nt_kernel<POOLV> (conv2 forward, {f6}; writes V of its pooled output for conv3)": ["conv2_fwd"],
                    f"wino63v_nt_kernel<POOL> (conv3 forward, {f6}{s16})": ["conv3_fwd"],
                    f"wino63v_nt_kernel<C1WGRAD> (conv2 input gradient + conv1 weight gradient, {f6})": ["conv2_dgrad"],
                    }
            if self.f63_yprod3:
                gy = self.gy4
                src = "the epilogue of conv4's input gradient" if gy else "wino63_unpool_yvd_kernel"
                ops = "Y3" if seq16 else "Y3 / Vd3"
                fams[f"wino63v_tn4y_kernel (conv3 weight gradient, {f6}: both operands by LDS-DMA, no transform in the kernel; {ops} "
                     f"from {src})"] = ["conv3_wgrad"]
            else:
                fams[f"{tn} (conv3 weight gradient, {f6}; also writes Vd)"] = ["conv3_wgrad"]
            if seq16:
                fams[f"wino63v_nt_kernel<MASKY_SEQ> (conv3 input gradient on Y3, {f6}{s16}; writes Y of conv2 instead of the gradient "
                     "rows)"] = ["conv3_dgrad"]
                fams[f"wino63v_tn4y_kernel (conv2 weight gradient, {f6}: both operands by LDS-DMA, no transform in the kernel)"] = ["conv2_wgrad"]
            elif self.f63_yprod:
                both = "Y and Vd" if self.store_p1 else "Y"
                fams[f"wino63v_nt_kernel<MASKY> (conv3 input gradient, {f6}; writes {both} of conv2 instead of the gradient rows)"] = ["conv3_dgrad"]
                fams[f"wino63v_tn4y_kernel (conv2 weight gradient, {f6}: both operands by LDS-DMA, no transform in the kernel)"] = ["conv2_wgrad"]
            else:
                fams[f"wino63v_nt_kernel<MASK> (conv3 input gradient, {f6})"] = ["conv3_dgrad"]
                fams[f"{tn2} (conv2 weight gradient, {f6}; also writes Vd)"] = ["conv2_wgrad"]
            # (by the launch's timer tag: the labels name their neighbours too)
            issued = {k: self.f63_issue_factor(st2 if tags[0].startswith("conv2") else st3, wgrad=tags[0].endswith("_wgrad"))
                      for k, tags in fams.items()}
            return fams, issued
        self._fam_share = {}         # family -> share of its stages' algorithmic FLOPs it computes (default 1)
        if not all(self._v43(st) for st in self.stages[:2]):
            fams = {"nt_window_kernel<128,UNPOOL,MASK> (conv input-gradient)": ["conv2_dgrad", "conv3_dgrad", "conv4_dgrad"],
                    "nt_window_kernel<128,DIRECT,POOL> (conv forward)": ["conv2_fwd", "conv3_fwd", "conv4_fwd"],
                    "tn3_kernel<UNPOOL> (conv weight-gradient)": ["conv2_wgrad", "conv3_wgrad"]}
            return fams, {k: 1.0 for k in fams}      # (mixed shapes: a stage the V form does not cover runs direct)
        form = "Winograd F(4,3) on pre-transformed operands, LDS-DMA"
        fused = self.fuse_c1 and self._c1_fusable()
        bm = self._tn_bm(self.stages[0])
        extra = {}
        if bm == 128:
            # one launch: its workgroups take turns at writing Vd, the operand of the input gradient
            tn = f"wino43v_tn8_kernel<true> (conv2/conv3 weight gradient, {form}; also writes Vd for the input gradient)"
        else:
            # the op is two launches, named apart by rocprofv3: the first C_in tile (1 / ntm of the MFMA work) also writes Vd
            ntm = (self.stages[0].cin + 63) // 64
            tn = f"wino43v_tn_kernel<false, 2> (conv2/conv3 weight gradient, C_in tiles 1..{ntm - 1} of {ntm}, {form})"
            vdn = f"wino43v_tn_kernel<true, 2> (conv2/conv3 weight gradient, C_in tile 0 of {ntm}, {form}, + writes Vd for the input gradient)"
            extra[vdn] = ["conv2_wgrad_vd", "conv3_wgrad_vd"]
            self._fam_share = {tn: (ntm - 1) / ntm, vdn: 1.0 / ntm}
        fams = {tn: ["conv2_wgrad", "conv3_wgrad"]}
        if self._writes_v(self.stages[0]):
            # stage 2's forward launch also writes V of its output for stage 3 (epilogue 5): its own kernel name
            fams[f"wino43v_nt_kernel<POOLV> (conv2 forward, {form}; writes V of its pooled output for conv3 instead of the raw rows)"] = ["conv2_fwd"]
            fams[f"wino43v_nt_kernel<POOL> (conv3 forward, {form})"] = ["conv3_fwd"]
        else:
            fams[f"wino43v_nt_kernel<POOL> (conv2/conv3 forward, {form})"] = ["conv2_fwd", "conv3_fwd"]
        fams.update(extra)
        if fused:       # the stage-2 launch carries the fused conv1 weight-gradient epilogue: its own kernel name
            fams[f"wino43v_nt_kernel<UNPOOL,C1WGRAD> (conv2 input gradient + conv1 weight gradient, {form})"] = ["conv2_dgrad"]
            fams[f"wino43v_nt_kernel<UNPOOL,MASK> (conv3 input gradient, {form})"] = ["conv3_dgrad"]
        else:
            fams[f"wino43v_nt_kernel<UNPOOL,MASK> (conv2/conv3 input gradient, {form})"] = ["conv2_dgrad", "conv3_dgrad"]
        return fams, {k: 0.5 for k in fams}

    def _pack_wino43(self, w, forward: bool):
        """torch (O, I, 3, 1) -> the 6 F(4,3) taps: forward [6][O][I] or input-gradient [6][I][O]."""
        O, I = w.shape[0], w.shape[1]
        dst = torch.empty(6, O, I, dtype=torch.float32, device=w.device) if forward else \
            torch.empty(6, I, O, dtype=torch.float32, device=w.device)
        check(self.lib.tl_wino43_weights(ptr(w), ptr(dst) if forward else None, None if forward else ptr(dst), O, I, I, O,
                                         self._stream()), "tl_wino43_weights")
        return dst

    # ------------------------------------------------------------------ stage 1, then one ecog stage (2..5)
    def conv1_forward(self, x, w1, b1) -> None:
        """Stage 1 (C_in = 1) of a forward pass over ``x``: pooled rows P1 and / or their transform V1, arg-max and sign bits."""
        lib, st_ = self.lib, self._stream()
        S, T, dev = self.S, self.T, self._dev
        self._x = x
        self._v_ready = {}
        w1 = w1.reshape(self.c1, self.k1).contiguous()
        sbits = ptr(self.sbits.get(1))
        if self.store_p1 and 1 not in self.P:
            self.P[1] = torch.zeros(S * self.tp1, self.c1, dtype=torch.float32, device=dev)
        P1 = ptr(self.P[1]) if self.store_p1 else None          # (the V-writing kernels: raw rows only on request)
        geom = (S, T, self.k1, self.c1, self.tp1, self.tout1, self.slope, st_)
        if self.wino63:
            V1 = self._v_hex_buffer(self.V, 1, S * self.tp1, self.c1)
            ev = self._tick("conv1_fwd")
            check(lib.tl_conv1_fwd_v6(ptr(x), ptr(w1), ptr(b1), P1, ptr(V1), ptr(self.bits[1]), sbits, *geom), "tl_conv1_fwd_v6")
            if ev:
                ev[1].record()
            self._v_ready[1] = V1
        elif self._conv1_writes_v():
            V1 = self._v_buffer(1, S * self.tp1, self.c1)
            check(lib.tl_conv1_fwd_v(ptr(x), ptr(w1), ptr(b1), P1, ptr(V1), ptr(self.bits[1]), sbits, *geom), "tl_conv1_fwd_v")
            self._v_ready[1] = V1
        else:
            check(lib.tl_conv1_fwd(ptr(x), ptr(w1), ptr(b1), ptr(self.P[1]), ptr(self.bits[1]), sbits, *geom), "tl_conv1_fwd")

    STAGE_NAMES = {2: "ecog_conv_block.3", 3: "ecog_conv_block.6", 4: "ecog_conv_block.9", 5: "ecog_conv_block.12"}

    def stage_forward(self, st: _Stage, w: torch.Tensor, bia: torch.Tensor) -> None:
        """conv (k,1) + bias + LeakyReLU (+ max-pool, arg-max bits): P[idx-1] -> P[idx]."""
        if self._f63(st):
            return self._stage_forward63(st, w, bia)
        S = self.S
        v43 = self._v43(st)
        wp = self._pack_wino43(w, True) if v43 else self._pack_conv(w, st.cin, False)
        src = self._pin(st)
        vout = self._writes_v(st)
        if vout and self.store_p1 and st.idx not in self.P:
            self.P[st.idx] = torch.zeros(S * st.tp_out, st.cout, dtype=torch.float32, device=self._dev)
        Pout = self.P.get(st.idx) if (not vout or self.store_p1) else None
        kw = dict(A=ptr(src), Bw=ptr(wp), bias=ptr(bia), out=ptr(Pout), M=S * st.tp_in,
                  A_rows=S * st.tp_in, N=st.cout, K=st.cin, lda=st.cin, ldb=st.cin,
                  ldo=Pout.shape[1] if Pout is not None else st.cout, J=st.k, row_shift=0, Tp=st.tp_in, slope=self.slope,
                  loader=LOAD_DIRECT)
        if st.pool:
            kw.update(epilogue=EPI_POOL, obits=ptr(self.bits[st.idx]), osign=ptr(self.sbits[st.idx]),
                      ld_obits=st.cout // 32, Tvalid=2 * st.tout)
        else:
            kw.update(epilogue=EPI_LRELU, Tvalid=st.tout)
        if not v43:
            self._nt(tag=f"conv{st.idx}_fwd", fn="tl_gemm_nt_window", **kw)
            return
        V = self._v_ready.get(st.idx - 1)
        if V is None:
            V = self._v_ready[st.idx - 1] = self._input_transform(st)
        kw.update(A=ptr(V), A_rows=V.shape[0], lda=V.shape[2], loader=LOAD_V)
        if vout:
            rows_out = S * st.tp_out
            Vn = self._v_buffer(st.idx, rows_out, st.cout)
            ntm = (S * st.tp_in + 511) // 512
            halo = self._halo_buffer(st.idx, ntm, st.cout)
            kw.update(epilogue=EPI_POOLV, vout=ptr(Vn), vhalo=ptr(halo), vout_quads=Vn.shape[0], ld_vout=Vn.shape[2])
            self._nt(tag=f"conv{st.idx}_fwd", fn="tl_conv3_wino43v_nt", **kw)
            check(self.lib.tl_wino43_v_fixup(ptr(Vn), ptr(halo), rows_out // 4, ntm, st.tp_out, st.cout, Vn.shape[2],
                                             self._stream()), "tl_wino43_v_fixup")
            self._v_ready[st.idx] = Vn
            return
        self._nt(tag=f"conv{st.idx}_fwd", fn="tl_conv3_wino43v_nt", **kw)

    def _colsum(self, Gm, rows, ncols, ld, Tp, Tvalid, dst):
        nc4 = r4(ncols)                       # pad columns of G are zero by construction
        rpb = max(1, 256 // (nc4 // 4))
        nblk = int(min(2048, max(1, rows // (rpb * 16))))
        part = torch.empty(nblk, nc4, dtype=torch.float32, device=Gm.device)
        check(self.lib.tl_colsum(ptr(Gm), ptr(part), nblk, rows, nc4, ld, Tp, Tvalid, self._stream()), "tl_colsum")
        self._permute(part, dst, (1, 1, 1, ncols), (0, 0, 0, 1), nz=nblk, zs=nc4)

    def _reduce_c1_partials(self, part: torch.Tensor, gw: torch.Tensor, gb: torch.Tensor) -> None:
        """Partial sums of the first stage's weight / bias gradient, ``part[tile][(k1 + 1) * c1]`` in the layout of
        ``tl_conv1_wgrad`` (tap-major weight sums, then the bias sums), -> torch's (c1, 1, k1, 1) weight and (c1,) bias."""
        f32 = dict(dtype=torch.float32, device=part.device)
        nblk = part.shape[0]
        zs = (self.k1 + 1) * self.c1
        if nblk >= 256 and zs % 4 == 0:
            # many partial rows (one per row tile of the fused epilogue: 8 704 x 2 048 floats at the north-star shape): sum them
            # with the column-sum kernel (reads run along the row) and permute the 2 048 results - the slab-parallel permute
            # reads such a matrix one element per cache line (94 + 78 us for 71 MB)
            red = torch.empty(zs, **f32)
            flat = part.view(-1)
            for c0 in range(0, zs, 1024):
                nc = min(1024, zs - c0)
                self._colsum(flat[c0:], nblk, nc, zs, 1, 1, red[c0:c0 + nc])
            self._permute(red, gw, (1, 1, self.c1, self.k1), (0, 0, 1, self.c1))
            self._permute(red, gb, (1, 1, 1, self.c1), (0, 0, 0, 1), src_off=self.k1 * self.c1)
        else:
            self._permute(part, gw, (1, 1, self.c1, self.k1), (0, 0, 1, self.c1), nz=nblk, zs=zs)
            self._permute(part, gb, (1, 1, 1, self.c1), (0, 0, 0, 1), nz=nblk, zs=zs, src_off=self.k1 * self.c1)

    def stage_wgrad(self, st: _Stage, gw: torch.Tensor, gb: torch.Tensor) -> None:
        """dW, db of one stage from its input P[idx-1] and G[idx] (pooled gradient + arg-max bits)."""
        if self._f63(st):
            return self._stage_wgrad63(st, gw, gb)
        S = self.S
        f32 = dict(dtype=torch.float32, device=self._dev)
        Xin = self._pin(st)
        Gs = self.G[st.idx]
        rows_in = S * st.tp_in
        ldg = Gs.shape[1]
        nd = r4(st.cout)
        if self._v43(st):
            # F(4,3) on V: 6 transform accumulators; split-K slabs summed afterwards.  (Measured at conv2: the 8-wave kernel,
            # one workgroup per CU, runs 0.3 ms better with 8 rounds of 256 workgroups than with 16 - 42.2 / 42.55 ms)
            tiles = ((st.cin + 63) // 64) * ((nd + 63) // 64)
            bm = self._tn_bm(st)
            sk = self._splitk(tiles, (rows_in + 31) // 32, 4096 if bm in (127, 128) else 8192)
            slab = torch.empty(sk, 6 * st.cin, ldg, **f32)
            bias_part = torch.empty(sk, nd, **f32)     # the kernel's Y1 = sum of the quad's dZ rows doubles as the bias gradient
            V = self._v_ready.get(st.idx - 1)          # normally written in the forward pass
            if V is None:
                V = self._v_ready[st.idx - 1] = self._input_transform(st)
            Vd = self._v_buffer(st.idx, rows_in, nd, self.Vd)
            kw = dict(A=ptr(V), B=ptr(Gs), slab=ptr(slab), Krows=rows_in, A_rows=V.shape[0], B_rows=Gs.shape[0],
                      Mdim=st.cin, Ndim=nd, lda=V.shape[2], ldb=ldg, ldc=ldg, J=3, Tp=st.tp_in, splitk=sk,
                      slab_stride=6 * st.cin * ldg, loader=LOAD_UNPOOL, bbits=ptr(self.bits[st.idx]),
                      ld_bbits=st.cout // 32, Tvalid=2 * st.tout, colsum=ptr(bias_part), bm=bm, vd=ptr(Vd), ld_vd=nd)
            self._vd_ready[st.idx] = self.generation
            if self.timers is not None and bm != 128:
                # two calls so that the two launches of the op get their own HIP-event timers (rocprofv3 names them apart too)
                self._tn(tag=f"conv{st.idx}_wgrad_vd", fn="tl_conv3_wino43v_tn", part=1, **kw)
                self._tn(tag=f"conv{st.idx}_wgrad", fn="tl_conv3_wino43v_tn", part=2, **kw)
            else:
                self._tn(tag=f"conv{st.idx}_wgrad", fn="tl_conv3_wino43v_tn", **kw)
            self._wino_wgrad_tail(st, slab, bias_part, 6, "tl_wino43_wgrad_finalize", gw, gb)
            return
        if st.k == 3:      # all-taps kernel: 128 x 64 tiles
            tiles = ((st.cin + 127) // 128) * ((nd + 63) // 64)
        else:
            tiles = st.k * ((st.cin + 127) // 128) * ((nd + 127) // 128)
        sk = self._splitk(tiles, (rows_in + 31) // 32, 1024)     # two rounds of 512 resident workgroups
        slab = torch.empty(sk, st.k * st.cin, ldg, **f32)
        kw = dict(A=ptr(Xin), B=ptr(Gs), slab=ptr(slab), Krows=rows_in, A_rows=Xin.shape[0], B_rows=Gs.shape[0],
                  Mdim=st.cin, Ndim=nd, lda=st.cin, ldb=ldg, ldc=ldg, J=st.k, Tp=st.tp_in, splitk=sk,
                  slab_stride=st.k * st.cin * ldg)
        if st.pool:
            kw.update(loader=LOAD_UNPOOL, bbits=ptr(self.bits[st.idx]), ld_bbits=st.cout // 32, Tvalid=2 * st.tout)
        else:
            kw.update(loader=LOAD_DIRECT, Tvalid=st.tout)
        # one-tap direct kernel: the bias gradient rides in the launch (see the 1x1 stack in backward())
        fold = (not st.pool) and st.k == 1 and rows_in > 512 and st.cin > 32
        bpart = torch.empty(sk, nd, **f32) if fold else None
        if fold:
            kw.update(colsum=ptr(bpart))
        self._tn(tag=f"conv{st.idx}_wgrad", **kw)
        # sum the split-K slabs with coalesced reads first ([j][i][o], o contiguous), then permute the
        # small result to torch's (O, I, J, 1)
        if sk > 1:
            red = torch.empty(st.k * st.cin, ldg, **f32)
            n = st.k * st.cin * ldg
            self._permute(slab, red, (1, 1, 1, n), (0, 0, 0, 1), nz=sk, zs=n)
        else:
            red = slab
        self._permute(red, gw, (1, st.cout, st.cin, st.k), (0, 1, ldg, st.cin * ldg))
        if fold:
            self._permute(bpart, gb, (1, 1, 1, st.cout), (0, 0, 0, 1), nz=sk, zs=nd)
        else:
            self._colsum(Gs, Gs.shape[0], st.cout, ldg, st.tp_out, st.tout, gb)

    def stage_dgrad(self, st: _Stage, w: torch.Tensor):
        """G[idx-1] = (dZ[idx] (*) flipped W) * LeakyReLU'(P[idx-1]).

        For stage 2 on the Winograd kernels G[1] is not stored: the epilogue contracts it with the raw
        signal into per-row-tile partial sums of the first stage's weight / bias gradient, which are
        returned (shape (tiles, (k1 + 1) * c1), layout of ``tl_conv1_wgrad``'s partials)."""
        if self._f63(st):
            return self._stage_dgrad63(st, w)
        if self._gy_stage(st):
            return self._stage_dgrad_gy(st, w)
        S = self.S
        Xin = self._pin(st)
        Gs = self.G[st.idx]
        rows_in = S * st.tp_in
        ldg = Gs.shape[1]
        v43 = self._v43(st)
        wd = self._pack_wino43(w, False) if v43 else self._pack_conv(w, st.cin, True)   # [6 or J][cin][r4(cout)]
        kd = wd.shape[2]
        fuse = st.idx == 2 and v43 and self.fuse_c1 and self._c1_fusable()
        kw = dict(A=ptr(Gs), Bw=ptr(wd), aux=ptr(Xin), out=None if fuse else ptr(self.G[st.idx - 1]), M=rows_in,
                  A_rows=Gs.shape[0], N=st.cin, K=kd, lda=ldg, ldb=kd, ldo=st.cin, ldaux=st.cin, J=st.k,
                  row_shift=-(st.k - 1), Tp=st.tp_in, epilogue=EPI_MASK, slope=self.slope)
        if (st.idx - 1) in self.sbits:            # the input of this stage came out of a pooling epilogue
            kw.update(auxbits=ptr(self.sbits[st.idx - 1]), ld_auxbits=self.sbits[st.idx - 1].shape[1])
        if st.pool:
            kw.update(loader=LOAD_UNPOOL, abits=ptr(self.bits[st.idx]), ld_abits=st.cout // 32,
                      Tvalid_in=2 * st.tout)
        else:
            kw.update(loader=LOAD_DIRECT)
        if not v43:
            self._nt(tag=f"conv{st.idx}_dgrad", fn="tl_gemm_nt_window", **kw)
            return None
        part = None
        if fuse:
            ntm = (rows_in + 511) // 512
            part = torch.empty(ntm, (self.k1 + 1) * self.c1, dtype=torch.float32, device=self._dev)
            kw.update(epilogue=EPI_C1WGRAD, out=None, c1x=ptr(self._x), c1bits=ptr(self.bits[1]), c1partial=ptr(part),
                      c1T=self.T, c1kt=self.k1, Tvalid=self.tout1)
        if self._vd_ready.get(st.idx) != self.generation or st.idx not in self.Vd:
            raise RuntimeError("F(4,3) input gradient: the stage's weight-gradient pass (which writes Vd) must run first")
        # the weight-gradient kernel of this stage (run just before) left Vd = B^T (un-pooled dZ rows 4q-2 .. 4q+3)
        Vd = self.Vd[st.idx]
        kw.update(A=ptr(Vd), A_rows=Vd.shape[0], lda=Vd.shape[2], loader=LOAD_V)
        self._vd_ready[st.idx] = -1
        self._nt(tag=f"conv{st.idx}_dgrad", fn="tl_conv3_wino43v_nt", **kw)
        return part
