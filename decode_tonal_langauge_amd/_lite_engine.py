"""Host-side plan of the SynthesisLite forward / backward on MI355X (reference
models/synthesis_models.py:201-296): two Conv1d+BatchNorm1d+LeakyReLU+MaxPool1d blocks
(``tl_lite_*`` kernels), the small label LSTM (one launch per direction), concat + dropout, and the
two Linear layers on the fp32-MFMA GEMM kernels.  Layout is the reference's own (B, C, T).

The plan is written once, for M models of equal shape side by side ("members"; ``_lite_ensemble_engine.LiteEnsembleEngine``
derives from ``LiteEngine``): every intermediate is (M, B, ...), every launch goes to the ``_group`` entry of its kernel with the
member on the grid and member strides that are products of sizes.  ``LiteEngine`` is M = 1, where a ``_group`` entry makes the
launch of its single neighbour (csrc/tonal_lite.hip, csrc/tonal_misc.hip: one launch function per pair) and a member stride is
never used, so x (B, C, T), labels, dout and the gradient tensors are taken without the leading 1.  What the two engines do
differently sits in small methods: the GEMM launches ``_nt`` / ``_tn`` (``tl_gemm_nt_window`` / ``tl_gemm_tn_window`` with every
kernel form here, their member forms in the ensemble) and ``_fc3_sum``, which the ensemble overrides, and ``_cat`` / ``_uncat``,
which pass the dropout seed by value while there is no seed table in device memory (an eager step of one model)."""
from __future__ import annotations

from typing import Callable, Dict, Optional, Protocol

import torch

from . import _lib
from ._launch import launch_nt, launch_tn, permute_reduce, r4
from ._lib import EPI_MASK, EPI_STORE, LOAD_DIRECT, check, ptr

# what the short-reduction TN kernel (tn_short_kernel) takes: the one that writes the bias gradient (the column sums of its A
# operand) beside the weight gradient, and the only TN kernel with a member dimension
MAX_ROWS = 512        # Krows (8 chunks of 64 rows)
MAX_OUT = 1 << 20     # Mdim * Ndim


class TrainEngine(Protocol):
    """What ``SynthesisTrainer`` reads on ``model._engine`` (``LiteEngine``, ``_cnn_engine.CnnEngine``), besides ``forward`` /
    ``backward``, ``ldd`` and ``p_drop``.  An engine states what it does not offer as a class-level default."""
    lowrank_param: Optional[str]      # the parameter whose gradient leaves ``backward`` as factors (the label LSTM's W_hh); only
    #                                   an engine that names one can shard that LSTM by gate rows
    whh_factors: Optional[tuple]      # the factors of the last ``backward(whh_factors=True)``, None when it wrote the gradient
    lstm_shard: Optional[tuple]       # (rank, world) set by the trainer: shard the label LSTM where a step allows it
    ran_sharded: bool                 # the last forward did run row-sharded (decided per forward)
    grad_order: Optional[Callable]    # () -> parameter names, first-finished first: the layout of ``parallel.FlatGrads``
    graph_capable: bool               # the step may be captured into a HIP graph (``seed_dev``: dropout seed in device memory)


class LiteEngine:
    NAME = "SynthesisLite"
    lowrank_param = whh_factors = lstm_shard = grad_order = None
    ran_sharded, graph_capable = False, True

    def __init__(self, output_dim, n_channels, n_timepoints, label_dim, conv_channels, lstm_hidden, dropout,
                 negative_slope, M: int = 1):
        if negative_slope < 0:
            raise ValueError("the MI355X path needs negative_slope >= 0")
        if label_dim > 8:
            raise ValueError("label_dim > 8 is not supported by the LSTM input-gradient kernel")
        # the direct conv kernels stage a 64-sample time tile plus the k - 1 halo of every input channel (forward) / output
        # channel (input gradient) in 64 KB of LDS (csrc/tonal_lite.hip): refuse here, before any launch
        if n_channels * (64 + 4) * 4 > 64 * 1024:
            raise ValueError(f"n_channels = {n_channels}: at most 240 ECoG channels fit the conv kernel's LDS tile")
        if conv_channels * (64 + 2) * 4 > 64 * 1024:
            raise ValueError(f"conv_channels = {conv_channels}: at most 248 fit the conv kernel's LDS tile")
        self.M = M
        self.active = None            # the ensemble's mask of members that take part (int32 words in device memory)
        # the dropout seeds in device memory, one int64 word per member: set by the trainer's HIP-graph mode, always there in
        # the ensemble; None: the seed of a forward call travels by value
        self.seed_dev = None
        self.lib = _lib.load()
        self.out_dim, self.C, self.T, self.in_dim = output_dim, n_channels, n_timepoints, label_dim
        self.CC, self.H = conv_channels, lstm_hidden
        self.p_drop, self.slope = float(dropout), float(negative_slope)
        self.T1, self.T2 = n_timepoints // 2, n_timepoints // 2 // 2
        self.F = conv_channels * self.T2
        self.ldf = r4(self.F + lstm_hidden)
        self.ldd = r4(output_dim)
        self.hid = 512
        self.generation = 0
        self._saved_generation = -1

    def _begin(self):
        """The library and the tail of every launch of one pass: the members' mask and the current stream, read once a pass and
        not once a launch (profiles/lite_engine_fold.md)."""
        self._tail = (ptr(self.active), torch.cuda.current_stream().cuda_stream)
        return self.lib, self._tail

    def _permute(self, src, dst, dims, strides, *args, **kw):
        permute_reduce(self.lib, src, dst, dims, strides, *args, stream=self._tail[1], **kw)

    # ------------------------------------------------------------------ what the ensemble does differently
    def _nt(self, s_A, s_Bw, s_bias, s_aux, s_out, **fields):
        launch_nt(self.lib, stream=self._tail[1], **fields)

    def _tn(self, s_A, s_B, s_slab, s_colsum, **fields):
        launch_tn(self.lib, stream=self._tail[1], **fields)

    def _fc3_sum(self, slab3, bias, out, sk3, B):
        """out (M, B, out_dim) = the sum of fc.3's ``sk3`` split-K slabs + the bias row."""
        D = self.out_dim
        self._permute(slab3, out, (1, 1, B, D), (0, 0, D, 1), nz=sk3, zs=B * D, bias=bias)

    def _cat(self, y2, B, L, p_drop):
        lib, tail, F, H, ldf = self.lib, self._tail, self.F, self.H, self.ldf
        if self.seed_dev is None:          # an eager step: no seed table to fill, no launch or copy for it
            check(lib.tl_lite_cat(ptr(y2), ptr(self.hs), ptr(self.feat), B, F, H, L, ldf, p_drop, self._seed,
                                  tail[1]), "tl_lite_cat")
        else:
            check(lib.tl_lite_cat_group(ptr(y2), ptr(self.hs), ptr(self.feat), self.M, B, F, H, L, ldf, p_drop,
                                        ptr(self.seed_dev), B * F, B * L * H, B * ldf, *tail), "tl_lite_cat_group")

    def _uncat(self, dfeat, dy2, dh, B):
        lib, tail, F, H, ldf = self.lib, self._tail, self.F, self.H, self.ldf
        if self.seed_dev is None:
            check(lib.tl_lite_uncat(ptr(dfeat), ptr(dy2), ptr(dh), B, F, H, ldf, self._p_used, self._seed,
                                    tail[1]), "tl_lite_uncat")
        else:
            check(lib.tl_lite_uncat_group(ptr(dfeat), ptr(dy2), ptr(dh), self.M, B, F, H, ldf, self._p_used, ptr(self.seed_dev),
                                          B * ldf, B * F, B * H, *tail), "tl_lite_uncat_group")

    # ------------------------------------------------------------------ M = 1: tensors without the member dimension
    def forward(self, t: Dict[str, torch.Tensor], x, labels, training: bool, save: bool, seed: int = 0, row0: int = 0):
        B, Cn, T = x.shape
        if Cn != self.C or T != self.T:
            raise ValueError(f"expected ECoG input (B, {self.C}, {self.T}), got {tuple(x.shape)}")
        if labels.dim() != 3 or labels.shape[0] != B or labels.shape[1] != self.in_dim:
            raise ValueError(f"expected labels (B, {self.in_dim}, L), got {tuple(labels.shape)}")
        self._seed = (seed + 0x9E3779B97F4A7C15 * int(row0)) & 0xFFFFFFFFFFFFFFFF   # data-parallel shards draw different masks
        return self._forward(t, x, labels, B, training, save)[0]

    def backward(self, t: Dict[str, torch.Tensor], dout: torch.Tensor, grads: Dict[str, torch.Tensor],
                 gather_whh=None, whh_factors: bool = False, reduce_rows=None, on_factors=None) -> None:
        self._backward(t, dout, grads)

    def _colsum(self, G, rows, ncols, ld, s_G, dst):
        """Column sums per member: G (M, rows, ld) -> dst (M, ncols)."""
        M = self.M
        nc4 = r4(ncols)
        rpb = max(1, 256 // (nc4 // 4))
        nblk = int(min(256, max(1, rows // (rpb * 4))))
        part = torch.empty(M, nblk, nc4, dtype=torch.float32, device=G.device)
        check(self.lib.tl_colsum_group(ptr(G), ptr(part), nblk, rows, nc4, ld, 1, 1, M, s_G, nblk * nc4,
                                       *self._tail), "tl_colsum_group")
        # the reduction takes the wave-parallel kernel for nz >= 64 slabs and at most 16384 outputs: keep a launch's outputs
        # inside the bound one member (ncols outputs) meets, so that every member is summed in the order of M = 1
        per = M if nblk < 64 or M * ncols <= 16384 else max(1, 16384 // ncols)
        for m0 in range(0, M, per):
            n = min(per, M - m0)
            self._permute(part[m0:], dst[m0:], (1, 1, n, ncols), (0, 0, nblk * nc4, 1), nz=nblk, zs=nc4)

    # ------------------------------------------------------------------ forward
    def _forward(self, t: Dict[str, torch.Tensor], x, labels, B: int, training: bool, save: bool):
        """x (M, B, C, T), labels (M, B, label_dim, L), every tensor of ``t`` (M, ...) -> (M, B, out_dim)."""
        M, (lib, tail) = self.M, self._begin()
        f32 = dict(dtype=torch.float32, device=x.device)
        x = x.contiguous().float()
        self.generation += 1
        self._B, self._x, self._training = B, x, training
        p_drop = self._p_used = self.p_drop if training else 0.0
        Cn, T, CC, T1, T2, H, D = self.C, self.T, self.CC, self.T1, self.T2, self.H, self.out_dim
        nt1, nt2 = (T + 63) // 64, (T1 + 63) // 64
        # block 1
        self.z1 = torch.empty(M, B, CC, T, **f32)
        part = torch.empty(M, B * nt1, CC, 2, **f32)
        check(lib.tl_lite_conv_fwd_group(ptr(x), ptr(t["ecog_conv.0.weight"]), ptr(t["ecog_conv.0.bias"]), ptr(self.z1),
                                         ptr(part), M, B, Cn, CC, T, 5, 2, B * Cn * T, CC * Cn * 5, CC, B * CC * T,
                                         B * nt1 * CC * 2, *tail), "tl_lite_conv_fwd_group")
        self.m1, self.r1 = torch.empty(M, CC, **f32), torch.empty(M, CC, **f32)
        check(lib.tl_lite_bn_finalize_group(ptr(part), ptr(self.m1), ptr(self.r1), ptr(t["ecog_conv.1.running_mean"]),
                                            ptr(t["ecog_conv.1.running_var"]), M, B * nt1, CC, B * T, T, 0.1, 1e-5, int(training),
                                            ptr(t["ecog_conv.1.num_batches_tracked"]), B * nt1 * CC * 2, CC, CC, 1,
                                            *tail), "tl_lite_bn_finalize_group")
        self.y1 = torch.empty(M, B, CC, T1, **f32)
        check(lib.tl_lite_bn_act_pool_fwd_group(ptr(self.z1), ptr(self.m1), ptr(self.r1), ptr(t["ecog_conv.1.weight"]),
                                                ptr(t["ecog_conv.1.bias"]), ptr(self.y1), M, B, CC, T, self.slope, B * CC * T, CC,
                                                CC, B * CC * T1, *tail), "tl_lite_bn_act_pool_fwd_group")
        # block 2
        self.z2 = torch.empty(M, B, CC, T1, **f32)
        part2 = torch.empty(M, B * nt2, CC, 2, **f32)
        check(lib.tl_lite_conv_fwd_group(ptr(self.y1), ptr(t["ecog_conv.4.weight"]), ptr(t["ecog_conv.4.bias"]), ptr(self.z2),
                                         ptr(part2), M, B, CC, CC, T1, 3, 1, B * CC * T1, CC * CC * 3, CC, B * CC * T1,
                                         B * nt2 * CC * 2, *tail), "tl_lite_conv_fwd_group")
        self.m2, self.r2 = torch.empty(M, CC, **f32), torch.empty(M, CC, **f32)
        check(lib.tl_lite_bn_finalize_group(ptr(part2), ptr(self.m2), ptr(self.r2), ptr(t["ecog_conv.5.running_mean"]),
                                            ptr(t["ecog_conv.5.running_var"]), M, B * nt2, CC, B * T1, T1, 0.1, 1e-5,
                                            int(training), ptr(t["ecog_conv.5.num_batches_tracked"]), B * nt2 * CC * 2, CC, CC, 1,
                                            *tail), "tl_lite_bn_finalize_group")
        y2 = torch.empty(M, B, CC, T2, **f32)
        check(lib.tl_lite_bn_act_pool_fwd_group(ptr(self.z2), ptr(self.m2), ptr(self.r2), ptr(t["ecog_conv.5.weight"]),
                                                ptr(t["ecog_conv.5.bias"]), ptr(y2), M, B, CC, T1, self.slope, B * CC * T1, CC,
                                                CC, B * CC * T2, *tail), "tl_lite_bn_act_pool_fwd_group")
        # label LSTM
        L = self._L = labels.shape[-1]
        self.xl = labels.float().transpose(-1, -2).contiguous()
        self.act = torch.empty(M, B, L, 4 * H, **f32)
        self.cs = torch.empty(M, B, L, H, **f32)
        self.hs = torch.empty(M, B, L, H, **f32)
        check(lib.tl_lite_lstm_fwd_group(ptr(self.xl), ptr(t["label_lstm.weight_ih_l0"]), ptr(t["label_lstm.weight_hh_l0"]),
                                         ptr(t["label_lstm.bias_ih_l0"]), ptr(t["label_lstm.bias_hh_l0"]), ptr(self.act),
                                         ptr(self.cs), ptr(self.hs), M, B, L, H, self.in_dim, B * L * self.in_dim,
                                         4 * H * self.in_dim, 4 * H * H, 4 * H, B * L * 4 * H, B * L * H,
                                         *tail), "tl_lite_lstm_fwd_group")
        # concat + dropout, fc.1 + LeakyReLU, fc.3
        ldf, hid, fh = self.ldf, self.hid, self.F + H
        self.feat = torch.empty(M, B, ldf, **f32)
        self._cat(y2, B, L, p_drop)
        w1 = t["fc.1.weight"]
        if ldf != fh:
            w1p = torch.empty(M, hid, ldf, **f32)
            self._permute(w1, w1p, (1, M, hid, ldf), (0, hid * fh, fh, 1), (1, M, hid, fh))
            w1 = w1p
        # fc.1: M = B is small, so the grid comes from split-K (32-row tiles x 4 column tiles x splits)
        bm = 32 if B <= 64 else 128
        tiles = ((B + bm - 1) // bm) * ((hid + 127) // 128)
        sk = int(max(1, min((ldf + 31) // 32, 256 // tiles)))
        slab = torch.empty(M, sk, B, hid, **f32)
        self._nt(B * ldf, hid * ldf, 0, 0, sk * B * hid, A=ptr(self.feat), Bw=ptr(w1), out=ptr(slab), M=B, A_rows=B, N=hid,
                 K=ldf, lda=ldf, ldb=ldf, ldo=hid, loader=LOAD_DIRECT, epilogue=EPI_STORE, bm=bm, splitk=sk, slab_stride=B * hid)
        self.a1 = torch.empty(M, B, hid, **f32)
        check(lib.tl_splitk_bias_lrelu_group(ptr(slab), ptr(t["fc.1.bias"]), ptr(self.a1), sk, B * hid, hid, self.slope, M,
                                             B * hid, sk * B * hid, hid, B * hid, *tail), "tl_splitk_bias_lrelu_group")
        out = torch.empty(M, B, D, **f32)
        tiles3 = ((B + bm - 1) // bm) * ((D + 127) // 128)
        sk3 = int(max(1, min((hid + 31) // 32, 64 // tiles3)))
        w3, b3 = t["fc.3.weight"], t["fc.3.bias"]
        if sk3 > 1:           # one or two tiles of a 16-step K loop are latency-bound (48 us): split K, reduce + bias after
            slab3 = torch.empty(M, sk3, B, D, **f32)
            self._nt(B * hid, D * hid, 0, 0, sk3 * B * D, A=ptr(self.a1), Bw=ptr(w3), out=ptr(slab3), M=B, A_rows=B, N=D, K=hid,
                     lda=hid, ldb=hid, ldo=D, loader=LOAD_DIRECT, epilogue=EPI_STORE, bm=bm, splitk=sk3, slab_stride=B * D)
            self._fc3_sum(slab3, b3, out, sk3, B)
        else:
            self._nt(B * hid, D * hid, D, 0, B * D, A=ptr(self.a1), Bw=ptr(w3), bias=ptr(b3), out=ptr(out), M=B, A_rows=B, N=D,
                     K=hid, lda=hid, ldb=hid, ldo=D, loader=LOAD_DIRECT, epilogue=EPI_STORE, bm=bm)
        if save:
            self._saved_generation = self.generation
        return out

    # ------------------------------------------------------------------ backward
    def _backward(self, t: Dict[str, torch.Tensor], dout: torch.Tensor, grads: Dict[str, torch.Tensor]) -> None:
        """dout (M, B, ldd) -> ``grads`` (every entry (M, ...))."""
        if self._saved_generation != self.generation:
            raise RuntimeError(f"{self.NAME} backward: the forward intermediates were overwritten by a later forward")
        M, B, L, (lib, tail) = self.M, self._B, self._L, self._begin()
        f32 = dict(dtype=torch.float32, device=dout.device)
        CC, T, T1, T2, H, D = self.CC, self.T, self.T1, self.T2, self.H, self.out_dim
        fh = self.F + H
        hid, ldd, ldf = self.hid, self.ldd, self.ldf
        # fc.3
        # the weight-gradient GEMMs write straight into the gradient tensors when their padded extents equal the true
        # ones (out_dim and F + H multiples of 4 - the reference's sizes are): no slab, no copy
        direct3 = ldd == D and grads["fc.3.weight"].is_contiguous()
        slab = grads["fc.3.weight"] if direct3 else torch.empty(M, ldd, hid, **f32)
        # (short reductions: the bias gradient = the column sums of the same operand comes out of the weight-gradient kernel)
        cs3 = ldd == D and B <= MAX_ROWS and ldd * hid <= MAX_OUT
        self._tn(B * ldd, B * hid, ldd * hid, D, A=ptr(dout), B=ptr(self.a1), slab=ptr(slab), Krows=B, A_rows=B, B_rows=B,
                 Mdim=ldd, Ndim=hid, lda=ldd, ldb=hid, ldc=hid, loader=LOAD_DIRECT, colsum=ptr(grads["fc.3.bias"]) if cs3 else None)
        if not direct3:
            grads["fc.3.weight"].view(M, D, hid).copy_(slab[:, :D])
        if not cs3:
            self._colsum(dout, B, D, ldd, B * ldd, grads["fc.3.bias"])
        w2t = torch.empty(M, hid, ldd, **f32)
        self._permute(t["fc.3.weight"], w2t, (1, M, hid, ldd), (0, D * hid, 1, hid), (1, M, hid, D))
        g1 = torch.empty(M, B, hid, **f32)
        bm = 32 if B <= 64 else 128            # small batches: 32-row tiles, the grid comes from columns / split-K
        self._nt(B * ldd, hid * ldd, 0, B * hid, B * hid, A=ptr(dout), Bw=ptr(w2t), aux=ptr(self.a1), out=ptr(g1), M=B, A_rows=B,
                 N=hid, K=ldd, lda=ldd, ldb=ldd, ldo=hid, ldaux=hid, loader=LOAD_DIRECT, epilogue=EPI_MASK, slope=self.slope, bm=bm)
        # fc.1
        direct1 = ldf == fh and grads["fc.1.weight"].is_contiguous()
        slab1 = grads["fc.1.weight"] if direct1 else torch.empty(M, hid, ldf, **f32)
        cs1 = B <= MAX_ROWS and hid * ldf <= MAX_OUT
        self._tn(B * hid, B * ldf, hid * ldf, hid, A=ptr(g1), B=ptr(self.feat), slab=ptr(slab1), Krows=B, A_rows=B, B_rows=B,
                 Mdim=hid, Ndim=ldf, lda=hid, ldb=ldf, ldc=ldf, loader=LOAD_DIRECT, colsum=ptr(grads["fc.1.bias"]) if cs1 else None)
        if not direct1:
            grads["fc.1.weight"].view(M, hid, fh).copy_(slab1[:, :, :fh])
        if not cs1:
            self._colsum(g1, B, hid, hid, B * hid, grads["fc.1.bias"])
        w1t = torch.empty(M, ldf, hid, **f32)
        self._permute(t["fc.1.weight"], w1t, (1, M, ldf, hid), (0, hid * fh, 1, fh), (1, M, fh, hid))
        dfeat = torch.empty(M, B, ldf, **f32)
        tiles = ((B + bm - 1) // bm) * ((ldf + 127) // 128)
        sk = int(max(1, min((hid + 31) // 32, 256 // tiles)))
        if sk > 1:
            slab_d = torch.empty(M, sk, B, ldf, **f32)
            self._nt(B * hid, ldf * hid, 0, 0, sk * B * ldf, A=ptr(g1), Bw=ptr(w1t), out=ptr(slab_d), M=B, A_rows=B, N=ldf, K=hid,
                     lda=hid, ldb=hid, ldo=ldf, loader=LOAD_DIRECT, epilogue=EPI_STORE, bm=bm, splitk=sk, slab_stride=B * ldf)
            self._permute(slab_d, dfeat, (1, 1, M, B * ldf), (0, 0, sk * B * ldf, 1), nz=sk, zs=B * ldf)
        else:
            self._nt(B * hid, ldf * hid, 0, 0, B * ldf, A=ptr(g1), Bw=ptr(w1t), out=ptr(dfeat), M=B, A_rows=B, N=ldf, K=hid,
                     lda=hid, ldb=hid, ldo=ldf, loader=LOAD_DIRECT, epilogue=EPI_STORE, bm=bm)
        dy2 = torch.empty(M, B, CC, T2, **f32)
        dh = torch.empty(M, B, H, **f32)
        self._uncat(dfeat, dy2, dh, B)
        # LSTM
        dg = torch.empty(M, B, L, 4 * H, **f32)
        check(lib.tl_lite_lstm_bwd_group(ptr(dh), ptr(t["label_lstm.weight_hh_l0"]), ptr(self.act), ptr(self.cs), ptr(dg), M, B,
                                         L, H, H, B * H, 4 * H * H, B * L * 4 * H, B * L * H, *tail), "tl_lite_lstm_bwd_group")
        gwhh = grads["label_lstm.weight_hh_l0"]
        if L > 1:
            kr = B * L - 1          # pairs (dg[b,t], h[b,t-1]): A row R+1, B row R, rows with R%L == L-1 masked
            if r4(H) != H:
                raise ValueError("lstm_hidden must be a multiple of 4 on the MI355X path")
            # a few hundred rows: the reduction is split over 64-row chunks (tn_short_kernel), the slabs summed in order
            sk = max(1, min(8, (kr + 63) // 64))
            slab = gwhh if sk == 1 else torch.empty(M, sk, 4 * H, H, **f32)
            self._tn(B * L * 4 * H, B * L * H, sk * 4 * H * H, 0, A=dg.data_ptr() + 4 * 4 * H, B=ptr(self.hs), slab=ptr(slab),
                     Krows=kr, A_rows=kr, B_rows=kr, Mdim=4 * H, Ndim=H, lda=4 * H, ldb=H, ldc=H, loader=LOAD_DIRECT, Tp=L,
                     Tvalid=L - 1, splitk=sk, slab_stride=4 * H * H)
            if sk > 1:
                self._permute(slab, gwhh, (1, 1, M, 4 * H * H), (0, 0, sk * 4 * H * H, 1), nz=sk, zs=4 * H * H)
        else:
            gwhh.zero_()
        check(lib.tl_lstm_ih_grad_group(ptr(dg), ptr(self.xl), ptr(grads["label_lstm.weight_ih_l0"]),
                                        ptr(grads["label_lstm.bias_ih_l0"]), ptr(grads["label_lstm.bias_hh_l0"]), M, 1, B * L, H,
                                        self.in_dim, B * L * 4 * H, B * L * self.in_dim, 4 * H * self.in_dim, 4 * H,
                                        *tail), "tl_lstm_ih_grad_group")
        # block 2
        n_work = B * CC * 2 + CC * 2
        work = torch.empty(M, n_work, **f32)
        dz2 = torch.empty(M, B, CC, T1, **f32)
        check(lib.tl_lite_bn_act_pool_bwd_group(ptr(dy2), ptr(self.z2), ptr(self.m2), ptr(self.r2), ptr(t["ecog_conv.5.weight"]),
                                                ptr(t["ecog_conv.5.bias"]), ptr(dz2), ptr(grads["ecog_conv.5.weight"]),
                                                ptr(grads["ecog_conv.5.bias"]), ptr(work), M, B, CC, T1, self.slope,
                                                int(self._training), B * CC * T2, B * CC * T1, CC, CC, B * CC * T1, CC, n_work,
                                                *tail), "tl_lite_bn_act_pool_bwd_group")
        dy1 = torch.empty(M, B, CC, T1, **f32)
        n2 = CC * CC * 3
        dwp = torch.empty(M, B, n2, **f32)
        dbp = torch.empty(M, B, CC, **f32)
        check(lib.tl_lite_conv_bwd_group(ptr(dz2), ptr(self.y1), ptr(t["ecog_conv.4.weight"]), ptr(dy1), ptr(dwp), ptr(dbp), M, B,
                                         CC, CC, T1, 3, 1, B * CC * T1, B * CC * T1, n2, B * CC * T1, B * n2, B * CC,
                                         *tail), "tl_lite_conv_bwd_group")
        check(lib.tl_sum_slabs2_group(ptr(dwp), ptr(grads["ecog_conv.4.weight"]), n2, ptr(dbp), ptr(grads["ecog_conv.4.bias"]),
                                      CC, B, M, B * n2, n2, B * CC, CC, *tail), "tl_sum_slabs2_group")
        # block 1
        dz1 = torch.empty(M, B, CC, T, **f32)
        check(lib.tl_lite_bn_act_pool_bwd_group(ptr(dy1), ptr(self.z1), ptr(self.m1), ptr(self.r1), ptr(t["ecog_conv.1.weight"]),
                                                ptr(t["ecog_conv.1.bias"]), ptr(dz1), ptr(grads["ecog_conv.1.weight"]),
                                                ptr(grads["ecog_conv.1.bias"]), ptr(work), M, B, CC, T, self.slope,
                                                int(self._training), B * CC * T1, B * CC * T, CC, CC, B * CC * T, CC, n_work,
                                                *tail), "tl_lite_bn_act_pool_bwd_group")
        n1 = CC * self.C * 5
        dwp1 = torch.empty(M, B, n1, **f32)
        check(lib.tl_lite_conv_bwd_group(ptr(dz1), ptr(self._x), ptr(t["ecog_conv.0.weight"]), None, ptr(dwp1), ptr(dbp), M, B,
                                         self.C, CC, T, 5, 2, B * CC * T, B * self.C * T, n1, 0, B * n1, B * CC,
                                         *tail), "tl_lite_conv_bwd_group")
        check(lib.tl_sum_slabs2_group(ptr(dwp1), ptr(grads["ecog_conv.0.weight"]), n1, ptr(dbp), ptr(grads["ecog_conv.0.bias"]),
                                      CC, B, M, B * n1, n1, B * CC, CC, *tail), "tl_sum_slabs2_group")
