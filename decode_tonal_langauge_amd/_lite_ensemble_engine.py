"""All repeats of a SynthesisLite experiment in one pass: M ``SynthesisLite`` models of equal shape ("members") trained side by
side by the launches that train one (``_lite_engine.LiteEngine``).

The Lite step is ~55 launches of 4-20 us that occupy a few of the 256 CUs each: it is bound by launches, not by the GPU.  The
group kernels (``tl_lite_*_group`` and their neighbours, include/tonal_hip.h) are the same kernels with a member dimension on
the grid - the single entries launch them with M = 1 - so a step of M members is the same number of launches, and every member
gets the bits ``LiteEngine`` gives it on the same inputs.  ``forward`` / ``backward`` below mirror ``LiteEngine``'s launch for
launch: the same split-K factors, the same ``bm``, the same direct-vs-slab choices, each taken from one member's sizes.

Storage is stacked: every parameter, BatchNorm buffer, gradient and (in the optimiser) NAdam moment is (M, ...), and each
member's module holds views of the stacks, so ``state_dict()``, ``torch.save``, ``model(x, labels)`` and
``SynthesisTrainer.evaluate`` on a member keep working through the single path.

Where ``tl_permute_reduce`` is used the member rides a free dimension of its 4-d view.  The kernel it picks depends on the last
dimension, on the number of slabs nz and - its wave-parallel form, nz >= 64 and at most 16384 outputs - on the number of outputs,
which grows with M: the pad, the transposes and the split-K sums have nz <= 16 and so take the single launch's kernel for any
M; the ``_colsum`` fallback (up to 256 slabs) cuts the members into launches that stay inside the bound, so only there can the
launch count depend on M (M > 32 with out_dim >= 512).  fc.3's split-K reduction adds a per-member bias row and therefore runs
on ``tl_splitk_bias_lrelu_group`` with slope 1 (the identity: the same sum in the same order).

Out of scope (refused with the supported set): other model classes, members of unequal constructor arguments, parameters that
are not fp32 on one CUDA device, a multi-rank process group, and what takes one of the three weight-gradient GEMMs off the
short-reduction kernel, the only TN kernel with a member dimension: training batches with B > 512 or B L - 1 > 512, and
models with 512 * r4(conv_channels * (n_timepoints // 4) + lstm_hidden) > 2^20 or r4(output_dim) * 512 > 2^20 (the fc.1 / fc.3
weight gradient; the default model from 252 time points on).  No CPU fallback."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Sequence

import torch

from . import _lib, parallel
from ._launch import permute_reduce, r4
from ._lib import EPI_MASK, EPI_STORE, LOAD_DIRECT, NtParams, TnParams, check, ptr

MAX_ROWS = 512        # Krows of tn_short_kernel (8 chunks of 64 rows)
MAX_OUT = 1 << 20     # Mdim * Ndim of tn_short_kernel

SUPPORTED = ("the synthesis ensemble supports one or more SynthesisLite models of equal constructor arguments (output_dim, "
             "n_channels, n_timepoints, label_dim, conv_channels, lstm_hidden, dropout, negative_slope) with fp32 parameters on "
             "one CUDA device, in a single process (no multi-rank process group), fc.1 of at most 2048 padded inputs "
             "(r4(conv_channels * (n_timepoints // 4) + lstm_hidden) <= 2048) and output_dim <= 2048 (the weight gradients of "
             "wider layers run on GEMM kernels without a member dimension), and training batches of B <= 512 rows with "
             "B * L - 1 <= 512 (L = length of the label sequence)")


def refuse(why: str):
    raise ValueError(f"{why}: {SUPPORTED}")


def _signature(m) -> tuple:
    e = m._engine
    return (e.out_dim, e.C, e.T, e.in_dim, e.CC, e.H, e.p_drop, e.slope)


def check_supported(models: Sequence) -> None:
    """Raise ``ValueError`` (stating the supported set) unless ``models`` can be trained by ``LiteEnsembleEngine``."""
    from .models.synthesis_models import SynthesisLite
    models = list(models)
    if not models:
        refuse("no models")
    for m in models:
        if not isinstance(m, SynthesisLite):
            refuse(f"model {type(m).__name__}")
    first = _signature(models[0])
    for i, m in enumerate(models):
        if _signature(m) != first:
            refuse(f"member {i} was built with {_signature(m)}, member 0 with {first}")
    e = models[0]._engine
    if e.hid * e.ldf > MAX_OUT:
        refuse(f"fc.1 with {e.ldf} padded inputs (conv_channels {e.CC} * (n_timepoints {e.T} // 4) + lstm_hidden {e.H})")
    if e.ldd * e.hid > MAX_OUT:
        refuse(f"output_dim {e.out_dim}")
    if parallel.world()[1] > 1:
        refuse(f"a process group of {parallel.world()[1]} ranks")
    dev = None
    for m in models:
        for name, t in list(m.named_parameters()) + list(m.named_buffers()):
            if t.is_floating_point() and t.dtype != torch.float32:
                refuse(f"'{name}' of dtype {t.dtype}")
            if t.device.type != "cuda":
                refuse(f"'{name}' on '{t.device}'")
            if dev is not None and t.device != dev:
                refuse(f"parameters on '{t.device}' and '{dev}'")
            dev = t.device


def check_train_batch(B: int, L: int) -> None:
    """Raise ``ValueError`` for a training batch the group cannot take: B <= 512 and B L - 1 <= 512."""
    if B > MAX_ROWS or B * L - 1 > MAX_ROWS:
        refuse(f"a training batch of B = {B} rows with label length L = {L} (B * L - 1 = {B * L - 1})")


class LiteEnsembleEngine:
    def __init__(self, models: Sequence):
        check_supported(models)
        self.models = list(models)
        self.lib = _lib.load()
        M = self.M = len(self.models)
        e = self.models[0]._engine
        self.out_dim, self.C, self.T, self.in_dim, self.CC, self.H = e.out_dim, e.C, e.T, e.in_dim, e.CC, e.H
        self.p_drop, self.slope = e.p_drop, e.slope
        self.T1, self.T2, self.F, self.ldf, self.ldd, self.hid = e.T1, e.T2, e.F, e.ldf, e.ldd, e.hid
        first = self.models[0]
        self.device = next(first.parameters()).device
        self.names = list(first._pnames)
        # parameters and buffers move into the stacks; the modules keep views of them
        self.params: Dict[str, torch.Tensor] = {}
        self.buffers: Dict[str, torch.Tensor] = {}
        with torch.no_grad():
            for name in self.names:
                ps = [dict(m.named_parameters())[name] for m in self.models]
                stack = torch.stack([p.detach() for p in ps]).contiguous()
                for m, p in enumerate(ps):
                    p.data = stack[m]
                self.params[name] = stack
            for name, _ in first.named_buffers():
                bs = [dict(m.named_buffers())[name] for m in self.models]
                stack = torch.stack([b.detach() for b in bs]).contiguous()
                for m, b in enumerate(bs):
                    b.data = stack[m]
                self.buffers[name] = stack
        self.grads = {k: torch.zeros_like(v) for k, v in self.params.items()}
        self.seeds = torch.zeros(M, dtype=torch.int64, device=self.device)       # the dropout seed table, one word per member
        self.active: Optional[torch.Tensor] = None
        self.generation = 0
        self._saved_generation = -1

    # ------------------------------------------------------------------ launch helpers
    def _stream(self):
        return torch.cuda.current_stream().cuda_stream

    def _call(self, name: str, *args) -> None:
        check(getattr(self.lib, name)(*args, ptr(self.active), self._stream()), name)

    def _nt(self, s_A, s_Bw, s_bias, s_aux, s_out, **fields) -> None:
        p = NtParams(**{**dict(splitk=1, bm=128, J=1, Tp=1, slope=0.0), **fields})
        self._call("tl_gemm_nt_window_group_fc", C.byref(p), self.M, s_A, s_Bw, s_bias, s_aux, s_out)

    def _tn(self, s_A, s_B, s_slab, s_colsum, **fields) -> None:
        p = TnParams(**{**dict(splitk=1, J=1, Tp=1, Tvalid=1), **fields})
        self._call("tl_gemm_tn_window_group", C.byref(p), self.M, s_A, s_B, s_slab, s_colsum)

    def _permute(self, src, dst, dims, strides, *args, **kw):
        permute_reduce(self.lib, src, dst, dims, strides, *args, **kw)

    def _colsum(self, G, rows, ncols, ld, s_G, dst):
        """``LiteEngine._colsum`` per member: G (M, rows, ld) -> dst (M, ncols)."""
        M = self.M
        nc4 = r4(ncols)
        rpb = max(1, 256 // (nc4 // 4))
        nblk = int(min(256, max(1, rows // (rpb * 4))))
        part = torch.empty(M, nblk, nc4, dtype=torch.float32, device=G.device)
        self._call("tl_colsum_group", ptr(G), ptr(part), nblk, rows, nc4, ld, 1, 1, M, s_G, nblk * nc4)
        # the reduction takes the wave-parallel kernel for nz >= 64 slabs and at most 16384 outputs: keep a launch's outputs
        # inside the bound the single launch (ncols outputs) meets, so that every member is summed in the single launch's order
        per = M if nblk < 64 or M * ncols <= 16384 else max(1, 16384 // ncols)
        for m0 in range(0, M, per):
            n = min(per, M - m0)
            self._permute(part[m0:], dst[m0:], (1, 1, n, ncols), (0, 0, nblk * nc4, 1), nz=nblk, zs=nc4)

    # ------------------------------------------------------------------ forward
    def forward(self, x: torch.Tensor, labels: torch.Tensor, training: bool, save: bool = True) -> torch.Tensor:
        """x (M, B, C, T), labels (M, B, label_dim, L) -> (M, B, out_dim).  The dropout seeds are read from ``self.seeds``."""
        M = self.M
        if x.dim() != 4 or x.shape[0] != M or x.shape[2] != self.C or x.shape[3] != self.T:
            raise ValueError(f"expected ECoG input ({M}, B, {self.C}, {self.T}), got {tuple(x.shape)}")
        B = x.shape[1]
        if labels.dim() != 4 or tuple(labels.shape[:3]) != (M, B, self.in_dim):
            raise ValueError(f"expected labels ({M}, B, {self.in_dim}, L), got {tuple(labels.shape)}")
        L = labels.shape[3]
        if training:
            check_train_batch(B, L)
        t = {**self.params, **self.buffers}
        f32 = dict(dtype=torch.float32, device=x.device)
        x = x.contiguous().float()
        self.generation += 1
        self._B, self._L, self._x, self._training = B, L, x, training
        p_drop = self.p_drop if training else 0.0
        self._p_used = p_drop
        Cn, T, CC, T1, T2, H = self.C, self.T, self.CC, self.T1, self.T2, self.H
        nt1, nt2 = (T + 63) // 64, (T1 + 63) // 64
        call = self._call
        # block 1
        self.z1 = torch.empty(M, B, CC, T, **f32)
        part = torch.empty(M, B * nt1, CC, 2, **f32)
        w0, b0 = t["ecog_conv.0.weight"], t["ecog_conv.0.bias"]
        call("tl_lite_conv_fwd_group", ptr(x), ptr(w0), ptr(b0), ptr(self.z1), ptr(part), M, B, Cn, CC, T, 5, 2,
             x.stride(0), w0.stride(0), b0.stride(0), self.z1.stride(0), part.stride(0))
        self.m1, self.r1 = torch.empty(M, CC, **f32), torch.empty(M, CC, **f32)
        call("tl_lite_bn_finalize_group", ptr(part), ptr(self.m1), ptr(self.r1), ptr(t["ecog_conv.1.running_mean"]),
             ptr(t["ecog_conv.1.running_var"]), M, B * nt1, CC, B * T, T, 0.1, 1e-5, int(training),
             ptr(t["ecog_conv.1.num_batches_tracked"]), part.stride(0), CC, CC, 1)
        self.y1 = torch.empty(M, B, CC, T1, **f32)
        call("tl_lite_bn_act_pool_fwd_group", ptr(self.z1), ptr(self.m1), ptr(self.r1), ptr(t["ecog_conv.1.weight"]),
             ptr(t["ecog_conv.1.bias"]), ptr(self.y1), M, B, CC, T, self.slope, self.z1.stride(0), CC, CC, self.y1.stride(0))
        # block 2
        self.z2 = torch.empty(M, B, CC, T1, **f32)
        part2 = torch.empty(M, B * nt2, CC, 2, **f32)
        w4, b4 = t["ecog_conv.4.weight"], t["ecog_conv.4.bias"]
        call("tl_lite_conv_fwd_group", ptr(self.y1), ptr(w4), ptr(b4), ptr(self.z2), ptr(part2), M, B, CC, CC, T1, 3, 1,
             self.y1.stride(0), w4.stride(0), b4.stride(0), self.z2.stride(0), part2.stride(0))
        self.m2, self.r2 = torch.empty(M, CC, **f32), torch.empty(M, CC, **f32)
        call("tl_lite_bn_finalize_group", ptr(part2), ptr(self.m2), ptr(self.r2), ptr(t["ecog_conv.5.running_mean"]),
             ptr(t["ecog_conv.5.running_var"]), M, B * nt2, CC, B * T1, T1, 0.1, 1e-5, int(training),
             ptr(t["ecog_conv.5.num_batches_tracked"]), part2.stride(0), CC, CC, 1)
        y2 = torch.empty(M, B, CC, T2, **f32)
        call("tl_lite_bn_act_pool_fwd_group", ptr(self.z2), ptr(self.m2), ptr(self.r2), ptr(t["ecog_conv.5.weight"]),
             ptr(t["ecog_conv.5.bias"]), ptr(y2), M, B, CC, T1, self.slope, self.z2.stride(0), CC, CC, y2.stride(0))
        # label LSTM
        self.xl = labels.float().permute(0, 1, 3, 2).contiguous()
        self.act = torch.empty(M, B, L, 4 * H, **f32)
        self.cs = torch.empty(M, B, L, H, **f32)
        self.hs = torch.empty(M, B, L, H, **f32)
        call("tl_lite_lstm_fwd_group", ptr(self.xl), ptr(t["label_lstm.weight_ih_l0"]), ptr(t["label_lstm.weight_hh_l0"]),
             ptr(t["label_lstm.bias_ih_l0"]), ptr(t["label_lstm.bias_hh_l0"]), ptr(self.act), ptr(self.cs), ptr(self.hs), M, B, L,
             H, self.in_dim, self.xl.stride(0), 4 * H * self.in_dim, 4 * H * H, 4 * H, self.act.stride(0), self.cs.stride(0))
        # concat + dropout, fc.1 + LeakyReLU, fc.3
        ldf, hid, fh = self.ldf, self.hid, self.F + H
        self.feat = torch.empty(M, B, ldf, **f32)
        call("tl_lite_cat_group", ptr(y2), ptr(self.hs), ptr(self.feat), M, B, self.F, H, L, ldf, p_drop, ptr(self.seeds),
             y2.stride(0), self.hs.stride(0), self.feat.stride(0))
        w1 = t["fc.1.weight"]
        if ldf != fh:
            w1p = torch.empty(M, hid, ldf, **f32)
            self._permute(w1, w1p, (1, M, hid, ldf), (0, hid * fh, fh, 1), (1, M, hid, fh))
            w1 = w1p
        bm = 32 if B <= 64 else 128
        tiles = ((B + bm - 1) // bm) * ((hid + 127) // 128)
        sk = int(max(1, min((ldf + 31) // 32, 256 // tiles)))
        slab = torch.empty(M, sk, B, hid, **f32)
        self._nt(B * ldf, hid * ldf, 0, 0, sk * B * hid, A=ptr(self.feat), Bw=ptr(w1), out=ptr(slab), M=B, A_rows=B, N=hid,
                 K=ldf, lda=ldf, ldb=ldf, ldo=hid, loader=LOAD_DIRECT, epilogue=EPI_STORE, bm=bm, splitk=sk, slab_stride=B * hid)
        self.a1 = torch.empty(M, B, hid, **f32)
        call("tl_splitk_bias_lrelu_group", ptr(slab), ptr(t["fc.1.bias"]), ptr(self.a1), sk, B * hid, hid, self.slope, M,
             B * hid, sk * B * hid, hid, B * hid)
        D = self.out_dim
        out = torch.empty(M, B, D, **f32)
        tiles3 = ((B + bm - 1) // bm) * ((D + 127) // 128)
        sk3 = int(max(1, min((hid + 31) // 32, 64 // tiles3)))
        w3, b3 = t["fc.3.weight"], t["fc.3.bias"]
        if sk3 > 1:
            slab3 = torch.empty(M, sk3, B, D, **f32)
            self._nt(B * hid, D * hid, 0, 0, sk3 * B * D, A=ptr(self.a1), Bw=ptr(w3), out=ptr(slab3), M=B, A_rows=B, N=D, K=hid,
                     lda=hid, ldb=hid, ldo=D, loader=LOAD_DIRECT, epilogue=EPI_STORE, bm=bm, splitk=sk3, slab_stride=B * D)
            # sum of the slabs + the member's bias row: the reduction of the single step (tl_permute_reduce with a bias) as
            # tl_splitk_bias_lrelu with slope 1 - the same additions in the same order, and v * 1 = v
            call("tl_splitk_bias_lrelu_group", ptr(slab3), ptr(b3), ptr(out), sk3, B * D, D, 1.0, M, B * D, sk3 * B * D, D, B * D)
        else:
            self._nt(B * hid, D * hid, D, 0, B * D, A=ptr(self.a1), Bw=ptr(w3), bias=ptr(b3), out=ptr(out), M=B, A_rows=B, N=D,
                     K=hid, lda=hid, ldb=hid, ldo=D, loader=LOAD_DIRECT, epilogue=EPI_STORE, bm=bm)
        if save:
            self._saved_generation = self.generation
        return out

    # ------------------------------------------------------------------ backward
    def backward(self, dout: torch.Tensor) -> None:
        """dout (M, B, ldd) -> ``self.grads`` (every entry (M, ...))."""
        if self._saved_generation != self.generation:
            raise RuntimeError("SynthesisLite ensemble backward: the forward intermediates were overwritten by a later forward")
        M, B, L = self.M, self._B, self._L
        t = {**self.params, **self.buffers}
        grads = self.grads
        f32 = dict(dtype=torch.float32, device=dout.device)
        CC, T, T1, T2, H, D = self.CC, self.T, self.T1, self.T2, self.H, self.out_dim
        fh = self.F + H
        hid, ldd, ldf = self.hid, self.ldd, self.ldf
        call = self._call
        # fc.3
        direct3 = ldd == D
        slab = grads["fc.3.weight"] if direct3 else torch.empty(M, ldd, hid, **f32)
        cs3 = ldd == D              # (B <= 512 and ldd * hid <= 2^20 hold for every batch and model the group takes)
        self._tn(B * ldd, B * hid, ldd * hid, D, A=ptr(dout), B=ptr(self.a1), slab=ptr(slab), Krows=B, A_rows=B, B_rows=B,
                 Mdim=ldd, Ndim=hid, lda=ldd, ldb=hid, ldc=hid, loader=LOAD_DIRECT, colsum=ptr(grads["fc.3.bias"]) if cs3 else None)
        if not direct3:
            grads["fc.3.weight"].copy_(slab[:, :D])
        if not cs3:
            self._colsum(dout, B, D, ldd, B * ldd, grads["fc.3.bias"])
        w2t = torch.empty(M, hid, ldd, **f32)
        self._permute(t["fc.3.weight"], w2t, (1, M, hid, ldd), (0, D * hid, 1, hid), (1, M, hid, D))
        g1 = torch.empty(M, B, hid, **f32)
        bm = 32 if B <= 64 else 128
        self._nt(B * ldd, hid * ldd, 0, B * hid, B * hid, A=ptr(dout), Bw=ptr(w2t), aux=ptr(self.a1), out=ptr(g1), M=B, A_rows=B,
                 N=hid, K=ldd, lda=ldd, ldb=ldd, ldo=hid, ldaux=hid, loader=LOAD_DIRECT, epilogue=EPI_MASK, slope=self.slope, bm=bm)
        # fc.1
        direct1 = ldf == fh
        slab1 = grads["fc.1.weight"] if direct1 else torch.empty(M, hid, ldf, **f32)
        # (the bias gradient always rides in the kernel: B <= 512 and hid * ldf <= 2^20 for everything the group takes)
        self._tn(B * hid, B * ldf, hid * ldf, hid, A=ptr(g1), B=ptr(self.feat), slab=ptr(slab1), Krows=B, A_rows=B, B_rows=B,
                 Mdim=hid, Ndim=ldf, lda=hid, ldb=ldf, ldc=ldf, loader=LOAD_DIRECT, colsum=ptr(grads["fc.1.bias"]))
        if not direct1:
            grads["fc.1.weight"].copy_(slab1[:, :, :fh])
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
        call("tl_lite_uncat_group", ptr(dfeat), ptr(dy2), ptr(dh), M, B, self.F, H, ldf, self._p_used, ptr(self.seeds), B * ldf,
             dy2.stride(0), B * H)
        # LSTM
        dg = torch.empty(M, B, L, 4 * H, **f32)
        call("tl_lite_lstm_bwd_group", ptr(dh), ptr(t["label_lstm.weight_hh_l0"]), ptr(self.act), ptr(self.cs), ptr(dg), M, B, L,
             H, H, B * H, 4 * H * H, self.act.stride(0), self.cs.stride(0))
        gwhh = grads["label_lstm.weight_hh_l0"]
        if L > 1:
            kr = B * L - 1
            if r4(H) != H:
                raise ValueError("lstm_hidden must be a multiple of 4 on the MI355X path")
            sk = max(1, min(8, (kr + 63) // 64))
            slab = gwhh if sk == 1 else torch.empty(M, sk, 4 * H, H, **f32)
            self._tn(dg.stride(0), self.hs.stride(0), sk * 4 * H * H, 0, A=dg.data_ptr() + 4 * 4 * H, B=ptr(self.hs),
                     slab=ptr(slab), Krows=kr, A_rows=kr, B_rows=kr, Mdim=4 * H, Ndim=H, lda=4 * H, ldb=H, ldc=H,
                     loader=LOAD_DIRECT, Tp=L, Tvalid=L - 1, splitk=sk, slab_stride=4 * H * H)
            if sk > 1:
                self._permute(slab, gwhh, (1, 1, M, 4 * H * H), (0, 0, sk * 4 * H * H, 1), nz=sk, zs=4 * H * H)
        else:
            gwhh.zero_()
        call("tl_lstm_ih_grad_group", ptr(dg), ptr(self.xl), ptr(grads["label_lstm.weight_ih_l0"]),
             ptr(grads["label_lstm.bias_ih_l0"]), ptr(grads["label_lstm.bias_hh_l0"]), M, 1, B * L, H, self.in_dim, dg.stride(0),
             self.xl.stride(0), 4 * H * self.in_dim, 4 * H)
        # block 2
        work = torch.empty(M, B * CC * 2 + CC * 2, **f32)
        dz2 = torch.empty(M, B, CC, T1, **f32)
        call("tl_lite_bn_act_pool_bwd_group", ptr(dy2), ptr(self.z2), ptr(self.m2), ptr(self.r2), ptr(t["ecog_conv.5.weight"]),
             ptr(t["ecog_conv.5.bias"]), ptr(dz2), ptr(grads["ecog_conv.5.weight"]), ptr(grads["ecog_conv.5.bias"]), ptr(work),
             M, B, CC, T1, self.slope, int(self._training), dy2.stride(0), self.z2.stride(0), CC, CC, dz2.stride(0), CC,
             work.stride(0))
        dy1 = torch.empty(M, B, CC, T1, **f32)
        n2 = CC * CC * 3
        dwp = torch.empty(M, B, n2, **f32)
        dbp = torch.empty(M, B, CC, **f32)
        call("tl_lite_conv_bwd_group", ptr(dz2), ptr(self.y1), ptr(t["ecog_conv.4.weight"]), ptr(dy1), ptr(dwp), ptr(dbp), M, B,
             CC, CC, T1, 3, 1, dz2.stride(0), self.y1.stride(0), n2, dy1.stride(0), B * n2, B * CC)
        call("tl_sum_slabs2_group", ptr(dwp), ptr(grads["ecog_conv.4.weight"]), n2, ptr(dbp), ptr(grads["ecog_conv.4.bias"]), CC,
             B, M, B * n2, n2, B * CC, CC)
        # block 1
        dz1 = torch.empty(M, B, CC, T, **f32)
        call("tl_lite_bn_act_pool_bwd_group", ptr(dy1), ptr(self.z1), ptr(self.m1), ptr(self.r1), ptr(t["ecog_conv.1.weight"]),
             ptr(t["ecog_conv.1.bias"]), ptr(dz1), ptr(grads["ecog_conv.1.weight"]), ptr(grads["ecog_conv.1.bias"]), ptr(work),
             M, B, CC, T, self.slope, int(self._training), dy1.stride(0), self.z1.stride(0), CC, CC, dz1.stride(0), CC,
             work.stride(0))
        n1 = CC * self.C * 5
        dwp1 = torch.empty(M, B, n1, **f32)
        call("tl_lite_conv_bwd_group", ptr(dz1), ptr(self._x), ptr(t["ecog_conv.0.weight"]), None, ptr(dwp1), ptr(dbp), M, B,
             self.C, CC, T, 5, 2, dz1.stride(0), self._x.stride(0), n1, 0, B * n1, B * CC)
        call("tl_sum_slabs2_group", ptr(dwp1), ptr(grads["ecog_conv.0.weight"]), n1, ptr(dbp), ptr(grads["ecog_conv.0.bias"]), CC,
             B, M, B * n1, n1, B * CC, CC)
