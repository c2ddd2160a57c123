"""Host-side plan of the SynthesisModelCNN forward / backward on MI355X.

The convolution stack (geometry, workspaces, the three passes per stage) is ``_conv_stack.ConvStack``; this class adds the
synthesis model around it: the label LSTM and its BPTT, the concat, the 1x1 stack, the output Linear and the data-parallel
hooks, and the order in which the HIP entry points of ``libtonal_hip.so`` are enqueued.  Everything numerical happens inside
those kernels; torch is used for buffer allocation, the label de-duplication (``torch.unique``) and the current stream only.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import torch

from . import _kernels
from ._conv_stack import ConvStack
from ._launch import r4
from ._lib import EPI_LRELU, EPI_MASK, EPI_STORE, LOAD_DIRECT, check, ptr


class CnnEngine(ConvStack):
    whh_factors = None             # (``_lite_engine.TrainEngine``: what the trainer reads)
    graph_capable = False          # GPU-bound; its W_hh update takes launch-argument scalars

    @property
    def ran_sharded(self) -> bool:
        return self._sh is not None

    def __init__(self, output_dim: int, n_channels: int, n_timepoints: int, lstm_channels: int,
                 conv_channels: int, dropout: float, negative_slope: float, stage_defs, concat_widths):
        super().__init__(n_channels, n_timepoints, stage_defs, negative_slope, conv_channels)
        self.out_dim = output_dim
        self.Lc = lstm_channels
        self.Cc = conv_channels
        self.p_drop = float(dropout)
        self.cslope = 0.1                      # concat block slope, models/synthesis_models.py:118-130
        self.H = self.lat * n_channels * lstm_channels
        self.ldx = r4(conv_channels + lstm_channels)
        self.concat_dims = []                  # (cin_true, cin_ld, cout_true, cout_ld)
        cin_t, cin_ld = conv_channels + lstm_channels, self.ldx
        for w in concat_widths:
            self.concat_dims.append((cin_t, cin_ld, w, r4(w)))
            cin_t, cin_ld = w, r4(w)
        self.ldy5 = self.concat_dims[-1][3]
        self.kflat = n_channels * self.tp5 * self.ldy5
        self.ldd = r4(output_dim)
        self.lowrank_param = "label_lstm.weight_hh_l0"   # reduced via gathered factors under DP
        # data-parallel row shard of the label LSTM (rank, world) - set by the trainer (parallel.py docstring);
        # used for a step when the caller hands the label table (identical distinct rows on every rank)
        self.lstm_shard = None
        self._sh = None
        self._saved_generation = -1

    # ------------------------------------------------------------------ buffers
    def _alloc(self, B: int, dev) -> bool:
        if not super()._alloc(B, dev):
            return False
        z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
        self.rows5 = rows5 = self.S * self.tp5
        self.Xc = z(rows5, self.ldx)
        self.Y = [z(rows5, d[3]) for d in self.concat_dims]
        return True

    def _alloc_bwd(self) -> bool:
        if not super()._alloc_bwd():
            return False
        z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=self._dev)
        self.GY = [z(self.rows5, d[3]) for d in self.concat_dims]
        self.dXc = z(self.rows5, self.ldx)
        return True

    @staticmethod
    def _splitk_rounds(tiles: int, ksteps: int, slots: int = 512, max_sk: int = 32, min_rounds: float = 1.9) -> int:
        """Split-K factor for the HBM-streaming GEMMs over W_hh: the workgroup count should fill whole
        rounds of the 512 resident workgroup slots (256 CUs x 2) - a partial last round streams at a
        fraction of the bandwidth.  Smallest factor whose last round is >= 95 % full with ``min_rounds``
        rounds or more; failing that the fullest."""
        cands = []
        for sk in range(1, max(1, min(max_sk, ksteps)) + 1):
            n = tiles * sk
            cands.append((sk, n, n / (-(-n // slots) * slots)))
        full = [c for c in cands if c[2] >= 0.95]
        for sk, n, _ in full:
            if n >= min_rounds * slots:
                return sk
        if full:
            return full[-1][0]
        return max(cands, key=lambda c: c[2])[0]

    def _lstm_forward(self, prm, xu, U, L, dev, training, label_table) -> None:
        """The label LSTM on the U distinct label rows (torch's current stream; it does not depend on the convolution stack -
        four 5.4 GB streams of W_hh)."""
        lib, st_ = self.lib, self._stream()
        H = self.H
        f32 = dict(dtype=torch.float32, device=dev)
        self._act = torch.empty(L, U, 4 * H, **f32)
        self._c = torch.empty(L, U, H, **f32)
        self._h = torch.empty(L, U, H, **f32)
        hh = torch.empty(U, 4 * H, **f32) if L > 1 else None
        w_ih, w_hh = prm["label_lstm.weight_ih_l0"], prm["label_lstm.weight_hh_l0"]
        b_ih, b_hh = prm["label_lstm.bias_ih_l0"], prm["label_lstm.bias_hh_l0"]
        bm = 32 if U <= 64 else 128
        # row shard of W_hh for this step: needs the caller's label table (same U rows on every rank), an even
        # split of the 4H gate rows and a factor rank the fused optimiser takes
        self._sh = None
        if (self.lstm_shard is not None and label_table is not None and training and L > 1 and (L - 1) * U <= 64
                and (4 * H) % (4 * self.lstm_shard[1]) == 0):
            rk, wd = self.lstm_shard
            self._sh = (rk * (4 * H // wd), 4 * H // wd, wd)
        nloc = self._sh[1] if self._sh else 4 * H
        # (measured at the north-star shape, 576 column tiles: 7 splits 1.048 ms, 8 0.996, 16 0.990, 32 1.017 - the 32-row kernel
        # keeps three workgroups per CU, so nine rounds of 512 are six whole rounds of 768: profiles/r06_kernel_notes.md 7)
        sk_f = self._splitk_rounds(((U + bm - 1) // bm) * ((nloc + 127) // 128), (H + 31) // 32, min_rounds=8.9) if L > 1 else 1
        slab_f = torch.empty(sk_f, U, nloc, **f32) if sk_f > 1 else None
        if self._sh:
            from . import parallel
            hh_loc = torch.empty(U, nloc, **f32)
            hh_all = torch.empty(self._sh[2], U, nloc, **f32)
        for t in range(L):
            if t > 0 and self._sh:
                # this rank's gate rows of h W_hh^T, all-gathered: every rank then holds the full (U, 4H) product
                r0, R, wd = self._sh
                self._nt(A=ptr(self._h[t - 1]), Bw=w_hh.data_ptr() + 4 * r0 * H, out=ptr(slab_f if sk_f > 1 else hh_loc),
                         M=U, A_rows=U, N=R, K=H, lda=H, ldb=H, ldo=R, loader=LOAD_DIRECT, epilogue=EPI_STORE, bm=bm,
                         splitk=sk_f, slab_stride=U * R)
                if sk_f > 1:
                    self._permute(slab_f, hh_loc, (1, 1, 1, U * R), (0, 0, 0, 1), nz=sk_f, zs=U * R)
                parallel.all_gather_blocks(hh_all, hh_loc)
                self._permute(hh_all, hh, (1, U, wd, R), (0, R, U * R, 1))
            elif t > 0:
                self._nt(A=ptr(self._h[t - 1]), Bw=ptr(w_hh), out=ptr(slab_f if sk_f > 1 else hh), M=U, A_rows=U,
                         N=4 * H, K=H, lda=H, ldb=H, ldo=4 * H, loader=LOAD_DIRECT, epilogue=EPI_STORE, bm=bm,
                         splitk=sk_f, slab_stride=U * 4 * H)
                if sk_f > 1:
                    n = U * 4 * H
                    self._permute(slab_f, hh, (1, 1, 1, n), (0, 0, 0, 1), nz=sk_f, zs=n)
            check(lib.tl_lstm_cell_fwd(ptr(hh) if t > 0 else None, ptr(xu[t]), ptr(w_ih), ptr(b_ih), ptr(b_hh),
                                       ptr(self._c[t - 1]) if t > 0 else None, ptr(self._act[t]), ptr(self._c[t]),
                                       ptr(self._h[t]), U, H, 2, 4 * H, st_), "tl_lstm_cell_fwd")

    # ------------------------------------------------------------------ forward
    def forward(self, prm: Dict[str, torch.Tensor], x: torch.Tensor, labels: torch.Tensor, training: bool,
                save: bool, seed: int = 0, row0: int = 0, label_ids: Optional[torch.Tensor] = None,
                label_table: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``row0``: index of this shard's first window in the global batch (data parallel): the dropout
        hash is indexed by the global element, so N ranks draw the masks of one process.
        ``label_ids`` (B,) int32 + ``label_table`` (U, 2, L): the caller already knows the distinct label
        sequences (the trainer builds them from (tone, syllable) class pairs) - ``labels[b] == label_table[ids[b]]``;
        the LSTM then runs on the table rows and no ``torch.unique`` (a host synchronisation) is needed."""
        B, Cn, T = x.shape
        if Cn != self.C or T != self.T:
            raise ValueError(f"expected ECoG input (B, {self.C}, {self.T}), got {tuple(x.shape)}")
        if labels.dim() != 3 or labels.shape[0] != B or labels.shape[1] != 2:
            raise ValueError(f"expected labels (B, 2, L), got {tuple(labels.shape)}")
        x = x.contiguous().float()
        labels = labels.contiguous().float()
        dev = x.device
        self._alloc(B, dev)
        lib, st_ = self.lib, self._stream()
        self.generation += 1
        p_drop = self.p_drop if training else 0.0
        self._p_drop_used, self._seed_used = p_drop, seed
        self._drop_row0 = int(row0) * self.C * self.tp5
        # ---- stage 1 (C_in = 1) ----
        self.conv1_forward(x, prm["ecog_conv_block.0.weight"], prm["ecog_conv_block.0.bias"])
        # ---- label LSTM on the distinct label sequences ----
        L = labels.shape[2]
        flat = labels.reshape(B, 2 * L)
        self._table_labels = label_ids is not None and label_table is not None
        if self._table_labels:
            uniq, inv = label_table.reshape(label_table.shape[0], 2 * L).float(), label_ids
        else:
            uniq, inv = torch.unique(flat, dim=0, return_inverse=True)
        U = uniq.shape[0]
        self._U, self._L = U, L
        self._uid = inv.to(torch.int32).contiguous()
        H = self.H
        xu = uniq.reshape(U, 2, L).permute(2, 0, 1).contiguous()          # (L, U, 2) time-major
        self._xu = xu
        f32 = dict(dtype=torch.float32, device=dev)
        # ---- stages 2..5: windowed implicit GEMM on fp32 MFMA ----
        for st in self.stages:
            self.stage_forward(st, prm[self.STAGE_NAMES[st.idx] + ".weight"], prm[self.STAGE_NAMES[st.idx] + ".bias"])
        self._lstm_forward(prm, xu, U, L, dev, training, label_table)
        # ---- dropout + concat ----
        check(lib.tl_concat_pack(ptr(self.P[5]), ptr(self._h[L - 1]), ptr(self._uid), ptr(self.Xc), B, self.C,
                                 self.tp5, self.lat, self.Cc, self.Lc, self.ld5, H, self.ldx, p_drop, seed,
                                 self._drop_row0, st_), "tl_concat_pack")
        # ---- concat 1x1 stack ----
        src = self.Xc
        self._wc = []
        for i, (cin_t, cin_ld, cout_t, cout_ld) in enumerate(self.concat_dims):
            w = prm[f"concat_conv_block.{2 * i}.weight"]
            bia = prm[f"concat_conv_block.{2 * i}.bias"]
            wp = self._pack_conv(w, cin_ld, False)
            self._nt(A=ptr(src), Bw=ptr(wp), bias=ptr(bia), out=ptr(self.Y[i]), M=self.rows5, A_rows=self.rows5,
                     N=cout_t, K=cin_ld, lda=cin_ld, ldb=cin_ld, ldo=cout_ld, loader=LOAD_DIRECT,
                     epilogue=EPI_LRELU, slope=self.cslope, Tp=self.tp5, Tvalid=self.lat)
            src = self.Y[i]
        # ---- output Linear: (B, kflat) x (out_dim, kflat)^T, split-K ----
        wo = prm["output_layer.weight"]
        wpo = torch.empty(self.out_dim, self.kflat, **f32)
        latC = self.lat * self.C
        self._permute(wo, wpo, (self.out_dim, self.C, self.tp5, self.ldy5), (self.Cc * latC, 1, self.C, latC),
                      (self.out_dim, self.C, self.lat, self.Cc))
        self._wpo = wpo
        nkc = (self.kflat + 31) // 32
        tiles = ((B + 127) // 128) * ((self.out_dim + 127) // 128)
        sk = self._splitk(tiles, nkc, 1024)
        slab = torch.empty(sk, B, self.out_dim, **f32)
        self._nt(A=ptr(self.Y[-1]), Bw=ptr(wpo), out=ptr(slab), M=B, A_rows=B, N=self.out_dim, K=self.kflat,
                 lda=self.kflat, ldb=self.kflat, ldo=self.out_dim, loader=LOAD_DIRECT, epilogue=EPI_STORE,
                 splitk=sk, slab_stride=B * self.out_dim)
        out = torch.empty(B, self.out_dim, **f32)
        self._permute(slab, out, (1, 1, B, self.out_dim), (0, 0, self.out_dim, 1), nz=sk, zs=B * self.out_dim,
                      bias=prm["output_layer.bias"])
        if save:
            self._saved_generation = self.generation
        return out

    def _lstm_backward(self, prm, grads, dh_ext, gather_whh, whh_factors, reduce_rows, on_factors) -> None:
        """BPTT of the label LSTM on the distinct rows, its W_ih / bias gradients and the W_hh gradient (dense, or left as
        factors in ``self.whh_factors``) - on torch's current stream.  ``on_factors()`` is called at the end (the trainer
        updates W_hh there, on the same stream)."""
        lib, st_ = self.lib, self._stream()
        dev = self._dev
        f32 = dict(dtype=torch.float32, device=dev)
        H, U, L = self.H, self._U, self._L
        # ---- LSTM BPTT on the distinct rows ----
        sh = self._sh
        if sh:      # every rank runs the same BPTT on the gradient of the GLOBAL batch
            from . import parallel
            parallel.all_reduce_(dh_ext)
        w_hh = prm["label_lstm.weight_hh_l0"]
        ldt = (U + 31) // 32 * 32
        dg = torch.empty(L, U, 4 * H, **f32)
        # dgates . W_hh on tl_lstm_gw (reads dg[t] itself: no transposed copy)
        stream_gw = U <= 8 and H % 4 == 0 and _kernels.get("whh_stream") != "0"
        dgt = torch.zeros(4 * H, ldt, **f32) if (L > 1 and not stream_gw) else None
        dc = [torch.empty(U, H, **f32), torch.empty(U, H, **f32)]
        dhrec = torch.empty(U, H, **f32) if L > 1 else None
        if L > 1 and not stream_gw:
            kloc = sh[1] if sh else 4 * H                      # gate rows this rank contracts over
            if ldt <= 32:        # skinny streaming kernel: 32 x 512 tiles, 16-deep K stages
                sk_h = self._splitk_rounds((H + 511) // 512, (kloc + 15) // 16)
            else:
                sk_h = self._splitk((ldt + 127) // 128 * ((H + 127) // 128), (kloc + 31) // 32, 1024)
            slab_h = torch.empty(sk_h, ldt, H, **f32)
        # single process, factored update: the last BPTT product dh_1 = dgates_2 . W_hh comes out of the W_hh NAdam pass itself
        # (tl_nadam_lowrank_dh): the factors are complete one step before the BPTT ends - h_0 = 0, the gradient has no term for the
        # first step - and that product needs only the OLD weight.  One 5.4 GB stream of W_hh less per step
        fuse_dh = (L > 1 and not sh and gather_whh is None and whh_factors and (L - 1) * U <= 64 and U <= 8
                   and on_factors is not None and getattr(on_factors, "fuse_dh", False) and _kernels.get("whh_dh") != "0")
        fused_done = False
        slab_g = None
        for t in range(L - 1, -1, -1):
            check(lib.tl_lstm_cell_bwd(ptr(dh_ext) if t == L - 1 else None, ptr(dhrec) if t < L - 1 else None,
                                       ptr(dc[(t + 1) & 1]) if t < L - 1 else None, ptr(self._act[t]), ptr(self._c[t]),
                                       ptr(self._c[t - 1]) if t > 0 else None, ptr(dg[t]),
                                       ptr(dgt) if (t > 0 and dgt is not None) else None, ptr(dc[t & 1]), U, H, ldt, st_),
                  "tl_lstm_cell_bwd")
            if t == 1 and fuse_dh:
                kr = (L - 1) * U
                self.whh_factors = (dg[1:].reshape(kr, 4 * H), self._h[:L - 1].reshape(kr, H))
                row_tiles = 16
                nslab = -(-(-(-4 * H // 32)) // row_tiles)
                slab_d = torch.empty(nslab, U, H, **f32)
                on_factors(dh=(slab_d, U, row_tiles))
                self._permute(slab_d, dhrec, (1, 1, U, H), (0, 0, H, 1), nz=nslab, zs=U * H)
                fused_done = True
            elif t > 0 and sh:
                # partial dgates . W_hh over this rank's gate rows, summed over the ranks
                r0, R, _wd = sh
                if stream_gw:
                    rpb = 512
                    nb = -(-R // rpb)
                    if slab_g is None:
                        slab_g = torch.empty(nb, U, H, **f32)
                    check(lib.tl_lstm_gw(dg[t].data_ptr() + 4 * r0, w_hh.data_ptr() + 4 * r0 * H, ptr(slab_g), U, R, H, 4 * H, H,
                                         rpb, st_), "tl_lstm_gw")
                    self._permute(slab_g, dhrec, (1, 1, U, H), (0, 0, H, 1), nz=nb, zs=U * H)
                else:
                    self._tn(A=dgt.data_ptr() + 4 * r0 * ldt, B=w_hh.data_ptr() + 4 * r0 * H, slab=ptr(slab_h), Krows=R,
                             A_rows=R, B_rows=R, Mdim=ldt, Ndim=H, lda=ldt, ldb=H, ldc=H, loader=LOAD_DIRECT, splitk=sk_h,
                             slab_stride=ldt * H)
                    self._permute(slab_h, dhrec, (1, 1, U, H), (0, 0, H, 1), nz=sk_h, zs=ldt * H)
                parallel.all_reduce_(dhrec)
            elif t > 0 and stream_gw:
                # dgates_t . W_hh as a pure stream of the 5.4 GB weight (tl_lstm_gw, round 6): 512-row blocks, the partial
                # products of the 144 blocks summed behind it
                rpb = 512
                nb = -(-4 * H // rpb)
                if slab_g is None:
                    slab_g = torch.empty(nb, U, H, **f32)
                check(lib.tl_lstm_gw(ptr(dg[t]), ptr(w_hh), ptr(slab_g), U, 4 * H, H, 4 * H, H, rpb, st_), "tl_lstm_gw")
                self._permute(slab_g, dhrec, (1, 1, U, H), (0, 0, H, 1), nz=nb, zs=U * H)
            elif t > 0:
                self._tn(A=ptr(dgt), B=ptr(w_hh), slab=ptr(slab_h), Krows=4 * H, A_rows=4 * H, B_rows=4 * H, Mdim=ldt,
                         Ndim=H, lda=ldt, ldb=H, ldc=H, loader=LOAD_DIRECT, splitk=sk_h, slab_stride=ldt * H)
                self._permute(slab_h, dhrec, (1, 1, U, H), (0, 0, H, 1), nz=sk_h, zs=ldt * H)
        def dense_whh():                       # allocated on demand: the trainer path never needs it
            if "label_lstm.weight_hh_l0" not in grads:
                grads["label_lstm.weight_hh_l0"] = torch.empty(4 * H, H, **f32)
            return grads["label_lstm.weight_hh_l0"]
        if fused_done:
            pass                                   # factors handed over and consumed inside the loop
        elif L > 1:
            kr = (L - 1) * U
            fa, fb = dg[1:].reshape(kr, 4 * H), self._h[:L - 1].reshape(kr, H)
            if sh:
                # dgates already belong to the global batch (identical on every rank): this rank updates its own
                # rows of W_hh from the matching columns of the factor - nothing to gather
                if not whh_factors:
                    raise RuntimeError("the row-sharded label LSTM needs the factored W_hh update (whh_factors=True)")
                self.whh_factors = (fa[:, sh[0]:sh[0] + sh[1]], fb.contiguous(), sh[0], sh[1])
                fa = fb = None
            elif gather_whh is not None and self._table_labels and reduce_rows is not None:
                # the label table is the same on every rank: row (t, u) of the factors means the same (step, label
                # sequence) everywhere and carries bit-identical h, so the factor of the GLOBAL gradient is simply the sum
                # of the ranks' dgates rows - one small all-reduce ((L-1) U x 4H floats), no gather, no host sync
                fa = fa.clone()                  # dg itself stays local: the W_ih / bias gradients are reduced with the buckets
                reduce_rows(fa)
            elif gather_whh is not None:
                # arbitrary label tensors: the distinct rows differ per rank (torch.unique above already synchronised)
                # key of row (t, u): the step and the label sequence h_t was unrolled from
                steps = torch.arange(L - 1, device=dev, dtype=torch.float32).repeat_interleave(U).unsqueeze(1)
                keys = torch.cat([steps, self._xu.permute(1, 0, 2).reshape(U, 2 * L).repeat(L - 1, 1)], dim=1)
                fa, fb = gather_whh(fa, fb, keys)
                kr = fa.shape[0]
            if sh:
                pass
            elif whh_factors and kr <= 64:
                # hand the factors to the optimiser (tl_nadam_lowrank): the 5.4 GB gradient is never formed
                self.whh_factors = (fa.contiguous(), fb.contiguous())
            else:
                self._tn(A=ptr(fa), B=ptr(fb), slab=ptr(dense_whh()), Krows=kr, A_rows=kr, B_rows=kr, Mdim=4 * H,
                         Ndim=H, lda=4 * H, ldb=H, ldc=H, loader=LOAD_DIRECT)
            del fa, fb
        elif whh_factors:
            self.whh_factors = (None, None)
        else:
            dense_whh().zero_()
        gb = grads["label_lstm.bias_ih_l0"]
        check(lib.tl_lstm_ih_grad(ptr(dg), ptr(self._xu), ptr(grads["label_lstm.weight_ih_l0"]), ptr(gb),
                                  ptr(grads["label_lstm.bias_hh_l0"]), L, U, H, 2, st_), "tl_lstm_ih_grad")
        del dg, dgt
        if on_factors is not None and not fused_done:
            on_factors()

    # ------------------------------------------------------------------ backward
    def grad_order(self) -> List[str]:
        """Parameter names in the order ``backward`` finishes their gradients (the layout of a flat gradient buffer whose
        exchange buckets are contiguous slices): output layer, 1x1 stack last to first, label LSTM, ecog stages 5..1."""
        order = ["output_layer.weight", "output_layer.bias"]
        for i in range(len(self.concat_dims) - 1, -1, -1):
            order += [f"concat_conv_block.{2 * i}.weight", f"concat_conv_block.{2 * i}.bias"]
        order += ["label_lstm.weight_ih_l0", "label_lstm.bias_ih_l0", "label_lstm.bias_hh_l0"]
        for st in reversed(self.stages):
            order += [self.STAGE_NAMES[st.idx] + ".weight", self.STAGE_NAMES[st.idx] + ".bias"]
        order += ["ecog_conv_block.0.weight", "ecog_conv_block.0.bias"]
        return order

    def backward(self, prm: Dict[str, torch.Tensor], dout: torch.Tensor, grads: Dict[str, torch.Tensor],
                 gather_whh=None, whh_factors: bool = False, reduce_rows=None, on_factors=None, on_grad_ready=None) -> None:
        """dout: (B, ldd) gradient of the loss w.r.t. the output (pad columns zero).
        Fills ``grads[name]`` (torch layouts) for every parameter.  ``gather_whh(dg, h)`` may
        return the low-rank factors of every data-parallel rank (parallel.gather_lowrank): the
        W_hh gradient written is then already the sum over ranks.  With ``whh_factors`` the W_hh
        gradient is not written at all: ``self.whh_factors = (fa, fb)`` (gradient = fa^T . fb) is left for
        ``FusedNAdam.step(lowrank=...)``; ``None`` afterwards means the dense gradient was written instead
        (rank above 64)."""
        self.whh_factors = None
        if self._saved_generation != self.generation:
            raise RuntimeError("SynthesisModelCNN backward: the forward intermediates were overwritten by a later "
                               "forward pass (one forward/backward pair at a time per model)")
        self._alloc_bwd()
        lib, st_ = self.lib, self._stream()
        B, S, dev = self._B, self.S, self._dev
        f32 = dict(dtype=torch.float32, device=dev)
        H, U, L = self.H, self._U, self._L
        rows5 = self.rows5

        # ---- output layer ----
        gw = grads["output_layer.weight"]
        slab = torch.empty(self.ldd, self.kflat, **f32)
        self._tn(A=ptr(dout), B=ptr(self.Y[-1]), slab=ptr(slab), Krows=B, A_rows=B, B_rows=B, Mdim=self.ldd,
                 Ndim=self.kflat, lda=self.ldd, ldb=self.kflat, ldc=self.kflat, loader=LOAD_DIRECT)
        latC = self.lat * self.C
        self._permute(slab, gw, (self.out_dim, self.Cc, self.lat, self.C),
                      (self.kflat, 1, self.ldy5, self.tp5 * self.ldy5))
        self._colsum(dout, B, self.out_dim, self.ldd, 1, 1, grads["output_layer.bias"])
        if on_grad_ready is not None:
            on_grad_ready("output_layer")           # both gradients of the Linear layer are final (enqueued) from here on
        # dY5 = dout . Wp_out, masked by lrelu'(Y5)
        wpt = torch.empty(self.kflat, self.ldd, **f32)
        self._permute(prm["output_layer.weight"], wpt, (self.C, self.tp5, self.ldy5, self.ldd),
                      (1, self.C, latC, self.Cc * latC), (self.C, self.lat, self.Cc, self.out_dim))
        self._nt(A=ptr(dout), Bw=ptr(wpt), aux=ptr(self.Y[-1]), out=ptr(self.GY[-1]), M=B, A_rows=B, N=self.kflat,
                 K=self.ldd, lda=self.ldd, ldb=self.ldd, ldo=self.kflat, ldaux=self.kflat, loader=LOAD_DIRECT,
                 epilogue=EPI_MASK, slope=self.cslope)
        del wpt
        # ---- concat 1x1 stack, last to first ----
        for i in range(len(self.concat_dims) - 1, -1, -1):
            cin_t, cin_ld, cout_t, cout_ld = self.concat_dims[i]
            src = self.Xc if i == 0 else self.Y[i - 1]
            Gi = self.GY[i]
            name = f"concat_conv_block.{2 * i}"
            tiles = ((cin_ld + 127) // 128) * ((cout_ld + 127) // 128)
            # (512 splits: the launch itself is flat between 256 and 1 024 - scripts/bench_tn1.py -, the slab reduction behind
            # it reads half of what 1 024 leave)
            sk = self._splitk(tiles, (rows5 + 31) // 32, 512)
            slab = torch.empty(sk, cin_ld, cout_ld, **f32)
            # the bias gradient (column sums of Gi over the valid rows) rides in the weight-gradient launch where that is the
            # one-tap direct kernel (not its short-reduction / skinny forms, whose colsum means something else): Gi is not read
            # a third time
            fold = rows5 > 512 and cin_ld > 32
            bpart = torch.empty(sk, cout_ld, **f32) if fold else None
            self._tn(A=ptr(src), B=ptr(Gi), slab=ptr(slab), Krows=rows5, A_rows=rows5, B_rows=rows5, Mdim=cin_ld,
                     Ndim=cout_ld, lda=cin_ld, ldb=cout_ld, ldc=cout_ld, loader=LOAD_DIRECT, Tp=self.tp5,
                     Tvalid=self.lat, splitk=sk, slab_stride=cin_ld * cout_ld, colsum=ptr(bpart))
            self._permute(slab, grads[name + ".weight"], (1, 1, cout_t, cin_t), (0, 0, 1, cout_ld), nz=sk,
                          zs=cin_ld * cout_ld)
            if fold:
                self._permute(bpart, grads[name + ".bias"], (1, 1, 1, cout_t), (0, 0, 0, 1), nz=sk, zs=cout_ld)
            else:
                self._colsum(Gi, rows5, cout_t, cout_ld, self.tp5, self.lat, grads[name + ".bias"])
            wd = self._pack_conv(prm[name + ".weight"], cin_ld, True)          # [1][cin_ld][cout_ld]
            if i > 0:
                self._nt(A=ptr(Gi), Bw=ptr(wd), aux=ptr(src), out=ptr(self.GY[i - 1]), M=rows5, A_rows=rows5,
                         N=cin_ld, K=cout_ld, lda=cout_ld, ldb=cout_ld, ldo=cin_ld, ldaux=cin_ld, loader=LOAD_DIRECT,
                         epilogue=EPI_MASK, slope=self.cslope)
            else:
                self._nt(A=ptr(Gi), Bw=ptr(wd), out=ptr(self.dXc), M=rows5, A_rows=rows5, N=cin_ld, K=cout_ld,
                         lda=cout_ld, ldb=cout_ld, ldo=cin_ld, loader=LOAD_DIRECT, epilogue=EPI_STORE)
        # ---- un-concat: G5 (dropout + lrelu') and dh summed over duplicates ----
        # duplicates of a label sequence: the kernel scans the batch's label ids in batch order (what a stable argsort
        # would list) - no argsort / scatter_add_ / cumsum in front of it
        dh_ext = torch.empty(U, H, **f32)
        check(lib.tl_concat_unpack_bwd(ptr(self.dXc), ptr(self.P[5]), None, ptr(self._uid), ptr(self.G[5]),
                                       ptr(dh_ext), B, U, self.C, self.tp5, self.lat, self.Cc, self.Lc, self.ld5, H,
                                       self.ldx, self.slope, self._p_drop_used, self._seed_used, self._drop_row0,
                                       st_), "tl_concat_unpack_bwd")
        # ---- LSTM BPTT on the distinct rows: independent of the convolution backward below; the trainer's W_hh update
        # rides along (on_factors) ----
        self._lstm_backward(prm, grads, dh_ext, gather_whh, whh_factors, reduce_rows, on_factors)
        # ---- ecog stages 5..2 ----
        for st in reversed(self.stages):
            name = self.STAGE_NAMES[st.idx]
            self.stage_wgrad(st, grads[name + ".weight"], grads[name + ".bias"])
            part = self.stage_dgrad(st, prm[name + ".weight"])
        # ---- stage 1 weight / bias gradient (partials come out of the stage-2 epilogue when fused) ----
        if part is None:
            nblk = int(min(2048, S))
            part = torch.empty(nblk, (self.k1 + 1) * self.c1, **f32)
            check(lib.tl_conv1_wgrad(ptr(self._x), ptr(self.G[1]), ptr(self.bits[1]), ptr(part), nblk, S, self.T, self.k1,
                                     self.c1, self.tp1, self.tout1, st_), "tl_conv1_wgrad")
        self._reduce_c1_partials(part, grads["ecog_conv_block.0.weight"], grads["ecog_conv_block.0.bias"])
