"""GPU: the F(6,3) backward of the CNN-RNN classifier's 7-tap stages (``TONAL_KERNELS conv7=wino63bwd``).

Kernel level, against float64 (transform matrices of tests/wino63_ref.py), relative L2 <= 5e-5 - the bound the step tests hold the
F(6,3) passes to:
  * ``tl_wino63_ydz``: Y = A dz of un-pooled gradient rows;
  * the weight gradient: three ``tl_conv3_wino63v_tn`` launches (loader 3) on V0(x), V1(x) and V0(x) one hex on (``a_hex``), each
    finished by ``tl_wino63_wgrad_finalize``, against ``sum_R dz[R] (x) x[R + j]``;
  * the input gradient: ``tl_wino63_xform2s`` (dz moved down six rows inside its sequence) + ``tl_conv7_wino63v_dgrad_nt`` with the
    taps of the flipped, transposed weight, against ``conv_transpose1d`` times the LeakyReLU' mask, with both mask sources.
Step level: the method of ``test_one_step_gradients_on_shared_branches`` under the new value.
Every figure is printed and recorded (``tests/parity_record.py``) before it is asserted."""
import copy
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from tests import cnnrnn_classifier_ref as rref
from tests import parity_record, wino63_ref
from tests import classifier_train_ref as ref
from tests.test_gpu_cnnrnn_classifier_train import _engine, _one_step

pytestmark = pytest.mark.gpu
DEV = "cuda"
BOUND = 5e-5
_REC = {}


def _within(section, name, dev, bound=BOUND):
    print(f"[conv7_bwd.{section}] {name}: gpu {dev:.3e}  bound {bound:.3e}")
    _REC.setdefault(section, {})[name] = dev
    parity_record.record("conv7_bwd_" + section, _REC[section])
    return dev <= bound


def _lib():
    from decode_tonal_langauge_amd import _lib as L
    return L, L.load(), torch.cuda.current_stream().cuda_stream


def _pad_hexes(nhex):
    """whole 128-hex tiles of the NT kernel (+ one hex on) AND whole 6-hex K-steps of the weight-gradient kernel"""
    return (nhex + 6 + 127) // 128 * 128


# ---------------------------------------------------------------------------------------------- the Y transform
@pytest.mark.parametrize("nseq,Tp,t_out,Cc", [(3, 24, 15, 64), (5, 12, 6, 8), (7, 18, 1, 40)])
def test_y_transform_of_unpooled_rows(nseq, Tp, t_out, Cc):
    L, lib, st = _lib()
    rows, nhex, ldg, ldv = nseq * Tp, nseq * Tp // 6, Cc + 4, Cc + 8            # (both leading dimensions above the minimum)
    g = torch.Generator().manual_seed(nseq * Tp + t_out)
    dz = torch.randn(rows, ldg, generator=g)
    clean = dz.clone()
    clean.view(nseq, Tp, ldg)[:, t_out:] = 0
    dz.view(nseq, Tp, ldg)[:, t_out:] = float("nan")                             # rows from t_out on must not be read into Y

    def run(src):
        Y = torch.full((_pad_hexes(nhex), 8, ldv), float("nan"), device=DEV)
        L.check(lib.tl_wino63_ydz(src.to(DEV).data_ptr(), Y.data_ptr(), rows, Tp, t_out, Cc, ldg, ldv, st), "tl_wino63_ydz")
        torch.cuda.synchronize()
        return Y.cpu()
    Y, Yc = run(dz), run(clean)
    got = wino63_ref.logical(Y[:(nhex + 1) // 2 * 2])[:nhex]
    got_c = wino63_ref.logical(Yc[:(nhex + 1) // 2 * 2])[:nhex]
    assert torch.equal(got[:, :, :Cc], got_c[:, :, :Cc])                         # exactly what zeros in those rows give
    assert not bool(torch.isnan(got[:, :, :Cc]).any()) and bool(torch.isnan(got[:, :, Cc:]).all())
    assert bool(torch.isnan(Y[(nhex + 1) // 2 * 2:]).all())                      # nothing behind the last hex pair is written
    want = wino63_ref.y_transform(clean[:, :Cc].contiguous(), nseq, Tp)
    # hexes that hold no valid row: exactly zero
    dead = (torch.arange(nhex) % (Tp // 6)) * 6 >= t_out
    assert bool((got[dead][:, :, :Cc] == 0).all())
    # plane 1 is the plain sum of the six rows (the weight-gradient kernel's colsum = the bias gradient)
    assert ref.rel_l2(got[:, 1, :Cc].double(), clean[:, :Cc].double().view(nhex, 6, Cc).sum(1)) <= 1e-6
    assert _within("ydz", f"S{nseq}Tp{Tp}t{t_out}C{Cc}", ref.rel_l2(got[:, :, :Cc].double(), want))


# ---------------------------------------------------------------------------------------------- the weight gradient
def _engine_splitk(rows, cin, cout):
    from decode_tonal_langauge_amd._conv_stack import ConvStack
    return ConvStack._splitk((cin // 64) * (cout // 64), (rows + 35) // 36, 4096)


@pytest.mark.parametrize("nseq,Tp,t_in,cin,cout,splitk", [(3, 24, 21, 256, 64, 1), (5, 12, 12, 256, 64, 2),
                                                          (40, 24, 19, 256, 128, "engine"),
                                                          # 253 hexes: ceil128(253 + 2) = 256 hexes are no whole 6-hex K-steps (258)
                                                          (11, 138, 131, 256, 64, "engine")])
def test_weight_gradient_of_a_7tap_stage(nseq, Tp, t_in, cin, cout, splitk):
    L, lib, st = _lib()
    t_out = t_in - 6
    rows, nhex = nseq * Tp, nseq * Tp // 6
    sk = _engine_splitk(rows, cin, cout) if splitk == "engine" else splitk
    assert sk >= 1 and (splitk != "engine" or sk > 1)
    g = torch.Generator().manual_seed(1000 * nseq + t_in)
    x = torch.randn(rows, cin, generator=g)
    x.view(nseq, Tp, cin)[:, t_in:] = 1e3                                        # rows the stage never produced
    dz = torch.randn(rows, cout, generator=g)
    dzv = dz.view(nseq, Tp, cout)
    dzv[:, t_out:] = 0                                                           # as G[idx] holds them
    dzv[:, max(0, t_out - 2):t_out, ::7] = 1e3                                   # a few valid rows just below t_out
    xd, dzd = x.to(DEV), dz.to(DEV)
    nh_pad = _pad_hexes(nhex)
    V0, V1, Y = (torch.zeros(nh_pad, 8, c, device=DEV) for c in (cin, cin, cout))
    L.check(lib.tl_wino63_xform2(xd.data_ptr(), V0.data_ptr(), V1.data_ptr(), rows, Tp, t_in, cin, cin, cin, st), "tl_wino63_xform2")
    L.check(lib.tl_wino63_ydz(dzd.data_ptr(), Y.data_ptr(), rows, Tp, t_out, cout, cout, cout, st), "tl_wino63_ydz")

    def run():
        slab = torch.full((3, sk, 8 * cin, cout), float("nan"), device=DEV)
        bias = torch.full((sk, cout), float("nan"), device=DEV)
        gw = torch.zeros(cout, cin, 7, device=DEV)
        g3 = torch.empty(cout, cin, 3, device=DEV)
        for s, (V, a_hex) in enumerate(((V0, 0), (V1, 0), (V0, 1))):
            p = L.TnParams()
            p.A, p.B, p.slab = V.data_ptr(), Y.data_ptr(), slab[s].data_ptr()
            p.Krows, p.A_rows, p.B_rows, p.Mdim, p.Ndim = rows, nh_pad, nh_pad, cin, cout
            p.lda, p.ldb, p.ldc, p.J, p.Tp, p.Tvalid, p.loader = cin, cout, cout, 3, Tp, t_out, L.LOAD_Y
            p.splitk, p.slab_stride, p.a_hex = sk, 8 * cin * cout, a_hex
            p.colsum = bias.data_ptr() if s == 0 else None
            L.check(lib.tl_conv3_wino63v_tn(C.byref(p), st), "tl_conv3_wino63v_tn")
            red = slab[s].sum(0)
            L.check(lib.tl_wino63_wgrad_finalize(red.data_ptr(), g3.data_ptr(), cout, cin, cout, st), "tl_wino63_wgrad_finalize")
            nt = min(3, 7 - 3 * s)
            gw[:, :, 3 * s:3 * s + nt] = g3[:, :, :nt]
        torch.cuda.synchronize()
        return gw.cpu(), bias.sum(0).cpu(), slab.cpu()
    gw, gb, slab = run()
    gw2, gb2, slab2 = run()
    assert torch.equal(slab, slab2) and torch.equal(gw, gw2) and torch.equal(gb, gb2)      # no atomics: the same bits
    assert not bool(torch.isnan(slab).any())
    x64, dz64 = x.double().view(nseq, Tp, cin), dz.double().view(nseq, Tp, cout)
    want = torch.stack([torch.einsum("sto,sti->oi", dz64[:, :t_out], x64[:, j:j + t_out]) for j in range(7)], dim=2)
    tag = f"S{nseq}Tp{Tp}t{t_in}I{cin}O{cout}sk{sk}"
    ok = [_within("wgrad", tag + ".dW", ref.rel_l2(gw.double(), want)),
          _within("wgrad", tag + ".db", ref.rel_l2(gb.double(), dz64.sum((0, 1))))]
    ok += [_within("wgrad", f"{tag}.dW_tap{j}", ref.rel_l2(gw[:, :, j].double(), want[:, :, j])) for j in range(7)]
    assert all(ok), tag


# ---------------------------------------------------------------------------------------------- the input gradient
@pytest.mark.parametrize("mask", ["bits", "rows"])
@pytest.mark.parametrize("nseq,Tp,t_in,K,N", [(3, 24, 21, 64, 96), (5, 12, 12, 16, 32), (700, 198, 197, 64, 64), (2, 36, 14, 16, 32)])
def test_input_gradient_of_a_7tap_stage(nseq, Tp, t_in, K, N, mask):
    """K = C_out (the channels of dz), N = C_in (the channels of dx)."""
    L, lib, st = _lib()
    t_out, slope = t_in - 6, 0.3
    rows, nhex = nseq * Tp, nseq * Tp // 6
    g = torch.Generator().manual_seed(77 * nseq + t_in)
    dz = torch.randn(rows, K, generator=g)
    dzv = dz.view(nseq, Tp, K)
    dzv[:, t_out:] = 0
    dzv[:, max(0, t_out - 2):t_out, ::5] = 1e3         # the last valid rows of every sequence (in front of the next one's rows 0 .. 5)
    dzv[:, 0:2, 1::5] = 1e3                            # ... and its first rows (behind the previous one's last hex)
    w = torch.randn(K, N, 7, generator=g) / (7 * K) ** 0.5                       # torch's (O, I, 7)
    xin = torch.randn(rows, N, generator=g)                                       # the stage input: only its sign matters
    dzd = dz.to(DEV)
    nh_pad = _pad_hexes(nhex)
    D0, D1 = torch.zeros(nh_pad, 8, K, device=DEV), torch.zeros(nh_pad, 8, K, device=DEV)
    L.check(lib.tl_wino63_xform2s(dzd.data_ptr(), D0.data_ptr(), D1.data_ptr(), rows, Tp, t_out, 6, K, K, K, st), "tl_wino63_xform2s")
    wf = w.flip(2).permute(1, 0, 2).contiguous().to(DEV)                          # (I, O, 7): wf[i][o][j] = w[o][i][6 - j]
    wp = torch.empty(3 * K // 8, 8, N, 8, device=DEV)
    L.check(lib.tl_wino63_weights7(wf.data_ptr(), wp.data_ptr(), N, K, 7, st), "tl_wino63_weights7")
    ldw = N // 32 + 1
    sh = torch.arange(32, dtype=torch.int64)
    words = ((xin > 0).view(rows, N // 32, 32).to(torch.int64) << sh).sum(2)
    bits = torch.zeros(rows, ldw, dtype=torch.int64)
    bits[:, :N // 32] = words
    bits = torch.where(bits >= 2 ** 31, bits - 2 ** 32, bits).to(torch.int32).to(DEV)
    ldm = N + 8
    xm = torch.full((rows, ldm), float("nan"))
    xm[:, :N] = xin
    xm = xm.to(DEV)
    p = L.NtParams()

    def params(out):
        p.A, p.aux, p.Bw, p.out = D0.data_ptr(), D1.data_ptr(), wp.data_ptr(), out.data_ptr()
        p.M, p.A_rows, p.N, p.K, p.lda, p.ldb, p.ldo = rows, nh_pad, N, K, K, 3 * K, out.shape[1]
        p.J, p.row_shift, p.Tp, p.Tvalid, p.slope = 7, 0, Tp, Tp, slope
        p.loader, p.epilogue, p.splitk, p.bm = L.LOAD_V, L.EPI_MASK, 1, 128
        p.auxbits, p.ld_auxbits, p.mask, p.ld_mask = (bits.data_ptr(), ldw, None, 0) if mask == "bits" else (None, 0, xm.data_ptr(), ldm)
    outs = []
    for _ in range(2):
        out = torch.full((rows, N + 4), float("nan"), device=DEV)                # NaN canaries behind the leading dimension
        params(out)
        L.check(lib.tl_conv7_wino63v_dgrad_nt(C.byref(p), st), "tl_conv7_wino63v_dgrad_nt")
        outs.append(out)
    torch.cuda.synchronize()
    assert torch.equal(outs[0][:, :N], outs[1][:, :N])                           # a second launch: the same bits
    assert bool(torch.isnan(outs[0][:, N:]).all())
    got = outs[0][:, :N].cpu().double().view(nseq, Tp, N)
    assert bool(torch.isfinite(got).all())
    dx = F.conv_transpose1d(dz.double().view(nseq, Tp, K)[:, :t_out].permute(0, 2, 1), w.double())     # (nseq, N, t_in)
    want = torch.zeros(nseq, Tp, N, dtype=torch.float64)
    want[:, :t_in] = dx.permute(0, 2, 1)
    want = want * torch.where(xin.view(nseq, Tp, N) > 0, 1.0, slope).double()
    tag = f"S{nseq}Tp{Tp}t{t_in}K{K}N{N}_{mask}"
    ok = [_within("dgrad", tag + ".all_rows", ref.rel_l2(got, want)),
          _within("dgrad", tag + ".rows0_5_first_seq", ref.rel_l2(got[0, :6], want[0, :6])),
          _within("dgrad", tag + ".rows0_5_later_seqs", ref.rel_l2(got[1:, :6], want[1:, :6])),
          _within("dgrad", tag + ".rows_tout_tin", ref.rel_l2(got[:, t_out:t_in], want[:, t_out:t_in]))]
    assert all(ok), tag
    # hexes behind t_in whose three windows hold nothing but zeros (the sequence's last one sees the next sequence): exactly zero
    assert bool((got[:, -(-t_in // 6) * 6:Tp - 6] == 0).all())
    # bad arguments are refused
    params(outs[0])
    p.mask, p.ld_mask, p.auxbits, p.ld_auxbits = xm.data_ptr(), ldm, bits.data_ptr(), ldw
    assert lib.tl_conv7_wino63v_dgrad_nt(C.byref(p), st) != 0 and b"mask source" in lib.tl_last_error()
    params(outs[0])
    p.ldb = 2 * K
    assert lib.tl_conv7_wino63v_dgrad_nt(C.byref(p), st) != 0 and b"leading" in lib.tl_last_error()
    params(outs[0])
    p.row_shift = -6
    assert lib.tl_conv7_wino63v_dgrad_nt(C.byref(p), st) != 0
    params(outs[0])
    p.A_rows = 2
    assert lib.tl_conv7_wino63v_dgrad_nt(C.byref(p), st) != 0 and b"128-hex" in lib.tl_last_error()
    assert lib.tl_wino63_xform2s(dzd.data_ptr(), D0.data_ptr(), D1.data_ptr(), rows, Tp, t_out, 7, K, K, K, st) != 0


# ---------------------------------------------------------------------------------------------- one step
@pytest.mark.parametrize("dropout", [0.0, 0.5])
@pytest.mark.parametrize("shape,seed", rref.SHAPES[:3])
def test_one_step_gradients_under_wino63bwd(shape, seed, dropout, monkeypatch):
    _one_step(shape, seed, dropout, "wino63bwd", monkeypatch)


def test_one_step_where_tiles_and_k_steps_round_differently(monkeypatch):
    """B (w1 + C) Tp / 6 = 1 x 23 x 11 = 253 hexes: whole 128-hex tiles of the NT kernel (256) hold fewer hexes than the whole
    6-hex K-steps the weight-gradient kernel reads (258) - the workspaces must cover both."""
    shape, seed = (1, 22, 138, 138, 3), 4
    _one_step(shape, seed, 0.0, "wino63bwd", monkeypatch)
    from decode_tonal_langauge_amd._cnnrnn_classifier_train_engine import geometry
    geo = geometry(shape[1], shape[2], shape[3])
    assert shape[0] * geo["W"] * ((geo["t1"] + 5) // 6) == 253


def _grads(shape, seed, form, monkeypatch):
    monkeypatch.setenv("TONAL_KERNELS", f"conv7={form}")
    model, x, y = rref.build(shape, seed, 0.0)
    eng = _engine(model)
    eng.model.train()
    assert eng.conv7_form == "wino63" and eng.conv7_bwd == (form == "wino63bwd")
    out = {k: g.detach().clone().cpu() for k, g in eng.backward_only(x.to(DEV), y.to(DEV)).items()}
    torch.cuda.synchronize()
    return out


def test_gradients_agree_with_the_default_backward(monkeypatch):
    shape, seed = rref.SHAPES[1]
    new, old = _grads(shape, seed, "wino63bwd", monkeypatch), _grads(shape, seed, "wino63", monkeypatch)
    assert set(new) == set(old) and len(new) == 18
    tag = "B{}C{}T{}L{}n{}".format(*shape)
    ok = [_within("agree", f"{tag}.{k}", ref.rel_l2(new[k], old[k]), 2 * BOUND) for k in sorted(new)]
    assert all(ok)
    # what lies above the two wide stages does not depend on the form of their backward
    for k in new:
        if k.startswith(("output.", "lstm2.")):
            assert torch.equal(new[k], old[k]), k


def test_train_batch_never_reads_the_device_under_wino63bwd(monkeypatch):
    monkeypatch.setenv("TONAL_KERNELS", "conv7=wino63bwd")
    shape, seed = rref.SHAPES[0]
    B = shape[0]
    model, x, y = rref.build(shape, seed)
    eng = _engine(model, 0.001, 0.01)
    eng.model.train()
    x, y = x.to(DEV), y.float().to(DEV)
    eng.train_batch(x, y)                          # first call: workspaces, packs, optimizer state
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        eng.train_batch(x, y)
        eng.eval_batch(x, y)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert eng.epoch_stats()[1] == 3 * B


def test_flipped_packs_follow_the_update(monkeypatch):
    """Two steps, then the gradients at the moved weights: an engine that kept the first step's flipped tap packs would differ
    from a fresh engine built on a copy of the moved model - they must agree bit for bit (same kernels, same operands)."""
    monkeypatch.setenv("TONAL_KERNELS", "conv7=wino63bwd")
    shape, seed = rref.SHAPES[0]
    model, x, y = rref.build(shape, seed, 0.0)
    eng = _engine(model, 5e-3, 0.01)
    eng.model.train()
    xd, yd = x.to(DEV), y.to(DEV)
    first = {k: g.detach().clone() for k, g in eng.backward_only(xd, yd).items()}
    packs0 = {k: v[1].clone() for k, v in eng.packs._packed.items() if k.endswith("_dgrad")}
    assert set(packs0) == {"conv2_dgrad", "conv3_dgrad"}
    for _ in range(2):
        eng.train_batch(xd, yd)
    moved = {k: g.detach().clone() for k, g in eng.backward_only(xd, yd).items()}
    fresh_eng = _engine(copy.deepcopy(eng.model).cpu())
    fresh_eng.model.train()
    fresh = fresh_eng.backward_only(xd, yd)
    torch.cuda.synchronize()
    for k in moved:
        assert torch.equal(moved[k], fresh[k]), k
    for k, old in packs0.items():
        assert not torch.equal(eng.packs._packed[k][1], old), k                         # the packs were rebuilt from the moved weights
    assert not torch.equal(first["conv_pool_block1.0.weight"], moved["conv_pool_block1.0.weight"])
