"""GPU: conv2's input gradient on Y2 (the operand its weight gradient already reads) instead of Vd2.

The gradient of a Winograd convolution with respect to its input is the transposition of ``y = A^T [(G g) . (B^T d)]``:
``dd[rows 6H .. 6H+7] = B [sum_cout (G g)_i . (A dz)_i]`` - the batched NT GEMM of ``tl_conv3_wino63v_nt`` on Y = A dz with the
un-flipped taps (``tl_wino63_weights_y``) and ``B`` in the epilogue (epilogue 4 with ``row_shift = 0``).  Rows 6, 7 of a hex are
rows 0, 1 of the next one; the fused conv1 weight gradient is linear in a row, so they are carried inside a lane or contracted
on their own, and dropped where the next hex starts a sequence.  With that reader gone, conv3's input gradient (epilogue 6)
writes Y2 only; Vd2 is kept under ``store_p1``.

1. epilogue 4 on Y through the C ABI against a float64 restatement, against the Vd form, and twice (bit-identical);
2. epilogue 6 without vout2 / vhalo: Y2 bit-identical to the Vd-writing variant's, nothing written beside it;
3. a small engine: every parameter gradient against the f63_yprod=0 engine, Vd2 absent by default, present under store_p1.
"""
import numpy as np
import pytest
import torch

from tests import parity_record
from tests.wino63_ref import hex_transform, logical, unpool, y_transform

pytestmark = pytest.mark.gpu

SLOPE = 0.01


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch.device("cuda:0")


def rel_l2(a, b):
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def pair_layout(V, nh_pad):
    """channels-last (hexes, 8, C) float64 -> the kernels' pair layout, float32, zero hexes appended to ``nh_pad``"""
    nh, _, C = V.shape
    out = torch.zeros(nh_pad, 8, C, dtype=torch.float32, device=V.device)
    out[:nh] = V.float()
    return out.reshape(nh_pad // 2, 2, 8, C // 8, 8).permute(0, 3, 2, 1, 4).contiguous().reshape(nh_pad, 8, C)


def unpack_bits(words, n):
    sh = torch.arange(32, device=words.device, dtype=torch.int32)
    return ((words[..., None] >> sh) & 1).reshape(*words.shape[:-1], n).bool()


def hex_pad(rows):
    return (rows // 6 + 24 + 127) // 128 * 128


# (S sequences, Tp, Tvalid, Tvalid_in = rows of dz2 that are not zero, T samples per sequence, N = C_out of conv1, K = C_out of conv2)
C1W_SHAPES = [
    # two row tiles, the second ragged; every lane-half crosses several sequence ends.  dz2 fills the whole sequence: rows 6, 7
    # of a sequence's last hex are not zero and must not reach the next sequence
    (70, 12, 9, 12, 26, 128, 48),
    (70, 12, 9, 12, 26, 128, 64),
    (70, 12, 9, 10, 26, 256, 64),
    # three hexes per sequence: lane-halves (16 hexes) start mid-sequence.  Tvalid_in 12: rows 12, 13 come out of rows 6, 7 of
    # the sequence's second hex alone; Tvalid_in 18: row 16, the last one that counts, sits beside a row 17 that does not
    (100, 18, 17, 12, 36, 128, 48),
    (100, 18, 17, 18, 36, 128, 64),
    # the timed geometry (400 samples -> 199 pooled rows in 204), and more row tiles (301) than persistent workgroups (256)
    (8, 204, 199, 196, 400, 128, 64),
    (1130, 204, 199, 196, 400, 128, 48),
]


def _c1w_case(dev, shape):
    from decode_tonal_langauge_amd import _lib
    from decode_tonal_langauge_amd._launch import launch_nt
    from decode_tonal_langauge_amd._lib import EPI_C1WGRAD, LOAD_V, check, ptr
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    S, Tp, Tvalid, Tin, T, N, K = shape
    g = torch.Generator(device=dev).manual_seed(1000 * S + Tp + K)
    M = S * Tp
    dz = torch.randn(S, Tp, K, device=dev, generator=g)
    dz[:, Tin:] = 0
    w = torch.randn(K, N, 3, 1, device=dev, generator=g) / (3 * K) ** 0.5
    rnd = lambda *s: torch.randint(-2 ** 31, 2 ** 31 - 1, s, device=dev, generator=g, dtype=torch.int64).to(torch.int32)
    sbits, cbits = rnd(M, N // 32), rnd(M, N // 32)
    x = torch.randn(S, T, device=dev, generator=g)
    # ---- float64 restatement: full correlation (cut at the sequence end), LeakyReLU', contraction with x[2 t + a + j], t < Tvalid
    dzd, wd = dz.double(), w.double()[..., 0]
    G1 = torch.zeros(S, Tp, N, dtype=torch.float64, device=dev)
    for j in range(3):
        G1[:, j:] += dzd[:, :Tp - j] @ wd[:, :, j]
    G1 *= torch.where(unpack_bits(sbits, N).view(S, Tp, N), 1.0, SLOPE)
    G1 = G1[:, :Tvalid]
    a = unpack_bits(cbits, N).view(S, Tp, N)[:, :Tvalid].long()
    t2 = 2 * torch.arange(Tvalid, device=dev)[None, :, None]
    xd = x.double()[:, :, None].expand(S, T, N)
    ref = torch.cat([(G1 * torch.gather(xd, 1, t2 + a + j)).sum((0, 1)) for j in range(3)] + [G1.sum((0, 1))])
    del xd
    # ---- operands of the two forms
    nh_pad = hex_pad(M)
    dz2 = dz.reshape(M, K)
    Y = pair_layout(y_transform(dz2, S, Tp), nh_pad)
    Vd = pair_layout(hex_transform(dz2, S, Tp, shift=-2), nh_pad)
    taps_y = torch.empty(8, N, K, device=dev)
    taps_d = torch.empty(8, N, K, device=dev)
    check(lib.tl_wino63_weights_y(ptr(w), ptr(taps_y), K, N, K, st), "tl_wino63_weights_y")
    check(lib.tl_wino63_weights(ptr(w), None, ptr(taps_d), K, N, N, K, st), "tl_wino63_weights")
    ntm = -(-M // lib.tl_wino63_nt_tile_rows())

    def run(A, taps, row_shift):
        part = torch.full((ntm, 4 * N), float("nan"), device=dev)
        launch_nt(lib, "tl_conv3_wino63v_nt", A=ptr(A), A_rows=nh_pad, lda=K, loader=LOAD_V, Bw=ptr(taps), M=M, N=N, K=K, ldb=K,
                  ldo=N, J=3, row_shift=row_shift, Tp=Tp, slope=SLOPE, auxbits=ptr(sbits), ld_auxbits=N // 32,
                  epilogue=EPI_C1WGRAD, out=None, c1x=ptr(x), c1bits=ptr(cbits), c1partial=ptr(part), c1T=T, c1kt=3, Tvalid=Tvalid)
        torch.cuda.synchronize()
        return part

    py, py2, pv = run(Y, taps_y, 0), run(Y, taps_y, 0), run(Vd, taps_d, -2)
    sy, sv = py.double().sum(0), pv.double().sum(0)
    obs = {"y_vs_f64": rel_l2(sy, ref), "vd_vs_f64": rel_l2(sv, ref), "y_vs_vd": rel_l2(sy, sv),
           "y_weights_vs_f64": rel_l2(sy[:3 * N], ref[:3 * N]), "y_bias_vs_f64": rel_l2(sy[3 * N:], ref[3 * N:])}
    print("c1w on Y", shape, obs)
    parity_record.record("c2_dgrad_on_y/" + "x".join(str(v) for v in shape), obs)
    assert bool(torch.isfinite(py).all())
    assert torch.equal(py, py2)
    assert obs["y_vs_f64"] < 1e-5 and obs["y_weights_vs_f64"] < 1e-5 and obs["y_bias_vs_f64"] < 1e-5, obs
    assert obs["y_vs_vd"] < 1e-5, obs


@pytest.mark.parametrize("shape", C1W_SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_conv1_weight_gradient_epilogue_on_y_matches_float64_and_the_vd_form(dev, shape):
    """1e-5 relative L2 on the summed partials: the bound the stage test holds this quantity to (test_gpu_parity.py,
    f63_stage_check).  Observed on the MI355X: see profiles/parity_observed.json, section c2_dgrad_on_y."""
    _c1w_case(dev, shape)


def test_epilogue_4_refuses_other_row_shifts(dev):
    from decode_tonal_langauge_amd import _lib
    import ctypes as C_
    lib = _lib.load()
    p = _lib.NtParams()
    d = torch.zeros(64, device=dev)
    for k in ("A", "Bw", "auxbits", "c1x", "c1bits", "c1partial"):
        setattr(p, k, d.data_ptr())
    p.loader, p.J, p.M, p.N, p.K, p.lda, p.ldb, p.Tp, p.A_rows, p.epilogue = 2, 3, 12, 32, 48, 48, 48, 12, 128, 4
    p.c1kt, p.c1T, p.Tvalid, p.row_shift = 3, 40, 8, -1
    assert lib.tl_conv3_wino63v_nt(C_.byref(p), None) != 0 and b"row_shift" in lib.tl_last_error()
    # epilogue 6 takes vout2 and vhalo together or not at all
    for k in ("abits", "vout", "vout2"):
        setattr(p, k, d.data_ptr())
    p.epilogue, p.row_shift, p.ld_abits, p.Tvalid_in, p.ld_vout, p.vout_quads = 6, -2, 1, 8, 32, 128
    assert lib.tl_conv3_wino63v_nt(C_.byref(p), None) != 0 and b"together" in lib.tl_last_error()


# (B, C, T, c2, c3) of the stage test's shapes (test_gpu_parity.py): the stage-3 input gradient, N = c2 columns, K = c3; the last
# one has 34 x 8 = 272 tiles for the 256 persistent workgroups
MASKY_SHAPES = [(2, 3, 200, 128, 64), (3, 5, 236, 256, 128), (1, 1, 44, 128, 128), (7, 3, 100, 128, 64), (8, 32, 400, 512, 512)]


@pytest.mark.parametrize("shape", MASKY_SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_masky_without_vd_writes_the_same_y_and_nothing_else(dev, shape):
    from decode_tonal_langauge_amd import _lib
    from decode_tonal_langauge_amd._launch import launch_nt
    from decode_tonal_langauge_amd._lib import EPI_MASKY, LOAD_V, check, ptr
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    B, C, T, c2, c3 = shape
    S = B * C
    tout1 = (T - 2) // 2
    tp2 = (tout1 + 11) // 12 * 12                   # rows per sequence of stage 2 (hexes of six)
    tout2 = (tout1 - 2) // 2
    tp3 = tp2 // 2                                  # ... of stage 3 = rows of this GEMM: three per hex of stage 2
    M = S * tp3
    g = torch.Generator(device=dev).manual_seed(S * 100 + T)
    dz3 = torch.randn(S, tp3, c3, device=dev, generator=g)
    dz3[:, 2 * ((tout2 - 2) // 2):] = 0
    Vd3 = pair_layout(hex_transform(dz3.reshape(M, c3), S, tp3, shift=-2), hex_pad(M))
    w = torch.randn(c3, c2, 3, 1, device=dev, generator=g) / (3 * c3) ** 0.5
    taps = torch.empty(8, c2, c3, device=dev)
    check(lib.tl_wino63_weights(ptr(w), None, ptr(taps), c3, c2, c2, c3, st), "tl_wino63_weights")
    rnd = lambda *s: torch.randint(-2 ** 31, 2 ** 31 - 1, s, device=dev, generator=g, dtype=torch.int64).to(torch.int32)
    sbits, abits = rnd(M, c2 // 32), rnd(M, c2 // 32)
    nh2 = S * tp2 // 6                              # hexes of stage 2 (M / 3), an even number
    nh2_pad = hex_pad(S * tp2)
    ntm = -(-M // lib.tl_wino63_nt_tile_rows())

    def run(Y, Vd2, halo):
        launch_nt(lib, "tl_conv3_wino63v_nt", A=ptr(Vd3), A_rows=Vd3.shape[0], lda=c3, loader=LOAD_V, Bw=ptr(taps), M=M, N=c2, K=c3,
                  ldb=c3, ldo=c2, J=3, row_shift=-2, Tp=tp3, slope=SLOPE, auxbits=ptr(sbits), ld_auxbits=c2 // 32,
                  epilogue=EPI_MASKY, out=None, vout=ptr(Y), vout2=ptr(Vd2), vhalo=ptr(halo), vout_quads=nh2_pad, ld_vout=c2,
                  abits=ptr(abits), ld_abits=c2 // 32, Tvalid_in=2 * tout2)
        torch.cuda.synchronize()

    Ya, Vda, halo = torch.zeros(nh2_pad, 8, c2, device=dev), torch.zeros(nh2_pad, 8, c2, device=dev), torch.zeros(ntm, 2, c2, device=dev)
    run(Ya, Vda, halo)
    assert float(Ya[:nh2].abs().max()) > 0 and float(Vda[:nh2].abs().max()) > 0
    # Y alone, in front of a poisoned buffer that lies where Vd2 would (one allocation: [Y2 | poison])
    both = torch.empty(2 * nh2_pad, 8, c2, device=dev)
    Yb, poison = both[:nh2_pad], both[nh2_pad:]
    outs = []
    for _ in range(2):
        Yb.zero_()
        Yb[:nh2] = float("nan")                     # every hex of the matrix is written; the pad hexes are not
        poison.fill_(-777.0)
        run(Yb, None, None)
        outs.append(Yb.clone())
        assert bool((poison == -777.0).all())
    assert torch.equal(outs[0], Ya) and torch.equal(outs[1], Ya)
    assert float(outs[0][nh2:].abs().max()) == 0.0


def _small_model(n_ch, T):
    """SynthesisModelCNN with a narrow conv stack (256, 256, 128, 64 channels): C_in of conv2 % 256 == 0, so f63_yprod applies"""
    from torch import nn
    from decode_tonal_langauge_amd._cnn_engine import CnnEngine
    from decode_tonal_langauge_amd.models.synthesis_models import SynthesisModelCNN
    m = SynthesisModelCNN(80, n_ch, T, dropout=0.0)
    ns, cc = 0.01, m.conv_channels
    m.ecog_conv_block = nn.Sequential(
        nn.Conv2d(1, 256, kernel_size=(3, 1)), nn.LeakyReLU(ns), nn.MaxPool2d((2, 1), (2, 1)),
        nn.Conv2d(256, 256, kernel_size=(3, 1)), nn.LeakyReLU(ns), nn.MaxPool2d((2, 1), (2, 1)),
        nn.Conv2d(256, 128, kernel_size=(3, 1)), nn.LeakyReLU(ns), nn.MaxPool2d((2, 1), (2, 1)),
        nn.Conv2d(128, 64, kernel_size=(1, 1)), nn.LeakyReLU(ns), nn.MaxPool2d((2, 1), (2, 1)),
        nn.Conv2d(64, cc, kernel_size=(1, 1)), nn.LeakyReLU(ns))
    defs = [(256, 3, True), (256, 3, True), (128, 3, True), (64, 1, True), (cc, 1, False)]
    widths = [c.out_channels for c in m.concat_conv_block if isinstance(c, nn.Conv2d)]
    m._pnames = [n for n, _ in m.named_parameters()]
    m._engine = CnnEngine(80, n_ch, T, m.lstm_channels, cc, 0.0, ns, defs, widths)
    assert m._engine.lat == m.latent_len
    return m


def test_engine_gradients_on_y_match_the_vd_partner_and_vd2_is_gone(dev, monkeypatch):
    from tests import golden_inputs as gi
    B, n_ch, T = 2, 3, 400
    xs, _t, _s, labs, tg = gi.train_batches(1, B, n_ch, T)
    torch.manual_seed(0)
    models = {}
    for key, yprod, keep in (("y", "1", False), ("vd", "0", False), ("kept", "1", True)):
        monkeypatch.setenv("TONAL_F63_YPROD", yprod)
        m = _small_model(n_ch, T)
        if models:
            m.load_state_dict(models["y"].state_dict())
        m._engine.store_p1 = keep
        models[key] = m.to(dev).train()
        out = m(xs[0].to(dev), labs[0].to(dev))
        (out - tg[0].to(dev).long()).abs().mean().backward()
    ey, ev, ek = (models[k]._engine for k in ("y", "vd", "kept"))
    assert ey.wino63 and ey.f63_yprod and not ev.f63_yprod and ek.f63_yprod
    worst = {}
    for (k, py), (_, pv), (_, pk) in zip(*(models[n].named_parameters() for n in ("y", "vd", "kept"))):
        worst[k] = rel_l2(py.grad, pv.grad)
        assert worst[k] < 1e-5, (k, worst[k])
        assert torch.equal(py.grad, pk.grad), k          # writing Vd2 as well changes nothing
    print("engine gradients, Y form against f63_yprod=0:", worst)
    parity_record.record("c2_dgrad_on_y/engine", {"worst_param_grad_rel_l2": max(worst.values())})
    assert 2 not in ey.Vd and 2 in ey.Yt
    assert 2 in ek.Vd
    # Vd2's content: B^T of the un-pooled gradient rows of stage 2, which the f63_yprod=0 engine stores (G2)
    s2 = ev.stages[0]
    assert torch.equal(ev.bits[2], ek.bits[2])
    dz2 = unpool(ev.G[2], ev.bits[2], ev.S, s2.tp_out, 2 * s2.tout, s2.cout)
    if 2 * s2.tp_out < s2.tp_in:
        dz2 = torch.nn.functional.pad(dz2, (0, 0, 0, s2.tp_in - 2 * s2.tp_out))
    ref = hex_transform(dz2[:, :s2.tp_in].reshape(-1, s2.cout), ev.S, s2.tp_in, shift=-2)
    got = logical(ek.Vd[2])
    assert float((got[:ref.shape[0]].double() - ref).abs().max()) <= 1e-5 * float(ref.abs().max())
    assert float(got[ref.shape[0]:].abs().max()) == 0.0
    assert np.isfinite(max(worst.values()))
