"""GPU: conv3 on whole-sequence tiles (the default; TONAL_KERNELS f63_yprod=vd3 is the partner).

At the reference shape a sequence of stage 3 stores 17 hexes (102 rows) and has 96 valid conv rows: exactly 16 hexes.  The
compact-M mode of ``tl_conv3_wino63v_nt`` (``a_hps_extra``) computes 16 hexes per sequence from the 17-hex layout - a lane owns
one whole sequence, a 128-hex tile eight.  The forward launch then never issues the padding hex; the input gradient runs on Y3
(the un-flipped taps, ``B`` in the epilogue) where its 17th hex is padding too, the two rows a hex hands to the next one stay in
the lane, and rows 96, 97 of a sequence become hex 32 of stage 2.  Vd3 has no reader left: conv4's input gradient (epilogue 7)
writes Y3 only.

1. forward, compact M, through the C ABI: pooled rows, arg-max and sign words bit-equal to the 17-hex launch, rows against float64;
2. the input gradient on Y3: Y2 against a float64 restatement and against the Vd-form launch, hex 33 and the pad hexes zero;
3. epilogue 7 without vout2 / vhalo: the same Y3, nothing written beside it;
4. a small engine, key on against key off; a shape where the path must not engage.
Every launch twice, bit-identical.  Observed values: profiles/parity_observed.json, section c3_seq_tiles.
"""
import ctypes as C_

import pytest
import torch

from tests import parity_record
from tests.wino63_ref import hex_transform, logical, unpool, y_transform

pytestmark = pytest.mark.gpu

SLOPE = 0.01
HPS = 17                                            # stored hexes per sequence of stage 3 (102 rows)


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


def hex_pad(S):
    """hexes of a stage-3 operand: whole 128-hex tiles, at least 24 zero hexes, and 8 stored sequences for every row tile"""
    return max((S * HPS + 24 + 127) // 128 * 128, (-(-S // 8) * 8 * HPS + 127) // 128 * 128)


def geometry(T):
    """rows of the stages behind conv1 (3 taps, pool 2) for ``T`` samples, from the engine's own ``_Stage``"""
    from decode_tonal_langauge_amd._conv_stack import _Stage
    tout1 = (T - 2) // 2
    tp1 = (tout1 + 11) // 12 * 12
    s2 = _Stage(2, 128, 128, 3, True, tout1, tp1)
    s3 = _Stage(3, 128, 64, 3, True, s2.tout, s2.tp_out)
    return s2, s3


def test_the_two_sample_counts_store_17_hexes_and_fill_16_or_fewer():
    s2, s3 = geometry(400)
    assert (s2.tp_in, s2.tout, s3.tp_in, s3.tc, s3.tout) == (204, 98, 102, 96, 48)
    s2, s3 = geometry(388)                          # the last hex of a lane is half padding: rows 93 .. 95 must be masked
    assert (s2.tp_in, s2.tout, s3.tp_in, s3.tc, s3.tout) == (204, 95, 102, 93, 46)


# (S sequences, T samples, K = C_in, N = C_out): one full tile, one partial tile, two full tiles and a partial one; 1037 sequences
# are 130 row tiles x 2 column tiles = 260 workgroups' worth for the 256 persistent ones - a workgroup walks on to a second tile
FWD_SHAPES = [(8, 400, 128, 64), (3, 400, 136, 96), (17, 400, 128, 96), (8, 388, 128, 64), (17, 388, 136, 96), (1037, 400, 128, 128)]


@pytest.mark.parametrize("shape", FWD_SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_forward_on_16_hexes_equals_the_17_hex_launch_and_matches_float64(dev, shape):
    """Bound against float64: 1e-5 relative L2 on the pooled rows, the bound of the c2_dgrad_on_y section of
    profiles/parity_observed.json (the forward GEMM is the same reduction over K x 3 taps)."""
    from decode_tonal_langauge_amd import _lib
    from decode_tonal_langauge_amd._launch import launch_nt
    from decode_tonal_langauge_amd._lib import EPI_POOL, LOAD_V, check, ptr
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    S, T, K, N = shape
    s2, s3 = geometry(T)
    tp, tin, tvalid, out_tp = s3.tp_in, s3.tin, 2 * s3.tout, 50
    g = torch.Generator(device=dev).manual_seed(31 * S + T + K)
    x = torch.randn(S, tp, K, device=dev, generator=g)
    x[:, tin:] = 0
    w = torch.randn(N, K, 3, 1, device=dev, generator=g) / (3 * K) ** 0.5
    bias = torch.randn(N, device=dev, generator=g) * 0.1
    nh_pad = hex_pad(S)
    V = pair_layout(hex_transform(x.reshape(S * tp, K), S, tp), nh_pad)
    taps = torch.empty(8, N, K, device=dev)
    check(lib.tl_wino63_weights(ptr(w), ptr(taps), None, N, K, K, N, st), "tl_wino63_weights")
    # ---- float64 restatement: conv, bias, LeakyReLU, max over row pairs of the valid rows
    xd, wd = x.double(), w.double()[..., 0]
    z = sum(xd[:, j:j + tvalid] @ wd[:, :, j].T for j in range(3)) + bias.double()
    z = torch.where(z > 0, z, SLOPE * z).view(S, tvalid // 2, 2, N)
    ref = z.max(2).values

    def run(compact):
        out = torch.zeros(S * out_tp, N, device=dev)
        bits, sbits = (torch.zeros(S * out_tp, N // 32, dtype=torch.int32, device=dev) for _ in range(2))
        geo = dict(M=S * 96, Tp=96, a_hps_extra=tp // 6 - 16) if compact else dict(M=S * tp, Tp=tp)
        launch_nt(lib, "tl_conv3_wino63v_nt", A=ptr(V), A_rows=nh_pad, lda=K, loader=LOAD_V, Bw=ptr(taps), bias=ptr(bias), out=ptr(out),
                  N=N, K=K, ldb=K, ldo=N, J=3, row_shift=0, slope=SLOPE, obits=ptr(bits), osign=ptr(sbits), ld_obits=N // 32,
                  Tvalid=tvalid, epilogue=EPI_POOL, out_tp=out_tp, **geo)
        torch.cuda.synchronize()
        return out, bits, sbits

    a, a2, b = run(True), run(True), run(False)
    for u, v, v2 in zip(b, a, a2):
        assert torch.equal(u, v) and torch.equal(v, v2)
    got = a[0].view(S, out_tp, N)
    assert float(got[:, tvalid // 2:].abs().max()) == 0.0
    obs = {"rows_vs_f64": rel_l2(got[:, :tvalid // 2], ref)}
    print("conv3 forward on 16 hexes", shape, obs)
    parity_record.record("c3_seq_tiles/forward/" + "x".join(str(v) for v in shape), obs)
    assert obs["rows_vs_f64"] < 1e-5, obs
    # the words are those of the rows: arg-max of every pair whose two values differ clearly, sign of every clear output
    odd = unpack_bits(a[1], N).view(S, out_tp, N)[:, :tvalid // 2]
    clear = (z[:, :, 1] - z[:, :, 0]).abs() > 1e-4
    assert torch.equal(odd[clear], (z[:, :, 1] > z[:, :, 0])[clear])
    pos = unpack_bits(a[2], N).view(S, out_tp, N)[:, :tvalid // 2]
    assert torch.equal(pos[ref.abs() > 1e-4], (ref > 0)[ref.abs() > 1e-4])


# (S, T, N = C_out of conv2 = columns, K = C_out of conv3 = reduction)
DGRAD_SHAPES = [(8, 400, 128, 64), (3, 400, 160, 72), (17, 400, 128, 64), (8, 388, 128, 64), (17, 388, 160, 72), (1037, 400, 128, 64)]


@pytest.mark.parametrize("shape", DGRAD_SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_input_gradient_on_y3_matches_float64_and_the_vd_form(dev, shape):
    """1e-5 relative L2 against float64 on Y2: the bound of the c2_dgrad_on_y section of profiles/parity_observed.json, which
    holds the same quantity (an input gradient on Y with B in the epilogue) one stage down.  The two forms reach the float64
    values along different roundings: apart by no more than the sum of their distances from it (recorded)."""
    from decode_tonal_langauge_amd import _lib
    from decode_tonal_langauge_amd._launch import launch_nt
    from decode_tonal_langauge_amd._lib import EPI_MASKY, LOAD_V, check, ptr
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    S, T, N, K = shape
    s2, s3 = geometry(T)
    tp3, tp2 = s3.tp_in, s2.tp_in                   # 102 rows of this GEMM per stored sequence, 204 conv rows of stage 2
    g = torch.Generator(device=dev).manual_seed(17 * S + T + N)
    dz3 = torch.randn(S, tp3, K, device=dev, generator=g)
    dz3[:, 2 * s3.tout:] = 0
    w = torch.randn(K, N, 3, 1, device=dev, generator=g) / (3 * K) ** 0.5
    rnd = lambda *s: torch.randint(-2 ** 31, 2 ** 31 - 1, s, device=dev, generator=g, dtype=torch.int64).to(torch.int32)
    sbits, abits = rnd(S * tp3, N // 32), rnd(S * tp3, N // 32)
    # ---- float64 restatement: full correlation inside the sequence, LeakyReLU', un-pool with the arg-max words, Y = A dz
    dzd, wd = dz3.double(), w.double()[..., 0]
    G2 = torch.zeros(S, tp3, N, dtype=torch.float64, device=dev)
    for j in range(3):
        G2[:, j:] += dzd[:, :tp3 - j] @ wd[:, :, j]
    G2 *= torch.where(unpack_bits(sbits, N).view(S, tp3, N), 1.0, SLOPE)
    dz2 = unpool(G2.reshape(S * tp3, N), abits, S, tp3, 2 * s2.tout, N)
    # the last gradient row that is valid and within two rows of a non-zero dz3 row carries gradient (97 at T = 400: hex 32)
    last = min(s2.tout, 2 * s3.tout + 2) - 1
    assert float(dz2[:, 2 * last:2 * last + 2].abs().max()) > 0 and (last == 97) == (T == 400)
    ref = y_transform(dz2.reshape(S * tp2, N), S, tp2)
    nh2 = S * tp2 // 6
    assert float(ref.view(S, 34, 8, N)[:, 33].abs().max()) == 0.0
    # ---- operands of the two forms
    nh_pad, nh2_pad = hex_pad(S), (nh2 + 24 + 127) // 128 * 128
    Y3 = pair_layout(y_transform(dz3.reshape(S * tp3, K), S, tp3), nh_pad)
    Vd3 = pair_layout(hex_transform(dz3.reshape(S * tp3, K), S, tp3, shift=-2), nh_pad)
    taps_y, taps_d = torch.empty(8, N, K, device=dev), torch.empty(8, N, K, device=dev)
    check(lib.tl_wino63_weights_y(ptr(w), ptr(taps_y), K, N, K, st), "tl_wino63_weights_y")
    check(lib.tl_wino63_weights(ptr(w), None, ptr(taps_d), K, N, N, K, st), "tl_wino63_weights")

    def run(on_y):
        both = torch.empty(2 * nh2_pad, 8, N, device=dev)       # [Y2 | poison where a Vd2 would lie]
        Y2, poison = both[:nh2_pad], both[nh2_pad:]
        Y2.zero_()
        Y2[:nh2] = float("nan")                     # every hex of the matrix is written (hex 33 as zeros); the pad hexes are not
        poison.fill_(-777.0)
        geo = (dict(A=ptr(Y3), Bw=ptr(taps_y), M=S * 96, Tp=96, a_hps_extra=tp3 // 6 - 16, row_shift=0) if on_y else
               dict(A=ptr(Vd3), Bw=ptr(taps_d), M=S * tp3, Tp=tp3, row_shift=-2))
        launch_nt(lib, "tl_conv3_wino63v_nt", A_rows=nh_pad, lda=K, loader=LOAD_V, N=N, K=K, ldb=K, ldo=N, J=3, slope=SLOPE,
                  auxbits=ptr(sbits), ld_auxbits=N // 32, epilogue=EPI_MASKY, out=None, vout=ptr(Y2), vout2=None, vhalo=None,
                  vout_quads=nh2_pad, ld_vout=N, abits=ptr(abits), ld_abits=N // 32, Tvalid_in=2 * s2.tout, **geo)
        torch.cuda.synchronize()
        assert bool((poison == -777.0).all())
        return Y2.clone()

    ya, ya2, yv = run(True), run(True), run(False)
    assert bool(torch.isfinite(ya).all()) and torch.equal(ya, ya2)
    la = logical(ya)
    assert float(la[nh2:].abs().max()) == 0.0                                      # pad hexes
    assert float(la[:nh2].view(S, 34, 8, N)[:, 33].abs().max()) == 0.0             # hex 33 of every sequence
    obs = {"y_vs_f64": rel_l2(la[:nh2], ref), "vd_vs_f64": rel_l2(logical(yv)[:nh2], ref), "y_vs_vd": rel_l2(la[:nh2], logical(yv)[:nh2]),
           "hex32_vs_f64": rel_l2(la[:nh2].view(S, 34, 8, N)[:, 32], ref.view(S, 34, 8, N)[:, 32])}
    print("conv3 input gradient on Y3", shape, obs)
    parity_record.record("c3_seq_tiles/dgrad/" + "x".join(str(v) for v in shape), obs)
    assert obs["y_vs_f64"] < 1e-5 and obs["hex32_vs_f64"] < 1e-5, obs
    assert obs["y_vs_vd"] <= 1.05 * (obs["y_vs_f64"] + obs["vd_vs_f64"]), obs


# (S, c3 = columns, c4 = reduction) at the reference geometry: 51 gradient rows per sequence, bit arrays of 50
GY_SHAPES = [(8, 64, 64), (3, 96, 72), (17, 64, 64)]


@pytest.mark.parametrize("shape", GY_SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_epilogue_7_without_vd_writes_the_same_y3_and_nothing_else(dev, shape):
    from decode_tonal_langauge_amd import _lib
    from decode_tonal_langauge_amd._lib import EPI_GY, LOAD_V, check, ptr
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    S, c3, c4 = shape
    tp3, tout3, gtp3 = 102, 48, 50
    tpg, tout4, gtp4 = tp3 // 2, tout3 // 2, (gtp3 + 1) // 2
    g = torch.Generator(device=dev).manual_seed(5 + S)
    G4 = torch.randn(S * gtp4, c4, device=dev, generator=g)
    G4.view(S, gtp4, c4)[:, tout4:] = 0
    rnd = lambda *s: torch.randint(-2 ** 31, 2 ** 31 - 1, s, device=dev, generator=g, dtype=torch.int64).to(torch.int32)
    ld4 = -(-c4 // 32)
    bits4, bits3, sbits3 = rnd(S * gtp4, ld4), rnd(S * gtp3, c3 // 32), rnd(S * gtp3, c3 // 32)
    W = torch.randn(c4, c3, device=dev, generator=g) / c4 ** 0.5
    rows = S * tpg
    nh_pad = (-(-rows // 6) + 127) // 128 * 128
    A = torch.zeros(nh_pad, 8, c4, device=dev)
    nh3, nh3_pad = S * HPS, hex_pad(S)
    ntm = -(-rows // lib.tl_wino63_nt_tile_rows())
    taps = torch.empty(c4 // 8, 8, c3, 8, device=dev)
    check(lib.tl_wino63_unpool_rows6(ptr(G4), ptr(bits4), ptr(A), rows, G4.shape[0], tpg, gtp4, 2 * tout4, c4, c4, ld4, c4, 0, st),
          "tl_wino63_unpool_rows6")
    check(lib.tl_wino63_weights1(ptr(W), ptr(taps), c4, c3, c4, st), "tl_wino63_weights1")

    def run(Y, Vd, halo):
        p = _lib.NtParams()
        p.splitk, p.bm = 1, 128
        for k, v in dict(A=ptr(A), A_rows=nh_pad, lda=c4, loader=LOAD_V, Bw=ptr(taps), M=rows, N=c3, K=c4, ldb=c4, ldo=c3, J=1,
                         row_shift=0, Tp=tpg, slope=SLOPE, auxbits=ptr(sbits3), ld_auxbits=c3 // 32, abits=ptr(bits3),
                         ld_abits=c3 // 32, out_tp=gtp3, Tvalid_in=2 * tout3, epilogue=EPI_GY, vout=ptr(Y), vout2=ptr(Vd),
                         vhalo=ptr(halo), vout_quads=nh3_pad, ld_vout=c3).items():
            setattr(p, k, v)
        check(lib.tl_conv1_wino63v_dgrad_nt(C_.byref(p), st), "tl_conv1_wino63v_dgrad_nt")
        torch.cuda.synchronize()

    Ya, Vda, halo = (torch.zeros(nh3_pad, 8, c3, device=dev), torch.zeros(nh3_pad, 8, c3, device=dev), torch.zeros(ntm, 2, c3, device=dev))
    run(Ya, Vda, halo)
    assert float(Ya[:nh3].abs().max()) > 0 and float(Vda[:nh3].abs().max()) > 0
    both = torch.empty(2 * nh3_pad, 8, c3, device=dev)
    Yb, poison = both[:nh3_pad], both[nh3_pad:]
    for _ in range(2):
        # (an odd hex count ends inside a pair: poison the hexes of the matrix in the logical order, not the memory order)
        Yb.copy_(pair_layout(torch.full((nh3, 8, c3), float("nan"), dtype=torch.float64, device=dev), nh3_pad))
        poison.fill_(-777.0)
        run(Yb, None, None)
        assert bool((poison == -777.0).all())
        assert torch.equal(Yb, Ya)
    # hex 16 of every sequence of Y3 is padding: the input gradient on whole-sequence tiles never reads it
    assert float(logical(Ya)[:nh3].view(S, HPS, 8, c3)[:, 16].abs().max()) == 0.0


def _small_model(n_ch, T):
    """SynthesisModelCNN with a narrow conv stack (256, 256, 128, 64 channels): C_in of conv2 and conv3 % 256 == 0, so both stages
    take their backward operands as Y and conv4's input gradient runs on the NT63 kernel"""
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


class _Launches:
    """names of the C-ABI entry points an engine calls, in order"""

    def __init__(self, lib):
        self._lib, self.names = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name.startswith("tl_") and callable(fn) and name != "tl_wino63_nt_tile_rows":      # (a query, not a launch)
            def wrapped(*a, _fn=fn, _n=name):
                self.names.append(_n)
                return _fn(*a)
            return wrapped
        return fn


def _step(m, dev, xs, labs, tg):
    m._engine.lib = _Launches(m._engine.lib)
    out = m(xs.to(dev), labs.to(dev))
    (out - tg.to(dev).long()).abs().mean().backward()
    torch.cuda.synchronize()
    return out.detach().clone(), m._engine.lib.names


# (one full row tile; one partial tile of 4 sequences with 93 valid rows - the model needs latent rows x channels % 4 == 0)
@pytest.mark.parametrize("T,B,n_ch", [(400, 2, 4), (388, 1, 4)], ids=["T400-S8", "T388-S4"])
def test_engine_key_on_against_key_off(dev, monkeypatch, T, B, n_ch):
    """Forward, bits and every gradient downstream of conv3's input gradient identical; conv2's and conv1's gradients within the
    stage bound (1e-5 relative L2); Vd3 and its halo rows gone; hex 33 of every sequence of Y2 and the pad hexes exactly zero."""
    from tests import golden_inputs as gi
    xs, _t, _s, labs, tg = gi.train_batches(1, B, n_ch, T)
    torch.manual_seed(0)
    models, outs, calls = {}, {}, {}
    for key in ("1", "0"):
        monkeypatch.setenv("TONAL_KERNELS", "f63_yprod=" + ("1" if key == "1" else "vd3"))
        m = _small_model(n_ch, T)
        if models:
            m.load_state_dict(models["1"].state_dict())
        models[key] = m.to(dev).train()
        outs[key], calls[key] = _step(m, dev, xs[0], labs[0], tg[0])
    e1, e0 = models["1"]._engine, models["0"]._engine
    assert e1.f63_seq16 and not e0.f63_seq16 and e1.gy4 and e0.gy4
    assert torch.equal(outs["1"], outs["0"])
    for i in (1, 2, 3, 4):
        assert torch.equal(e1.bits[i], e0.bits[i]) and torch.equal(e1.sbits[i], e0.sbits[i]), i
    assert torch.equal(e1.P[3], e0.P[3])
    upstream = ("ecog_conv_block.0.", "ecog_conv_block.3.")
    worst = {}
    for (k, p1), (_, p0) in zip(models["1"].named_parameters(), models["0"].named_parameters()):
        if k.startswith(upstream):
            worst[k] = rel_l2(p1.grad, p0.grad)
            assert worst[k] < 1e-5, (k, worst[k])
        else:
            assert torch.equal(p1.grad, p0.grad), k
    print("engine gradients, whole-sequence tiles against f63_yprod=vd3:", worst)
    parity_record.record(f"c3_seq_tiles/engine/T{T}", {"worst_upstream_grad_rel_l2": max(worst.values()), **worst})
    # the launch tables: one fix-up pass fewer (Vd3's), everything else the same entry points in the same order
    # (and conv3's input gradient packs the un-flipped taps)
    from collections import Counter
    assert calls["0"].count("tl_wino63_vd_fixup") == 1 and calls["1"].count("tl_wino63_vd_fixup") == 0
    assert Counter(calls["1"]) - Counter(calls["0"]) == Counter({"tl_wino63_weights_y": 1})
    assert Counter(calls["0"]) - Counter(calls["1"]) == Counter({"tl_wino63_vd_fixup": 1, "tl_wino63_weights": 1})
    # (no Vd3 of its own: Vd[3], the operand of stage 3's input gradient, is Y3 itself)
    assert e1.Vd[3] is e1.Yt[3] and "d3" not in e1._vhalo and e0.Vd[3] is not e0.Yt[3] and "d3" in e0._vhalo
    n3 = e0.Yt[3].shape[0]                           # (the whole-sequence operand may hold more zero hexes)
    assert torch.equal(e1.Yt[3][:n3], e0.Yt[3]) and not bool(e1.Yt[3][n3:].any())
    S = e1.S
    y2 = logical(e1.Yt[2])
    assert float(y2[:S * 34].view(S, 34, 8, -1)[:, 33].abs().max()) == 0.0 and float(y2[S * 34:].abs().max()) == 0.0
    assert float(y2[:S * 34].view(S, 34, 8, -1)[:, 32].abs().max()) > 0 or T != 400
    assert rel_l2(y2, logical(e0.Yt[2])) < 1e-5


def test_17_hexes_of_valid_rows_keep_the_old_launch_table(dev, monkeypatch):
    """412 samples: 99 valid conv rows at stage 3, 18 stored hexes - the path must not engage, key on or off"""
    from tests import golden_inputs as gi
    B, n_ch, T = 1, 3, 412
    xs, _t, _s, labs, tg = gi.train_batches(1, B, n_ch, T)
    torch.manual_seed(0)
    res = {}
    for key in ("1", "0"):
        monkeypatch.setenv("TONAL_KERNELS", "f63_yprod=" + ("1" if key == "1" else "vd3"))
        m = _small_model(n_ch, T)
        if res:
            m.load_state_dict(res["1"][0].state_dict())
        m = m.to(dev).train()
        assert m._engine.wino63 and m._engine.gy4 and not m._engine.f63_seq16 and m._engine.stages[1].tc == 99
        res[key] = (m,) + _step(m, dev, xs[0], labs[0], tg[0])
    assert res["1"][2] == res["0"][2] and res["1"][2].count("tl_wino63_vd_fixup") == 1
    assert torch.equal(res["1"][1], res["0"][1])
    for (k, p1), (_, p0) in zip(res["1"][0].named_parameters(), res["0"][0].named_parameters()):
        assert torch.equal(p1.grad, p0.grad), k
    e = res["1"][0]._engine
    assert e.Vd[3] is not e.Yt[3]
