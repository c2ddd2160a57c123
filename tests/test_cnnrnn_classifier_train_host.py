"""CPU: the float64 restatement of ``CNNRNNClassifier`` the GPU tests compare against IS the stock module; the geometry and the
``lstm2``-input index map of the training engine agree with torch; the new entry points are declared, bound, exported and
validate their arguments without a launch; ``ClassifierTrainer`` picks the engine (and names the device it refuses)."""
import os
import re

import pytest
import torch

from tests import classifier_train_ref as ref
from tests import cnnrnn_classifier_ref as rref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"tl_lstm_train_seq": 11, "tl_lstm_bptt_seq": 12, "tl_pool3_fwd": 14, "tl_pool3_bwd": 17, "tl_conv1_dgrad": 15}


@pytest.mark.parametrize("shape,seed", rref.SHAPES[:3])
def test_restatement_is_the_stock_module(shape, seed):
    model, x, y = rref.build(shape, seed)
    s32 = rref.forward(model, rref.leaves(model, torch.float32), x).detach()
    with torch.no_grad():
        stock32 = model.eval()(x)
    dev32 = float((s32 - stock32).abs().max())
    print(f"{shape}: float32 scores {dev32:.2e} from the stock module")
    assert dev32 <= 1e-6
    own = {}
    s, loss, g = rref.loss_and_grads(model, rref.leaves(model, torch.float64), x, y, own=own)
    s0, loss0, g0 = rref.stock_loss_and_grads(model, x, y, torch.float64)
    assert ref.rel_l2(s, s0) <= 1e-12 and ref.rel_l2(loss, loss0) <= 1e-12
    assert set(g) == set(g0) and len(g) == 18
    for k in g0:
        assert ref.rel_l2(g[k], g0[k]) <= 1e-12, k
    assert set(own) == set(rref.PLANES)
    # its OWN planes fed back: the same bits
    s1, loss1, g1 = rref.loss_and_grads(model, rref.leaves(model, torch.float64), x, y, planes=own)
    assert torch.equal(s1, s) and torch.equal(loss1, loss)
    assert all(torch.equal(g1[k], g[k]) for k in g)


@pytest.mark.parametrize("shape,seed", rref.SHAPES)
def test_geometry_and_lstm2_index_map_agree_with_torch(shape, seed):
    from decode_tonal_langauge_amd import _cnnrnn_classifier_train_engine as eng
    B, Cn, T, lstm_dim, _ = shape
    geo = eng.geometry(Cn, T, lstm_dim)
    model, x, _ = rref.build(shape, seed)
    with torch.no_grad():
        xt = x.permute(0, 2, 1)
        a = model.conv_pool_block1(xt.unsqueeze(1))
        b = model.conv_pool_block2(torch.zeros(B, 1, T, geo["w1"]))
        fa = model.conv_block3[0](torch.cat((b, a), dim=3))
        fb = model.conv_block3[2](fa)
        f = model.conv_block3[4](fb)
    assert (a.shape[2], fa.shape[2], fb.shape[2], f.shape[2], f.shape[3]) == (geo["t1"], geo["ta"], geo["tb"], geo["tq"], geo["W"])
    assert model.lstm2.input_size == 256 * geo["W"]
    tq, W = geo["tq"], geo["W"]
    idx = torch.arange(B * 256 * tq * W).view(B, 256, tq, W)            # a tensor of distinct integers through the raw view
    want = idx.contiguous().view(B, tq, -1)
    got = torch.full((tq * B, 256 * W), -1, dtype=torch.int64)
    g = torch.Generator().manual_seed(seed)
    picks = torch.stack([torch.randint(0, n, (400,), generator=g) for n in (B, 256, tq, W)], dim=1).tolist()
    picks += [[0, 0, 0, 0], [B - 1, 255, tq - 1, W - 1], [B - 1, 0, tq - 1, 0], [0, 255, 0, W - 1]]
    for bb, ch, s, w in picks:
        row, col = eng.lstm2_input_index(bb, ch, s, w, B, tq, W)
        assert row % B == bb
        got[row, col] = idx[bb, ch, s, w]
        assert int(want[bb, row // B, col]) == int(idx[bb, ch, s, w])   # (rows are time-major: row = step * B + b)


def test_new_entry_points_are_declared_bound_and_exported():
    from decode_tonal_langauge_amd import _lib
    lib = _lib.load()
    with open(os.path.join(ROOT, "include", "tonal_hip.h")) as f:
        header = f.read()
    for name, nargs in NEW.items():
        assert re.search(rf"\bint\s+{name}\s*\(", header), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        assert len(_lib.SIGNATURES[name][1]) == nargs, name


def test_new_entry_points_validate_their_arguments_without_gpu():
    from decode_tonal_langauge_amd import _lib
    lib = _lib.load()
    err = lib.tl_last_error
    fwd = lambda xp=16, rs=64, ss=256, wp=16, hs=16, cs=16, act=16, B=4, H=16, T=3: \
        lib.tl_lstm_train_seq(xp, rs, ss, wp, hs, cs, act, B, H, T, None)
    for name in ("xp", "wp", "hs", "cs", "act"):
        assert fwd(**{name: None}) == -1 and b"null" in err(), name
    assert fwd(H=12, rs=48, ss=192) == -1 and b"multiple of 8" in err()
    assert fwd(rs=60) == -1 and b"stride" in err()
    assert fwd(ss=60) == -1 and b"stride" in err()
    assert fwd(T=0) == -1 and b"T >= 1" in err()
    assert fwd(wp=20) == -1 and b"aligned" in err()
    bwd = lambda whT=16, dh=16, act=16, cs=16, dc=16, dg=16, dgt=16, ldt=12, B=4, H=16, T=3: \
        lib.tl_lstm_bptt_seq(whT, dh, act, cs, dc, dg, dgt, ldt, B, H, T, None)
    for name in ("whT", "dh", "act", "cs", "dc", "dg"):
        assert bwd(**{name: None}) == -1 and b"null" in err(), name
    assert bwd(H=20) == -1 and b"multiple of 8" in err()
    assert bwd(ldt=11) == -1 and b"ldt" in err()
    assert bwd(T=0) == -1 and b"T >= 1" in err()
    assert bwd(dg=20) == -1 and b"aligned" in err()
    pf = lambda Y=16, X=16, B=2, w1=1, Cn=2, C=256, Tp=12, tq=3, ldy=256, rb=1, rt=2, p=0.5: \
        lib.tl_pool3_fwd(Y, X, B, w1, Cn, C, Tp, tq, ldy, rb, rt, p, 7, None)
    assert pf(Y=None) == -1 and b"null" in err()
    assert pf(X=None) == -1 and b"null" in err()
    assert pf(tq=0) == -1 and b"tq" in err()
    assert pf(tq=5) == -1 and b"tq" in err()                              # 3 tq > Tp
    assert pf(ldy=255) == -1 and b"row stride" in err()
    assert pf(rt=0) == -1 and b"strides" in err()
    assert pf(p=1.0) == -1 and b"[0, 1)" in err()
    pb = lambda Y=16, dX=16, dZ=16, ldy=256, lddz=256, tq=3: \
        lib.tl_pool3_bwd(Y, dX, dZ, 2, 1, 2, 256, 12, tq, ldy, lddz, 1, 2, 0.5, 7, 0.01, None)
    for name in ("Y", "dX", "dZ"):
        assert pb(**{name: None}) == -1 and b"null" in err(), name
    assert pb(lddz=252) == -1 and b"row stride" in err()
    assert pb(ldy=128) == -1 and b"row stride" in err()
    assert pb(tq=0) == -1 and b"tq" in err()
    cd = lambda G=16, bits=16, w=16, dx=16, S=3, T=20, kt=7, C1=1024, Tp=8, Tout=7, ni=1, so=20, st=1, si=0: \
        lib.tl_conv1_dgrad(G, bits, w, dx, S, T, kt, C1, Tp, Tout, ni, so, st, si, None)
    for name in ("G", "bits", "w", "dx"):
        assert cd(**{name: None}) == -1 and b"null" in err(), name
    assert cd(S=0) == -1 and b"bad S" in err()
    assert cd(kt=9) == -1 and b"ktaps" in err()
    assert cd(C1=768) == -1 and b"C1" in err()
    assert cd(Tout=8) == -1 and b"inconsistent" in err()                  # 2 * 8 + 6 > 20
    assert cd(Tp=6) == -1 and b"inconsistent" in err()                    # Tout > Tp
    assert cd(T=20000, Tout=7) == -1 and b"too large" in err()
    assert cd(ni=0) == -1 and b"output map" in err()
    assert cd(G=20) == -1 and b"aligned" in err()
    # the 7-tap weight gradient of the two wide stages runs on the windowed TN GEMM: J up to 7 is taken, 8 is not
    t = _lib.TnParams()
    t.A = t.B = t.slab = 16
    t.Krows, t.Mdim, t.Ndim, t.lda, t.ldb, t.ldc, t.Tp, t.J = 64, 128, 128, 128, 128, 128, 8, 8
    import ctypes as C
    assert lib.tl_gemm_tn_window(C.byref(t), None) == -1 and b"J must be 1..7" in err()


def test_trainer_picks_the_engine_and_names_the_device_it_refuses():
    from decode_tonal_langauge_amd import _cnnrnn_classifier_train_engine as eng
    from decode_tonal_langauge_amd.models.classifier_trainer import ClassifierTrainer
    from decode_tonal_langauge_amd.models.deep_classifiers import CNNClassifier, CNNRNNClassifier
    model = CNNRNNClassifier(2, 60, 2, lstm_dim=60)
    with pytest.raises(ValueError, match="CNNRNNClassifier") as e:
        ClassifierTrainer(model, fused=True)
    assert "parameters on 'cpu'" in str(e.value)
    tr = ClassifierTrainer(model, fused=False)
    assert tr.engine is None and isinstance(tr.optimizer, torch.optim.NAdam)
    for bad, why in ((CNNRNNClassifier(2, 60, 2, lstm_dim=60, negative_slope=-0.1), "negative_slope -0.1"),
                     (CNNRNNClassifier(2, 60, 65, lstm_dim=60), "n_classes 65"),
                     (CNNRNNClassifier(2, 60, 2, lstm_dim=60, dropout=1.0), "dropout 1.0"),
                     (CNNRNNClassifier(2, 34, 2, lstm_dim=34), "input_length 34"),          # tb = 2: nothing behind the pool
                     (CNNClassifier(2, 150, 2), "model CNNClassifier")):
        with pytest.raises(ValueError, match="CNNRNNClassifier") as e:
            eng.check_supported(bad)
        assert why in str(e.value), (why, str(e.value))
