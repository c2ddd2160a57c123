"""CPU: the oracle (oracle/*.py) against the committed golden vectors of the real reference."""
import os
import re
from argparse import Namespace

import numpy as np
import torch

from oracle import signal_oracle as sg
from oracle import synthesis_oracle as so
from tests import golden_inputs as gi

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def rel(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(float(np.max(np.abs(b))), 1e-30))


def test_g1_cnn_forward():
    g = np.load(os.path.join(GOLD, "g1_cnn_forward.npz"))
    torch.manual_seed(0)
    p = so.init_cnn_params(80, 4, 100)
    x, lab = gi.g1_inputs()
    assert abs(gi.checksum(x, lab) - float(g["in_checksum"])) < 1e-6 * float(g["in_checksum"])
    assert abs(gi.checksum(*p.values()) - float(g["param_checksum"])) < 1e-6 * float(g["param_checksum"])
    with torch.no_grad():
        out, inter = so.cnn_forward(p, x, lab, return_intermediates=True)
    assert rel(out, g["out"]) < 1e-5
    assert rel(inter["ecog5"], g["ecog5"]) < 1e-5
    assert rel(inter["lstm_h"], g["lstm_h"]) < 1e-5
    assert so.latent_length(100) == 5 and so.latent_length(400) == 24 and so.latent_length(200) == 11
    assert sum(int(np.prod(s)) for s in so.cnn_param_shapes(80, 128, 400).values()) == 1376768720


def test_g2_lite_forward():
    g = np.load(os.path.join(GOLD, "g2_lite_forward.npz"))
    torch.manual_seed(0)
    p, b = so.init_lite_params(80, 32, 200)
    x, lab = gi.g2_inputs()
    with torch.no_grad():
        out = so.lite_forward(p, b, x, lab, training=False)
    assert rel(out, g["out"]) < 1e-5
    assert sum(v.numel() for v in p.values()) == 919312


def _check_train(kind, gname, B, C, T, f64name=None):
    g = np.load(os.path.join(GOLD, gname))
    xs, _t, _s, labs, tg = gi.train_batches(3, B, C, T)
    assert abs(gi.checksum(*xs, *labs, *tg) - float(g["in_checksum"])) < 1e-6 * float(g["in_checksum"])
    torch.manual_seed(0)
    if kind == "lite":
        p, b = so.init_lite_params(80, C, T)
    else:
        p, b = so.init_cnn_params(80, C, T), None
    init = {k: v.clone().numpy() for k, v in p.items()}
    st = so.NAdamState(p)
    losses, mcds = [], []
    for s in range(3):
        l_, m_, gr, out = so.train_step(kind, p, b, st, xs[s], labs[s], tg[s], return_grads=True)
        losses.append(l_)
        mcds.append(m_)
        if s == 0:
            assert rel(out, g["out_step0"]) < 1e-5
            for k, v in gr.items():
                if "grad1." + k in g and np.abs(g["grad1." + k]).max() < 1e-6:
                    # analytically zero (a conv bias feeding BatchNorm): only rounding noise
                    assert float(v.abs().max()) < 1e-6, k
                elif "grad1." + k in g:
                    assert rel(v, g["grad1." + k]) < 1e-4, k
                else:
                    assert rel(v.numpy().reshape(-1)[::97], g["grad1." + k + "@s97"]) < 1e-4, k
    assert rel(losses, g["losses"]) < 1e-5 and rel(mcds, g["mcds"]) < 1e-5
    if f64name is None:
        for k, v in p.items():
            fin = v.numpy()
            if "final." + k in g:
                assert gi.update_rel_l2(fin, g["final." + k], init[k]) < 1e-3, k
            else:
                assert gi.update_rel_l2(fin.reshape(-1)[::97], g["final." + k + "@s97"], init[k].reshape(-1)[::97]) < 1e-3, k
    else:
        # G4's conv biases with cancelling fp32 gradient sums: their fp32 three-step update moves by up to 3e-3 with the
        # summation order of the host (oracle/make_golden_f64.py) - the update is pinned with both sides in float64
        g64 = np.load(os.path.join(GOLD, f64name))
        torch.manual_seed(0)
        p64 = {k: v.double() for k, v in so.init_cnn_params(80, C, T).items()}
        st64 = so.NAdamState(p64)
        for s in range(3):
            so.train_step(kind, p64, None, st64, xs[s].double(), labs[s].double(), tg[s].double())
        for k, v in p64.items():
            upd = v.numpy() - init[k]
            ref = g64["upd." + k] if "upd." + k in g64 else None
            if ref is None:
                upd, ref = upd.reshape(-1)[::97], g64["upd." + k + "@s97"]
            assert upd.shape == ref.shape, k
            assert np.linalg.norm(upd - ref) / np.linalg.norm(ref) < 1e-6, k
    return b, g


def test_g3_lite_train_steps():
    b, g = _check_train("lite", "g3_lite_train.npz", 64, 32, 200)
    assert rel(b["ecog_conv.1.running_mean"], g["run_mean0"]) < 1e-5
    assert rel(b["ecog_conv.1.running_var"], g["run_var0"]) < 1e-5
    assert rel(b["ecog_conv.5.running_var"], g["run_var1"]) < 1e-5


def test_g4_cnn_train_steps():
    _check_train("cnn", "g4_cnn_train.npz", 8, 16, 200, f64name="g4f64_cnn_update.npz")


def test_g5_tone_dynamics():
    g = np.load(os.path.join(GOLD, "g5_tone_dynamics.npz"))
    out = so.prepare_tone_dynamics({"0": [3, 3, 3], "1": [1, 2, 3]}, [1, 0], [0, 1])
    assert np.array_equal(out, g["out_small"]) and out.tolist() == [[[0, 0, 0], [1, 2, 3]], [[1, 1, 1], [3, 3, 3]]]
    assert np.array_equal(so.prepare_tone_dynamics(gi.TONE_MAP, g["tones"], g["syls"]), g["out"])
    try:
        so.prepare_tone_dynamics({"0": [1]}, [2], [0])
        raise AssertionError("expected ValueError")
    except ValueError:
        pass


def test_g6_signal_filters():
    g = np.load(os.path.join(GOLD, "g6_signal.npz"))
    x, x2 = gi.g6_inputs()
    assert abs(gi.checksum(x, x2) - float(g["in_checksum"])) < 1e-9 * float(g["in_checksum"])
    assert rel(sg.hilbert_filter(x, 400, [70., 150.]), g["hilbert"]) < 1e-12
    assert abs(float(g["hilbert"].sum()) - 560.469727933) < 1e-6          # SURVEY.md G6 session value
    assert rel(sg.hilbert_filter(x, 400, [70., 150.], envelope=False), g["hilbert_real"]) < 1e-12
    assert rel(sg.butter_filter(x, [0.3, 100], 400), g["butter"]) < 1e-12
    assert rel(sg.butter_filter(x, [0.3, 100], 400, causal=True), g["butter_causal"]) < 1e-10
    assert rel(sg.fir_bandpass_filter(x, 400, 390, [100.]), g["fir"]) < 1e-12
    assert rel(sg.fir_bandpass_filter(x, 400, 64, [60., 120.]), g["fir2"]) < 1e-12
    assert rel(sg.hilbert_filter(x2, 400, [(70., 110.), (110., 150.)]), g["hilbert2"]) < 1e-5
    prm = Namespace(signal_freq=400, bands=[
        {"method": "hilbert", "params": {"freq_ranges": [70., 150.], "envelope": True}},
        {"method": "butter", "params": {"freqs": [0.3, 100], "filter_type": "bandpass"}},
        {"method": "fir", "params": {"order": 390, "center_frequencies": [100.]}}])
    assert rel(sg.run(x, prm), g["run"]) < 1e-12
    cfs, sds = sg.gaussian_bank([70., 150.], 400)
    assert len(cfs) == 8 and abs(cfs[0] - 73.73) < 0.01 and abs(cfs[-1] - 147.46) < 0.01


def test_g8_split_and_g9_trainer_history():
    from decode_tonal_langauge_amd.data_loading.dataloaders import split_dataset
    from decode_tonal_langauge_amd.models.simple_classifiers import LogisticRegressionClassifier
    g8 = np.load(os.path.join(GOLD, "g8_split.npz"))
    idx = so.split_indices(100, [0.9, 0.1], 42)
    assert idx[0] == g8["train_idx"].tolist() and idx[1] == g8["test_idx"].tolist()
    ds = torch.utils.data.TensorDataset(torch.arange(100).float())
    loaders = split_dataset(ds, [0.9, 0.1], [True, False], batch_size=8, seed=42)
    assert list(loaders[0].dataset.indices) == g8["train_idx"].tolist()
    first = np.concatenate([b[0].numpy() for b in loaders[0]])
    assert np.array_equal(first, g8["first_epoch"])
    # G9: the reference's SynthesisTrainer.train history, replayed with the oracle step
    g9 = np.load(os.path.join(GOLD, "g9_trainer.npz"))
    N, C, T = 96, 32, 200
    e_non, e_syl, e_tone, tgt = gi.g9_dataset(N, C, T)
    assert abs(gi.checksum(e_non, e_syl, e_tone, tgt) - float(g9["in_checksum"])) < 1e-6 * float(g9["in_checksum"])
    ds = torch.utils.data.TensorDataset(e_non, e_syl, e_tone, tgt)
    torch.manual_seed(7)
    tone_model = LogisticRegressionClassifier(8 * T, 4)
    syl_model = LogisticRegressionClassifier(8 * T, 2)
    assert abs(gi.checksum(tone_model.linear.weight, syl_model.linear.weight) - float(g9["cls_checksum"])) < 1e-6
    loaders = split_dataset(ds, [0.75, 0.25], [True, False], batch_size=16, seed=11)
    torch.manual_seed(0)
    p, b = so.init_lite_params(80, C, T)
    st = so.NAdamState(p)
    hist = []
    for _epoch in range(2):
        el, em, nb = 0.0, 0.0, 0
        for xn, xs_, xt, tg in loaders[0]:
            with torch.no_grad():
                tone = torch.argmax(tone_model(xt), dim=1)
                syl = torch.argmax(syl_model(xs_), dim=1)
            lab = torch.Tensor(so.prepare_tone_dynamics(gi.TONE_MAP, tone.numpy(), syl.numpy()))
            l_, m_ = so.train_step("lite", p, b, st, xn, lab, tg)
            el += l_
            em += m_
            nb += 1
        hist.append((el / nb, em / nb))
    assert rel(np.array(hist), g9["history"]) < 1e-4


def test_g7_other_signal_steps():
    g = np.load(os.path.join(GOLD, "g7_steps.npz"))
    x = np.random.default_rng(7).standard_normal((5, 900)) * 3.0 + 1.5
    assert abs(gi.checksum(x) - float(g["in_checksum"])) < 1e-9 * float(g["in_checksum"])
    assert rel(sg.channel_zscore(x), g["channel_zscore"]) < 1e-12
    assert rel(sg.zscore_rereference(x, 50, 300), g["zscore_rereference"]) < 1e-12
    assert rel(sg.car_rereference(x, [1, 3]), g["car"]) < 1e-12
    rz = sg.rolling_zscore(x, 50)
    assert np.array_equal(np.isnan(rz), np.isnan(g["rolling"])) and rel(np.nan_to_num(rz), np.nan_to_num(g["rolling"])) < 1e-12
    xn = x.copy()
    xn[2, 100:130] = np.nan
    assert rel(sg.rolling_zscore(xn, 50, preserve_nans=False), g["rolling_nan"]) < 1e-12
    ds, fs = sg.downsample(x, 1000, 400)
    assert fs == 400 and rel(ds, g["downsample"]) < 1e-12
    assert rel(sg.downsample(x.astype(np.float32), 1000)[0], g["downsample_f32"]) < 1e-5
    assert rel(sg.downsample(x[:, :601], 300, 400)[0], g["downsample_up"]) < 1e-12


RESAMPLE_GRID = [(900, 1200), (901, 1200), (900, 1201), (1000, 1000), (1001, 1001), (1200, 900), (1201, 900), (2, 5),
                 (7, 1)]


def test_resample_oracle_is_scipy_resample_bit_for_bit():
    from scipy.signal import resample
    rng = np.random.default_rng(11)
    for nx, num in RESAMPLE_GRID:
        x = rng.standard_normal((3, nx)) * 2.0 + 0.5
        assert np.array_equal(sg.resample_fft(x, num), resample(x, num, axis=1)), (nx, num)


def test_rolling_zscore_oracle_matches_pandas_on_edge_windows():
    """Constant stretches (pandas: mean = the value, std = 0, so NaN), NaN stretches giving windows with 0 and 1
    valid values, W > T and W = 2: the NaN pattern is pandas' exactly; finite values agree with the exact two-pass
    statement to 1e-10 and with pandas to 1e-7 (pandas moves its window sums sample by sample; at W = 2 that drift
    reaches 1.2e-8 here, on a pair of samples 1e-3 apart)."""
    from tests.signal_refs import pandas_rolling_zscore, rolling_cases, two_pass_rolling_zscore
    rng = np.random.default_rng(5)
    for C, T, W in ((4, 700, 10), (4, 700, 50), (4, 301, 2), (4, 300, 450), (3, 250, 120)):
        x = rolling_cases(rng, C, T, W)
        for keep in (True, False):
            o = sg.rolling_zscore(x, W, preserve_nans=keep)
            p = pandas_rolling_zscore(x, W, preserve_nans=keep)
            assert np.array_equal(np.isnan(o), np.isnan(p)), (C, T, W, keep)
            assert rel(np.nan_to_num(o), np.nan_to_num(two_pass_rolling_zscore(x, W, keep))) < 1e-10, (C, T, W, keep)
            assert rel(np.nan_to_num(o), np.nan_to_num(p)) < 1e-7, (C, T, W, keep)
    # the reported case: N(0,1), then a flat 0.1 - pandas gives NaN on the whole flat stretch
    x = np.concatenate([np.random.default_rng(0).standard_normal(40), np.full(60, 0.1)])[None]
    for W in (10, 50):
        assert np.isnan(sg.rolling_zscore(x, W)[0, 40 + W - 1:]).all()
        assert np.array_equal(np.isnan(sg.rolling_zscore(x, W)), np.isnan(pandas_rolling_zscore(x, W)))


def _g_sample(g, full):
    if full in g.files:
        return g[full], None
    key = next(k for k in g.files if k.startswith(full + "@s") and not k.endswith("@sum"))
    return g[key], int(key.rsplit("@s", 1)[1])


def test_g11_c3_shape_conv_stack():
    """Golden G11 (reference train step at the north-star shape, B = 2): the oracle's ECoG conv stack on
    the same input.  The five conv layers are the first modules the constructor draws, so seeding and
    building only them reproduces the golden's conv weights without the 5.4 GB LSTM."""
    g = np.load(os.path.join(GOLD, "g11_c3_step.npz"))
    D, C, T, B = (int(v) for v in g["dims"])
    xs, _t, _s, labs, tg = gi.train_batches(1, B, C, T, seed=int(g["data_seed"]))
    assert abs(gi.checksum(xs[0], labs[0], tg[0]) - float(g["in_checksum"])) < 1e-6 * float(g["in_checksum"])
    torch.manual_seed(0)
    p = {}
    cin = 1
    for idx, (cout, k, _pool) in zip((0, 3, 6, 9, 12), so.ECOG_STAGES):
        conv = torch.nn.Conv2d(cin, cout or 64, kernel_size=(k, 1))
        p[f"ecog_conv_block.{idx}.weight"], p[f"ecog_conv_block.{idx}.bias"] = conv.weight.detach(), conv.bias.detach()
        cin = cout or 64
    x = xs[0].unsqueeze(1).permute(0, 1, 3, 2)
    with torch.no_grad():
        for si, (idx, (_c, _k, pool)) in enumerate(zip((0, 3, 6, 9, 12), so.ECOG_STAGES)):
            x = torch.nn.functional.leaky_relu(torch.nn.functional.conv2d(
                x, p[f"ecog_conv_block.{idx}.weight"], p[f"ecog_conv_block.{idx}.bias"]), 0.01)
            if pool:
                x = torch.nn.functional.max_pool2d(x, (2, 1), (2, 1))
            ref, stride = _g_sample(g, f"act.ecog{si + 1}")
            got = x.reshape(-1)[::stride].numpy() if stride else x.numpy()
            assert rel(got, ref.reshape(got.shape)) < 1e-5, si
    assert x.shape == (B, 64, 24, C)
    # keys of the golden cover every parameter's gradient and final value
    names = list(so.cnn_param_shapes(D, C, T))
    for n in names:
        assert any(k.startswith("grad." + n) for k in g.files) and any(k.startswith("final." + n) for k in g.files), n


def test_g12_deep_classifier_mirrors_cpu_graph():
    """The mirror modules' own (CPU, stock torch) graph against the reference's outputs: same seeds,
    same state_dict keys, same numbers - this is what makes them usable as the C5 oracle."""
    from decode_tonal_langauge_amd.models.deep_classifiers import CNNClassifier, CNNRNNClassifier
    g = np.load(os.path.join(GOLD, "g12_deep_classifiers.npz"))
    for i in range(2):
        C, T, ncls, B, seed = (int(v) for v in g[f"cnn{i}.cfg"])
        torch.manual_seed(seed)
        net = CNNClassifier(input_channels=C, input_length=T, n_classes=ncls).eval()
        x = torch.randn(B, C, T)
        with torch.no_grad():
            assert rel(net(x), g[f"cnn{i}.out"]) < 1e-6
        assert list(net.state_dict().keys()) == list(g[f"cnn{i}.keys"])
    for i in range(2):
        C, T, ncls, B, ld, seed = (int(v) for v in g[f"cnnrnn{i}.cfg"])
        torch.manual_seed(seed)
        net = CNNRNNClassifier(input_channels=C, input_length=T, n_classes=ncls, lstm_dim=ld).eval()
        x = torch.randn(B, C, T)
        with torch.no_grad():
            assert rel(net(x), g[f"cnnrnn{i}.out"]) < 1e-6
        assert list(net.state_dict().keys()) == list(g[f"cnnrnn{i}.keys"])


def test_g13_preprocess_chain_oracle():
    g = np.load(os.path.join(GOLD, "g13_preprocess_chain.npz"))
    x = gi.chain_input()
    assert abs(gi.checksum(x) - float(g["in_checksum"])) < 1e-9 * float(g["in_checksum"])
    d, f = sg.downsample(x, 1000, 400)
    d = sg.car_rereference(d, [2])
    d = sg.run(d, Namespace(signal_freq=f, bands=gi.CHAIN_STEPS[2]["params"]["bands"]))
    d = sg.channel_zscore(d)
    assert f == int(g["freq"]) and rel(d, g["out"]) < 1e-10


def test_g14_trajectory_oracle_follows_the_reference():
    """G14: 30 NAdam steps of the reference's SynthesisModelCNN(80, 16, 200) - the oracle's loss and mel MSE stay
    within 1e-4 of the reference at every step (observed 1.1e-6)."""
    g = np.load(os.path.join(GOLD, "g14_cnn_trajectory.npz"))
    D, C, T, B, N = (int(v) for v in g["dims"])
    xs, _t, _s, labs, tg = gi.train_batches(N, B, C, T, seed=int(g["data_seed"]))
    assert abs(gi.checksum(*xs, *labs, *tg) - float(g["in_checksum"])) < 1e-6 * float(g["in_checksum"])
    torch.manual_seed(int(g["seed"]))
    p = so.init_cnn_params(D, C, T)
    st = so.NAdamState(p)
    for s in range(N):
        loss, mcd, _g, out = so.train_step("cnn", p, None, st, xs[s], labs[s], tg[s], return_grads=True)
        mse = float(((out.double() - tg[s].double()) ** 2).mean())
        assert abs(loss - g["losses"][s]) < 1e-4 * g["losses"][s], s
        assert abs(mcd - g["mcds"][s]) < 1e-4 * g["mcds"][s], s
        assert abs(mse - g["mses"][s]) < 1e-4 * g["mses"][s], s


def test_g15_hilbert_low_band_at_raw_rate():
    """G15: the reference's hilbert_filter for a 1-4 Hz band and the high-gamma band at 3 kHz."""
    g = np.load(os.path.join(GOLD, "g15_hilbert_low_band.npz"))
    fs = int(g["fs"])
    x = np.random.default_rng(15).standard_normal((2, 9000))
    assert abs(float(np.abs(x).sum()) - float(g["x_checksum"])) < 1e-9
    for name, fr, env in (("low_env", [1.0, 4.0], True), ("low_real", [1.0, 4.0], False), ("hg_env", [70.0, 150.0], True)):
        assert rel(sg.hilbert_filter(x, fs, fr, envelope=env), g[name]) < 1e-12, name


def test_f63_matrices_of_the_kernels_are_the_exact_cook_toom_construction():
    """The constants the F(6,3) kernels and their GPU tests use (tests/wino63_ref.py: B^T, A^T; csrc/tonal_wino63.hip: the same
    plus G) are the exact rational Cook-Toom matrices of the numerics gate (oracle/winograd_f63_gate.py) for the points
    0, +-1, +-2, +-1/2, inf - and together they ARE the 3-tap correlation: sum_j A^T[i][j] G[j][k] B^T[j][s] = [s == i + k]."""
    from fractions import Fraction
    import numpy as np
    import torch
    from oracle.winograd_f63_gate import cook_toom
    from tests.wino63_ref import AT, BT, hex_transform, logical, y_transform
    At, G, Bt = cook_toom(6, 3, (0, 1, -1, 2, -2, Fraction(1, 2), Fraction(-1, 2)))
    assert torch.equal(At.double(), AT) and torch.equal(Bt.double(), BT)
    Gk = torch.tensor([[-1, 0, 0], [-2 / 9, -2 / 9, -2 / 9], [-2 / 9, 2 / 9, -2 / 9], [1 / 90, 2 / 90, 4 / 90], [1 / 90, -2 / 90, 4 / 90],
                       [32 / 45, 16 / 45, 8 / 45], [32 / 45, -16 / 45, 8 / 45], [0, 0, 1]], dtype=torch.float64)       # tl_wino63_weights
    assert torch.allclose(G.double(), Gk, rtol=0, atol=1e-7)
    ident = torch.einsum("ij,jk,js->iks", AT, Gk, BT)
    want = torch.zeros(6, 3, 8, dtype=torch.float64)
    for i in range(6):
        for k in range(3):
            want[i, k, i + k] = 1
    assert torch.allclose(ident, want, atol=1e-12)
    # the reference forms of the operand layouts: a random stage through hexes equals the direct correlation
    g = torch.Generator().manual_seed(3)
    S, Tp, C, O = 2, 12, 8, 5
    x = torch.randn(S * Tp, C, generator=g, dtype=torch.float64)
    w = torch.randn(O, C, 3, generator=g, dtype=torch.float64)
    V = hex_transform(x, S, Tp)                                    # (S * Tp / 6, 8, C)
    U = torch.einsum("jk,ock->joc", Gk, w)
    M = torch.einsum("hjc,joc->hjo", V, U)
    y = torch.einsum("ij,hjo->hio", AT, M).reshape(S, Tp, O)       # six conv rows per hex
    xp = torch.nn.functional.pad(x.view(S, Tp, C), (0, 0, 0, 2))
    ref = sum(torch.einsum("stc,oc->sto", xp[:, k:k + Tp], w[:, :, k]) for k in range(3))
    assert torch.allclose(y, ref, atol=1e-10)
    # weight gradient through Y = A dz: dW[o][c][k] = sum_rows dz[r][o] x[r + k][c]
    dz = torch.randn(S * Tp, O, generator=g, dtype=torch.float64)
    Y = y_transform(dz, S, Tp)
    slab = torch.einsum("hjc,hjo->jco", V, Y)
    dW = torch.einsum("jk,jco->ock", Gk, slab)
    refW = torch.stack([torch.einsum("sto,stc->oc", dz.view(S, Tp, O), xp[:, k:k + Tp]) for k in range(3)], dim=2)
    assert torch.allclose(dW, refW, atol=1e-9)
    # the pair layout is a permutation: logical() undoes it
    nh, Cc = 4, 16
    lin = torch.arange(nh * 8 * Cc, dtype=torch.float32).reshape(nh, 8, Cc)
    pair = lin.reshape(nh // 2, 2, 8, Cc // 8, 8).permute(0, 3, 2, 1, 4).reshape(nh, 8, Cc)       # store channels-last data pair-wise
    assert torch.equal(logical(pair), lin)
    assert np.isfinite(float(ident.sum()))


def test_decided_backward_is_torchs_own_given_torchs_own_branches():
    """oracle.synthesis_oracle._ActPoolDecided (the backward pass on externally supplied LeakyReLU' / arg-max branches, used
    by the GPU tests to separate flipped near-ties from arithmetic): with the branches torch takes by itself it reproduces
    F.leaky_relu + F.max_pool2d bit for bit - forward and every gradient - and a flipped arg-max plane moves the gradients
    upstream of it only."""
    from oracle import synthesis_oracle as so
    torch.manual_seed(0)
    p = so.init_cnn_params(80, 4, 100)
    x, lab, tg = torch.randn(3, 4, 100), torch.randn(3, 2, 5), torch.randn(3, 80)

    def run(dec=None, own=None):
        leaves = {k: v.clone().requires_grad_(True) for k, v in p.items()}
        out = so.cnn_forward(leaves, x, lab, decisions=dec, own=own)
        return out, dict(zip(leaves, torch.autograd.grad(so.l1_loss(out, tg), list(leaves.values()))))

    o1, g1 = run()
    own = {}
    run(own=own)
    assert sorted(own) == sorted([f"ecog{i}.{k}" for i in (1, 2, 3, 4) for k in ("odd", "pos")] + ["ecog5.pos"]
                                 + [f"concat{i}.pos" for i in (1, 2, 3, 4, 5)])
    o2, g2 = run(dec=own)
    assert torch.equal(o1, o2) and all(torch.equal(g1[k], g2[k]) for k in g1)
    flipped = dict(own, **{"ecog3.odd": ~own["ecog3.odd"]})
    o3, g3 = run(dec=flipped)
    assert torch.equal(o1, o3)                                   # forward values never depend on the supplied branches
    for k in g1:
        upstream = k.startswith("ecog_conv_block.") and int(k.split(".")[1]) <= 6
        assert torch.equal(g1[k], g3[k]) != upstream, k


def test_flip_checker_rejects_corrupted_planes_and_accepts_a_near_tie():
    """tests/branch_planes.check_flips (the GPU tests check the HIP path's sign / arg-max planes with it instead of trusting
    them): the oracle's own planes pass, one flip at the smallest margin passes (a near-tie), and each corruption a pooling
    epilogue could make - channels shifted by one, one 32-bit word inverted, the last row tile left zero - is rejected."""
    import pytest
    from tests.branch_planes import check_flips
    torch.manual_seed(0)
    p = so.init_cnn_params(80, 4, 100)
    x, lab = torch.randn(3, 4, 100), torch.randn(3, 2, 5)
    own, margins = {}, {}
    with torch.no_grad():
        so.cnn_forward(p, x, lab, own=own, margins=margins)
    assert sorted(k for k in margins if not k.endswith(".scale")) == sorted(own)
    for k, v in own.items():
        assert margins[k].shape == v.shape, k
    flips = check_flips({k: v.clone() for k, v in own.items()}, own, margins)
    assert all(n == 0 for n, _ in flips.values()), flips
    # one flip where the oracle's own pre-activations are closest to a tie: what two correct fp32 implementations may differ by
    rel_min = {k: float(margins[k].min()) / margins[k.rsplit(".", 1)[0] + ".scale"] for k in own}
    k_tie = min(rel_min, key=rel_min.get)
    assert rel_min[k_tie] < 1e-6, rel_min                # (else the shape is too small to hold a near-tie)
    dec = {k: v.clone() for k, v in own.items()}
    flat = dec[k_tie].view(-1)
    i = int(margins[k_tie].reshape(-1).argmin())
    flat[i] = ~flat[i]
    flips = check_flips(dec, own, margins)
    assert flips[k_tie][0] == 1 and flips[k_tie][1] == rel_min[k_tie]
    assert sum(n for n, _ in flips.values()) == 1

    def corrupted(k, fn):
        dec = {q: v.clone() for q, v in own.items()}
        dec[k] = fn(dec[k].clone())
        assert not torch.equal(dec[k], own[k]), k
        return dec

    def invert_word(v):                                  # channels 32 w .. 32 w + 31 of one (window, ECoG channel, t)
        v[1, 32:64, v.shape[2] // 2, 2] = ~v[1, 32:64, v.shape[2] // 2, 2]
        return v

    def zero_last_row_tile(v):                           # rows (window, ECoG channel, t) x channels, as the epilogue writes them
        B, ch, t, C = v.shape
        rows = v.permute(0, 3, 2, 1).reshape(B * C * t, ch).clone()
        rows[-128:] = False
        return rows.view(B, C, t, ch).permute(0, 3, 2, 1).contiguous()

    for k in own:
        for fn in (lambda v: torch.roll(v, 1, dims=1), invert_word, zero_last_row_tile):     # shifted, inverted, zero tile
            with pytest.raises(AssertionError, match=re.escape(k + ":")):
                check_flips(corrupted(k, fn), own, margins)


BAND_REF_CASES = [(400, [70., 150.], 5003), (500, [70., 150.], 1024), (512, [70., 150.], 2449), (1000, [70., 150.], 5003),
                  (2000, [70., 150.], 1024), (400, [30., 70.], 1025), (1000, [150., 300.], 1000), (400, [70., 199.], 7169),
                  (400, [1., 4.], 7170)]


def test_band_filter_references_are_pinned_to_extended_precision():
    """The references tests/test_gpu_band_filters.py holds the kernels to: the float64 Hilbert oracle within 1e-12 of the
    ``np.longdouble`` statement of the same function on zero-mean noise and on a DC level of 1000 standard deviations
    (observed 7.6e-16 and 6.7e-13; the deviation grows with the level, which is why the GPU test takes the longdouble
    statement itself at an offset), over nine (rate, range, length) cases that cover every row kind of its decision table;
    ``scipy.signal.lfilter`` per band and the oracle's FIR bank within 1e-14 of a longdouble ``np.convolve``."""
    from tests.signal_refs import band_cases, fir_bank_longdouble, hilbert_filter_longdouble, scipy_fir_bank
    assert np.finfo(np.longdouble).eps < 1e-18, "np.longdouble is not an extended format on this platform"

    def relq(a, b):
        return float(np.max(np.abs(a.astype(np.longdouble) - b)) / np.max(np.abs(b)))

    for off in (0.0, 1e3):
        worst = 0.0
        for fs, fr, T in BAND_REF_CASES:
            x = band_cases(np.random.default_rng(T), 4, T, offset=off)
            for env in (True, False):
                d = relq(sg.hilbert_filter(x, fs, fr, envelope=env), hilbert_filter_longdouble(x, fs, fr, envelope=env))
                assert d < 1e-12, (off, fs, fr, T, env, d)
                worst = max(worst, d)
        print(f"float64 Hilbert oracle vs longdouble, offset {off:g} sd: {worst:.2e}")
    x = band_cases(np.random.default_rng(1), 3, 700, offset=1e3)
    for order, cfs in ((64, [60., 120.]), (390, [100.])):
        taps = sg.fir_taps(400, order, cfs)
        ref = fir_bank_longdouble(x, taps)
        assert relq(scipy_fir_bank(x, taps), ref) < 1e-14
        assert relq(sg.fir_bandpass_filter(x, 400, order, cfs), ref) < 1e-14
