"""SynthesisLite (reference models/synthesis_models.py:201-296) against the float64 oracle OFF the golden geometry.

The golden tests (G2, G3, G9, graph vs eager) all run 32 channels x 200 samples, conv_channels 32, lstm_hidden 64, label_dim 2
and output 80, where every pool is even, F + H and out_dim are multiples of 4 and B <= 64: most branches of
``_lite_engine.py`` / ``csrc/tonal_lite.hip`` never meet a reference there.  Here each parametrised shape reaches some of them
(annotated per row), and the HIP path's output, every parameter gradient and the BatchNorm buffers are held to
``oracle.synthesis_oracle.lite_forward`` in float64: forward 2e-5 max-relative, gradients 1e-4 relative L2 - a 0.1 % error in
a kernel fails.  Observed deviations go to tests/parity_record.py.

Lite keeps no branch planes (tests/branch_planes.py does that for the CNN), so every seed below is one whose float64
pre-activations hold no near-tie, asserted on the CPU before the GPU is touched: each max-pool pair gap, each pooled
LeakyReLU input and each fc.1 pre-activation is at least ``TIE`` x max |z| of its layer, in train mode and in eval mode.
``TIE`` is 2.5e-7, four fp32 roundings of a layer's largest pre-activation.  A margin of 1e-4 x max |z| cannot be met: at
830 000 pool pairs (batch 513) hundreds sit closer than that for any seed, and the best of 400 seeds at that shape has its
nearest tie at 2.95e-7.  (A CPU fp32 run of the oracle, flipped near-ties included, stays within 4e-6 of float64 in every
gradient at these shapes, far inside the bounds.)
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import golden_inputs as gi
from tests.parity_record import record
from tests.test_gpu_parity import rel, rel_l2

pytestmark = pytest.mark.gpu

FWD_BOUND, GRAD_BOUND = 2e-5, 1e-4
ZERO_GRAD_BOUND = 1e-5                     # conv biases in front of BatchNorm: analytically zero gradient (as golden G3)
TIE = 2.5e-7

# (B, C, T, out_dim, conv_channels, lstm_hidden, label_dim, L), seed
SHAPES = [
    # B = 1; T = 203 and T/2 = 101: both pools drop a trailing sample (lite_bn_act_pool_bwd's odd tail); out_dim 7 (padded
    # dout, fc.3 weight gradient through a slab, its bias gradient by _colsum); conv_channels 16: generic conv loops
    ((1, 4, 203, 7, 16, 64, 2, 5), 0),
    # F + H = 1650 + 12 -> ldf 1664: fc.1 weight permute, slab copy and w1t; H = 12: generic LSTM loops; label_dim 1;
    # L = 1: W_hh's gradient is zero; T/2 = 101 odd; conv_channels 33: generic conv loops
    ((3, 5, 202, 80, 33, 12, 1, 1), 0),
    # B = 65: 128-row GEMM tiles; label_dim 8 (the limit); register-resident LSTM (H = 64)
    ((65, 32, 200, 80, 32, 64, 8, 6), 7),
    # B = 513: both fc bias gradients by _colsum; T = 101 odd
    ((513, 8, 101, 80, 32, 64, 2, 5), 215),
    # C * T = 51 200 floats: conv 1's weight gradient from global memory (use_lds = 0); hid * ldf = 512 * 3328 > 2^20
    # (fc.1 bias by _colsum); 4H = 512 > 256 gate rows per thread stride
    ((4, 128, 400, 80, 32, 128, 2, 5), 0),
    # C = 240: the largest the conv kernel's LDS tile admits; conv_channels 48: generic loops
    ((2, 240, 64, 80, 48, 64, 2, 5), 0),
]
DC_CASE = ((3, 5, 202, 80, 33, 12, 1, 1), 0, 20.0)          # x = 20 + randn: mean / std of conv 1's output up to ~27
DROPOUT_CASE = ((3, 5, 202, 80, 33, 12, 1, 1), 0)
ZERO_GRAD = ("ecog_conv.0.bias", "ecog_conv.4.bias")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch.device("cuda:0")


def _model(cfg, seed, dropout=0.0):
    from decode_tonal_langauge_amd.models.synthesis_models import SynthesisLite
    B, C, T, D, cc, H, ld, L = cfg
    torch.manual_seed(seed)
    return SynthesisLite(D, C, T, label_dim=ld, conv_channels=cc, lstm_hidden=H, dropout=dropout)


def _inputs(cfg, seed, dc=0.0):
    B, C, T, D, cc, H, ld, L = cfg
    g = torch.Generator().manual_seed(seed)
    x = dc + torch.randn(B, C, T, generator=g)
    return x, torch.randn(B, ld, L, generator=g), torch.randn(B, D, generator=g)


def _f64(model):
    p = {k: v.detach().cpu().double() for k, v in model.named_parameters()}
    b = {k: v.detach().cpu().clone() if v.dtype == torch.long else v.detach().cpu().double() for k, v in model.named_buffers()}
    return p, b


def nearest_ties(p, b, x, lab, training, mask=None, slope=0.01):
    """{layer: smallest margin / max |z|} of the float64 forward pass (running buffers ``b`` updated in training like
    ``lite_forward`` does): pool-pair gaps and pooled LeakyReLU inputs of both blocks, fc.1 pre-activations."""
    from oracle import synthesis_oracle as so
    out = {}

    def block(i, z, bn):
        n = so.batchnorm1d(z, p[f"ecog_conv.{bn}.weight"], p[f"ecog_conv.{bn}.bias"], b[f"ecog_conv.{bn}.running_mean"],
                           b[f"ecog_conv.{bn}.running_var"], training)
        m = n.shape[2] // 2
        a0, a1 = n[:, :, 0:2 * m:2], n[:, :, 1:2 * m:2]
        s = float(n.abs().max())
        out[f"block{i}.pool_gap"] = float((a1 - a0).abs().min()) / s
        out[f"block{i}.pooled_sign"] = float(torch.maximum(a0, a1).abs().min()) / s
        return F.max_pool1d(F.leaky_relu(n, slope), 2)

    with torch.no_grad():
        y = block(1, F.conv1d(x, p["ecog_conv.0.weight"], p["ecog_conv.0.bias"], padding=2), 1)
        y = block(2, F.conv1d(y, p["ecog_conv.4.weight"], p["ecog_conv.4.bias"], padding=1), 5)
        h = so.lstm_last_hidden(lab.permute(0, 2, 1), p["label_lstm.weight_ih_l0"], p["label_lstm.weight_hh_l0"],
                                p["label_lstm.bias_ih_l0"], p["label_lstm.bias_hh_l0"])
        f = torch.cat([y.flatten(1), h], -1)
        if mask is not None:
            f = f * mask
        a = f @ p["fc.1.weight"].t() + p["fc.1.bias"]
        out["fc1.sign"] = float(a.abs().min() / a.abs().max())
    return out


def _assert_no_ties(ties, what):
    assert min(ties.values()) >= TIE, (what, ties)


def _oracle(p, b, x, lab, tgt, training, mask=None):
    from oracle import synthesis_oracle as so
    leaves = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    out = so.lite_forward(leaves, b, x.double(), lab.double(), training=training, dropout_mask=mask)
    grads = torch.autograd.grad(((out - tgt.double()) ** 2).mean(), list(leaves.values()))
    return out.detach(), dict(zip(leaves, grads))


def _hip(model, x, lab, tgt, dev):
    model.zero_grad(set_to_none=True)
    out = model(x.to(dev), lab.to(dev))
    ((out - tgt.to(dev)) ** 2).mean().backward()
    return out.detach().cpu(), {k: q.grad.detach().cpu() for k, q in model.named_parameters()}


def _compare(out, grads, ref, ref_grads, section, training=True):
    zero = ZERO_GRAD if training else ()          # (in eval mode BatchNorm is affine and the conv biases get a gradient)
    obs = {"out": rel(out.numpy(), ref.numpy())}
    for k, g in grads.items():
        obs["grad." + k] = (float(g.abs().max()) if k in zero else rel_l2(g.numpy(), ref_grads[k].numpy()))
    record(section, obs)
    assert obs["out"] < FWD_BOUND, (section, obs)
    for k in grads:
        assert obs["grad." + k] < (ZERO_GRAD_BOUND if k in zero else GRAD_BOUND), (section, k, obs["grad." + k])
    return obs


def _train_and_eval(dev, cfg, seed, dc=0.0, label=""):
    model = _model(cfg, seed)
    x, lab, tgt = _inputs(cfg, seed, dc)
    p, b = _f64(model)
    b_train = {k: v.clone() for k, v in b.items()}
    # ---- no near-tie in the float64 pre-activations, train mode and eval mode (on the buffers one step leaves) ----
    _assert_no_ties(nearest_ties(p, b_train, x.double(), lab.double(), True), "train")
    _assert_no_ties(nearest_ties(p, b_train, x.double(), lab.double(), False), "eval")
    # ---- train mode, dropout 0 ----
    b_ref = {k: v.clone() for k, v in b.items()}
    ref, ref_grads = _oracle(p, b_ref, x, lab, tgt, True)
    model.to(dev).train()
    out, grads = _hip(model, x, lab, tgt, dev)
    _compare(out, grads, ref, ref_grads, f"Lite {cfg}{label} train mode vs float64 oracle")
    bufs = {k: v.detach().cpu() for k, v in model.named_buffers()}
    obs = {}
    for k, v in b_ref.items():
        if v.dtype == torch.long:
            assert int(bufs[k]) == 1, k                             # num_batches_tracked, exact (the oracle keeps no count)
        else:
            obs[k] = rel(bufs[k].numpy(), v.numpy())
    record(f"Lite {cfg}{label} BatchNorm buffers vs float64 oracle", obs)
    for k, v in obs.items():
        assert v < FWD_BOUND, (k, v)
    # ---- eval mode (running statistics; the eval branch of lite_bn_dz_kernel), gradients with grad enabled ----
    _p, b_eval = _f64(model)
    ref, ref_grads = _oracle(p, b_eval, x, lab, tgt, False)
    model.eval()
    out, grads = _hip(model, x, lab, tgt, dev)
    _compare(out, grads, ref, ref_grads, f"Lite {cfg}{label} eval mode vs float64 oracle", training=False)
    assert all(int(v) == 1 for k, v in model.named_buffers() if v.dtype == torch.long)    # eval does not count


@pytest.mark.parametrize("cfg,seed", SHAPES, ids=[str(s[0]) for s in SHAPES])
def test_lite_shapes_against_float64_oracle(dev, cfg, seed):
    _train_and_eval(dev, cfg, seed)


def test_lite_shapes_dc_offset_input(dev):
    """High-gamma envelopes are positive: with x = 20 + randn the BatchNorm statistics of conv 1 see mean / std up to ~27.
    The per-tile partials of lite_conv_fwd_kernel are centred on the tile mean (E[z^2] - m^2 from fp32 tile sums lost
    1.4e-5 of rstd here), so the same bounds hold."""
    cfg, seed, dc = DC_CASE
    _train_and_eval(dev, cfg, seed, dc=dc, label=f" x = {dc:g} + randn")


def test_lite_shapes_train_mode_dropout_mask(dev):
    """Dropout 0.3 (fc.0): the keep mask of lite_cat is read back through tl_lite_cat on all-ones inputs, checked (values,
    rate, zero padding columns F + H .. ldf) and fed to the oracle; output and every gradient agree, so lite_uncat applies
    the forward mask."""
    from decode_tonal_langauge_amd._lib import check, ptr
    cfg, seed = DROPOUT_CASE
    B, C, T, D, cc, H, ld, L = cfg
    model = _model(cfg, seed, dropout=0.3)
    x, lab, tgt = _inputs(cfg, seed)
    p, b = _f64(model)
    ties = nearest_ties(p, {k: v.clone() for k, v in b.items()}, x.double(), lab.double(), True)
    _assert_no_ties({k: v for k, v in ties.items() if k.startswith("block")}, "train, conv blocks")
    model.to(dev).train()
    out, grads = _hip(model, x, lab, tgt, dev)
    eng = model._engine
    assert eng._p_used == 0.3 and eng.ldf != eng.F + eng.H
    st = torch.cuda.current_stream().cuda_stream
    y2, hs = torch.ones(B, eng.F, device=dev), torch.ones(B, L, H, device=dev)
    feat = torch.full((B, eng.ldf), float("nan"), device=dev)
    check(eng.lib.tl_lite_cat(ptr(y2), ptr(hs), ptr(feat), B, eng.F, H, L, eng.ldf, 0.3, eng._seed, st), "tl_lite_cat")
    feat = feat.cpu()
    keep = float(np.float32(1) / (np.float32(1) - np.float32(0.3)))
    mask = feat[:, :eng.F + H]
    assert torch.unique(mask).tolist() == [0.0, keep]
    assert bool((feat[:, eng.F + H:] == 0).all())                  # padding columns of the fc.1 operand
    n = mask.numel()
    rate = float((mask > 0).double().mean())
    assert abs(rate - 0.7) < 4 * math.sqrt(0.7 * 0.3 / n), (rate, n)
    mask = mask.double()
    _assert_no_ties({k: v for k, v in nearest_ties(p, {k: v.clone() for k, v in b.items()}, x.double(), lab.double(), True,
                                                   mask=mask).items() if k.startswith("fc1")}, "train, fc.1 under the mask")
    ref, ref_grads = _oracle(p, {k: v.clone() for k, v in b.items()}, x, lab, tgt, True, mask=mask)
    _compare(out, grads, ref, ref_grads, f"Lite {cfg} dropout 0.3, HIP mask fed to the float64 oracle")


@pytest.mark.parametrize("graph", ["0", "1"])
def test_lite_trainer_steps_follow_float64_oracle(dev, graph, monkeypatch):
    """Five SynthesisTrainer steps (NAdam, L1 on integer-truncated targets) at the ldf != F + H geometry (label_dim 2: the
    trainer's tone dynamics) against ``oracle.train_step("lite")`` in float64: loss, MCD and the parameters after every
    step.  TONAL_GRAPH=1 captures the step after three eager ones, so steps 4 and 5 are graph replays."""
    from decode_tonal_langauge_amd.models.simple_classifiers import LogisticRegressionClassifier
    from decode_tonal_langauge_amd.models.synthesis_trainer import SynthesisTrainer
    from oracle import synthesis_oracle as so
    monkeypatch.setenv("TONAL_GRAPH", graph)
    B, C, T, D, cc, H = 3, 5, 202, 80, 33, 12
    model = _model((B, C, T, D, cc, H, 2, 5), 0)
    torch.manual_seed(1)
    tr = SynthesisTrainer(model, LogisticRegressionClassifier(8 * T, 4), LogisticRegressionClassifier(8 * T, 2), gi.TONE_MAP,
                          device=dev, verbose=False)
    assert model._engine.ldf != model._engine.F + H
    p, b = _f64(model)
    init = {k: v.clone() for k, v in p.items()}
    state = so.NAdamState(p)
    gen = torch.Generator().manual_seed(41)
    model.train()
    obs = {}
    for s in range(5):
        x, syl, tone = torch.randn(B, C, T, generator=gen), torch.randn(B, 8, T, generator=gen), torch.randn(B, 8, T, generator=gen)
        tgt = 10 * torch.randn(B, D, generator=gen)
        with torch.no_grad():
            lab = tr._labels(tone.to(dev), syl.to(dev)).cpu()
        tr.train_step(x, syl, tone, tgt)
        torch.cuda.synchronize()
        loss, mcd = so.train_step("lite", p, b, state, x.double(), lab.double(), tgt.double())
        stats = tr._stats.cpu().double().numpy()
        obs[f"step{s + 1}.loss"] = abs(stats[2] - loss) / loss
        obs[f"step{s + 1}.mcd"] = abs(stats[3] - mcd) / mcd
        for k, q in model.named_parameters():
            obs[f"step{s + 1}.upd.{k}"] = gi.update_rel_l2(q.detach().cpu().numpy(), p[k].numpy(), init[k].numpy())
        assert obs[f"step{s + 1}.loss"] < FWD_BOUND and obs[f"step{s + 1}.mcd"] < FWD_BOUND, (s, obs)
    captured = sum(1 for v in tr._graphs.values() if v["graph"] is not None)
    assert captured == (1 if graph == "1" else 0)
    record(f"Lite trainer, 5 steps at {(B, C, T, D, cc, H)} vs float64 oracle (TONAL_GRAPH={graph})", obs)
    # NAdam divides each update by the root of its own second moment, which amplifies the gradient's deviation where single
    # entries are near zero: observed at most 9.8e-5 of the whole update vector (BatchNorm weights, step 1); 5e-4 allowed
    for k, v in obs.items():
        if ".upd." in k:
            assert v < 5e-4, (k, v)


def test_lite_trainer_holds_at_most_two_captured_shapes(dev, monkeypatch):
    """15 ``train_step``s with batch sizes cycling 5, 3, 2: the first two shapes are captured after their three eager steps, the
    third stays eager while two graphs are held - and the run leaves the bits of the same run with TONAL_GRAPH=0."""
    from decode_tonal_langauge_amd.models.simple_classifiers import LogisticRegressionClassifier
    from decode_tonal_langauge_amd.models.synthesis_models import SynthesisLite
    from decode_tonal_langauge_amd.models.synthesis_trainer import SynthesisTrainer
    C, T, D = 4, 64, 80
    gen = torch.Generator().manual_seed(29)
    data = [(torch.randn(B, C, T, generator=gen), torch.randn(B, 8, T, generator=gen), torch.randn(B, 8, T, generator=gen),
             10 * torch.randn(B, D, generator=gen)) for B in (5, 3, 2) * 5]
    res = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("TONAL_GRAPH", mode)
        torch.manual_seed(0)
        model = SynthesisLite(D, C, T, dropout=0.3)
        torch.manual_seed(1)
        tr = SynthesisTrainer(model, LogisticRegressionClassifier(8 * T, 4), LogisticRegressionClassifier(8 * T, 2), gi.TONE_MAP,
                              device=dev, verbose=False)
        model.train()
        for b in data:
            tr.train_step(*b)
        torch.cuda.synchronize()
        held = sorted(k[0][0] for k, v in tr._graphs.items() if v["graph"] is not None)
        assert held == ([3, 5] if mode == "1" else []), held
        res[mode] = ({k: v.detach().clone() for k, v in model.state_dict().items()}, tr._stats.clone(), tr._last_out.clone())
    assert set(res["1"][0]) == set(dict(model.named_parameters())) | set(dict(model.named_buffers()))
    for k, v in res["1"][0].items():
        assert torch.equal(v, res["0"][0][k]), k
    assert torch.equal(res["1"][1], res["0"][1]) and torch.equal(res["1"][2], res["0"][2])


@pytest.mark.parametrize("kw,match", [
    (dict(n_channels=241), "240 ECoG channels"),
    (dict(lstm_hidden=6), "multiple of 4"),
    (dict(label_dim=9), "label_dim"),
])
def test_lite_rejects_sizes_the_kernels_do_not_take(dev, kw, match):
    """Sizes the engine does not take raise a ValueError from the constructor, before any kernel is launched."""
    from decode_tonal_langauge_amd.models.synthesis_models import SynthesisLite
    args = dict(output_dim=80, n_channels=8, n_timepoints=100)
    args.update(kw)
    with pytest.raises(ValueError, match=match):
        SynthesisLite(**args)
