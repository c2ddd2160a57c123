"""GPU: training ``CNNRNNClassifier`` on the HIP path - ``tl_lstm_train_seq`` / ``tl_lstm_bptt_seq``, ``tl_pool3_fwd`` /
``tl_pool3_bwd``, ``tl_conv1_dgrad``, ``CnnRnnClassifierTrainEngine``, ``ClassifierTrainer(fused=True)`` and the pipeline key.

How the bounds are formed.  The reference of every comparison is torch on the CPU in float64.
  * the LSTM kernels, ``tl_conv1_dgrad`` and the optimiser routing: 10 yardsticks (``classifier_train_ref.FACTOR``), a yardstick
    being the distance (``rel_l2``) of the float32 CPU evaluation of the same thing from the float64 one, computed in the test,
    with a floor of 1e-6;
  * the pool kernels: exact - the pool is a selection and the dropout scale one rounding;
  * one step's gradients: the planes HIP took are first held to the float64 reference's own decisions by
    ``branch_planes.check_flips`` (tau 1e-4, max_frac 1e-4, slack 4), then every parameter gradient is within 5e-5 relative L2 of
    the float64 restatement run on HIP's planes and keep mask, scores within 2e-5 absolute, the loss sum within 2 B 2e-5 - the
    bounds tests/test_gpu_cnn_classifier_train.py holds the same kernels to.
Integer results are compared exactly.  Every figure is printed and recorded before it is asserted."""
import copy
import functools
import os

import pytest
import torch
import torch.nn.functional as F

from tests import branch_planes, parity_record
from tests import classifier_train_ref as ref
from tests import cnnrnn_classifier_ref as rref

pytestmark = pytest.mark.gpu
DEV = "cuda"
FLOOR = 1e-6
_REC = {}


def _note(section, values):
    _REC.setdefault(section, {}).update(values)
    parity_record.record("cnnrnn_classifier_train_" + section, _REC[section])


def _held(section, name, dev, yard):
    """Print and record one figure; returns whether it is within 10 yardsticks (a yardstick is at least 1e-6)."""
    bound = ref.FACTOR * max(yard, FLOOR)
    print(f"[{section}] {name}: gpu {dev:.3e}  yardstick {yard:.3e}  bound {bound:.3e}")
    _note(section, {name + "_gpu": dev, name + "_bound": bound})
    return dev <= bound


def _within(section, name, dev, bound):
    print(f"[{section}] {name}: gpu {dev:.3e}  bound {bound:.3e}")
    _note(section, {name: dev})
    return dev <= bound


def _lib():
    from decode_tonal_langauge_amd import _lib as L
    return L, L.load(), torch.cuda.current_stream().cuda_stream


# ---------------------------------------------------------------------------------------------- 1. the LSTM kernels alone
def _lstm_reference(lstm, x, dh_last, dtype):
    m = copy.deepcopy(lstm).to(dtype)
    xin = x.to(dtype).requires_grad_(True)
    h = m(xin)[0][:, -1]
    h.backward(dh_last.to(dtype))
    return h.detach(), {k: v.grad.detach() for k, v in m.named_parameters()}, xin.grad.detach()


def _run_lstm_kernels(lstm, x, dh_last):
    """Forward and BPTT of ``lstm`` over x (B, T, in) on the two kernels; (hs, dgates, dgT, x rows) as padded device tensors."""
    L, lib, st = _lib()
    B, T, D = x.shape
    H = lstm.hidden_size
    Hp, Kp = (H + 7) // 8 * 8, (D + 3) // 4 * 4
    f32 = dict(dtype=torch.float32, device=DEV)
    w_ih, w_hh = lstm.weight_ih_l0.detach().to(DEV), lstm.weight_hh_l0.detach().to(DEV)
    wi = torch.zeros(4, Hp, Kp, **f32)
    wi[:, :H, :D] = w_ih.view(4, H, D)
    wh = torch.zeros(4, Hp, Hp, **f32)
    wh[:, :H, :H] = w_hh.view(4, H, H)
    bs = torch.zeros(4, Hp, **f32)
    bs[:, :H] = (lstm.bias_ih_l0 + lstm.bias_hh_l0).detach().to(DEV).view(4, H)
    whp = wh.permute(1, 0, 2).contiguous().view(4 * Hp, Hp)                    # unit-major: row 4 u + g
    whT = wh.view(4 * Hp, Hp).t().contiguous()                                 # (Hp, 4 Hp)
    xr = torch.zeros(T * B, Kp, **f32)
    xr[:, :D] = x.to(DEV).permute(1, 0, 2).reshape(T * B, D)                   # rows time-major
    xp = (xr @ wi.view(4 * Hp, Kp).t() + bs.view(-1)).contiguous()
    nan = lambda *s: torch.full(s, float("nan"), **f32)
    hs, cs, act, dg, dc = nan(T * B, Hp), nan(T * B, Hp), nan(T * B, 4 * Hp), nan(T * B, 4 * Hp), nan(B, Hp)
    ldt = (T * B + 31) // 32 * 32
    dgT = torch.zeros(4 * Hp, ldt, **f32)
    dh = torch.zeros(B, Hp, **f32)
    dh[:, :H] = dh_last.to(DEV)
    L.check(lib.tl_lstm_train_seq(xp.data_ptr(), 4 * Hp, B * 4 * Hp, whp.data_ptr(), hs.data_ptr(), cs.data_ptr(), act.data_ptr(),
                                  B, Hp, T, st), "tl_lstm_train_seq")
    L.check(lib.tl_lstm_bptt_seq(whT.data_ptr(), dh.data_ptr(), act.data_ptr(), cs.data_ptr(), dc.data_ptr(), dg.data_ptr(),
                                 dgT.data_ptr(), ldt, B, Hp, T, st), "tl_lstm_bptt_seq")
    torch.cuda.synchronize()
    return hs, cs, dg, dgT, xr, wi


@pytest.mark.parametrize("B,T,D,H", [(2, 1, 4, 16), (3, 5, 4, 8), (33, 7, 6, 100), (65, 3, 12, 48)])
def test_lstm_kernels_match_float64_autograd(B, T, D, H):
    torch.manual_seed(100 * B + T)
    lstm = torch.nn.LSTM(D, H, batch_first=True)
    x, dh_last = torch.randn(B, T, D), torch.randn(B, H)
    h64, g64, dx64 = _lstm_reference(lstm, x, dh_last, torch.float64)
    h32, g32, dx32 = _lstm_reference(lstm, x, dh_last, torch.float32)
    hs, cs, dg, dgT, xr, wi = _run_lstm_kernels(lstm, x, dh_last)
    Hp, Kp = hs.shape[1], xr.shape[1]
    # the gradients the engine forms from the kept arrays with its GEMMs, here in float64 on the host
    d = dg.double().cpu().view(T, B, 4, Hp)
    hsd = hs.double().cpu().view(T, B, Hp)
    xrd = xr.double().cpu().view(T, B, Kp)
    rows = d.reshape(T * B, 4 * Hp)
    dW_ih = (rows.t() @ xrd.reshape(T * B, Kp)).view(4, Hp, Kp)[:, :H, :D].reshape(4 * H, D)
    dW_hh = (d[1:].reshape(-1, 4 * Hp).t() @ hsd[:-1].reshape(-1, Hp)).view(4, Hp, Hp)[:, :H, :H].reshape(4 * H, H)
    db = rows.sum(0).view(4, Hp)[:, :H].reshape(-1)
    dx = (rows @ wi.double().cpu().view(4 * Hp, Kp)).view(T, B, Kp)[:, :, :D].permute(1, 0, 2)
    tag = f"B{B}T{T}D{D}H{H}"
    ok = [_held("lstm", tag + "_h_last", ref.rel_l2(hsd[T - 1][:, :H], h64), ref.rel_l2(h32, h64)),
          _held("lstm", tag + "_dW_ih", ref.rel_l2(dW_ih, g64["weight_ih_l0"]), ref.rel_l2(g32["weight_ih_l0"], g64["weight_ih_l0"])),
          _held("lstm", tag + "_db", ref.rel_l2(db, g64["bias_ih_l0"]), ref.rel_l2(g32["bias_ih_l0"], g64["bias_ih_l0"])),
          _held("lstm", tag + "_dx", ref.rel_l2(dx, dx64), ref.rel_l2(dx32, dx64))]
    if T > 1:
        ok.append(_held("lstm", tag + "_dW_hh", ref.rel_l2(dW_hh, g64["weight_hh_l0"]),
                        ref.rel_l2(g32["weight_hh_l0"], g64["weight_hh_l0"])))
    assert all(ok), tag
    # pad units and pad columns: exactly zero (dh_last's pad columns were zero)
    assert bool((hs[:, H:] == 0).all()) and bool((cs[:, H:] == 0).all())
    assert bool((dg.view(T * B, 4, Hp)[:, :, H:] == 0).all())
    assert not bool(torch.isnan(hs).any() | torch.isnan(dg).any())
    assert torch.equal(dgT[:, :T * B], dg.t()) and bool((dgT[:, T * B:] == 0).all())       # the transposed copy, same bits
    again = _run_lstm_kernels(lstm, x, dh_last)                                              # a second run: the same bits
    assert torch.equal(again[0], hs) and torch.equal(again[2], dg) and torch.equal(again[3], dgT)


# ---------------------------------------------------------------------------------------------- 2. the (3,1) pool + dropout
def _seq_to_cat(t, B, w1, Cn):
    """(B * W, ...) branch-major sequences -> (B, W, ...) in torch.cat((x1, x), dim=3) order"""
    nb = B * w1
    return torch.cat((t[:nb].reshape(B, w1, *t.shape[1:]), t[nb:].reshape(B, Cn, *t.shape[1:])), dim=1)


def _cat_to_seq(t, B, w1, Cn):
    return torch.cat((t[:, :w1].reshape(B * w1, *t.shape[2:]), t[:, w1:].reshape(B * Cn, *t.shape[2:])), dim=0)


@pytest.mark.parametrize("p", [0.0, 0.5, 0.3])
@pytest.mark.parametrize("time_major", [False, True])
@pytest.mark.parametrize("B,w1,Cn,Tp,tq,slope", [(2, 2, 3, 12, 3, 0.0), (3, 1, 2, 16, 5, 0.01)])
def test_pool3_kernels_equal_torch_exactly(B, w1, Cn, Tp, tq, slope, time_major, p):
    L, lib, st = _lib()
    Cc, W, S = 256, w1 + Cn, B * (w1 + Cn)
    g = torch.Generator().manual_seed(7 * B + tq)
    if p == 0.0:       # distinct integers: the index map shows in every element
        Y = torch.randperm(S * Tp * Cc, generator=g).float().view(S * Tp, Cc) - 1000.0
    else:
        Y = torch.randn(S * Tp, Cc, generator=g)
    Yv = Y.view(S, Tp, Cc)
    Yv[0, 0:3, 5] = 0.75                                   # a triple of equal values: the first wins
    Yv[1, 3:6, 9] = torch.tensor([-3.0, -1.0, -2.0])       # an all-negative triple
    Yv[S - 1, 3 * tq - 3:3 * tq, 255] = torch.tensor([1.0, 2.0, 2.0])
    seed = 0x1234567 + tq
    rs_b, rs_t = (1, B) if time_major else (tq, 1)
    Yd = Y.to(DEV)
    X = torch.full((B * tq, Cc * W), float("nan"), device=DEV)
    L.check(lib.tl_pool3_fwd(Yd.data_ptr(), X.data_ptr(), B, w1, Cn, Cc, Tp, tq, Cc, rs_b, rs_t, p, seed, st), "tl_pool3_fwd")
    # torch: max_pool2d over the time axis of (S, 256, 3 tq, 1), the keep mask of tl_dropout_scale, one rounding for the scale
    tri = Yv[:, :3 * tq].permute(0, 2, 1).unsqueeze(-1)
    pooled, idx = F.max_pool2d(tri, (3, 1), return_indices=True)
    pooled, arg = pooled.squeeze(-1).permute(0, 2, 1), (idx.squeeze(-1) % 3).permute(0, 2, 1)          # (S, tq, 256)
    keep = torch.ones(S, tq, Cc, device=DEV)
    if p > 0:
        L.check(lib.tl_dropout_scale(keep.data_ptr(), keep.numel(), p, seed, st), "tl_dropout_scale")
    keep = (keep != 0).cpu()
    inv = torch.tensor(1.0, dtype=torch.float32) / (torch.tensor(1.0, dtype=torch.float32) - torch.tensor(p, dtype=torch.float32))
    want_seq = torch.where(keep, pooled * inv, torch.zeros(())) if p > 0 else pooled
    as_x = lambda t: _seq_to_cat(t, B, w1, Cn).permute(0, 3, 2, 1).contiguous().view(B, tq, -1)         # (B, 256, tq, W) raw view
    from_x = lambda t: _cat_to_seq(t.reshape(B, Cc, tq, W).permute(0, 3, 2, 1), B, w1, Cn)
    want = as_x(want_seq)
    got = X.cpu().view(tq, B, -1).permute(1, 0, 2) if time_major else X.cpu().view(B, tq, -1)
    assert not bool(torch.isnan(got).any())
    assert torch.equal(got, want)
    assert int(arg[0, 0, 5]) == 0 and float(pooled[1, 1, 9]) == -1.0 and int(arg[S - 1, tq - 1, 255]) == 1
    if p > 0:
        frac = float(keep.float().mean())
        assert abs(frac - (1 - p)) < 0.02, frac
    # backward: the gradient lands in the arg-max row only, at the pre-activation; everything else is zero
    dXc = torch.randn(B, tq, Cc * W, generator=g)
    dXd = (dXc.permute(1, 0, 2) if time_major else dXc).contiguous().to(DEV)
    dZ = torch.full((S * Tp, Cc), float("nan"), device=DEV)
    L.check(lib.tl_pool3_bwd(Yd.data_ptr(), dXd.data_ptr(), dZ.data_ptr(), B, w1, Cn, Cc, Tp, tq, Cc, Cc, rs_b, rs_t, p, seed,
                             slope, st), "tl_pool3_bwd")
    torch.cuda.synchronize()
    d = from_x(dXc)                                                                                     # (S, tq, 256)
    if p > 0:
        d = torch.where(keep, d * inv, torch.zeros(()))
    d = d * torch.where(pooled > 0, torch.tensor(1.0), torch.tensor(slope))
    want_dz = torch.zeros(S, Tp, Cc)
    want_dz[:, :3 * tq].view(S, tq, 3, Cc).scatter_(2, arg.unsqueeze(2), d.unsqueeze(2))
    got_dz = dZ.cpu().view(S, Tp, Cc)
    assert torch.equal(got_dz, want_dz)
    assert bool((got_dz[:, 3 * tq:] == 0).all())
    assert float(got_dz[1, 3:6, 9].abs().sum()) == (0.0 if slope == 0.0 else float(got_dz[1, 4, 9].abs()))


# ---------------------------------------------------------------------------------------------- 3. tl_conv1_dgrad
@pytest.mark.parametrize("S,T,n_inner", [(3, 20, 3), (5, 33, 1)])
def test_conv1_dgrad_matches_float64_conv_transpose(S, T, n_inner):
    L, lib, st = _lib()
    k, C1 = 7, 1024
    tout = (T - k + 1) // 2
    Tp = (tout + 3) // 4 * 4 + 4                                # pad rows behind every sequence (random: they must be ignored)
    g = torch.Generator().manual_seed(S * T)
    G = torch.randn(S * Tp, C1, generator=g)
    bits = torch.randint(-2 ** 31, 2 ** 31 - 1, (S * Tp, C1 // 32), generator=g, dtype=torch.int64).to(torch.int32)
    w = torch.randn(C1, k, generator=g)
    sh = torch.arange(32, dtype=torch.int32)
    odd = ((bits.view(S, Tp, -1, 1) >> sh) & 1).bool().reshape(S, Tp, C1)[:, :tout]                       # (S, tout, C1)

    def reference(dtype):
        Gv = G.to(dtype).view(S, Tp, C1)[:, :tout]
        dz = torch.zeros(S, tout, 2, C1, dtype=dtype)
        dz[:, :, 0] = torch.where(odd, torch.zeros((), dtype=dtype), Gv)
        dz[:, :, 1] = torch.where(odd, Gv, torch.zeros((), dtype=dtype))
        dz = dz.reshape(S, 2 * tout, C1).permute(0, 2, 1)                                                 # un-pooled (S, C1, 2 tout)
        dx = F.conv_transpose1d(dz, w.to(dtype).view(C1, 1, k))                                           # (S, 1, 2 tout + 6)
        return F.pad(dx[:, 0], (0, T - dx.shape[2]))
    want, want32 = reference(torch.float64), reference(torch.float32)
    n_outer = S // n_inner
    out = torch.full((n_outer, T * n_inner + 4), float("nan"), device=DEV)                                # row stride above T n_inner
    Gd, bd, wd = G.to(DEV), bits.to(DEV), w.to(DEV)
    L.check(lib.tl_conv1_dgrad(Gd.data_ptr(), bd.data_ptr(), wd.data_ptr(), out.data_ptr(), S, T, k, C1, Tp, tout, n_inner,
                               out.stride(0), n_inner, 1, st), "tl_conv1_dgrad")
    torch.cuda.synchronize()
    got = out[:, :T * n_inner].cpu().contiguous().view(n_outer, T, n_inner).permute(0, 2, 1).reshape(S, T)
    assert bool(torch.isnan(out[:, T * n_inner:]).all()) and not bool(torch.isnan(got).any())
    tag = f"S{S}T{T}"
    assert _held("conv1_dgrad", tag, ref.rel_l2(got, want), ref.rel_l2(want32, want)), tag
    assert bool((got[:, 2 * tout + k - 1:] == 0).all())
    out2 = torch.zeros_like(out)
    L.check(lib.tl_conv1_dgrad(Gd.data_ptr(), bd.data_ptr(), wd.data_ptr(), out2.data_ptr(), S, T, k, C1, Tp, tout, n_inner,
                               out.stride(0), n_inner, 1, st), "tl_conv1_dgrad")
    torch.cuda.synchronize()
    assert torch.equal(out2[:, :T * n_inner], out[:, :T * n_inner])                                       # the same bits


# ---------------------------------------------------------------------------------------------- the engine
def _engine(model, lr=0.0005, wd=0.0):
    from decode_tonal_langauge_amd._cnnrnn_classifier_train_engine import CnnRnnClassifierTrainEngine
    return CnnRnnClassifierTrainEngine(copy.deepcopy(model).to(DEV), lr, wd)


@functools.lru_cache(maxsize=None)
def _own64(shape, seed):
    """The float64 reference's own decisions and their margins.  Every plane is decided in front of the dropout, so HIP's keep
    mask does not move them: computed once per shape."""
    model, x, _ = rref.build(shape, seed)
    own, margins = {}, {}
    with torch.no_grad():
        rref.forward(model, rref.leaves(model, torch.float64), x, own=own, margins=margins)
    return own, margins


def _one_step(shape, seed, dropout, conv7, monkeypatch):
    if conv7 is not None:
        monkeypatch.setenv("TONAL_KERNELS", f"conv7={conv7}")
    B = shape[0]
    model, x, y = rref.build(shape, seed, dropout)
    eng = _engine(model)
    eng.model.train()
    got = {k: g.detach().clone().cpu() for k, g in eng.backward_only(x.to(DEV), y.to(DEV)).items()}
    torch.cuda.synchronize()
    scores = eng.scores(B).cpu()
    planes = rref.hip_planes(eng, B)
    keep = rref.hip_keep_mask(eng, B)
    assert (keep is not None) == (dropout > 0)
    if keep is not None:
        frac = float(keep.float().mean())
        assert abs(frac - (1 - dropout)) < 0.05, frac
    loss_sum, count, _ = eng.epoch_stats()
    assert count == B
    own, margins = _own64(shape, seed)
    tag = "B{}C{}T{}L{}n{}".format(*shape) + f"_p{dropout}_{conv7 or eng.conv7_form}"
    flips = branch_planes.check_flips(planes, own, margins)
    assert set(flips) == set(own) == set(rref.PLANES) and len(flips) == 7
    _note("flips", {f"{tag}.{k}": v for k, v in branch_planes.flip_record(flips).items()})
    print(f"[flips] {tag}: {sum(v[0] for v in flips.values())} branches differ")
    s64, loss64, g64 = rref.loss_and_grads(model, rref.leaves(model, torch.float64), x, y, planes=planes, keep=keep)
    assert set(got) == set(g64) and len(got) == 18
    ok = [_within("gradients", f"{tag}.{k}", ref.rel_l2(got[k], g64[k]), 5e-5) for k in sorted(g64)]
    ok.append(_within("gradients", f"{tag}.scores_abs", float((scores.double() - s64).abs().max()), 2e-5))
    ok.append(_within("gradients", f"{tag}.loss_sum_abs", abs(loss_sum - float(loss64) * B), 2 * B * 2e-5))
    assert all(ok), tag
    for name in ("lstm1", "lstm2"):
        assert torch.equal(got[name + ".bias_ih_l0"], got[name + ".bias_hh_l0"])


# ---------------------------------------------------------------------------------------------- 4. one step's gradients
@pytest.mark.parametrize("conv7", ["wino63", "direct"])
@pytest.mark.parametrize("dropout", [0.0, 0.5])
@pytest.mark.parametrize("shape,seed", rref.SHAPES[:3])
def test_one_step_gradients_on_shared_branches(shape, seed, dropout, conv7, monkeypatch):
    _one_step(shape, seed, dropout, conv7, monkeypatch)


def test_one_step_gradients_with_a_partial_second_row_block(monkeypatch):
    _one_step(*rref.SHAPES[3], 0.0, None, monkeypatch)


# ---------------------------------------------------------------------------------------------- 5. the update
def _nadam_twin(named, lr, wd, dtype):
    params = {k: v.detach().cpu().to(dtype).clone().requires_grad_(True) for k, v in named}
    decay = [p for p in params.values() if p.ndim >= 2]
    rest = [p for p in params.values() if p.ndim < 2]
    opt = torch.optim.NAdam([{"params": decay, "weight_decay": wd}, {"params": rest, "weight_decay": 0.0}], lr=lr)
    return params, opt


def test_update_follows_nadam_and_statistics_count():
    lr, wd = 5e-3, 0.01
    shape, seed = rref.SHAPES[0]
    B, n = shape[0], shape[4]
    model, _, _ = rref.build(shape, seed)
    eng = _engine(model, lr, wd)
    eng.model.train()
    assert [g["weight_decay"] for g in eng.optimizer.param_groups] == [wd, 0.0]
    g = torch.Generator().manual_seed(31)
    named = list(eng.model.named_parameters())
    p64, opt64 = _nadam_twin(named, lr, wd, torch.float64)
    p32, opt32 = _nadam_twin(named, lr, wd, torch.float32)
    ok, labels, preds = [], [], []
    for step in range(3):
        x, y = torch.randn(B, shape[1], shape[2], generator=g), torch.randint(0, n, (B,), generator=g)
        before = {k: v.detach().cpu().clone() for k, v in named}
        eng.train_batch(x.to(DEV), y.to(DEV))
        torch.cuda.synchronize()
        grads = {k: v.detach().clone().cpu() for k, v in eng.step_gradients().items()}
        assert set(grads) == set(p64)
        for name in ("lstm1", "lstm2"):
            assert torch.equal(grads[name + ".bias_ih_l0"], grads[name + ".bias_hh_l0"])
        labels.append(y)
        preds.append(eng.scores(B).argmax(1).cpu())
        for params, opt, dt in ((p64, opt64, torch.float64), (p32, opt32, torch.float32)):
            for k, p in params.items():
                # both twins start the step from the parameters the GPU had: the step's update alone is compared
                p.data.copy_(before[k].to(dt))
                p.grad = grads[k].to(dt)
            opt.step()
        for k, v in named:
            want = p64[k].detach() - before[k].double()
            yard = ref.rel_l2(p32[k].detach() - before[k], want)
            ok.append(_held("update", f"step{step}_{k}", ref.rel_l2(v.detach().cpu() - before[k], want), yard))
    assert all(ok)
    loss_sum, count, cm = eng.epoch_stats()
    y_all, p_all = torch.cat(labels), torch.cat(preds)
    assert count == 3 * B and torch.equal(cm, torch.bincount(y_all * n + p_all, minlength=n * n).reshape(n, n))
    assert loss_sum > 0 and eng.epoch_stats()[1] == 0                                      # reading zeroes the statistics
    bad = y.clone()
    bad[0] = n
    eng.eval_batch(x.to(DEV), bad.to(DEV))
    with pytest.raises(ValueError, match=rf"\[0, {n}\)"):
        eng.epoch_stats()


# ---------------------------------------------------------------------------------------------- 6. host independence, packs, mask
def test_train_and_eval_batch_never_read_the_device():
    shape, seed = rref.SHAPES[0]
    B = shape[0]
    model, x, y = rref.build(shape, seed)
    eng = _engine(model, 0.001, 0.01)
    eng.model.train()
    x, y = x.to(DEV), y.float().to(DEV)
    eng.train_batch(x, y)                          # first call: workspaces, optimizer state and its pointer table
    eng.eval_batch(x, y)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        eng.train_batch(x, y)
        eng.eval_batch(x, y)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert eng.epoch_stats()[1] == 4 * B


def test_inference_after_fused_training_uses_the_updated_weights():
    shape, seed = rref.SHAPES[0]
    model, x, y = rref.build(shape, seed)
    eng = _engine(model, 5e-3, 0.01)
    gpu = eng.model
    xd = x.to(DEV)
    gpu.eval()
    with torch.no_grad():
        stale = gpu(xd).cpu()                           # the inference engines pack (and cache) the weights as they are now
    gpu.train()
    for _ in range(2):
        eng.train_batch(xd, y.to(DEV))
    gpu.eval()
    with torch.no_grad():
        s = gpu(xd).cpu()
        want = rref.forward(gpu, rref.leaves(gpu, torch.float64), x)
    pred = eng.predict_batch(xd).cpu()
    own = eng.scores(shape[0]).cpu()
    moved = float((stale.double() - want).abs().max())
    dev = float((s.double() - want).abs().max())
    print(f"[stale_packs] scores moved by {moved:.3e} in two steps; model(x) is {dev:.3e} from the updated float64 scores")
    _note("stale_packs", {"moved": moved, "dev": dev})
    assert moved > 2e-4                                 # the counter-example: stale packs would sit this far away
    assert dev <= 2e-5
    assert float((own.double() - want).abs().max()) <= 2e-5
    assert torch.equal(pred, own.argmax(1))


def test_train_mode_forward_of_the_module_draws_the_engines_mask():
    """The module's train-mode HIP forward with the engine's seed gives the engine's scores: both run the same arithmetic on
    the same mask (a score is in (0, 1): 1e-6 is eight float32 steps at 1; another mask moves a score by 1e-3 and more)."""
    shape, seed = rref.SHAPES[1]
    B = shape[0]
    model, x, y = rref.build(shape, seed, 0.5)
    eng = _engine(model)
    gpu = eng.model.train()
    xd = x.to(DEV)
    eng.backward_only(xd, y.to(DEV))
    mine = eng.scores(B).clone()
    assert eng.last_seed != 0
    gpu._drop_calls -= 1                                # the module draws its next seed from the call count: rewind one call
    with torch.no_grad():
        theirs = gpu(xd)
    assert gpu._last_seed == eng.last_seed
    dev = float((mine - theirs).abs().max())
    with torch.no_grad():
        other = gpu(xd)                                 # the next seed: another mask
    moved = float((other - theirs).abs().max())
    print(f"[same_mask] engine against module {dev:.3e}; another mask moves the scores by {moved:.3e}")
    _note("same_mask", {"dev": dev, "moved": moved})
    assert dev <= 1e-6 and moved > 1e-4


# ---------------------------------------------------------------------------------------------- 7. trainer and pipeline
def test_fused_trainer_fits_a_cnnrnn_classifier(tmp_path):
    from decode_tonal_langauge_amd._cnnrnn_classifier_train_engine import CnnRnnClassifierTrainEngine
    from decode_tonal_langauge_amd.models.classifier_trainer import ClassifierTrainer
    from decode_tonal_langauge_amd.models.deep_classifiers import CNNRNNClassifier
    from decode_tonal_langauge_amd.optim import FusedNAdam
    x, y = ref.planted(24, n_cls=2, channels=2, length=60)
    x[y == 1] += 1.0                                    # separable: class 1 is lifted as a whole
    dev = lambda a, b: ref.batches(a.to(DEV), b.to(DEV), 8)
    torch.manual_seed(3)
    gpu_model = CNNRNNClassifier(2, 60, 2, lstm_dim=60, dropout=0.0).to(DEV)
    tr = ClassifierTrainer(gpu_model, 0.002, 0.01, log_dir=str(tmp_path), fused=True)
    assert isinstance(tr.engine, CnnRnnClassifierTrainEngine) and isinstance(tr.optimizer, FusedNAdam)
    assert [g["weight_decay"] for g in tr.optimizer.param_groups] == [0.01, 0.0]
    hist = tr.fit(dev(x, y), dev(x, y), max_epochs=2, patience=99)
    assert len(hist) == 2
    assert all(torch.isfinite(torch.tensor(float(v))) for row in hist for v in row.values())
    print(f"[trainer] train loss {hist[0]['train/loss_epoch']:.5f} -> {hist[1]['train/loss_epoch']:.5f}, "
          f"val loss {hist[0]['val/loss']:.5f} -> {hist[1]['val/loss']:.5f}")
    assert hist[1]["train/loss_epoch"] < hist[0]["train/loss_epoch"] and hist[1]["val/loss"] < hist[0]["val/loss"]
    assert os.path.isfile(tmp_path / "metrics.csv")
    res = tr.test(dev(x, y))
    assert int(res["confusion_matrix"].sum()) == 24
    pred = tr.predict(dev(x, y))
    with torch.no_grad():
        own = torch.cat([gpu_model.eval()(a).argmax(1) for a, _ in dev(x, y)])
    assert torch.equal(pred, own)


def test_pipeline_key_reaches_the_cnnrnn_classifier(tmp_path, monkeypatch):
    import pandas as pd
    from decode_tonal_langauge_amd import _cnnrnn_classifier_train_engine as cte
    from decode_tonal_langauge_amd import train_classifier
    from decode_tonal_langauge_amd.data_loading import synthetic
    written = synthetic.write_dataset(str(tmp_path / "data"), n_samples=48, n_channels=4, n_timepoints=60)
    calls = []
    step = cte.CnnRnnClassifierTrainEngine.train_batch
    monkeypatch.setattr(cte.CnnRnnClassifierTrainEngine, "train_batch",
                        lambda self, x, y: (calls.append(len(y)), step(self, x, y))[1])
    config = {
        "model": {"model": "models.deep_classifiers.CNNRNNClassifier", "model_name": "cnnrnn", "model_kwargs": {"lstm_dim": 60}},
        "dataset": {"class_labels": {"tone": None}},
        "training": {"module": "train_classifier", "params": {
            "fused": True,
            "io": {"log_dir": str(tmp_path / "logs"), "sample_dir": written["sample_dir"],
                   "channel_selection_dir": written["channel_selection_dir"]},
            "experiment": {"targets": ["tone"], "features": "ecog", "separate_models": False, "seed": 1, "repeat": 1,
                           "verbose": 0, "device": DEV},
            "training": {"train_ratio": 0.75, "vali_ratio": 0.125, "test_ratio": 0.125, "batch_size": 16, "epochs": 2,
                         "lr": 0.005, "patience": 5, "weight_decay": 0.01, "log_every_n_steps": 10}}},
        "evaluation": {"metrics": ["accuracy"]},
    }
    log_dir = train_classifier.run(config)
    df = pd.read_csv(os.path.join(log_dir, "results.csv"))
    assert len(df) == 1 and 0.0 <= float(df.iloc[0]["accuracy_mean"]) <= 1.0
    assert len(calls) == 2 * 3 and sum(calls) == 2 * 36                                    # 2 epochs x ceil(36 / 16) fused steps
