"""GPU: the classifier ensemble - every ``tl_*_group`` kernel bit for bit against its single-model launch (M = 1 and 3, every
member on inputs of its own), the active mask (a masked member's buffers, pre-filled with canaries, do not change by a bit),
``ClassifierEnsembleEngine`` against ``SimpleClassifierEngine`` on the low-rank, the dense and the mixed route,
``ClassifierEnsembleTrainer`` against sequential ``ClassifierTrainer(fused=True)`` runs with members that stop at different
epochs, and the pipeline key against the sequential pipeline.

All comparisons are exact (``torch.equal`` on the raw buffers): a group kernel IS the single kernel, launched with a member
dimension, and the single engine's own tests tie it to the float64 reference."""
import copy
import ctypes as C
import filecmp
import os
import sys

import numpy as np
import pytest
import torch
from torch.utils.data import TensorDataset

pytestmark = pytest.mark.gpu
DEV = "cuda"
CANARY = -777.25
MASKS = {1: [None], 3: [None, (1, 0, 1)]}
CASES = [(M, mask) for M in (1, 3) for mask in MASKS[M]]
IDS = [f"M{M}" + ("" if mask is None else "_masked") for M, mask in CASES]


def _r4(n):
    return (n + 3) // 4 * 4


def _lib():
    from decode_tonal_langauge_amd import _lib as L
    return L, L.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _mask(mask):
    return None if mask is None else torch.tensor(mask, dtype=torch.int32, device=DEV)


def _on(mask, m):
    return mask is None or bool(mask[m])


def _canary(*shape, dtype=torch.float32):
    return torch.full(shape, CANARY if dtype.is_floating_point else -7, dtype=dtype, device=DEV)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------------------------- forward and loss
@pytest.mark.parametrize("M,mask", CASES, ids=IDS)
@pytest.mark.parametrize("B,K,N", [(1, 4, 2), (7, 12, 3), (65, 260, 33)])
def test_linear_rows_and_ce_loss_group_equal_the_single_launches(M, mask, B, K, N):
    L, lib = _lib()
    g, ldd, words = _gen(B * 100 + N), _r4(N), 3 + N * N
    x = torch.randn(M, B, K, generator=g).to(DEV)
    W = (torch.randn(M, N, K, generator=g) * 0.3).to(DEV)
    bias = _canary(M, ldd)
    bias[:, :N] = torch.randn(M, N, generator=g).to(DEV)
    y = torch.randint(0, N, (M, B), generator=g).to(DEV)
    y[M - 1, 0] = N                                            # one label out of range, in one member only

    def stats_fill(rows):                                      # the statistics accumulate: start them from values of their own
        s = torch.arange(rows * words, dtype=torch.int64, device=DEV).reshape(rows, words) + 5
        s[:, 0] = torch.tensor([1.5], dtype=torch.float64).view(torch.int64).item()
        s[:, 2] = 0
        return s

    logits, dl, db, pred, stats = _canary(M, B, N), _canary(M, B, ldd), _canary(M, ldd), _canary(M, B, dtype=torch.int64), stats_fill(M)
    act = _mask(mask)
    L.check(lib.tl_linear_rows_group(x.data_ptr(), W.data_ptr(), bias.data_ptr(), logits.data_ptr(), M, B, K, N, K, 0, B * K, N * K,
                                     ldd, B * N, L.ptr(act), _stream()), "tl_linear_rows_group")
    base = stats.data_ptr()
    L.check(lib.tl_ce_loss_group(logits.data_ptr(), y.data_ptr(), dl.data_ptr(), db.data_ptr(), pred.data_ptr(), base, base + 8,
                                 base + 24, base + 16, M, B, N, N, ldd, 1.0 / B, B * N, B, B * ldd, ldd, B, words, L.ptr(act),
                                 _stream()), "tl_ce_loss_group")
    # prediction only (labels null): a second pred buffer, the statistics are not touched
    pred2, before = _canary(M, B, dtype=torch.int64), stats.clone()
    L.check(lib.tl_ce_loss_group(logits.data_ptr(), None, None, None, pred2.data_ptr(), None, None, None, None, M, B, N, N, ldd, 0.0,
                                 B * N, 0, 0, 0, B, 0, L.ptr(act), _stream()), "tl_ce_loss_group")
    torch.cuda.synchronize()
    assert torch.equal(stats, before)
    for m in range(M):
        if not _on(mask, m):
            assert torch.equal(logits[m], _canary(B, N)) and torch.equal(dl[m], _canary(B, ldd)) and torch.equal(db[m], _canary(ldd))
            assert torch.equal(pred[m], _canary(B, dtype=torch.int64)) and torch.equal(pred2[m], pred[m])
            assert torch.equal(stats[m], stats_fill(M)[m])
            continue
        s_logits, s_dl, s_db, s_pred, s_stats = _canary(B, N), _canary(B, ldd), _canary(N), _canary(B, dtype=torch.int64), stats_fill(M)[m]
        xm, wm, bm, ym = x[m].clone(), W[m].clone(), bias[m, :N].clone(), y[m].clone()
        L.check(lib.tl_linear_rows(xm.data_ptr(), wm.data_ptr(), bm.data_ptr(), s_logits.data_ptr(), B, K, N, K, 0, _stream()),
                "tl_linear_rows")
        sb = s_stats.data_ptr()
        L.check(lib.tl_ce_loss(s_logits.data_ptr(), ym.data_ptr(), s_dl.data_ptr(), s_db.data_ptr(), s_pred.data_ptr(), sb, sb + 8,
                               sb + 24, sb + 16, B, N, N, ldd, 1.0 / B, _stream()), "tl_ce_loss")
        torch.cuda.synchronize()
        assert torch.equal(logits[m], s_logits), m
        assert torch.equal(dl[m], s_dl) and torch.equal(db[m, :N], s_db) and torch.equal(db[m, N:], _canary(ldd - N)), m
        assert torch.equal(pred[m], s_pred) and torch.equal(pred2[m], s_pred), m
        assert torch.equal(stats[m], s_stats), m
        assert int(stats[m, 2]) == (1 if m == M - 1 else 0)                        # the range flag is the member's own


# ---------------------------------------------------------------------------------------------- updates
def _scalars(step, mu):
    from decode_tonal_langauge_amd.optim import nadam_scalars
    return nadam_scalars(step, mu, 0.01, 0.9, 0.999, 0.004)


@pytest.mark.parametrize("M,mask", CASES, ids=IDS)
@pytest.mark.parametrize("kr,rows,cols", [(1, 2, 4), (7, 3, 12), (64, 33, 260)])
def test_nadam_lowrank_group_equals_the_single_launch_over_two_steps(M, mask, kr, rows, cols):
    L, lib = _lib()
    g, ldfa = _gen(kr * 7 + rows), _r4(rows)
    p = torch.randn(M, rows, cols, generator=g).to(DEV)
    mo, vo = torch.zeros_like(p), torch.zeros_like(p)
    single = [(p[m].clone(), mo[m].clone(), vo[m].clone()) for m in range(M)]
    p0, act, mu = p.clone(), _mask(mask), 1.0
    for step in (1, 2):
        fa = torch.randn(M, kr, ldfa, generator=g).to(DEV)
        fb = torch.randn(M, kr, cols, generator=g).to(DEV)
        cg, cm, bc2, mu = _scalars(step, mu)
        args = (cg, cm, 0.9, 0.999, bc2, 1e-8, 0.01, 1.0)
        L.check(lib.tl_nadam_lowrank_group(p.data_ptr(), mo.data_ptr(), vo.data_ptr(), fa.data_ptr(), fb.data_ptr(), M, kr, rows, cols,
                                           ldfa, cols, rows * cols, kr * ldfa, kr * cols, *args, L.ptr(act), _stream()),
                "tl_nadam_lowrank_group")
        for m in range(M):
            sp, sm, sv = single[m]
            fam, fbm = fa[m].clone(), fb[m].clone()
            L.check(lib.tl_nadam_lowrank(sp.data_ptr(), sm.data_ptr(), sv.data_ptr(), fam.data_ptr(), fbm.data_ptr(), kr, rows, cols,
                                         ldfa, cols, *args, _stream()), "tl_nadam_lowrank")
        torch.cuda.synchronize()
    for m in range(M):
        if _on(mask, m):
            assert all(torch.equal(a[m], b) for a, b in zip((p, mo, vo), single[m])), m
            assert not torch.equal(p[m], p0[m])
        else:
            assert torch.equal(p[m], p0[m]) and not mo[m].any() and not vo[m].any()


@pytest.mark.parametrize("M,mask", CASES, ids=IDS)
@pytest.mark.parametrize("B,K,N", [(65, 260, 33), (70, 12, 3)])
def test_head_bwd_group_equals_the_single_launch(M, mask, B, K, N):
    L, lib = _lib()
    g, ldd = _gen(B + N), _r4(N)
    dl = torch.randn(M, B, ldd, generator=g).to(DEV)
    h = torch.randn(M, B, K, generator=g).to(DEV)
    W = torch.randn(M, N, K, generator=g).to(DEV)
    dw = _canary(M, N, K)
    L.check(lib.tl_head_bwd_group(dl.data_ptr(), h.data_ptr(), W.data_ptr(), dw.data_ptr(), M, B, K, N, ldd, B * ldd, B * K, N * K,
                                  N * K, L.ptr(_mask(mask)), _stream()), "tl_head_bwd_group")
    for m in range(M):
        if not _on(mask, m):
            assert torch.equal(dw[m], _canary(N, K))
            continue
        s_dw, dlm, hm, wm = _canary(N, K), dl[m].clone(), h[m].clone(), W[m].clone()
        L.check(lib.tl_head_bwd(dlm.data_ptr(), hm.data_ptr(), wm.data_ptr(), None, None, s_dw.data_ptr(), B, K, N, ldd, 0, 0.0,
                                _stream()), "tl_head_bwd")
        torch.cuda.synchronize()
        assert torch.equal(dw[m], s_dw), m


@pytest.mark.parametrize("M,mask", CASES, ids=IDS)
@pytest.mark.parametrize("n,stride", [(3, 4), (2, 4), (33, 36), (33 * 260, 33 * 260)])
def test_nadam_group_equals_the_single_launch(M, mask, n, stride):
    """The dense update: bias rows of N floats stored at row stride r4(N), and a whole weight gradient above rank 64."""
    L, lib = _lib()
    g = _gen(n)
    p = _canary(M, stride)
    p[:, :n] = torch.randn(M, n, generator=g).to(DEV)
    mo, vo = torch.zeros_like(p), torch.zeros_like(p)
    single = [(p[m].clone(), mo[m].clone(), vo[m].clone()) for m in range(M)]
    p0, act, mu = p.clone(), _mask(mask), 1.0
    for step in (1, 2):
        grad = _canary(M, stride)
        grad[:, :n] = torch.randn(M, n, generator=g).to(DEV)
        cg, cm, bc2, mu = _scalars(step, mu)
        args = (cg, cm, 0.9, 0.999, bc2, 1e-8, 0.0, 1.0)
        L.check(lib.tl_nadam_group(p.data_ptr(), grad.data_ptr(), mo.data_ptr(), vo.data_ptr(), M, n, stride, stride, *args,
                                   L.ptr(act), _stream()), "tl_nadam_group")
        for m in range(M):
            sp, sm, sv = single[m]
            gm = grad[m].clone()
            L.check(lib.tl_nadam(sp.data_ptr(), gm.data_ptr(), sm.data_ptr(), sv.data_ptr(), n, *args, _stream()), "tl_nadam")
        torch.cuda.synchronize()
    for m in range(M):
        if _on(mask, m):
            assert all(torch.equal(a[m], b) for a, b in zip((p, mo, vo), single[m])), m
            assert torch.equal(p[m, n:], _canary(stride - n)) and not mo[m, n:].any()      # the padding is nobody's
            assert not torch.equal(p[m, :n], p0[m, :n])
        else:
            assert torch.equal(p[m], p0[m]) and not mo[m].any() and not vo[m].any()


# ---------------------------------------------------------------------------------------------- gather
@pytest.mark.parametrize("M,mask", CASES, ids=IDS)
def test_gather_rows_group_against_torch_indexing(M, mask):
    """48-byte rows (16-byte accesses), 3-byte rows (byte accesses) and a channel list in one launch; repeated indices, a
    start offset into the table, canary rows behind every member's destination, one index out of range in one member."""
    L, lib = _lib()
    g, n, rows, pad, start, width = _gen(11), 29, 9, 2, 3, 16
    wide = torch.randn(n, 12, generator=g).to(DEV)
    small = torch.randint(0, 255, (n, 3), generator=g, dtype=torch.uint8).to(DEV)
    chans = torch.randn(n, 5, 4, generator=g).to(DEV)
    clist = torch.tensor([3, 0, 3], dtype=torch.int32, device=DEV)
    table = torch.randint(0, n, (M, width), generator=g)
    table[:, start + 2] = table[:, start + 1]                                  # a repeated index
    table[M - 1, start + 4] = n                                                # out of range: never read, never written
    table_dev = table.to(DEV)
    d_wide, d_small, d_chan = _canary(M, rows + pad, 12), torch.full((M, rows + pad, 3), 9, dtype=torch.uint8, device=DEV), \
        _canary(M, rows + pad, 3, 4)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    P4, L4 = C.c_void_p * 4, C.c_int64 * 4
    src = P4(wide.data_ptr(), small.data_ptr(), chans.data_ptr(), None)
    dst = P4(d_wide.data_ptr(), d_small.data_ptr(), d_chan.data_ptr(), None)
    stride = L4(*[t.stride(0) * t.element_size() for t in (d_wide, d_small, d_chan)], 0)
    L.check(lib.tl_gather_rows_group(src, dst, stride, L4(n, n, n, 0), L4(1, 1, 5, 0), L4(48, 3, 16, 0),
                                     P4(None, None, clist.data_ptr(), None), L4(0, 0, 3, 0), 3, table_dev.data_ptr() + 8 * start,
                                     width, rows, M, L.ptr(_mask(mask)), err.data_ptr(), _stream()), "tl_gather_rows_group")
    torch.cuda.synchronize()
    want_err = 1 if _on(mask, M - 1) else 0
    assert int(err.item()) == want_err
    for m in range(M):
        idx = table[m, start:start + rows]
        for got, source, fill in ((d_wide, wide, CANARY), (d_small, small, 9), (d_chan, chans[:, [3, 0, 3]], CANARY)):
            tail = torch.full_like(got[m, rows:], fill)
            assert torch.equal(got[m, rows:], tail), m                          # nothing behind the member's batch
            if not _on(mask, m):
                assert torch.equal(got[m, :rows], torch.full_like(got[m, :rows], fill)), m
                continue
            ok = (idx < n).to(DEV)
            assert torch.equal(got[m, :rows][ok], source[idx.to(DEV)[ok]]), m
            assert torch.equal(got[m, :rows][~ok], torch.full_like(got[m, :rows][~ok], fill)), m


def test_gather_group_of_the_resident_dataset():
    from decode_tonal_langauge_amd.data_loading.resident import ResidentDataset
    g = _gen(4)
    x, y = torch.randn(31, 2, 6, generator=g), torch.randint(0, 3, (31,), generator=g).float()
    rds = ResidentDataset.from_tensor_dataset(TensorDataset(x, y), device=DEV)
    table = torch.stack([torch.randperm(31, generator=g)[:20] for _ in range(3)])
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    gx, gy = rds.gather_group(table.to(DEV), 8, 13, err)
    assert gx.shape == (3, 5, 2, 6) and gy.shape == (3, 5) and int(err.item()) == 0
    for m in range(3):
        one = rds.gather(table[m].to(DEV), 8, 13, err)
        assert torch.equal(gx[m], one[0]) and torch.equal(gy[m], one[1])
        assert torch.equal(gx[m].cpu(), x[table[m, 8:13]])


# ---------------------------------------------------------------------------------------------- engine
def _member_models(n, K=12, N=3):
    from decode_tonal_langauge_amd.models.simple_classifiers import LogisticRegressionClassifier
    out = []
    for m in range(n):
        torch.manual_seed(100 + m)
        out.append(LogisticRegressionClassifier(K, N).to(DEV))
    return out


def _moments(eng):
    return {k: (eng.optimizer.state[p]["exp_avg"], eng.optimizer.state[p]["exp_avg_sq"]) for k, p in eng.params.items()}


@pytest.mark.parametrize("sizes", [(8, 8), (65, 65), (65, 19)], ids=["lowrank", "dense", "dense_then_lowrank"])
def test_engine_steps_equal_the_single_engine(sizes):
    from decode_tonal_langauge_amd._classifier_ensemble_engine import ClassifierEnsembleEngine
    from decode_tonal_langauge_amd._simple_classifier_engine import SimpleClassifierEngine
    models = _member_models(3)
    singles = [SimpleClassifierEngine(copy.deepcopy(m), 0.01, 0.02) for m in models]
    ens = ClassifierEnsembleEngine(models, 0.01, 0.02)
    assert all(torch.equal(a.linear.weight, s.model.linear.weight) for a, s in zip(models, singles))     # the views hold the values
    g = _gen(9)
    for B in sizes:
        x = torch.randn(3, B, 2, 6, generator=g).to(DEV)
        y = torch.randint(0, 3, (3, B), generator=g).float().to(DEV)
        ens.train_batch(x, y)
        for m, s in enumerate(singles):
            s.train_batch(x[m], y[m])
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")                    # warm: no step reads the device
    try:
        ens.eval_batch(x, y)
        ens.train_batch(x, y)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    for m, s in enumerate(singles):
        s.eval_batch(x[m], y[m])
        s.train_batch(x[m], y[m])
    stats = ens.epoch_stats()
    for m, s in enumerate(singles):
        for k, v in s.model.state_dict().items():
            assert torch.equal(models[m].state_dict()[k], v), (m, k)
        for k, (ma, va) in _moments(s).items():
            assert torch.equal(ens.moments(m)[k][0], ma) and torch.equal(ens.moments(m)[k][1], va), (m, k)
        loss, count, cm = s.epoch_stats()
        assert stats[m][0] == loss and stats[m][1] == count == sum(sizes) + 2 * sizes[-1] and torch.equal(stats[m][2], cm), m
    assert len({float(m.linear.weight.detach().sum()) for m in models}) == 3
    # inference through the module reads the stacked storage
    with torch.no_grad():
        assert torch.equal(models[1](x[1]).argmax(1), ens.predict_batch(x)[1])


def test_engine_mask_freezes_a_member_and_names_the_member_with_a_bad_label():
    from decode_tonal_langauge_amd._classifier_ensemble_engine import ClassifierEnsembleEngine
    from decode_tonal_langauge_amd._simple_classifier_engine import SimpleClassifierEngine
    models = _member_models(3)
    singles = [SimpleClassifierEngine(copy.deepcopy(m), 0.01, 0.0) for m in models]
    ens = ClassifierEnsembleEngine(models, 0.01, 0.0)
    g = _gen(2)
    batches = [(torch.randn(3, B, 12, generator=g).to(DEV), torch.randint(0, 3, (3, B), generator=g).to(DEV)) for B in (8, 65, 8)]
    ens.train_batch(*batches[0])
    frozen = copy.deepcopy(models[1].state_dict())
    ens.set_active([True, False, True])
    for x, y in batches[1:]:
        ens.train_batch(x, y)
    stats = ens.epoch_stats()
    for m, s in enumerate(singles):
        for x, y in batches[:1] if m == 1 else batches:
            s.train_batch(x[m], y[m])
        for k, v in s.model.state_dict().items():
            assert torch.equal(models[m].state_dict()[k], v), (m, k)
        assert stats[m][:2] == s.epoch_stats()[:2], m
    assert all(torch.equal(frozen[k], v) for k, v in models[1].state_dict().items())
    ens.set_active([True] * 3)
    x, y = batches[0][0], batches[0][1].clone()
    y[2, 3] = 3
    ens.eval_batch(x, y)
    with pytest.raises(ValueError, match=r"\[0, 3\).*member 2"):
        ens.epoch_stats()
    with pytest.raises(ValueError, match="expected input"):
        ens.train_batch(x[:2], y[:2])


# ---------------------------------------------------------------------------------------------- trainer
SEEDS, LR, WD = (3, 11, 42), 0.1, 0.01       # the float32 CPU loop stops these seeds after epochs 3, 2 and 1 (val/loss turns by > 4 %)


def _planted():
    g = _gen(1)
    y = torch.randint(0, 3, (53,), generator=g)
    x = torch.randn(53, 2, 6, generator=g)
    for k in range(3):
        x.view(53, 12)[y == k, 4 * k:4 * k + 4] += 1.0
    return TensorDataset(x, y.float())


def _prologue(dataset, seed):
    from decode_tonal_langauge_amd.data_loading.dataloaders import split_dataset
    from decode_tonal_langauge_amd.models.simple_classifiers import LogisticRegressionClassifier
    from decode_tonal_langauge_amd.utils.utils import set_seeds
    set_seeds(seed)
    loaders = split_dataset(dataset, [0.7, 0.1, 0.2], [True, False, False], batch_size=8, seed=seed, resident=True, device=DEV)
    list(loaders[2])                                           # the pipeline's `true` pass draws before the model is built
    return loaders, LogisticRegressionClassifier(12, 3).to(DEV), torch.get_rng_state()


def test_trainer_equals_sequential_fused_runs_with_members_stopping_apart(tmp_path):
    from decode_tonal_langauge_amd.data_loading.resident import ResidentDataset
    from decode_tonal_langauge_amd.models.classifier_ensemble_trainer import ClassifierEnsembleTrainer
    from decode_tonal_langauge_amd.models.classifier_trainer import ClassifierTrainer
    tds = _planted()
    seq = []
    for seed in SEEDS:
        loaders, model, state = _prologue(tds, seed)
        assert len(loaders[0]) == 5 and len(loaders[0].sampler.indices) == 37  # four full batches and a ragged one
        tr = ClassifierTrainer(model, LR, WD, log_dir=str(tmp_path / f"seq_{seed}"), fused=True)
        hist = tr.fit(loaders[0], loaders[1], max_epochs=6, patience=1)
        seq.append(dict(hist=hist, stopped=tr.stopped_epoch, test=tr.test(loaders[2]), pred=tr.predict(loaders[2]),
                        sd=copy.deepcopy(model.state_dict()), entered=state))
    final = torch.get_rng_state()
    print("stopped_epoch of the sequential runs:", [s["stopped"] for s in seq])
    assert len({s["stopped"] for s in seq}) > 1                # the masked path is exercised

    rds = ResidentDataset.from_tensor_dataset(tds, device=DEV)
    torch.manual_seed(777)
    pro = [_prologue(rds, seed) for seed in SEEDS]
    assert all(torch.equal(p[2], s["entered"]) for p, s in zip(pro, seq))
    torch.manual_seed(778)                                     # the trainer works from the states it is given
    dirs = [str(tmp_path / f"ens_{seed}") for seed in SEEDS]
    ens = ClassifierEnsembleTrainer([p[1] for p in pro], LR, WD, log_dirs=dirs, rng_states=[p[2] for p in pro])
    hists = ens.fit([p[0][0] for p in pro], [p[0][1] for p in pro], max_epochs=6, patience=1)
    tests = ens.test([p[0][2] for p in pro])
    preds = ens.predict([p[0][2] for p in pro])
    assert torch.equal(torch.get_rng_state(), final)
    for m, (seed, s) in enumerate(zip(SEEDS, seq)):
        assert ens.stopped_epoch[m] == s["stopped"] and len(hists[m]) == len(s["hist"]), seed
        for a, b in zip(hists[m], s["hist"]):
            assert list(a) == list(b)
            for key in a:
                if key == "train/weight_norm":
                    assert abs(a[key] - b[key]) <= 1e-6 * abs(b[key]), (seed, key)
                else:
                    assert a[key] == b[key], (seed, key, a[key], b[key])
        assert tests[m]["accuracy"] == s["test"]["accuracy"] == ens.test_accuracy[m] and tests[m]["f1"] == s["test"]["f1"]
        assert torch.equal(tests[m]["confusion_matrix"], s["test"]["confusion_matrix"])
        assert torch.equal(ens.confusion_matrix[m], s["test"]["confusion_matrix"]) and ens.test_f1[m] == s["test"]["f1"]
        assert preds[m].dtype == torch.int64 and preds[m].is_cuda and torch.equal(preds[m], s["pred"])
        sd = pro[m][1].state_dict()
        assert list(sd) == list(s["sd"]) and all(torch.equal(sd[k], v) for k, v in s["sd"].items()), seed
        for name in ("metrics.csv", "confusion_matrix_test.csv"):
            assert filecmp.cmp(os.path.join(dirs[m], name), str(tmp_path / f"seq_{seed}" / name), shallow=False), (seed, name)
    assert torch.equal(ens.rng_state(len(SEEDS) - 1), final)
    with pytest.raises(RuntimeError, match="runs once"):
        ens.fit([p[0][0] for p in pro], [p[0][1] for p in pro], max_epochs=1, patience=1)


# ---------------------------------------------------------------------------------------------- pipeline
def _run_pipeline(tmp_path, monkeypatch, tag, separate, ensemble):
    from decode_tonal_langauge_amd import train_classifier
    from decode_tonal_langauge_amd.data_loading import synthetic
    root = tmp_path / "data"
    if not root.exists():
        synthetic.write_dataset(str(root), n_samples=240, n_channels=8, n_timepoints=50)     # every joint class in every test split
    got = {}
    for name in ("train_joint_targets", "train_separate_targets"):
        fn = getattr(train_classifier, name)
        monkeypatch.setattr(train_classifier, name, lambda p, s, fn=fn: got.setdefault("out", fn(p, s)))
    params = {"fused": True, "resident": True,
              "io": {"log_dir": str(tmp_path / f"logs_{tag}"), "sample_dir": str(root / "samples"),
                     "channel_selection_dir": str(root / "channels"), "save_checkpoints": True},
              "experiment": {"targets": ["syllable", "tone"] if separate else ["tone"], "features": "ecog",
                             "separate_models": separate, "seed": 1, "repeat": 3, "verbose": 0, "device": DEV},
              "training": {"train_ratio": 0.7, "vali_ratio": 0.1, "test_ratio": 0.2, "batch_size": 16, "epochs": 4, "lr": 0.05,
                           "patience": 1, "weight_decay": 0.01, "log_every_n_steps": 10}}
    if ensemble is not None:
        params["ensemble"] = ensemble
    config = {"model": {"model": "models.simple_classifiers.LogisticRegressionClassifier", "model_name": "logistic",
                        "model_kwargs": {}},
              "dataset": {"class_labels": {"tone": None, "syllable": ["i", "a"]}},
              "training": {"module": "train_classifier", "params": params},
              "evaluation": {"metrics": ["accuracy", "f1_score", "confusion_matrix"], "aggregates": ["mean", "std"]}}
    log_dir = train_classifier.run(config)
    monkeypatch.undo()
    return log_dir, got["out"], torch.get_rng_state()


def _same(a, b, where=""):
    if isinstance(a, dict):
        assert isinstance(b, dict) and list(a) == list(b), where
        for k in a:
            _same(a[k], b[k], f"{where}/{k}")
    elif isinstance(a, np.ndarray):
        assert np.array_equal(a, b), where
    elif isinstance(a, (list, tuple)) and a and isinstance(a[0], (dict, np.ndarray)):
        assert len(a) == len(b), where
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{where}/{i}")
    else:
        assert a == b or (a is None and b is None), (where, a, b)


def _files(log_dir):
    out = []
    for base, _dirs, names in os.walk(log_dir):
        out += [os.path.relpath(os.path.join(base, n), log_dir) for n in names]
    return sorted(out)


@pytest.mark.parametrize("separate", [False, True], ids=["joint", "separate"])
def test_pipeline_with_the_key_equals_the_sequential_pipeline(tmp_path, monkeypatch, separate):
    import pandas as pd
    mods = ("decode_tonal_langauge_amd._classifier_ensemble_engine", "decode_tonal_langauge_amd.models.classifier_ensemble_trainer")
    kept = {k: sys.modules.pop(k) for k in mods if k in sys.modules}
    try:
        off_dir, off, off_state = _run_pipeline(tmp_path, monkeypatch, "off", separate, None)
        assert not any(k in sys.modules for k in mods)         # without the key nothing of the ensemble is imported
    finally:
        sys.modules.update(kept)
    on_dir, on, on_state = _run_pipeline(tmp_path, monkeypatch, "on", separate, True)
    assert all(k in sys.modules for k in mods) and on_dir != off_dir
    assert torch.equal(on_state, off_state)
    _same(on[0], off[0], "result_info")
    assert np.array_equal(on[1], off[1]) and list(on[2]) == list(off[2])
    assert int(on[1].sum()) == 3 * 48                          # 3 seeds x 20 % of 240
    files = _files(on_dir)
    assert files == _files(off_dir) and sum(f.endswith(".pt") for f in files) == (6 if separate else 3)
    assert sum(f.endswith("metrics.csv") for f in files) == (6 if separate else 3)
    for f in files:
        a, b = os.path.join(on_dir, f), os.path.join(off_dir, f)
        if f.endswith(".pt"):
            sa, sb = torch.load(a), torch.load(b)
            assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa), f
        elif f.endswith(".csv") and os.path.basename(f) != "results.csv":
            assert filecmp.cmp(a, b, shallow=False), f
    assert pd.read_csv(os.path.join(on_dir, "results.csv")).equals(pd.read_csv(os.path.join(off_dir, "results.csv")))
