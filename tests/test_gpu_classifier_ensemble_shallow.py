"""GPU: the ShallowNNClassifier ensemble - ``tl_gemm_nt_window_group`` and ``tl_head_bwd_act_group`` bit for bit against their
single launches (M = 1 and 3, every member on inputs of its own, a masked member's canaries untouched, member strides with
canaried padding), ``ClassifierEnsembleEngine`` against three ``SimpleClassifierEngine``s, the active mask, the 64-row limit of
training batches, ``ClassifierEnsembleTrainer`` against sequential ``ClassifierTrainer(fused=True)`` runs that stop at
different epochs, and the pipeline key against the sequential pipeline.

All comparisons are exact (``torch.equal`` on the raw buffers): a group kernel runs the single kernel's body with a member
dimension on the grid, and the single engine's own tests tie it to the float64 reference."""
import copy
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


# ---------------------------------------------------------------------------------------------- the hidden layer's forward
# (B, K, N): register-staged with one partial tile; register-staged, K % 16 != 0; direct-to-LDS narrow with a single K stage;
# direct-to-LDS wide with a partial second column tile; register-staged, two row tiles, K % 16 = 4; narrow, two row tiles
NT_SHAPES = [(1, 4, 4), (7, 12, 20), (65, 16, 8), (33, 48, 132), (130, 260, 36), (130, 32, 64)]


def _nt_group_against_singles(M, mask, B, K, N):
    from decode_tonal_langauge_amd._launch import launch_nt, launch_nt_group
    from decode_tonal_langauge_amd._lib import EPI_LRELU, LOAD_DIRECT
    L, lib = _lib()
    g = _gen(B * 1000 + K * 10 + N)
    # M = 3: every member stride is longer than the member's extent and the padding holds canaries
    pa, pw, pb, po = (8, 4, 3, 5) if M > 1 else (0, 0, 0, 0)
    sA, sW, sb, so = B * K + pa, N * K + pw, N + pb, B * N + po
    A, W, bias = _canary(M, sA), _canary(M, sW), _canary(M, sb)
    A[:, :B * K] = torch.randn(M, B * K, generator=g).to(DEV)
    W[:, :N * K] = (torch.randn(M, N * K, generator=g) * 0.3).to(DEV)
    bias[:, :N] = torch.randn(M, N, generator=g).to(DEV)
    A0, W0, b0 = A.clone(), W.clone(), bias.clone()
    act = _mask(mask)
    for slope in (0.0, 0.01):
        out = _canary(M, so)
        launch_nt_group(lib, M, sA, sW, sb, so, act, A=A.data_ptr(), Bw=W.data_ptr(), bias=bias.data_ptr(), out=out.data_ptr(), M=B,
                        A_rows=B, N=N, K=K, lda=K, ldb=K, ldo=N, Tvalid=1, loader=LOAD_DIRECT, epilogue=EPI_LRELU, slope=slope)
        torch.cuda.synchronize()
        assert torch.equal(A, A0) and torch.equal(W, W0) and torch.equal(bias, b0)
        assert torch.equal(out[:, B * N:], _canary(M, po))                       # nothing behind a member's rows
        for m in range(M):
            if not _on(mask, m):
                assert torch.equal(out[m], _canary(so)), m
                continue
            am, wm, bm, single = A[m, :B * K].clone(), W[m, :N * K].clone(), bias[m, :N].clone(), _canary(B, N)
            launch_nt(lib, A=am.data_ptr(), Bw=wm.data_ptr(), bias=bm.data_ptr(), out=single.data_ptr(), M=B, A_rows=B, N=N, K=K,
                      lda=K, ldb=K, ldo=N, Tvalid=1, loader=LOAD_DIRECT, epilogue=EPI_LRELU, slope=slope)
            torch.cuda.synchronize()
            assert not (single == CANARY).any()
            assert torch.equal(out[m, :B * N].view(B, N), single), (m, slope)
            if slope == 0.0:
                assert (single >= 0).all()                                           # ReLU is slope 0
    return out


@pytest.mark.parametrize("M,mask", CASES, ids=IDS)
@pytest.mark.parametrize("B,K,N", NT_SHAPES)
def test_nt_window_group_equals_the_single_launches(M, mask, B, K, N):
    _nt_group_against_singles(M, mask, B, K, N)


def test_nt_window_group_honours_the_register_staged_switch(monkeypatch):
    """Under TONAL_AB=1 TONAL_GLDS=0 both entries take the register-staged kernel at K % 16 == 0 as well."""
    plain = _nt_group_against_singles(3, (1, 0, 1), 33, 48, 132)
    monkeypatch.setenv("TONAL_AB", "1")
    monkeypatch.setenv("TONAL_GLDS", "0")
    staged = _nt_group_against_singles(3, (1, 0, 1), 33, 48, 132)
    assert plain.shape == staged.shape and torch.isfinite(staged[0]).all()


# ---------------------------------------------------------------------------------------------- the output layer's backward
@pytest.mark.parametrize("M,mask", CASES, ids=IDS)
@pytest.mark.parametrize("B,K,N", [(1, 4, 1), (7, 12, 3), (65, 260, 33), (70, 20, 9)])
def test_head_bwd_act_group_equals_the_single_launches(M, mask, B, K, N):
    L, lib = _lib()
    g, ldd = _gen(B + 3 * N), _r4(N)
    pd, ph, pw = (4, 8, 12) if M > 1 else (0, 0, 0)                               # padded member strides of the outputs
    dl = torch.randn(M, B, ldd, generator=g).to(DEV)
    h = torch.randn(M, B, K, generator=g).to(DEV)                                 # both signs: the derivative takes both values
    W = torch.randn(M, N, K, generator=g).to(DEV)
    act_words = _mask(mask)
    for act in (0, 1, 2):
        slope = 0.01 if act == 2 else 0.0
        for want in ((1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1)):
            dh, dbh, dw = _canary(M, B * K + pd), _canary(M, K + ph), _canary(M, N * K + pw)
            L.check(lib.tl_head_bwd_act_group(dl.data_ptr(), h.data_ptr(), W.data_ptr(), dh.data_ptr() if want[0] else None,
                                              dbh.data_ptr() if want[1] else None, dw.data_ptr() if want[2] else None, M, B, K, N,
                                              ldd, act, slope, B * ldd, B * K, N * K, B * K + pd, K + ph, N * K + pw,
                                              L.ptr(act_words), _stream()), "tl_head_bwd_act_group")
            torch.cuda.synchronize()
            for m in range(M):
                s_dh, s_dbh, s_dw = _canary(B * K + pd), _canary(K + ph), _canary(N * K + pw)
                if _on(mask, m):
                    dlm, hm, wm = dl[m].clone(), h[m].clone(), W[m].clone()
                    L.check(lib.tl_head_bwd(dlm.data_ptr(), hm.data_ptr(), wm.data_ptr(), s_dh.data_ptr() if want[0] else None,
                                            s_dbh.data_ptr() if want[1] else None, s_dw.data_ptr() if want[2] else None, B, K, N,
                                            ldd, act, slope, _stream()), "tl_head_bwd")
                    torch.cuda.synchronize()
                    for on, buf, n in zip(want, (s_dh, s_dbh, s_dw), (B * K, K, N * K)):
                        assert bool((buf[:n] != CANARY).all()) == bool(on)
                # a masked member, an output not asked for and the padding all keep the canary
                assert torch.equal(dh[m], s_dh) and torch.equal(dbh[m], s_dbh) and torch.equal(dw[m], s_dw), (m, act, want)


# ---------------------------------------------------------------------------------------------- engine
SHALLOW = {"relu": (12, 3, 8, "ReLU"), "lrelu": (16, 3, 20, "LeakyReLU")}


def _member_models(n, kind):
    from decode_tonal_langauge_amd.models.simple_classifiers import ShallowNNClassifier
    K, N, H, act = SHALLOW[kind]
    out = []
    for m in range(n):
        torch.manual_seed(100 + m)
        out.append(ShallowNNClassifier(K, N, H, act).to(DEV))
    return out


def _moments(eng):
    return {k: (eng.optimizer.state[p]["exp_avg"], eng.optimizer.state[p]["exp_avg_sq"]) for k, p in eng.params.items()}


def _assert_member_equals_single(ens, models, m, single):
    sd = models[m].state_dict()
    assert list(sd) == list(single.model.state_dict())
    for k, v in single.model.state_dict().items():
        assert torch.equal(sd[k], v), (m, k)
    mom = _moments(single)
    assert sorted(mom) == sorted(ens.moments(m)) == ["hidden.bias", "hidden.weight", "output.bias", "output.weight"]
    for k, (ma, va) in mom.items():
        assert torch.equal(ens.moments(m)[k][0], ma) and torch.equal(ens.moments(m)[k][1], va), (m, k)


@pytest.mark.parametrize("kind", list(SHALLOW))
@pytest.mark.parametrize("sizes", [(8, 8), (64, 19), (1,)], ids=["b8_b8", "b64_b19", "b1"])
def test_engine_steps_equal_the_single_engine(kind, sizes):
    from decode_tonal_langauge_amd._classifier_ensemble_engine import ClassifierEnsembleEngine
    from decode_tonal_langauge_amd._simple_classifier_engine import SimpleClassifierEngine
    K = SHALLOW[kind][0]
    models = _member_models(3, kind)
    singles = [SimpleClassifierEngine(copy.deepcopy(m), 0.01, 0.02) for m in models]
    ens = ClassifierEnsembleEngine(models, 0.01, 0.02)
    for a, s in zip(models, singles):                          # the views hold the values
        assert all(torch.equal(v, s.model.state_dict()[k]) for k, v in a.state_dict().items())
    g = _gen(9)
    for B in sizes:
        x = torch.randn(3, B, 2, K // 2, generator=g).to(DEV)
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
        _assert_member_equals_single(ens, models, m, s)
        loss, count, cm = s.epoch_stats()
        assert stats[m][0] == loss and stats[m][1] == count == sum(sizes) + 2 * sizes[-1] and torch.equal(stats[m][2], cm), m
    assert len({float(m.hidden.weight.detach().sum()) for m in models}) == 3
    assert len({float(m.output.weight.detach().sum()) for m in models}) == 3
    # inference through the module reads the stacked storage
    pred = ens.predict_batch(x)
    with torch.no_grad():
        for m in range(3):
            assert torch.equal(models[m](x[m]).argmax(1), pred[m]), m


def test_engine_refuses_training_batches_above_64_rows_and_evaluates_them():
    from decode_tonal_langauge_amd._classifier_ensemble_engine import ClassifierEnsembleEngine
    from decode_tonal_langauge_amd._simple_classifier_engine import SimpleClassifierEngine
    models = _member_models(3, "relu")
    singles = [SimpleClassifierEngine(copy.deepcopy(m), 0.01, 0.0) for m in models]
    ens = ClassifierEnsembleEngine(models, 0.01, 0.0)
    before = copy.deepcopy([m.state_dict() for m in models])
    g = _gen(5)
    x = torch.randn(3, 65, 12, generator=g).to(DEV)
    y = torch.randint(0, 3, (3, 65), generator=g).to(DEV)
    with pytest.raises(ValueError, match=r"65 rows.*at most 64 rows"):
        ens.train_batch(x, y)
    ens.force_dense = True
    with pytest.raises(ValueError, match="no dense route.*at most 64 rows"):
        ens.train_batch(x[:, :8], y[:, :8])
    ens.force_dense = False
    for sd, m in zip(before, models):                          # a refused step changed nothing
        assert all(torch.equal(sd[k], v) for k, v in m.state_dict().items())
    ens.eval_batch(x, y)                                       # evaluation and prediction take any batch size
    pred = ens.predict_batch(x)
    stats = ens.epoch_stats()
    for m, s in enumerate(singles):
        s.eval_batch(x[m], y[m])
        loss, count, cm = s.epoch_stats()
        assert stats[m][0] == loss and stats[m][1] == count == 65 and torch.equal(stats[m][2], cm), m
        assert torch.equal(pred[m], s.predict_batch(x[m])), m


def test_engine_mask_freezes_a_member():
    from decode_tonal_langauge_amd._classifier_ensemble_engine import ClassifierEnsembleEngine
    from decode_tonal_langauge_amd._simple_classifier_engine import SimpleClassifierEngine
    models = _member_models(3, "lrelu")
    singles = [SimpleClassifierEngine(copy.deepcopy(m), 0.01, 0.02) for m in models]
    ens = ClassifierEnsembleEngine(models, 0.01, 0.02)
    g = _gen(2)
    batches = [(torch.randn(3, B, 16, generator=g).to(DEV), torch.randint(0, 3, (3, B), generator=g).to(DEV))
               for B in (8, 8, 8, 5, 64)]
    for x, y in batches[:2]:
        ens.train_batch(x, y)
    frozen = copy.deepcopy(models[1].state_dict())
    frozen_moments = {k: (a.clone(), b.clone()) for k, (a, b) in ens.moments(1).items()}
    ens.set_active([True, False, True])
    for x, y in batches[2:]:
        ens.train_batch(x, y)
    stats = ens.epoch_stats()
    for m, s in enumerate(singles):
        for x, y in batches[:2] if m == 1 else batches:
            s.train_batch(x[m], y[m])
        _assert_member_equals_single(ens, models, m, s)
        assert stats[m][:2] == s.epoch_stats()[:2], m
    assert all(torch.equal(frozen[k], v) for k, v in models[1].state_dict().items())
    for k, (a, b) in frozen_moments.items():
        assert torch.equal(ens.moments(1)[k][0], a) and torch.equal(ens.moments(1)[k][1], b), k
        assert a.any() and b.any()                             # (two steps had been taken)


# ---------------------------------------------------------------------------------------------- trainer
# a float32 autograd loop on the CPU stops these seeds after epochs 3, 1 and 4, val/loss turning by more than 25 % each time
SEEDS, LR, WD = (3, 11, 1), 0.05, 0.01


def _planted():
    g = _gen(1)
    y = torch.randint(0, 3, (53,), generator=g)
    x = torch.randn(53, 2, 6, generator=g)
    for k in range(3):
        x.view(53, 12)[y == k, 4 * k:4 * k + 4] += 1.0
    return TensorDataset(x, y.float())


def _prologue(dataset, seed):
    from decode_tonal_langauge_amd.data_loading.dataloaders import split_dataset
    from decode_tonal_langauge_amd.models.simple_classifiers import ShallowNNClassifier
    from decode_tonal_langauge_amd.utils.utils import set_seeds
    set_seeds(seed)
    loaders = split_dataset(dataset, [0.7, 0.1, 0.2], [True, False, False], batch_size=8, seed=seed, resident=True, device=DEV)
    list(loaders[2])                                           # the pipeline's `true` pass draws before the model is built
    return loaders, ShallowNNClassifier(12, 3, 8).to(DEV), torch.get_rng_state()


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


def test_trainer_refuses_training_loaders_above_64_rows_before_the_first_epoch():
    from decode_tonal_langauge_amd.data_loading.dataloaders import split_dataset
    from decode_tonal_langauge_amd.data_loading.resident import ResidentDataset
    from decode_tonal_langauge_amd.models.classifier_ensemble_trainer import ClassifierEnsembleTrainer
    rds = ResidentDataset.from_tensor_dataset(_planted(), device=DEV)
    models = _member_models(2, "relu")
    before = copy.deepcopy([m.state_dict() for m in models])
    loaders = [split_dataset(rds, [0.7, 0.1, 0.2], [True, False, False], batch_size=65, seed=s, resident=True, device=DEV)
               for s in (1, 2)]
    ens = ClassifierEnsembleTrainer(models, LR, WD)
    state = torch.get_rng_state()
    with pytest.raises(ValueError, match="65 rows.*at most 64 rows"):
        ens.fit([lo[0] for lo in loaders], [lo[1] for lo in loaders], max_epochs=2, patience=1)
    assert ens.history == [[], []] and torch.equal(torch.get_rng_state(), state)   # nothing was drawn, nothing trained
    for sd, m in zip(before, models):
        assert all(torch.equal(sd[k], v) for k, v in m.state_dict().items())


# ---------------------------------------------------------------------------------------------- pipeline
def _run_pipeline(tmp_path, monkeypatch, tag, separate, ensemble, batch_size=16):
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
              "training": {"train_ratio": 0.7, "vali_ratio": 0.1, "test_ratio": 0.2, "batch_size": batch_size, "epochs": 4,
                           "lr": 0.05, "patience": 1, "weight_decay": 0.01, "log_every_n_steps": 10}}
    if ensemble is not None:
        params["ensemble"] = ensemble
    config = {"model": {"model": "models.simple_classifiers.ShallowNNClassifier", "model_name": "shallow",
                        "model_kwargs": {"hidden_dim": 40}},
              "dataset": {"class_labels": {"tone": None, "syllable": ["i", "a"]}},
              "training": {"module": "train_classifier", "params": params},
              "evaluation": {"metrics": ["accuracy", "f1_score", "confusion_matrix"], "aggregates": ["mean", "std"]}}
    try:
        log_dir = train_classifier.run(config)
    finally:
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
            assert list(sa) == list(sb) == ["hidden.weight", "hidden.bias", "output.weight", "output.bias"], f
            assert all(torch.equal(sa[k], sb[k]) for k in sa), f
        elif f.endswith(".csv") and os.path.basename(f) != "results.csv":
            assert filecmp.cmp(a, b, shallow=False), f
    assert pd.read_csv(os.path.join(on_dir, "results.csv")).equals(pd.read_csv(os.path.join(off_dir, "results.csv")))


def test_pipeline_refuses_a_batch_size_above_64_before_training_starts(tmp_path, monkeypatch):
    with pytest.raises(ValueError, match="128 rows.*at most 64 rows"):
        _run_pipeline(tmp_path, monkeypatch, "big", False, True, batch_size=128)
    assert not any(f.endswith("metrics.csv") or f.endswith(".pt") for f in _files(str(tmp_path / "logs_big")))
