"""What the two GPU modules of the classifier ensemble share: the member kinds (``logistic``, ``relu``, ``lrelu``) with the batch
sequences, seeds and learning rates each is tested at, the canary / mask helpers of the kernel tests, the planted dataset, a
seed's prologue, the pipeline run with its comparisons - and the bodies of the engine, mask, trainer and pipeline tests, which are
one test per member kind.  A plain module: nothing here touches the device until it is called."""
import copy
import filecmp
import os
import sys

import numpy as np
import pytest
import torch
from torch.utils.data import TensorDataset

DEV = "cuda"
CANARY = -777.25
MASKS = {1: [None], 3: [None, (1, 0, 1)]}
CASES = [(M, mask) for M in (1, 3) for mask in MASKS[M]]
IDS = [f"M{M}" + ("" if mask is None else "_masked") for M, mask in CASES]

# kind -> the engine tests' model (input_dim, n_classes[, hidden_dim, activation]) and the trainer tests' model for the 12
# features of the planted dataset; its parameters; the sequences of training batch sizes (the logistic ones cross the rank-64
# limit: low-rank, dense, dense then low-rank; shallow members stay at or below it); the trainer's seeds, learning rate and
# weight decay; the pipeline's model section
_SHALLOW = dict(names=["hidden.bias", "hidden.weight", "output.bias", "output.weight"], sizes=[(8, 8), (64, 19), (1,)],
                seeds=(3, 11, 1), lr=0.05, wd=0.01)
KINDS = {
    "logistic": dict(model=(12, 3), planted=(12, 3), names=["linear.bias", "linear.weight"], sizes=[(8, 8), (65, 65), (65, 19)],
                     seeds=(3, 11, 42), lr=0.1, wd=0.01,
                     config={"model": "models.simple_classifiers.LogisticRegressionClassifier", "model_name": "logistic",
                             "model_kwargs": {}}),
    "relu": dict(model=(12, 3, 8, "ReLU"), planted=(12, 3, 8, "ReLU"), **_SHALLOW,
                 config={"model": "models.simple_classifiers.ShallowNNClassifier", "model_name": "shallow",
                         "model_kwargs": {"hidden_dim": 40, "activation": "ReLU"}}),
    "lrelu": dict(model=(16, 3, 20, "LeakyReLU"), planted=(12, 3, 8, "LeakyReLU"), **_SHALLOW,
                  config={"model": "models.simple_classifiers.ShallowNNClassifier", "model_name": "shallow",
                          "model_kwargs": {"hidden_dim": 40, "activation": "LeakyReLU"}}),
}


def r4(n):
    return (n + 3) // 4 * 4


def lib():
    from decode_tonal_langauge_amd import _lib as L
    return L, L.load()


def stream():
    return torch.cuda.current_stream().cuda_stream


def mask_words(mask):
    return None if mask is None else torch.tensor(mask, dtype=torch.int32, device=DEV)


def on(mask, m):
    return mask is None or bool(mask[m])


def canary(*shape, dtype=torch.float32):
    return torch.full(shape, CANARY if dtype.is_floating_point else -7, dtype=dtype, device=DEV)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def build_model(kind, which="model"):
    """The kind's engine-test model (``model``) or its model for the planted dataset (``planted``), on the device."""
    from decode_tonal_langauge_amd.models.simple_classifiers import LogisticRegressionClassifier, ShallowNNClassifier
    return (LogisticRegressionClassifier if kind == "logistic" else ShallowNNClassifier)(*KINDS[kind][which]).to(DEV)


def member_models(n, kind):
    out = []
    for m in range(n):
        torch.manual_seed(100 + m)
        out.append(build_model(kind))
    return out


def moments(eng):
    return {k: (eng.optimizer.state[p]["exp_avg"], eng.optimizer.state[p]["exp_avg_sq"]) for k, p in eng.params.items()}


def assert_member_equals_single(kind, ens, models, m, single):
    sd = models[m].state_dict()
    assert list(sd) == list(single.model.state_dict())
    for k, v in single.model.state_dict().items():
        assert torch.equal(sd[k], v), (m, k)
    mom = moments(single)
    assert sorted(mom) == sorted(ens.moments(m)) == KINDS[kind]["names"]
    for k, (ma, va) in mom.items():
        assert torch.equal(ens.moments(m)[k][0], ma) and torch.equal(ens.moments(m)[k][1], va), (m, k)


def planted():
    """53 samples of 12 features, three classes, each class shifted in four features of its own."""
    g = gen(1)
    y = torch.randint(0, 3, (53,), generator=g)
    x = torch.randn(53, 2, 6, generator=g)
    for k in range(3):
        x.view(53, 12)[y == k, 4 * k:4 * k + 4] += 1.0
    return TensorDataset(x, y.float())


def prologue(dataset, seed, kind):
    """What the pipeline does for a seed before its trainer exists: (loaders, model on the planted dataset's 12 features,
    generator state)."""
    from decode_tonal_langauge_amd.data_loading.dataloaders import split_dataset
    from decode_tonal_langauge_amd.utils.utils import set_seeds
    set_seeds(seed)
    loaders = split_dataset(dataset, [0.7, 0.1, 0.2], [True, False, False], batch_size=8, seed=seed, resident=True, device=DEV)
    list(loaders[2])                                           # the pipeline's `true` pass draws before the model is built
    return loaders, build_model(kind, "planted"), torch.get_rng_state()


def run_pipeline(tmp_path, monkeypatch, tag, kind, separate, ensemble, batch_size=16):
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
    config = {"model": KINDS[kind]["config"],
              "dataset": {"class_labels": {"tone": None, "syllable": ["i", "a"]}},
              "training": {"module": "train_classifier", "params": params},
              "evaluation": {"metrics": ["accuracy", "f1_score", "confusion_matrix"], "aggregates": ["mean", "std"]}}
    try:
        log_dir = train_classifier.run(config)
    finally:
        monkeypatch.undo()
    return log_dir, got["out"], torch.get_rng_state()


def same(a, b, where=""):
    if isinstance(a, dict):
        assert isinstance(b, dict) and list(a) == list(b), where
        for k in a:
            same(a[k], b[k], f"{where}/{k}")
    elif isinstance(a, np.ndarray):
        assert np.array_equal(a, b), where
    elif isinstance(a, (list, tuple)) and a and isinstance(a[0], (dict, np.ndarray)):
        assert len(a) == len(b), where
        for i, (x, y) in enumerate(zip(a, b)):
            same(x, y, f"{where}/{i}")
    else:
        assert a == b or (a is None and b is None), (where, a, b)


def files(log_dir):
    out = []
    for base, _dirs, names in os.walk(log_dir):
        out += [os.path.relpath(os.path.join(base, n), log_dir) for n in names]
    return sorted(out)


# ---------------------------------------------------------------------------------------------- the tests of a member kind
# All comparisons are exact.  The trainer's seeds and learning rates stop the members at different epochs (a float32 autograd
# loop on the CPU stops the logistic seeds after epochs 3, 2 and 1 with val/loss turning by more than 4 %, the shallow ones -
# ReLU and LeakyReLU alike - after epochs 3, 1 and 4 with more than 20 %), so the group runs on with members masked out.
def engines(kind, weight_decay):
    from decode_tonal_langauge_amd._classifier_ensemble_engine import ClassifierEnsembleEngine
    from decode_tonal_langauge_amd._simple_classifier_engine import SimpleClassifierEngine
    models = member_models(3, kind)
    singles = [SimpleClassifierEngine(copy.deepcopy(m), 0.01, weight_decay) for m in models]
    return models, singles, ClassifierEnsembleEngine(models, 0.01, weight_decay)


def engine_steps_equal_the_single_engine(kind, sizes):
    """``sizes`` training batches, then a warm evaluation and training step that may not read the device: every member
    equals its ``SimpleClassifierEngine`` in parameters, moments, statistics and predictions."""
    K = KINDS[kind]["model"][0]
    models, singles, ens = engines(kind, 0.02)
    for a, s in zip(models, singles):                          # the views hold the values
        assert all(torch.equal(v, s.model.state_dict()[k]) for k, v in a.state_dict().items())
    g = gen(9)
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
        assert_member_equals_single(kind, ens, models, m, s)
        loss, count, cm = s.epoch_stats()
        assert stats[m][0] == loss and stats[m][1] == count == sum(sizes) + 2 * sizes[-1] and torch.equal(stats[m][2], cm), m
    for name in KINDS[kind]["names"]:
        if name.endswith(".weight"):
            assert len({float(m.state_dict()[name].sum()) for m in models}) == 3, name
    # inference through the module reads the stacked storage
    pred = ens.predict_batch(x)
    with torch.no_grad():
        for m in range(3):
            assert torch.equal(models[m](x[m]).argmax(1), pred[m]), m


def engine_mask_freezes_a_member(kind):
    """Logistic members also cross to the dense route while one is masked; the group names the member with a bad label."""
    K = KINDS[kind]["model"][0]
    sizes, before, wd = ((8, 65, 8), 1, 0.0) if kind == "logistic" else ((8, 8, 8, 5, 64), 2, 0.02)
    models, singles, ens = engines(kind, wd)
    g = gen(2)
    batches = [(torch.randn(3, B, K, generator=g).to(DEV), torch.randint(0, 3, (3, B), generator=g).to(DEV)) for B in sizes]
    for x, y in batches[:before]:
        ens.train_batch(x, y)
    frozen = copy.deepcopy(models[1].state_dict())
    frozen_moments = {k: (a.clone(), b.clone()) for k, (a, b) in ens.moments(1).items()}
    ens.set_active([True, False, True])
    for x, y in batches[before:]:
        ens.train_batch(x, y)
    stats = ens.epoch_stats()
    for m, s in enumerate(singles):
        for x, y in batches[:before] if m == 1 else batches:
            s.train_batch(x[m], y[m])
        assert_member_equals_single(kind, ens, models, m, s)
        assert stats[m][:2] == s.epoch_stats()[:2], m
    assert all(torch.equal(frozen[k], v) for k, v in models[1].state_dict().items())
    for k, (a, b) in frozen_moments.items():
        assert torch.equal(ens.moments(1)[k][0], a) and torch.equal(ens.moments(1)[k][1], b), k
        assert a.any() and b.any()                             # (steps had been taken)
    if kind == "logistic":
        ens.set_active([True] * 3)
        x, y = batches[0][0], batches[0][1].clone()
        y[2, 3] = 3
        ens.eval_batch(x, y)
        with pytest.raises(ValueError, match=r"\[0, 3\).*member 2"):
            ens.epoch_stats()
        with pytest.raises(ValueError, match="expected input"):
            ens.train_batch(x[:2], y[:2])


def trainer_equals_sequential_fused_runs(tmp_path, kind):
    from decode_tonal_langauge_amd.data_loading.resident import ResidentDataset
    from decode_tonal_langauge_amd.models.classifier_ensemble_trainer import ClassifierEnsembleTrainer
    from decode_tonal_langauge_amd.models.classifier_trainer import ClassifierTrainer
    seeds, lr, wd = (KINDS[kind][k] for k in ("seeds", "lr", "wd"))
    tds = planted()
    seq = []
    for seed in seeds:
        loaders, model, state = prologue(tds, seed, kind)
        assert len(loaders[0]) == 5 and len(loaders[0].sampler.indices) == 37  # four full batches and a ragged one
        tr = ClassifierTrainer(model, lr, wd, log_dir=str(tmp_path / f"seq_{seed}"), fused=True)
        hist = tr.fit(loaders[0], loaders[1], max_epochs=6, patience=1)
        seq.append(dict(hist=hist, stopped=tr.stopped_epoch, test=tr.test(loaders[2]), pred=tr.predict(loaders[2]),
                        sd=copy.deepcopy(model.state_dict()), entered=state))
    final = torch.get_rng_state()
    print("stopped_epoch of the sequential runs:", [s["stopped"] for s in seq])
    assert len({s["stopped"] for s in seq}) > 1                # the masked path is exercised

    rds = ResidentDataset.from_tensor_dataset(tds, device=DEV)
    torch.manual_seed(777)
    pro = [prologue(rds, seed, kind) for seed in seeds]
    assert all(torch.equal(p[2], s["entered"]) for p, s in zip(pro, seq))
    torch.manual_seed(778)                                     # the trainer works from the states it is given
    dirs = [str(tmp_path / f"ens_{seed}") for seed in seeds]
    ens = ClassifierEnsembleTrainer([p[1] for p in pro], lr, wd, log_dirs=dirs, rng_states=[p[2] for p in pro])
    hists = ens.fit([p[0][0] for p in pro], [p[0][1] for p in pro], max_epochs=6, patience=1)
    tests = ens.test([p[0][2] for p in pro])
    preds = ens.predict([p[0][2] for p in pro])
    assert torch.equal(torch.get_rng_state(), final)
    for m, (seed, s) in enumerate(zip(seeds, seq)):
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
    assert torch.equal(ens.rng_state(len(seeds) - 1), final)
    with pytest.raises(RuntimeError, match="runs once"):
        ens.fit([p[0][0] for p in pro], [p[0][1] for p in pro], max_epochs=1, patience=1)


def pipeline_with_the_key_equals_the_sequential_pipeline(tmp_path, monkeypatch, kind, separate):
    import pandas as pd
    mods = ("decode_tonal_langauge_amd._classifier_ensemble_engine", "decode_tonal_langauge_amd.models.classifier_ensemble_trainer")
    kept = {k: sys.modules.pop(k) for k in mods if k in sys.modules}
    try:
        off_dir, off, off_state = run_pipeline(tmp_path, monkeypatch, "off", kind, separate, None)
        assert not any(k in sys.modules for k in mods)         # without the key nothing of the ensemble is imported
    finally:
        sys.modules.update(kept)
    on_dir, got, on_state = run_pipeline(tmp_path, monkeypatch, "on", kind, separate, True)
    assert all(k in sys.modules for k in mods) and on_dir != off_dir
    assert torch.equal(on_state, off_state)
    same(got[0], off[0], "result_info")
    assert np.array_equal(got[1], off[1]) and list(got[2]) == list(off[2])
    assert int(got[1].sum()) == 3 * 48                         # 3 seeds x 20 % of 240
    listing = files(on_dir)
    assert listing == files(off_dir) and sum(f.endswith(".pt") for f in listing) == (6 if separate else 3)
    assert sum(f.endswith("metrics.csv") for f in listing) == (6 if separate else 3)
    names = {"logistic": ["linear.weight", "linear.bias"]}.get(kind, ["hidden.weight", "hidden.bias", "output.weight", "output.bias"])
    for f in listing:
        a, b = os.path.join(on_dir, f), os.path.join(off_dir, f)
        if f.endswith(".pt"):
            sa, sb = torch.load(a), torch.load(b)
            assert list(sa) == list(sb) == names, f
            assert all(torch.equal(sa[k], sb[k]) for k in sa), f
        elif f.endswith(".csv") and os.path.basename(f) != "results.csv":
            assert filecmp.cmp(a, b, shallow=False), f
    assert pd.read_csv(os.path.join(on_dir, "results.csv")).equals(pd.read_csv(os.path.join(off_dir, "results.csv")))
