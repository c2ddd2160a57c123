"""GPU: training ``CNNClassifier`` on the HIP path - ``tl_ce_scores_loss``, ``CnnClassifierTrainEngine``,
``ClassifierTrainer(fused=True)`` and the pipeline key.

How the bounds are formed.  The reference of every comparison is torch on the CPU in float64.
  * the loss kernel and the optimiser routing: 10 yardsticks, a yardstick being the distance (``rel_l2``) of the float32 CPU
    evaluation of the same thing from the float64 one, computed in the test (tests/test_gpu_classifier_train.py);
  * one step's gradients: the arg-max / sign planes HIP took are first held to the float64 reference's own decisions by
    ``branch_planes.check_flips`` (tau 1e-4, max_frac 1e-4, slack 4: a branch may differ only at a near-tie, and only a few
    may), then every parameter gradient is within 5e-5 relative L2 of the float64 restatement run on HIP's planes and keep
    mask (the bound tests/test_gpu_parity.py holds the conv-stack gradients to once branches are shared); scores within 2e-5
    absolute (tests/test_gpu_pipeline.py's bound for this model's HIP forward); the loss sum within 2 B 2e-5 (CE is 2-Lipschitz
    in the sup norm of its input).
Integer results are compared exactly.  Every figure is printed and recorded before it is asserted."""
import copy
import functools
import os

import pytest
import torch
import torch.nn.functional as F

from tests import branch_planes, parity_record
from tests import classifier_train_ref as ref
from tests import cnn_classifier_ref as cref

pytestmark = pytest.mark.gpu
DEV = "cuda"
_REC = {}


def _note(section, values):
    _REC.setdefault(section, {}).update(values)
    parity_record.record("cnn_classifier_train_" + section, _REC[section])


def _held(section, name, dev, yard):
    """Print and record one figure; returns whether it is within 10 yardsticks."""
    bound = ref.FACTOR * yard
    print(f"[{section}] {name}: gpu {dev:.3e}  yardstick {yard:.3e}  bound {bound:.3e}")
    _note(section, {name + "_gpu": dev, name + "_bound": bound})
    return dev <= bound


def _within(section, name, dev, bound):
    print(f"[{section}] {name}: gpu {dev:.3e}  bound {bound:.3e}")
    _note(section, {name: dev})
    return dev <= bound


def _r4(n):
    return (n + 3) // 4 * 4


# ---------------------------------------------------------------------------------------------- 1. tl_ce_scores_loss
class _CeOut:
    def __init__(self, B, N):
        self.dl = torch.full((B, _r4(N)), float("nan"), device=DEV)
        self.db = torch.full((N,), float("nan"), device=DEV)
        self.pred = torch.full((B,), -1, dtype=torch.int64, device=DEV)
        self.loss = torch.zeros(1, dtype=torch.float64, device=DEV)
        self.count = torch.zeros(1, dtype=torch.int64, device=DEV)
        self.cm = torch.zeros(N, N, dtype=torch.int64, device=DEV)
        self.err = torch.zeros(1, dtype=torch.int32, device=DEV)


def _ce(buf, labels, out, B, N, grads=True):
    from decode_tonal_langauge_amd import _lib as L
    L.check(L.load().tl_ce_scores_loss(buf.data_ptr(), labels.data_ptr(), out.dl.data_ptr() if grads else None,
                                       out.db.data_ptr(), out.pred.data_ptr(), out.loss.data_ptr(), out.count.data_ptr(),
                                       out.cm.data_ptr(), out.err.data_ptr(), B, N, buf.stride(0), out.dl.stride(0), 1.0 / B,
                                       torch.cuda.current_stream().cuda_stream), "tl_ce_scores_loss")
    torch.cuda.synchronize()


def _ce_reference(s, labels, dtype):
    """(dz, loss sum) of CE on the scores by autograd, the float32 scores cast to ``dtype`` as the leaf; dz = ds s (1 - s)."""
    leaf = s.to(dtype).requires_grad_(True)
    loss = F.cross_entropy(leaf, labels, reduction="sum")
    ds, = torch.autograd.grad(loss / len(labels), leaf)
    sd = leaf.detach()
    return ds * sd * (1 - sd), loss.detach()


@pytest.mark.parametrize("B", [1, 7, 64, 65, 300])
@pytest.mark.parametrize("N", [2, 3, 5, 64])
def test_ce_scores_loss_matches_float64_and_counts_exactly(N, B):
    g = torch.Generator().manual_seed(2000 * N + B)
    s = torch.sigmoid(3.0 * torch.randn(B, N, generator=g))
    c1, c2 = (N // 2 if N > 2 else 0), N - 1
    s[0, c1] = s[0, c2] = 1.0 if B == 1 else (1.0 + float(s[0].max())) / 2               # two equal maxima: the first one wins
    sat = (0, 0) if N > 2 else None                                                        # a row holding 1.0f and 0.0f
    if B > 1:
        sat = (B - 1, 1)
        s[B - 1, 0] = 1.0
    if sat is not None:
        s[sat] = 0.0
    labels = torch.randint(0, N, (B,), generator=g)
    dz64, loss64 = _ce_reference(s, labels, torch.float64)
    dz32, loss32 = _ce_reference(s, labels, torch.float32)
    pred_ref = s.argmax(1)
    assert int(pred_ref[0]) == c1
    cm_ref = torch.bincount(labels * N + pred_ref, minlength=N * N).reshape(N, N)

    buf = torch.zeros(B, N + B % 2, device=DEV)               # odd batches: a row stride above N
    buf[:, :N] = s.to(DEV)
    lab = labels.to(DEV)
    out = _CeOut(B, N)
    _ce(buf, lab, out, B, N)
    tag = f"N{N}_B{B}"
    ok = [_held("ce", tag + "_dz", ref.rel_l2(out.dl[:, :N], dz64), ref.rel_l2(dz32, dz64)),
          _held("ce", tag + "_dbias", ref.rel_l2(out.db, dz64.sum(0)), ref.rel_l2(dz32.sum(0), dz64.sum(0))),
          _held("ce", tag + "_loss_sum", ref.rel_l2(out.loss, loss64), ref.rel_l2(loss32, loss64))]
    assert all(ok), tag
    assert bool((out.dl[:, N:] == 0).all())                                                # the pad columns are zeros
    assert bool((out.dl[:, :N].cpu()[(s == 1.0) | (s == 0.0)] == 0).all())                 # saturated scores: dz == 0
    assert torch.equal(out.pred.cpu(), pred_ref) and torch.equal(out.cm.cpu(), cm_ref)
    assert int(out.count) == B and int(out.err) == 0
    first = (out.dl.clone(), out.db.clone(), out.loss.clone())
    _ce(buf, lab, out, B, N)                                                               # a second call accumulates
    assert float(out.loss) == 2 * float(first[2]) and int(out.count) == 2 * B and torch.equal(out.cm.cpu(), 2 * cm_ref)
    again = _CeOut(B, N)                                                                   # two runs: the same bits
    _ce(buf, lab, again, B, N)
    assert torch.equal(again.dl, first[0]) and torch.equal(again.db, first[1]) and torch.equal(again.loss, first[2])
    bare = _CeOut(B, N)                                                                    # without dlogits: the same statistics
    _ce(buf, lab, bare, B, N, grads=False)
    assert torch.equal(bare.db, first[1]) and torch.equal(bare.loss, first[2]) and torch.equal(bare.cm.cpu(), cm_ref)
    assert torch.equal(bare.pred, out.pred) and bool(torch.isnan(bare.dl).all())
    bad = lab.clone()                                                                      # a label of N: flagged, not counted
    bad[B // 2] = N
    flagged = _CeOut(B, N)
    _ce(buf, bad, flagged, B, N)
    keep = torch.arange(B) != B // 2
    cm_keep = torch.bincount(labels[keep] * N + pred_ref[keep], minlength=N * N).reshape(N, N)
    assert int(flagged.err) == 1 and int(flagged.count) == B - 1 and torch.equal(flagged.cm.cpu(), cm_keep)
    assert bool((flagged.dl[B // 2] == 0).all())


# ---------------------------------------------------------------------------------------------- the engine
def _engine(model, lr=0.0005, wd=0.0):
    from decode_tonal_langauge_amd._cnn_classifier_train_engine import CnnClassifierTrainEngine
    return CnnClassifierTrainEngine(copy.deepcopy(model).to(DEV), lr, wd)


def _dense(g):
    """A gradient from the engine's hook on the host: a low-rank one as fa^T . fb."""
    if isinstance(g, tuple):
        return (g[0].double().t() @ g[1].double()).float().cpu()
    return g.detach().clone().cpu()


@functools.lru_cache(maxsize=None)
def _own64_plain(shape, seed):
    return _own64(shape, seed, None, cached=False)


def _own64(shape, seed, keep, cached=True):
    """The float64 reference's own decisions and their margins (without dropout: computed once per shape)."""
    if keep is None and cached:
        return _own64_plain(shape, seed)
    model, x, _ = cref.build(shape, seed)
    own, margins = {}, {}
    with torch.no_grad():
        cref.forward(model, cref.leaves(model, torch.float64), x, keep=keep, own=own, margins=margins)
    return own, margins


# ---------------------------------------------------------------------------------------------- 2. one step's gradients
@pytest.mark.parametrize("wino", ["6", "4", "0"])
@pytest.mark.parametrize("dropout", [0.0, 0.5])
@pytest.mark.parametrize("shape,seed", cref.SHAPES[:3])
def test_one_step_gradients_on_shared_branches(shape, seed, dropout, wino, monkeypatch):
    monkeypatch.setenv("TONAL_KERNELS", f"wino={wino}")
    B = shape[0]
    model, x, y = cref.build(shape, seed, dropout)
    eng = _engine(model)
    eng.model.train()
    got = {k: _dense(g) for k, g in eng.backward_only(x.to(DEV), y.to(DEV)).items()}
    torch.cuda.synchronize()
    scores = eng.scores(B).cpu()
    planes = cref.hip_planes(eng, B)
    keep = cref.hip_keep_mask(eng, B)
    assert (keep is not None) == (dropout > 0)
    if keep is not None:
        frac = float(keep.float().mean())
        assert abs(frac - (1 - dropout)) < 0.05, frac
    loss_sum, count, _ = eng.epoch_stats()
    assert count == B

    # the planes are not trusted: held to the reference's own decisions (taken behind HIP's keep mask where dropout ran, so that
    # fc1's are decisions about the same input)
    own, margins = _own64(shape, seed, keep)
    tag = f"B{B}C{shape[1]}T{shape[2]}n{shape[3]}_p{dropout}_wino{wino}"
    flips = branch_planes.check_flips(planes, own, margins)
    assert set(flips) == set(own) and len(flips) == 12
    _note("flips", {f"{tag}.{k}": v for k, v in branch_planes.flip_record(flips).items()})
    print(f"[flips] {tag}: {sum(v[0] for v in flips.values())} branches differ")

    s64, loss64, g64 = cref.loss_and_grads(model, cref.leaves(model, torch.float64), x, y, planes=planes, keep=keep)
    assert set(got) == set(g64)
    ok = [_within("gradients", f"{tag}.{k}", ref.rel_l2(got[k], g64[k]), 5e-5) for k in sorted(g64)]
    ok.append(_within("gradients", f"{tag}.scores_abs", float((scores.double() - s64).abs().max()), 2e-5))
    ok.append(_within("gradients", f"{tag}.loss_sum_abs", abs(loss_sum - float(loss64) * B), 2 * B * 2e-5))
    assert all(ok), tag


# ---------------------------------------------------------------------------------------------- 3. update routing, 4. statistics
def _nadam_twin(named, lr, wd, dtype):
    params = {k: v.detach().cpu().to(dtype).clone().requires_grad_(True) for k, v in named}
    decay = [p for p in params.values() if p.ndim >= 2]
    rest = [p for p in params.values() if p.ndim < 2]
    opt = torch.optim.NAdam([{"params": decay, "weight_decay": wd}, {"params": rest, "weight_decay": 0.0}], lr=lr)
    return params, opt


@pytest.mark.parametrize("mode", ["lowrank", "force_dense", "dense_B65"])
def test_update_routing_and_statistics(mode):
    lr, wd = 5e-3, 0.01
    shape, sizes = ((65, 2, 150, 3), [65]) if mode == "dense_B65" else ((4, 2, 150, 3), [4, 4, 4, 3])
    model, _, _ = cref.build(shape, 7)
    eng = _engine(model, lr, wd)
    eng.force_dense = mode == "force_dense"
    eng.model.train()
    g = torch.Generator().manual_seed(31)
    named = list(eng.model.named_parameters())
    p64, opt64 = _nadam_twin(named, lr, wd, torch.float64)
    p32, opt32 = _nadam_twin(named, lr, wd, torch.float32)
    ok, labels, preds = [], [], []
    for step, B in enumerate(sizes):
        x, y = torch.randn(B, shape[1], shape[2], generator=g), torch.randint(0, shape[3], (B,), generator=g)
        before = {k: v.detach().cpu().clone() for k, v in named}
        eng.train_batch(x.to(DEV), y.to(DEV))
        torch.cuda.synchronize()
        hooked = eng.step_gradients()
        lin = [k for k, v in hooked.items() if isinstance(v, tuple)]
        assert sorted(lin) == ([] if mode != "lowrank" else ["classifier.1.weight", "classifier.3.weight"])
        grads = {k: _dense(v) for k, v in hooked.items()}
        assert set(grads) == set(p64)
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
            ok.append(_held("update", f"{mode}_step{step}_{k}", ref.rel_l2(v.detach().cpu() - before[k], want), yard))
    assert all(ok), mode
    loss_sum, count, cm = eng.epoch_stats()
    y_all, p_all, n = torch.cat(labels), torch.cat(preds), shape[3]
    assert count == sum(sizes) and torch.equal(cm, torch.bincount(y_all * n + p_all, minlength=n * n).reshape(n, n))
    assert loss_sum > 0 and eng.epoch_stats()[1] == 0                                      # reading zeroes the statistics
    bad = y.clone()
    bad[0] = n
    eng.eval_batch(x.to(DEV), bad.to(DEV))
    with pytest.raises(ValueError, match=rf"\[0, {n}\)"):
        eng.epoch_stats()


# ---------------------------------------------------------------------------------------------- 5. no host synchronisation
def test_train_and_eval_batch_never_read_the_device():
    for B in (4, 65):
        model, x, y = cref.build((B, 2, 150, 3), 9)
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


# ---------------------------------------------------------------------------------------------- 6. no stale packs
def test_inference_after_fused_training_uses_the_updated_weights():
    model, x, y = cref.build((4, 2, 150, 3), 11)
    eng = _engine(model, 5e-4, 0.01)                # (a step that leaves the scores unsaturated: a wrong weight shows)
    gpu = eng.model
    xd = x.to(DEV)
    gpu.eval()
    with torch.no_grad():
        stale = gpu(xd).cpu()                           # the inference engine packs (and caches) the weights as they are now
    gpu.train()
    for _ in range(2):
        eng.train_batch(xd, y.to(DEV))
    gpu.eval()
    with torch.no_grad():
        s = gpu(xd).cpu()
        want = cref.forward(gpu, cref.leaves(gpu, torch.float64), x)
    moved = float((stale.double() - want).abs().max())
    dev = float((s.double() - want).abs().max())
    print(f"[stale_packs] scores moved by {moved:.3e} in two steps; model(x) is {dev:.3e} from the updated float64 scores")
    _note("stale_packs", {"moved": moved, "dev": dev})
    assert moved > 2e-4                                 # the counter-example: stale packs would sit this far away
    assert dev <= 2e-5
    assert torch.equal(eng.predict_batch(xd).cpu(), s.argmax(1))


@pytest.mark.parametrize("kind", ["cnn", "cnnrnn"])
def test_a_direct_fused_update_reaches_the_inference_packs(kind):
    """``FusedNAdam`` driven directly - no train engine that could tell the inference engines: forward (the packs are built),
    one step, forward again.  The second output is, bit for bit, that of a copy of the updated model with fresh engines and
    fresh packs, and it is not the first one (2e-4: what the tests above take for "moved")."""
    from decode_tonal_langauge_amd.optim import FusedNAdam
    from tests import cnnrnn_classifier_ref as rref
    r = cref if kind == "cnn" else rref
    shape, seed = r.SHAPES[0]
    model, x, _ = r.build(shape, seed)
    model = model.to(DEV).eval()
    xd = x.to(DEV)
    with torch.no_grad():
        first = model(xd).clone()
    engines = {k: v for k, v in vars(model).items() if k.startswith("_hip") and k != "_hip_cfg"}
    assert engines["_hip"] is not None
    g = torch.Generator(device=DEV).manual_seed(seed)
    grads = {p: torch.randn(p.shape, device=DEV, generator=g) * 1e-2 for p in model.parameters()}
    versions = [p._version for p in model.parameters()]
    FusedNAdam(model.parameters()).step(grads=grads)
    assert all(p._version > v for p, v in zip(model.parameters(), versions))
    with torch.no_grad():
        second = model(xd).clone()
    assert all(getattr(model, k) is v for k, v in engines.items())          # the engines (and their caches) of the first pass
    for k in engines:                          # the copy: everything but the engines, which it then makes for itself
        setattr(model, k, None)
    fresh = copy.deepcopy(model)
    with torch.no_grad():
        want = fresh(xd)
    moved = float((second - first).abs().max())
    print(f"[direct_update] {kind}: scores moved by {moved:.3e} in one step")
    assert torch.equal(second, want)
    assert moved > 2e-4


# ---------------------------------------------------------------------------------------------- 7. trainer and pipeline
def test_fused_trainer_fits_a_cnn_classifier(tmp_path):
    from decode_tonal_langauge_amd._cnn_classifier_train_engine import CnnClassifierTrainEngine
    from decode_tonal_langauge_amd.models.classifier_trainer import ClassifierTrainer
    from decode_tonal_langauge_amd.models.deep_classifiers import CNNClassifier
    from decode_tonal_langauge_amd.optim import FusedNAdam
    x, y = ref.planted(24, n_cls=2, channels=4, length=150)
    dev = lambda a, b: ref.batches(a.to(DEV), b.to(DEV), 8)
    torch.manual_seed(3)
    cpu_model = CNNClassifier(4, 150, 2)
    keys = list(ClassifierTrainer(copy.deepcopy(cpu_model)).fit(ref.batches(x[:8], y[:8], 8), ref.batches(x[:8], y[:8], 8),
                                                                max_epochs=1, patience=9)[0])
    gpu_model = copy.deepcopy(cpu_model).to(DEV)
    tr = ClassifierTrainer(gpu_model, 0.005, 0.01, log_dir=str(tmp_path), fused=True)
    assert isinstance(tr.engine, CnnClassifierTrainEngine) and isinstance(tr.optimizer, FusedNAdam)
    assert [g["weight_decay"] for g in tr.optimizer.param_groups] == [0.01, 0.0]
    hist = tr.fit(dev(x, y), dev(x, y), max_epochs=2, patience=99)
    assert len(hist) == 2 and all(list(row) == keys for row in hist)
    assert all(torch.isfinite(torch.tensor(float(v))) for row in hist for v in row.values())
    assert os.path.isfile(tmp_path / "metrics.csv")
    res = tr.test(dev(x, y))
    assert int(res["confusion_matrix"].sum()) == 24
    pred = tr.predict(dev(x, y))
    with torch.no_grad():
        own = torch.cat([gpu_model.eval()(a).argmax(1) for a, _ in dev(x, y)])
    assert torch.equal(pred, own)


def test_pipeline_key_reaches_the_cnn_classifier(tmp_path, monkeypatch):
    import pandas as pd
    from decode_tonal_langauge_amd import _cnn_classifier_train_engine as cte
    from decode_tonal_langauge_amd import train_classifier
    from decode_tonal_langauge_amd.data_loading import synthetic
    written = synthetic.write_dataset(str(tmp_path / "data"), n_samples=48, n_channels=4, n_timepoints=150)
    calls = []
    step = cte.CnnClassifierTrainEngine.train_batch
    monkeypatch.setattr(cte.CnnClassifierTrainEngine, "train_batch", lambda self, x, y: (calls.append(len(y)), step(self, x, y))[1])
    config = {
        "model": {"model": "models.deep_classifiers.CNNClassifier", "model_name": "cnn", "model_kwargs": {}},
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
