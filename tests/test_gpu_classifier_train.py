"""GPU: the fused classifier train step - tl_ce_loss, tl_head_bwd, SimpleClassifierEngine, ClassifierTrainer(fused=True) and
the pipeline key.

How the numeric bounds are formed.  The reference of every comparison is torch on the CPU in float64 (the same modules,
F.cross_entropy, autograd, torch.optim.NAdam with the two decay groups).  The yardstick of a quantity is the distance of the
float32 CPU evaluation of the same thing from that float64 result, as ``rel_l2`` = ||a - ref||_2 / ||ref||_2 (for the
per-epoch losses: the largest relative deviation over the epochs); the GPU is allowed 10 yardsticks, computed inside the
test - room for a third summation order, far below the O(1) of a wrong scale, a missing term or a mis-indexed row.  Integer
results (arg-max, confusion matrix, counts) are compared exactly.  Every figure is printed and recorded before it is asserted."""
import copy
import functools
import os

import pytest
import torch
import torch.nn.functional as F

from tests import classifier_train_ref as ref
from tests import parity_record

pytestmark = pytest.mark.gpu
DEV = "cuda"
_REC = {}


def _held(section, name, dev, yard):
    """Print and record one figure; returns whether it is within 10 yardsticks."""
    bound = ref.FACTOR * yard
    print(f"[{section}] {name}: gpu {dev:.3e}  yardstick {yard:.3e}  bound {bound:.3e}")
    _REC.setdefault(section, {}).update({name + "_gpu": dev, name + "_bound": bound})
    parity_record.record("classifier_train_" + section, _REC[section])
    return dev <= bound


def _r4(n):
    return (n + 3) // 4 * 4


def _lib():
    from decode_tonal_langauge_amd import _lib as L
    return L, L.load()


# ---------------------------------------------------------------------------------------------- tl_ce_loss
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
    L, lib = _lib()
    L.check(lib.tl_ce_loss(buf.data_ptr(), labels.data_ptr(), out.dl.data_ptr() if grads else None, out.db.data_ptr(),
                           out.pred.data_ptr(), out.loss.data_ptr(), out.count.data_ptr(), out.cm.data_ptr(),
                           out.err.data_ptr(), B, N, buf.stride(0), out.dl.stride(0), 1.0 / B,
                           torch.cuda.current_stream().cuda_stream), "tl_ce_loss")
    torch.cuda.synchronize()


@pytest.mark.parametrize("B", [1, 7, 64, 65, 300])
@pytest.mark.parametrize("N", [2, 3, 5, 64])
def test_ce_loss_matches_float64_and_counts_exactly(N, B):
    g = torch.Generator().manual_seed(1000 * N + B)
    logits = 3.0 * torch.randn(B, N, generator=g)
    c1, c2 = (N // 2 if N > 2 else 0), N - 1
    logits[0, c1] = logits[0, c2] = 80.0 if B == 1 else float(logits[0].max()) + 1.0     # two equal maxima: the first one wins
    if B > 1:
        logits[B - 1, 0] = 80.0                                                            # exp(80) overflows float32
    labels = torch.randint(0, N, (B,), generator=g)
    lg64 = logits.double().requires_grad_(True)
    loss64 = F.cross_entropy(lg64, labels, reduction="sum")
    dl64, = torch.autograd.grad(loss64 / B, lg64)
    lg32 = logits.clone().requires_grad_(True)
    loss32 = F.cross_entropy(lg32, labels, reduction="sum")
    dl32, = torch.autograd.grad(loss32 / B, lg32)
    pred_ref = logits.argmax(1)
    cm_ref = torch.bincount(labels * N + pred_ref, minlength=N * N).reshape(N, N)

    buf = torch.zeros(B, N + B % 2, device=DEV)               # odd batches: a row stride above N
    buf[:, :N] = logits.to(DEV)
    lab = labels.to(DEV)
    out = _CeOut(B, N)
    _ce(buf, lab, out, B, N)
    tag = f"N{N}_B{B}"
    ok = [_held("ce", tag + "_dlogits", ref.rel_l2(out.dl[:, :N], dl64), ref.rel_l2(dl32, dl64)),
          _held("ce", tag + "_dbias", ref.rel_l2(out.db, dl64.sum(0)), ref.rel_l2(dl32.sum(0), dl64.sum(0))),
          _held("ce", tag + "_loss_sum", ref.rel_l2(out.loss, loss64), ref.rel_l2(loss32, loss64))]
    assert all(ok), tag
    assert bool((out.dl[:, N:] == 0).all())                                                # the pad columns are zeros
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
    if B > 1:
        per_row = F.cross_entropy(logits.double(), labels, reduction="none")
        assert abs(float(flagged.loss) - float(per_row[keep].sum())) <= 1e-9 * float(per_row.sum())


def test_ce_loss_without_labels_only_predicts():
    L, lib = _lib()
    logits = torch.randn(9, 5, generator=torch.Generator().manual_seed(5))
    logits[3, 1] = float("nan")                                                            # a NaN counts as the maximum
    dev = logits.to(DEV)
    pred = torch.full((9,), -1, dtype=torch.int64, device=DEV)
    L.check(lib.tl_ce_loss(dev.data_ptr(), None, None, None, pred.data_ptr(), None, None, None, None, 9, 5, 5, 8, 1.0,
                           torch.cuda.current_stream().cuda_stream), "tl_ce_loss")
    assert torch.equal(pred.cpu(), logits.argmax(1)) and int(pred[3]) == 1


# ---------------------------------------------------------------------------------------------- tl_head_bwd
def _head_bwd(dl, h, W, B, K, N, act, slope, want=(True, True, True)):
    L, lib = _lib()
    dh = torch.full((B, K), float("nan"), device=DEV) if want[0] else None
    db = torch.full((K,), float("nan"), device=DEV) if want[1] else None
    dw = torch.full((N, K), float("nan"), device=DEV) if want[2] else None
    L.check(lib.tl_head_bwd(dl.data_ptr(), h.data_ptr(), W.data_ptr(), L.ptr(dh), L.ptr(db), L.ptr(dw), B, K, N, dl.stride(0),
                            act, slope, torch.cuda.current_stream().cuda_stream), "tl_head_bwd")
    torch.cuda.synchronize()
    return dh, db, dw


@pytest.mark.parametrize("B,K,N", [(1, 4, 2), (7, 36, 3), (64, 260, 5), (65, 1600, 4), (300, 128, 64)])
def test_head_bwd_matches_float64_autograd(B, K, N):
    g = torch.Generator().manual_seed(B * 7 + K)
    z = torch.randn(B, K, generator=g)
    z[torch.rand(B, K, generator=g) < 0.1] = 0.0                                           # exact zeros: ReLU' = 0 there
    if B * K >= 8:
        assert bool((z == 0).any())
    W = torch.randn(N, K, generator=g) / K ** 0.5
    dl = torch.randn(B, N, generator=g) / B
    dl_dev = torch.zeros(B, _r4(N), device=DEV)
    dl_dev[:, :N] = dl.to(DEV)
    for code, name, act in ((0, "none", lambda t: t), (1, "relu", torch.relu), (2, "lrelu", lambda t: F.leaky_relu(t, 0.1))):
        def grads(dtype):
            zz = z.clone().to(dtype).requires_grad_(True)
            ww = W.clone().to(dtype).requires_grad_(True)
            ((act(zz) @ ww.t()) * dl.to(dtype)).sum().backward()
            return zz.grad, zz.grad.sum(0), ww.grad
        r64, r32 = grads(torch.float64), grads(torch.float32)
        h = act(z).to(DEV)
        got = _head_bwd(dl_dev, h, W.to(DEV), B, K, N, code, 0.1)
        tag = f"B{B}_K{K}_N{N}_{name}"
        ok = [_held("head_bwd", f"{tag}_{q}", ref.rel_l2(a, b64), ref.rel_l2(b32, b64))
              for q, a, b64, b32 in zip(("dh", "dbias_h", "dw"), got, r64, r32)]
        assert all(ok), tag
        for skip in range(3):                                                              # each output alone changes no other
            want = tuple(i != skip for i in range(3))
            part = _head_bwd(dl_dev, h, W.to(DEV), B, K, N, code, 0.1, want)
            assert part[skip] is None
            assert all(torch.equal(part[i], got[i]) for i in range(3) if i != skip), (tag, skip)


# ---------------------------------------------------------------------------------------------- engine
def _models(kind, seed=0):
    from decode_tonal_langauge_amd.models.simple_classifiers import LogisticRegressionClassifier, ShallowNNClassifier
    torch.manual_seed(seed)
    return {"logistic": lambda: LogisticRegressionClassifier(1600, 4),
            "shallow": lambda: ShallowNNClassifier(1600, 4, 800, "LeakyReLU"),
            "shallow_small": lambda: ShallowNNClassifier(36, 3, 20, "ReLU"),
            "shallow32": lambda: ShallowNNClassifier(1600, 4, 32, "ReLU")}[kind]()


def _engine(model, lr=0.0005, wd=0.0):
    from decode_tonal_langauge_amd._simple_classifier_engine import SimpleClassifierEngine
    return SimpleClassifierEngine(copy.deepcopy(model).to(DEV), lr, wd)


@pytest.mark.parametrize("kind", ["shallow_small", "logistic"])
def test_one_train_step_gradients_on_the_dense_path(kind):
    model = _models(kind, seed=2)
    K, N = model.input_dim, model.n_classes
    g = torch.Generator().manual_seed(8)
    x, y = torch.randn(65, K, generator=g), torch.randint(0, N, (65,), generator=g)
    m64, _ = ref.as_double(model, [])
    r64, r32 = ref.gradients(m64, x.double(), y), ref.gradients(model, x, y)
    eng = _engine(model)
    names = {p: k for k, p in eng.model.named_parameters()}
    eng.train_batch(x.to(DEV), y.to(DEV))
    torch.cuda.synchronize()
    got = {k: t for k, t in eng.grads.items()}
    assert set(got) == set(r64)                                                            # all four (both) gradients exist
    ok = [_held("gradients", f"{kind}_{k}", ref.rel_l2(got[k], r64[k]), ref.rel_l2(r32[k], r64[k])) for k in sorted(r64)]
    assert all(ok), kind
    loss_sum, count, cm = eng.epoch_stats()
    assert count == 65 and int(cm.sum()) == 65
    want = float(F.cross_entropy(m64(x.double()), y, reduction="sum"))
    yard = abs(float(F.cross_entropy(model(x), y, reduction="sum")) - want) / want
    assert _held("gradients", f"{kind}_loss_sum", abs(loss_sum - want) / want, yard)
    assert eng.epoch_stats()[1] == 0                                                       # reading zeroes the statistics


@pytest.mark.parametrize("kind", ["logistic", "shallow"])
def test_update_trajectory_lowrank_and_dense(kind):
    lr, wd = 0.001, 0.01
    model = _models(kind, seed=4)
    g = torch.Generator().manual_seed(21)
    data65 = [(torch.randn(65, 1600, generator=g), torch.randint(0, 4, (65,), generator=g)) for _ in range(3)]
    data64 = [(x[:64], y[:64]) for x, y in data65]

    def gpu_run(data, force_dense=False):
        eng = _engine(model, lr, wd)
        eng.force_dense = force_dense
        before = {k: v.detach().clone() for k, v in eng.model.named_parameters()}
        for x, y in data:
            eng.train_batch(x.to(DEV), y.to(DEV))
        torch.cuda.synchronize()
        return {k: (v.detach() - before[k]).cpu() for k, v in eng.model.named_parameters()}, eng

    ok = []
    yards = {}
    for data, tag, dense in ((data64, "lowrank_B64", False), (data65, "dense_B65", True)):
        m64, d64 = ref.as_double(model, data)
        r64, r32 = ref.updates_after(m64, d64, lr, wd), ref.updates_after(model, data, lr, wd)
        decayed = ref.updates_after(m64, d64, lr, wd, decay_biases=True)
        got, eng = gpu_run(data)
        assert (model.get_nparams() == sum(t.numel() for t in eng.grads.values())) is dense   # dW exists only on the dense path
        for k in sorted(r64):
            yards[tag, k] = ref.rel_l2(r32[k], r64[k])
            ok.append(_held("trajectory", f"{kind}_{tag}_{k}", ref.rel_l2(got[k], r64[k]), yards[tag, k]))
            if k.endswith("bias"):           # the biases are NOT decayed: the decayed update is the counter-example
                bound = ref.FACTOR * yards[tag, k]
                away = ref.rel_l2(decayed[k], r64[k])
                print(f"[trajectory] {kind}_{tag}_{k}: decayed variant at {away:.3e} of the reference, gpu at "
                      f"{ref.rel_l2(got[k], decayed[k]):.3e} of the decayed variant")
                assert away > bound and ref.rel_l2(got[k], decayed[k]) > bound, (k, away, bound)
    low, _ = gpu_run(data64)
    dense, eng = gpu_run(data64, force_dense=True)
    assert model.get_nparams() == sum(t.numel() for t in eng.grads.values())
    for k in sorted(low):
        ok.append(_held("trajectory", f"{kind}_lowrank_vs_dense_B64_{k}", ref.rel_l2(low[k], dense[k]), yards["lowrank_B64", k]))
    assert all(ok), kind


def _snapshot(eng):
    """Every parameter and every entry of the optimiser state (tensors cloned, the host scalars as they are)."""
    prm = {k: v.detach().clone() for k, v in eng.model.named_parameters()}
    names = {p: k for k, p in eng.model.named_parameters()}
    state = {(names[p], k): (v.clone() if torch.is_tensor(v) else v) for p, st in eng.optimizer.state.items() for k, v in st.items()}
    return prm, state


def _same_bits(a, b):
    return set(a) == set(b) and all(torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else a[k] == b[k] for k in a)


@pytest.mark.parametrize("route", ["lowrank", "dense"])
@pytest.mark.parametrize("kind", ["logistic", "shallow"])
def test_backward_only_returns_the_step_gradients_and_updates_nothing(kind, route):
    """``backward_only`` / ``step_gradients`` of the simple engine (inherited from the base class) at B = 5: the weights as
    factor pairs whose product is the gradient on the low-rank route, as tensors under ``force_dense``; yardstick as above."""
    from decode_tonal_langauge_amd.models.simple_classifiers import LogisticRegressionClassifier, ShallowNNClassifier
    torch.manual_seed(11)
    model = LogisticRegressionClassifier(8, 3) if kind == "logistic" else ShallowNNClassifier(8, 3, 8, "LeakyReLU")
    g = torch.Generator().manual_seed(12)
    x, y = torch.randn(5, 8, generator=g), torch.randint(0, 3, (5,), generator=g)
    m64, _ = ref.as_double(model, [])
    r64, r32 = ref.gradients(m64, x.double(), y), ref.gradients(model, x, y)

    def fresh():
        eng = _engine(model, 0.001, 0.01)
        eng.force_dense = route == "dense"
        return eng
    eng = fresh()
    before = _snapshot(eng)
    got = eng.backward_only(x.to(DEV), y.to(DEV))
    torch.cuda.synchronize()
    assert got.keys() == eng.step_gradients().keys() == r64.keys()
    got = {k: tuple(f.clone() for f in v) if isinstance(v, tuple) else v.clone() for k, v in got.items()}
    after = _snapshot(eng)
    assert _same_bits(before[0], after[0]) and before[1] == after[1] == {}             # no update, no optimiser state made
    ok = []
    for k in sorted(r64):
        if k.endswith("weight") and route == "lowrank":
            fa, fb = got[k]                                                                # (B, rows), (B, cols): dW = fa^T . fb
            assert fa.shape == (5, r64[k].shape[0]) and fb.shape == (5, r64[k].shape[1])
            full = fa.double().t() @ fb.double()
        else:
            assert torch.is_tensor(got[k])
            full = got[k]
        ok.append(_held("backward_only", f"{kind}_{route}_{k}", ref.rel_l2(full, r64[k]), ref.rel_l2(r32[k], r64[k])))
    assert all(ok), (kind, route)
    # with optimiser state in place: a second call moves neither it nor the parameters
    eng.train_batch(x.to(DEV), y.to(DEV))
    before = _snapshot(eng)
    assert sum(torch.is_tensor(v) for v in before[1].values()) == 2 * len(r64)             # both moments of every parameter
    eng.backward_only(x.to(DEV), y.to(DEV))
    torch.cuda.synchronize()
    after = _snapshot(eng)
    assert _same_bits(before[0], after[0]) and _same_bits(before[1], after[1])
    # a fresh engine on the same model: the gradients its train step applied are those bits
    twin = fresh()
    twin.train_batch(x.to(DEV), y.to(DEV))
    torch.cuda.synchronize()
    applied = twin.step_gradients()
    assert applied.keys() == got.keys()
    for k, v in got.items():
        if isinstance(v, tuple):
            assert all(torch.equal(a, b) for a, b in zip(applied[k], v)), k
        else:
            assert torch.equal(applied[k], v), k


def test_train_batch_never_reads_the_device():
    g = torch.Generator().manual_seed(3)
    for kind, B in (("logistic", 32), ("shallow32", 64), ("shallow32", 65)):
        eng = _engine(_models(kind, seed=1), 0.001, 0.01)
        x, y = torch.randn(B, 16, 100, generator=g).to(DEV), torch.randint(0, 4, (B,), generator=g).float().to(DEV)
        eng.train_batch(x, y)                          # first call: workspaces, optimizer state and its pointer table
        torch.cuda.synchronize()
        mode = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")
        try:
            eng.train_batch(x, y)
            eng.eval_batch(x, y)
        finally:
            torch.cuda.set_sync_debug_mode(mode)
        assert eng.epoch_stats()[1] == 3 * B
    bad = y.clone()
    bad[0] = 4
    eng.eval_batch(x, bad)
    with pytest.raises(ValueError, match=r"\[0, 4\)"):
        eng.epoch_stats()


# ---------------------------------------------------------------------------------------------- trainer and pipeline
@functools.lru_cache(maxsize=None)
def _trainer_data():
    return tuple(ref.planted(n, seed=s) for n, s in ((150, 3), (40, 4), (40, 5)))


@pytest.mark.parametrize("kind", ["logistic", "shallow32"])
def test_fused_trainer_fits_like_the_float64_loop(kind, tmp_path):
    from decode_tonal_langauge_amd.models.classifier_trainer import ClassifierTrainer
    (x, y), (vx, vy), (tx, ty) = _trainer_data()
    lr, wd, epochs = 0.005, 0.01, 5
    model = _models(kind, seed=6)
    cpu = lambda a, b, dt=torch.float32: ref.batches(a.to(dt), b, 64)
    h32 = ClassifierTrainer(copy.deepcopy(model), lr, wd).fit(cpu(x, y), cpu(vx, vy), max_epochs=epochs, patience=99)
    h64 = ref.parent_fit(copy.deepcopy(model).double(), lr, wd, cpu(x, y, torch.float64), cpu(vx, vy, torch.float64), epochs)
    dev = lambda a, b: ref.batches(a.to(DEV), b.to(DEV), 64)
    assert [len(b[1]) for b in dev(x, y)] == [64, 64, 22]                                  # a ragged last batch
    gpu_model = copy.deepcopy(model).to(DEV)
    tr = ClassifierTrainer(gpu_model, lr, wd, log_dir=str(tmp_path), fused=True)
    from decode_tonal_langauge_amd.optim import FusedNAdam
    assert isinstance(tr.optimizer, FusedNAdam) and [g["weight_decay"] for g in tr.optimizer.param_groups] == [wd, 0.0]
    hist = tr.fit(dev(x, y), dev(vx, vy), max_epochs=epochs, patience=99)
    assert len(hist) == epochs and all(list(a) == list(b) for a, b in zip(hist, h32))      # the same row keys
    ok = []
    for key in ("train/loss_epoch", "val/loss"):
        rel = lambda h: max(abs(a[key] - b[key]) / b[key] for a, b in zip(h, h64))
        ok.append(_held("trainer", f"{kind}_{key}", rel(hist), rel(h32)))
    assert all(ok), kind
    assert hist[-1]["val/loss"] < hist[0]["val/loss"]
    res = tr.test(dev(tx, ty))
    assert int(res["confusion_matrix"].sum()) == 40 and 0.0 <= res["accuracy"] <= 1.0
    pred = tr.predict(dev(tx, ty))
    with torch.no_grad():
        own = torch.cat([gpu_model.eval()(a).argmax(1) for a, _ in dev(tx, ty)])
    assert torch.equal(pred, own)
    assert torch.equal(torch.bincount(ty.long() * 4 + pred.cpu(), minlength=16).reshape(4, 4), res["confusion_matrix"])
    assert os.path.isfile(tmp_path / "metrics.csv") and os.path.isfile(tmp_path / "confusion_matrix_test.csv")


def test_pipeline_key_runs_the_fused_trainer(tmp_path, monkeypatch):
    import pandas as pd
    from decode_tonal_langauge_amd import _simple_classifier_engine as sce
    from decode_tonal_langauge_amd import train_classifier
    from decode_tonal_langauge_amd.data_loading import synthetic
    written = synthetic.write_dataset(str(tmp_path / "data"), n_samples=120, n_channels=8, n_timepoints=50)
    calls = []
    step = sce.SimpleClassifierEngine.train_batch
    monkeypatch.setattr(sce.SimpleClassifierEngine, "train_batch", lambda self, x, y: (calls.append(len(y)), step(self, x, y))[1])
    config = {
        "model": {"model": "models.simple_classifiers.ShallowNNClassifier", "model_name": "shallow",
                  "model_kwargs": {"hidden_dim": 32, "activation": "LeakyReLU"}},
        "dataset": {"class_labels": {"tone": None}},
        "training": {"module": "train_classifier", "params": {
            "fused": True,
            "io": {"log_dir": str(tmp_path / "logs"), "sample_dir": written["sample_dir"],
                   "channel_selection_dir": written["channel_selection_dir"]},
            "experiment": {"targets": ["tone"], "features": "ecog", "separate_models": False, "seed": 1, "repeat": 1,
                           "verbose": 0, "device": DEV},
            "training": {"train_ratio": 0.75, "vali_ratio": 0.125, "test_ratio": 0.125, "batch_size": 32, "epochs": 3,
                         "lr": 0.005, "patience": 5, "weight_decay": 0.01, "log_every_n_steps": 10}}},
        "evaluation": {"metrics": ["accuracy"]},
    }
    log_dir = train_classifier.run(config)
    df = pd.read_csv(os.path.join(log_dir, "results.csv"))
    assert len(df) == 1 and 0.0 <= float(df.iloc[0]["accuracy_mean"]) <= 1.0
    assert len(calls) == 3 * 3 and sum(calls) == 3 * 90                                    # 3 epochs x ceil(90 / 32) fused steps
