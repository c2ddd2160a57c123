"""CPU: the host side of data-parallel classifier training - the shard plan, the reduction of the epoch statistics words over
gloo, the new C-ABI symbols' argument checks (no GPU call is reached) and ``train_classifier.run``'s rank-0-only writing."""
import os
import re
import struct

import pytest
import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"tl_dropout_scale_at": 6, "tl_pool3_fwd_shard": 16, "tl_pool3_bwd_shard": 19}


# ---------------------------------------------------------------------------------------------- shard plan
@pytest.mark.parametrize("world", [1, 2, 3, 4])
@pytest.mark.parametrize("B", range(1, 10))
def test_shard_plan_covers_each_row_once_with_weights_summing_to_one(B, world):
    from decode_tonal_langauge_amd._classifier_dp import RowGather, shard_plan
    plans = [shard_plan(B, r, world) for r in range(world)]
    live = [p for p in plans if p.live]
    assert abs(sum(p.weight for p in plans) - 1.0) < 1e-15
    covered = [row for p in live for row in range(p.row0, p.row0 + p.rows)]
    assert covered == list(range(B))                                     # contiguous, in rank order, each row once
    for p in plans:
        assert p.B == B and p.rows >= 1 and 0 <= p.row0 and p.row0 + p.rows <= B      # every rank computes something
        assert p.weight == (p.rows / B if p.live else 0.0)
        assert p.rows_sent == (p.rows if p.live else 0)
    assert len(live) == min(B, world)
    for r, p in enumerate(plans):
        if not p.live:                                                   # fewer rows than ranks: a duplicate of row rank % B
            assert B < world and r >= B and (p.row0, p.rows) == (r % B, 1)
    if B >= world:
        assert max(p.rows for p in plans) - min(p.rows for p in plans) <= 1
    # the gather's pick list puts the live rows of the (world * kmax) gathered rows in global order
    g = RowGather(B, world, "cpu")
    sent = torch.full((world * g.kmax,), -1, dtype=torch.int64)
    for r, p in enumerate(plans):
        sent[r * g.kmax:r * g.kmax + p.rows_sent] = torch.arange(p.row0, p.row0 + p.rows_sent)
    assert torch.equal(sent[g.pick], torch.arange(B))


def test_shard_plan_refuses_nonsense():
    from decode_tonal_langauge_amd._classifier_dp import shard_plan
    for args in ((0, 0, 1), (4, 2, 2), (4, -1, 2)):
        with pytest.raises(ValueError):
            shard_plan(*args)


# ---------------------------------------------------------------------------------------------- statistics words over gloo
def _bits(x: float) -> int:
    return struct.unpack("q", struct.pack("d", x))[0]


def _words(rank: int, n: int = 3) -> torch.Tensor:
    loss = 0.1 * (rank + 1) + 1e-13 * rank
    cm = torch.arange(n * n, dtype=torch.int64) * (rank + 1)
    return torch.cat([torch.tensor([_bits(loss), int(cm.sum()), 0], dtype=torch.int64), cm])


def _stats_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    from decode_tonal_langauge_amd import _classifier_dp, parallel
    parallel.init_from_env(backend="gloo")
    total = _classifier_dp.reduce_stats_words(_words(rank))
    flagged = _words(rank)
    flagged[2] = rank                                                    # a bad label seen on rank 1 only
    q.put((rank, total.numpy(), _classifier_dp.reduce_stats_words(flagged).numpy(), parallel.is_writer()))
    torch.distributed.destroy_process_group()


def test_statistics_words_reduce_to_the_global_values_over_gloo():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29700 + os.getpid() % 200
    procs = [ctx.Process(target=_stats_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=120) for _ in procs), key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    w0, w1 = _words(0), _words(1)
    want = w0 + w1
    loss = struct.unpack("d", struct.pack("q", int(w0[0])))[0] + struct.unpack("d", struct.pack("q", int(w1[0])))[0]
    want[0] = _bits(loss)                                                # the loss word is summed as a double, in rank order
    for rank, total, flagged, writer in res:
        assert (total == want.numpy()).all(), rank                       # the same words on both ranks
        assert int(flagged[2]) == 1                                      # the flag reaches every rank
        assert writer == (rank == 0)


# ---------------------------------------------------------------------------------------------- C ABI
def test_new_entry_points_are_declared_bound_and_exported():
    from decode_tonal_langauge_amd import _lib
    lib = _lib.load()
    with open(os.path.join(ROOT, "include", "tonal_hip.h")) as f:
        header = f.read()
    for name, nargs in NEW.items():
        assert re.search(rf"\bint\s+{name}\s*\(", header), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
    with open(os.path.join(ROOT, "README.md")) as f:
        count = int(re.search(r"(\d+) entry points", f.read()).group(1))
    assert count == len(re.findall(r"^int\s+tl_\w+\s*\(", header, flags=re.M)) + \
        len(re.findall(r"^const char\*\s+tl_\w+\s*\(", header, flags=re.M))


def test_new_entry_points_refuse_null_pointers_and_negative_offsets():
    from decode_tonal_langauge_amd import _lib
    lib = _lib.load()
    err = lib.tl_last_error
    assert lib.tl_dropout_scale_at(None, 8, 0.5, 1, 0, None) == -1 and b"dropout_scale_at" in err()
    assert lib.tl_dropout_scale_at(16, 8, 0.5, 1, -1, None) == -1 and b"index0" in err()
    assert lib.tl_dropout_scale_at(16, 0, 0.5, 1, 0, None) == -1
    assert lib.tl_dropout_scale_at(16, 8, 1.0, 1, 0, None) == -1 and b"[0, 1)" in err()
    assert lib.tl_dropout_scale_at(16, 8, 0.5, 1, (1 << 63) - 4, None) == -1 and b"index0" in err()
    assert lib.tl_dropout_scale_at(16, 8, 0.0, 1, 5, None) == 0                            # p = 0: nothing to do, no launch
    fwd = lambda Y=16, X=16, B=2, b0=0, Bg=2: lib.tl_pool3_fwd_shard(Y, X, B, 1, 2, 256, 12, 3, 256, 1, B, 0.5, 7, b0, Bg, None)
    assert fwd(Y=None) == -1 and b"null" in err()
    assert fwd(X=None) == -1 and b"null" in err()
    assert fwd(b0=-1) == -1 and b"global batch" in err()
    assert fwd(b0=1, Bg=2) == -1 and b"global batch" in err()                               # rows 1, 2 of a batch of 2
    assert fwd(Bg=1) == -1 and b"global batch" in err()
    bwd = lambda Y=16, dX=16, dZ=16, B=2, b0=0, Bg=2: \
        lib.tl_pool3_bwd_shard(Y, dX, dZ, B, 1, 2, 256, 12, 3, 256, 256, 1, B, 0.5, 7, 0.01, b0, Bg, None)
    for name in ("Y", "dX", "dZ"):
        assert bwd(**{name: None}) == -1 and b"null" in err(), name
    assert bwd(b0=-3) == -1 and b"global batch" in err()
    assert bwd(b0=2, Bg=3) == -1 and b"global batch" in err()


# ---------------------------------------------------------------------------------------------- rank-0-only writing
def _config(tmp_path, written):
    return {
        "model": {"model": "models.simple_classifiers.LogisticRegressionClassifier", "model_name": "logistic"},
        "dataset": {"class_labels": {"tone": None}},
        "training": {"module": "train_classifier", "params": {
            "fused": True,
            "io": {"log_dir": str(tmp_path / "logs"), "sample_dir": written["sample_dir"],
                   "channel_selection_dir": written["channel_selection_dir"]},
            "experiment": {"targets": ["tone"], "features": "ecog", "separate_models": False, "seed": 1, "repeat": 1,
                           "verbose": 0, "device": "cpu", "save_checkpoints": True},
            "training": {"train_ratio": 0.75, "vali_ratio": 0.125, "test_ratio": 0.125, "batch_size": 32, "epochs": 2,
                         "lr": 0.005, "patience": 5, "weight_decay": 0.01, "log_every_n_steps": 10}}},
        "evaluation": {"metrics": ["accuracy", "confusion_matrix"]},
    }


class _StubTrainer:
    """``ClassifierTrainer`` without a model behind it: goes through the trainer's own writers."""
    made = []

    def __init__(self, model, learning_rate=0.0, weight_decay=0.0, log_dir=None, verbose=False, fused=False):
        from decode_tonal_langauge_amd.models.classifier_trainer import ClassifierTrainer
        self.real = ClassifierTrainer.__new__(ClassifierTrainer)
        self.real.log_dir, self.real.history, self.real.model = log_dir, [], model
        self.fused = fused
        _StubTrainer.made.append(self)

    def fit(self, train_loader, val_loader, max_epochs, patience):
        self.real.history = [{"epoch": 0, "val/loss": 1.0}]
        self.real._write_metrics()

    def test(self, loader):
        self.real.engine = None
        self.real.model.eval()
        return type(self.real).test(self.real, loader)

    def predict(self, loader):
        return torch.cat([b[1] for b in loader]).long()


def _all_files(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


@pytest.mark.parametrize("rank", [0, 1])
def test_run_writes_files_on_rank_zero_only(rank, tmp_path, monkeypatch):
    from decode_tonal_langauge_amd import parallel, train_classifier
    from decode_tonal_langauge_amd.data_loading import synthetic
    from decode_tonal_langauge_amd.training import classifier_pipeline
    written = synthetic.write_dataset(str(tmp_path / "data"), n_samples=320, n_channels=4, n_timepoints=20)
    monkeypatch.setattr(classifier_pipeline, "ClassifierTrainer", _StubTrainer)
    monkeypatch.setattr(parallel, "init_from_env", lambda backend=None: (rank, 2, 0))       # no process group is opened ...
    monkeypatch.setattr(parallel, "world", lambda: (rank, 2))                                # ... the run only asks who it is
    monkeypatch.setattr(parallel, "active", lambda: False)                                   # (keeps the CPU device of the config)
    _StubTrainer.made.clear()
    log_dir = train_classifier.run(_config(tmp_path, written))
    assert len(_StubTrainer.made) == 1 and _StubTrainer.made[0].fused                         # every rank trains
    files = _all_files(log_dir)
    if rank:
        assert files == []
        return
    names = {os.path.basename(f) for f in files}
    assert {"config.yaml", "metrics.csv", "confusion_matrix_test.csv", "results.csv", "confusion_matrix.csv",
            "confusion_matrix.png"} <= names
    assert any(f.startswith("model_checkpoints") and f.endswith(".pt") for f in files)


def test_unfused_trainer_under_two_ranks_is_refused(monkeypatch):
    from decode_tonal_langauge_amd import parallel
    from decode_tonal_langauge_amd.models.classifier_trainer import ClassifierTrainer
    from decode_tonal_langauge_amd.models.simple_classifiers import LogisticRegressionClassifier
    model = LogisticRegressionClassifier(16, 2)
    ClassifierTrainer(model, fused=False)                                                    # single process: as before
    monkeypatch.setattr(parallel, "world", lambda: (1, 2))
    with pytest.raises(ValueError, match="fused=True"):
        ClassifierTrainer(model, fused=False)
