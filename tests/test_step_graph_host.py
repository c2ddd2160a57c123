"""CPU: the state machine of ``_step_graph.StepGraphs`` (warm-up, capture, replay order, the two-shape cap, fingerprint
invalidation, a failed capture, graph=0) on stubs: recording fakes for ``torch.cuda``'s graph calls, for the library's two staging
entries and for the optimiser.  With CPU tensors as batches a replay stages through the ``copy_`` + ``tl_set_step_scalars``
fallback, the path no GPU test reaches."""
import warnings

import pytest
import torch


class _Graph:
    def __init__(self, log):
        self.log = log

    def replay(self):
        self.log.append(("replay", id(self)))


class _Recording:
    def __init__(self, log, g):
        self.log, self.g = log, g

    def __enter__(self):
        self.log.append(("capture_begin", id(self.g)))

    def __exit__(self, *exc):
        self.log.append(("capture_end", id(self.g)))
        return False


class _Stream:
    cuda_stream = 0


class _Lib:
    def __init__(self, log):
        self.log = log

    def tl_stage_step(self, scal, seed, cg, cm, bc2, word, src, dst, nby, n, stream):
        self.log.append(("tl_stage_step", n, word))
        return 0

    def tl_set_step_scalars(self, scal, seed, cg, cm, bc2, word, stream):
        self.log.append(("tl_set_step_scalars", (cg, cm, bc2), word))
        return 0


class _Optimizer:
    def __init__(self, log):
        self.log, self.t = log, 0
        self._tables = {"k": (torch.zeros(1), 1)}

    def advance_scalars(self, params):
        self.t += 1
        self.log.append(("advance_scalars", frozenset(params)))
        return 0.1 * self.t, 0.2 * self.t, 0.3 * self.t


@pytest.fixture
def rig(monkeypatch):
    """(make, log): ``make()`` builds a ``StepGraphs`` over the fakes, every fake appends to ``log``."""
    from decode_tonal_langauge_amd import _step_graph
    log = []
    monkeypatch.delenv("TONAL_GRAPH", raising=False)
    monkeypatch.delenv("TONAL_KERNELS", raising=False)
    monkeypatch.setattr(torch.cuda, "CUDAGraph", lambda: _Graph(log))
    monkeypatch.setattr(torch.cuda, "graph", lambda g: _Recording(log, g))
    monkeypatch.setattr(torch.cuda, "synchronize", lambda: log.append(("synchronize",)))
    monkeypatch.setattr(torch.cuda, "current_stream", lambda: _Stream())
    return (lambda: _step_graph.StepGraphs("FakeTrainer", _Lib(log), _Optimizer(log), torch.device("cpu"))), log


class _Trainer:
    """What a trainer hands to ``StepGraphs.step``."""

    def __init__(self, graphs, log, fail=False):
        self.graphs, self.log, self.fail = graphs, log, fail
        self.fp, self.seeds, self.captured = ("fp", 0), 0, []

    def fingerprint(self):
        return self.fp

    def seed(self):
        self.seeds += 1
        return 1000 + self.seeds

    def capture(self, recording, static):
        with recording:
            if self.fail:
                raise RuntimeError("operation not permitted when stream is capturing")
            self.captured.append(static)
            self.log.append(("captured_step",))

    def step(self, batch):
        return self.graphs.step(batch, ["p0", "p1"], self.fingerprint, self.capture, self.seed)


def _batch(B, fill=0.0):
    return (torch.full((B, 3), fill), torch.full((B, 2), fill + 1), torch.full((B, 2), fill + 2), torch.full((B, 4), fill + 3))


def _names(log):
    return [e[0] for e in log]


def _held(graphs):
    return sum(v["graph"] is not None for v in graphs.states.values())


def test_three_warm_ups_then_capture_then_replays(rig):
    make, log = rig
    graphs = make()
    tr = _Trainer(graphs, log)
    for i in range(3):
        assert tr.step(_batch(5, float(i))) is False
    assert log == [] and _held(graphs) == 0 and tr.seeds == 0          # nothing captured, staged or advanced while warming up
    # ---- the fourth call captures, runs the trainer's capture once on the static inputs, and replays
    b4 = _batch(5, 40.0)
    assert tr.step(b4) is True
    assert len(tr.captured) == 1 and _held(graphs) == 1
    static = tr.captured[0]
    (st,) = graphs.states.values()
    assert static is st["in"] and all(s is not b and torch.equal(s, b) for s, b in zip(static, b4))
    assert _names(log) == ["synchronize", "capture_begin", "captured_step", "capture_end", "advance_scalars", "tl_stage_step",
                           "replay"]
    assert log[-2] == ("tl_stage_step", 0, 1001)                       # nothing is staged on the capture step: n = 0
    assert log[-3] == ("advance_scalars", frozenset(["p0", "p1"]))
    assert st["keep"] == list(graphs.optimizer._tables.values()) and st["fingerprint"] == ("fp", 0)
    assert graphs.scalars.shape == (4,) and graphs.scalars.dtype == torch.float32
    assert graphs.seed.shape == (1,) and graphs.seed.dtype == torch.int64
    # ---- later calls: the batch goes into the SAME static inputs, no capture; advance_scalars < staging < replay
    for i in (5, 6):
        del log[:]
        b = _batch(5, 10.0 * i)
        assert tr.step(b) is True
        assert _names(log) == ["advance_scalars", "tl_set_step_scalars", "replay"]
        assert log[1][2] == 1000 + tr.seeds                            # the seed of this step, drawn once
        assert graphs.states[next(iter(graphs.states))]["in"] is static
        assert all(torch.equal(s, t) for s, t in zip(static, b))
    assert len(tr.captured) == 1 and tr.seeds == 3
    assert log[1][1] == pytest.approx((0.3, 0.6, 0.9))                 # the scalars of the third advance travel with it


def test_a_third_shape_never_captures_while_two_graphs_are_held(rig):
    make, log = rig
    graphs = make()
    tr = _Trainer(graphs, log)
    for _ in range(6):
        for B in (5, 3, 2):
            tr.step(_batch(B))
    held = {k[0][0]: v["graph"] is not None for k, v in graphs.states.items()}
    assert held == {5: True, 3: True, 2: False} and len(tr.captured) == 2
    del log[:]
    assert tr.step(_batch(2)) is False and log == []


def test_a_changed_fingerprint_drops_only_that_shapes_graph(rig):
    make, log = rig
    graphs = make()
    tr = _Trainer(graphs, log)
    for _ in range(4):
        tr.step(_batch(5))
        tr.step(_batch(3))
    assert _held(graphs) == 2
    tr.fp = ("fp", 1)
    del log[:]
    assert tr.step(_batch(5)) is False and log == []                   # dropped: the first of three new warm-ups
    by_rows = {k[0][0]: v for k, v in graphs.states.items()}
    assert by_rows[5]["graph"] is None and by_rows[5]["keep"] is None and by_rows[3]["graph"] is not None
    assert tr.step(_batch(5)) is False and tr.step(_batch(5)) is False and _held(graphs) == 1
    assert tr.step(_batch(5)) is True and _held(graphs) == 2 and len(tr.captured) == 3
    assert by_rows[5]["fingerprint"] == ("fp", 1)
    assert tr.step(_batch(3)) is False and _held(graphs) == 1          # the other shape notices at its own next step


def test_a_failed_capture_warns_once_and_stays_eager(rig):
    make, log = rig
    graphs = make()
    tr = _Trainer(graphs, log, fail=True)
    for _ in range(3):
        assert tr.step(_batch(5)) is False
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        assert tr.step(_batch(5)) is False
        tr.fail = False
        for _ in range(5):
            assert tr.step(_batch(5)) is False
    assert len(seen) == 1
    assert str(seen[0].message).startswith("FakeTrainer: HIP-graph capture of the train step failed (RuntimeError(")
    assert str(seen[0].message).endswith("; continuing eagerly")
    assert graphs.enabled is False and _held(graphs) == 0 and tr.captured == [] and tr.seeds == 0
    assert "replay" not in _names(log) and "advance_scalars" not in _names(log) and _names(log).count("capture_begin") == 1


def test_graph_switched_off_never_captures(rig, monkeypatch):
    make, log = rig
    monkeypatch.setenv("TONAL_KERNELS", "graph=0")
    graphs = make()
    tr = _Trainer(graphs, log)
    assert graphs.enabled is False
    for _ in range(8):
        assert tr.step(_batch(5)) is False
    assert log == [] and tr.captured == [] and _held(graphs) == 0
