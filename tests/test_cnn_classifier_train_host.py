"""CPU: ``tl_ce_scores_loss`` is declared, bound, exported and validates its arguments without a launch; the float64 restatement
of ``CNNClassifier`` the GPU tests compare against IS the stock module; float32 against float64 obeys the flip rule the GPU
planes are held to; ``ClassifierTrainer(fused=False)`` on a ``CNNClassifier`` is the loop it always was; the training engine
refuses what it does not take."""
import copy
import functools
import os
import re

import pytest
import torch

from tests import branch_planes
from tests import classifier_train_ref as ref
from tests import cnn_classifier_ref as cref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ce_scores_loss_is_declared_bound_and_exported():
    from decode_tonal_langauge_amd import _lib
    lib = _lib.load()
    with open(os.path.join(ROOT, "include", "tonal_hip.h")) as f:
        header = f.read()
    assert re.search(r"\bint\s+tl_ce_scores_loss\s*\(", header)
    assert "tl_ce_scores_loss" in _lib.SIGNATURES and hasattr(lib, "tl_ce_scores_loss")
    assert len(_lib.SIGNATURES["tl_ce_scores_loss"][1]) == 15
    assert _lib.SIGNATURES["tl_ce_scores_loss"] == _lib.SIGNATURES["tl_ce_loss"]           # same arguments, same order


def test_ce_scores_loss_validates_its_arguments_without_gpu():
    from decode_tonal_langauge_amd import _lib
    lib = _lib.load()
    ce = lambda logits=16, labels=16, dl=16, db=16, pred=16, ls=16, cnt=16, cm=16, err=16, B=4, N=4, ldl=4, ldd=4: \
        lib.tl_ce_scores_loss(logits, labels, dl, db, pred, ls, cnt, cm, err, B, N, ldl, ldd, 0.25, None)
    assert ce(logits=None) == -1 and b"null logits" in lib.tl_last_error()
    assert ce(labels=None, pred=None) == -1 and b"null labels" in lib.tl_last_error()
    assert ce(labels=None) == -1 and b"need labels" in lib.tl_last_error()
    for name in ("ls", "cnt", "cm", "err"):
        assert ce(**{name: None}) == -1 and b"not optional" in lib.tl_last_error(), name
    assert ce(N=0) == -1 and b"[1, 64]" in lib.tl_last_error()
    assert ce(N=65, ldl=65) == -1 and b"[1, 64]" in lib.tl_last_error()
    assert ce(B=0) == -1 and b"at least 1" in lib.tl_last_error()
    assert ce(ldl=3) == -1 and b"ldl" in lib.tl_last_error()
    assert ce(ldd=3) == -1 and b"ldd" in lib.tl_last_error()
    assert ce(N=62, ldl=62, ldd=68) == -1 and b"ldd" in lib.tl_last_error()


@functools.lru_cache(maxsize=None)
def _own(shape, seed, dtype):
    """(scores, loss, grads, own decisions, margins) of the restatement deciding for itself, dropout off."""
    model, x, y = cref.build(shape, seed)
    own, margins = {}, {}
    s, loss, g = cref.loss_and_grads(model, cref.leaves(model, dtype), x, y, own=own, margins=margins)
    return s, loss, g, own, margins


@pytest.mark.parametrize("shape,seed", cref.SHAPES[:2])
def test_restatement_is_the_stock_module_in_float64(shape, seed):
    model, x, y = cref.build(shape, seed)
    s, loss, g, own, _ = _own(shape, seed, torch.float64)
    s0, loss0, g0 = cref.stock_loss_and_grads(model, x, y, torch.float64)
    assert ref.rel_l2(s, s0) <= 1e-12 and ref.rel_l2(loss, loss0) <= 1e-12
    assert set(g) == set(g0)
    for k in g0:
        assert ref.rel_l2(g[k], g0[k]) <= 1e-12, k
    # its OWN planes fed back: the same bits
    s1, loss1, g1 = cref.loss_and_grads(model, cref.leaves(model, torch.float64), x, y, planes=own)
    assert torch.equal(s1, s) and torch.equal(loss1, loss)
    assert all(torch.equal(g1[k], g[k]) for k in g)


@pytest.mark.parametrize("shape,seed", cref.SHAPES)
def test_float32_decisions_obey_the_flip_rule(shape, seed):
    own64, margins64 = _own(shape, seed, torch.float64)[3:]
    own32 = _own(shape, seed, torch.float32)[3]
    flips = branch_planes.check_flips(own32, own64, margins64)                             # tau 1e-4, max_frac 1e-4, slack 4
    n = sum(v[0] for v in flips.values())
    print(f"{shape}: {n} of {sum(t.numel() for t in own64.values())} branches differ, worst margin "
          f"{max(v[1] for v in flips.values()):.1e} of max|z|")
    assert set(flips) == set(own64) and len(flips) == 12                                   # 5 x (odd, pos) + conv5.pos + fc1.pos


def test_unfused_trainer_on_the_cnn_reproduces_the_parent_loop_bit_for_bit():
    from decode_tonal_langauge_amd.models.classifier_trainer import ClassifierTrainer
    from decode_tonal_langauge_amd.models.deep_classifiers import CNNClassifier
    x, y = ref.planted(10, n_cls=2, channels=2, length=150, seed=5)
    vx, vy = ref.planted(6, n_cls=2, channels=2, length=150, seed=6)
    train, val = ref.batches(x, y, 4), ref.batches(vx, vy, 4)
    torch.manual_seed(12)
    model = CNNClassifier(2, 150, 2)
    twin = copy.deepcopy(model)
    torch.manual_seed(13)                                                                  # the dropout stream of both runs
    want = ref.parent_fit(twin, 0.005, 0.01, train, val, 2)
    torch.manual_seed(13)
    tr = ClassifierTrainer(model, learning_rate=0.005, weight_decay=0.01, fused=False)
    assert tr.engine is None and isinstance(tr.optimizer, torch.optim.NAdam)
    got = tr.fit(train, val, max_epochs=2, patience=99)
    assert got == want
    assert all(torch.equal(a, b) for a, b in zip(model.state_dict().values(), twin.state_dict().values()))


def test_training_engine_refuses_what_it_does_not_take():
    from decode_tonal_langauge_amd._cnn_classifier_train_engine import CnnClassifierTrainEngine
    from decode_tonal_langauge_amd.models.deep_classifiers import CNNClassifier, CNNRNNClassifier
    for model, why in ((CNNClassifier(2, 150, 2, negative_slope=-0.1), "negative_slope -0.1"),
                       (CNNClassifier(2, 150, 65), "n_classes 65"),
                       (CNNClassifier(2, 150, 2, dropout_rate=1.0), "dropout 1.0"),
                       (CNNClassifier(2, 150, 2), "parameters on 'cpu'"),
                       (CNNRNNClassifier(2, 100, 2, lstm_dim=100), "model CNNRNNClassifier")):
        with pytest.raises(ValueError, match="CNNClassifier") as e:
            CnnClassifierTrainEngine(model)
        assert why in str(e.value), (why, str(e.value))
