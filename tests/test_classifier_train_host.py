"""CPU: the classifier-training entry points (tl_ce_loss, tl_head_bwd) are exported and validate their arguments without a
launch; ``ClassifierTrainer(fused=True)`` refuses what the engine does not take; ``fused=False`` is the loop it always was."""
import copy

import pytest
import torch

from tests import classifier_train_ref as ref


def test_library_exports_the_classifier_training_entry_points():
    from decode_tonal_langauge_amd import _lib
    lib = _lib.load()
    for name, arity in (("tl_ce_loss", 15), ("tl_head_bwd", 13)):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        assert len(_lib.SIGNATURES[name][1]) == arity, name


def test_argument_validation_without_gpu():
    from decode_tonal_langauge_amd import _lib
    lib = _lib.load()
    ce = lambda logits=16, labels=16, dl=16, db=16, pred=16, ls=16, cnt=16, cm=16, err=16, B=4, N=4, ldl=4, ldd=4: \
        lib.tl_ce_loss(logits, labels, dl, db, pred, ls, cnt, cm, err, B, N, ldl, ldd, 0.25, None)
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
    hb = lambda dl=16, h=16, W=16, dh=16, db=16, dw=16, B=4, K=8, N=4, ldd=4, act=0: \
        lib.tl_head_bwd(dl, h, W, dh, db, dw, B, K, N, ldd, act, 0.1, None)
    for name in ("dl", "h", "W"):
        assert hb(**{name: None}) == -1 and b"null" in lib.tl_last_error(), name
    assert hb(dh=None, db=None, dw=None) == -1 and b"nothing to compute" in lib.tl_last_error()
    assert hb(N=0) == -1 and hb(N=65, ldd=68) == -1 and b"[1, 64]" in lib.tl_last_error()
    assert hb(B=0) == -1 and hb(K=6) == -1 and b"multiple of 4" in lib.tl_last_error()
    assert hb(ldd=3) == -1 and b"ldd" in lib.tl_last_error()
    assert hb(act=3) == -1 and b"act" in lib.tl_last_error()
    assert hb(h=20) == -1 and b"16-byte" in lib.tl_last_error()


def test_fused_trainer_refuses_what_the_engine_does_not_take():
    from decode_tonal_langauge_amd.models.classifier_trainer import ClassifierTrainer
    from decode_tonal_langauge_amd.models.deep_classifiers import CNNClassifier
    from decode_tonal_langauge_amd.models.simple_classifiers import LogisticRegressionClassifier, ShallowNNClassifier
    for model, what in ((LogisticRegressionClassifier(40, 3), "cpu"),                      # parameters on the CPU
                        (ShallowNNClassifier(40, 3, 20, "ReLU"), "cpu"),
                        (ShallowNNClassifier(40, 3, 20, "GELU"), "activation GELU"),
                        (ShallowNNClassifier(40, 3, 18, "ReLU"), "hidden_dim 18"),
                        (LogisticRegressionClassifier(42, 3), "input_dim 42"),
                        (LogisticRegressionClassifier(40, 65), "n_classes 65"),
                        (CNNClassifier(input_channels=2, input_length=150, n_classes=2), "CNNClassifier")):
        with pytest.raises(ValueError, match="supports LogisticRegressionClassifier and ShallowNNClassifier") as e:
            ClassifierTrainer(model, fused=True)
        assert what in str(e.value), (what, str(e.value))
    tr = ClassifierTrainer(LogisticRegressionClassifier(40, 3))                           # the default is off
    assert tr.fused is False and tr.engine is None and isinstance(tr.optimizer, torch.optim.NAdam)


@pytest.mark.parametrize("kind", ["logistic", "shallow"])
def test_unfused_trainer_reproduces_the_parent_loop_bit_for_bit(kind):
    from decode_tonal_langauge_amd.models.classifier_trainer import ClassifierTrainer
    from decode_tonal_langauge_amd.models.simple_classifiers import LogisticRegressionClassifier, ShallowNNClassifier
    x, y = ref.planted(150, seed=3)
    vx, vy = ref.planted(40, seed=4)
    train, val = ref.batches(x, y, 64), ref.batches(vx, vy, 64)
    torch.manual_seed(11)
    model = LogisticRegressionClassifier(1600, 4) if kind == "logistic" else ShallowNNClassifier(1600, 4, 32, "LeakyReLU")
    twin = copy.deepcopy(model)
    want = ref.parent_fit(twin, 0.005, 0.01, train, val, 3)
    got = ClassifierTrainer(model, learning_rate=0.005, weight_decay=0.01, fused=False).fit(train, val, max_epochs=3, patience=99)
    assert got == want                                                                     # every float of every row
    assert all(torch.equal(a, b) for a, b in zip(model.state_dict().values(), twin.state_dict().values()))
