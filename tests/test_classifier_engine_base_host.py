"""CPU: the three classifier train engines take their public steps from ``ClassifierTrainEngine``; ``_classifier_dp`` keeps the
free-standing parts the host tests import."""
import pytest

STEPS = ("train_batch", "backward_only", "step_gradients", "eval_batch", "predict_batch", "epoch_stats")


def _engines():
    from decode_tonal_langauge_amd._cnn_classifier_train_engine import CnnClassifierTrainEngine
    from decode_tonal_langauge_amd._cnnrnn_classifier_train_engine import CnnRnnClassifierTrainEngine
    from decode_tonal_langauge_amd._simple_classifier_engine import SimpleClassifierEngine
    return SimpleClassifierEngine, CnnClassifierTrainEngine, CnnRnnClassifierTrainEngine


@pytest.mark.parametrize("step", STEPS)
def test_public_steps_are_the_base_classes(step):
    from decode_tonal_langauge_amd._classifier_train_engine import ClassifierTrainEngine
    from decode_tonal_langauge_amd._conv_stack import ConvStack
    for Engine in _engines():
        assert issubclass(Engine, ClassifierTrainEngine)
        assert getattr(Engine, step) is getattr(ClassifierTrainEngine, step), (Engine.__name__, step)
        assert step not in vars(Engine)
    simple, cnn, cnnrnn = _engines()
    assert issubclass(cnn, ConvStack) and issubclass(cnnrnn, ConvStack) and not issubclass(simple, ConvStack)


def test_shared_pieces_exist_once():
    from decode_tonal_langauge_amd import _classifier_train_engine as base
    for Engine in _engines():
        for name in ("_labels", "_ce", "_workspace", "_setup_training", "_take", "_exchange", "_call", "scores"):
            assert name not in vars(Engine), (Engine.__name__, name)
            assert getattr(Engine, name) is getattr(base.ClassifierTrainEngine, name)
        assert "_make_workspace" in vars(Engine) and "_forward" in vars(Engine) and "_backward" in vars(Engine)
    from decode_tonal_langauge_amd import _simple_classifier_engine as simple
    assert simple.SUPPORTED is base.SUPPORTED                                              # (re-exported from where it was)


def test_classifier_dp_keeps_the_free_standing_parts():
    from decode_tonal_langauge_amd import _classifier_dp as dp
    for name in ("ShardPlan", "shard_plan", "reduce_stats_words", "RowGather", "_group_device"):
        assert hasattr(dp, name), name
    assert not hasattr(dp, "ClassifierDP")
    assert dp.shard_plan(5, 0, 1) == dp.ShardPlan(5, 0, 5, 1.0)                            # the plan of a single-process step
