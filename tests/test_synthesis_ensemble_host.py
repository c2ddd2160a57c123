"""The SynthesisLite ensemble without a GPU: every refusal names its condition, the batch-limit arithmetic, the CLI flag, and the
argument checks of every new C entry (null pointers, M = 0, a member stride shorter than a member's extent return -1 with a
message before any launch - the pattern of tests/test_abi_and_host.py)."""
import ctypes as C
from argparse import Namespace

import pytest
import torch
from torch import nn

from tests import golden_inputs as gi
from tests.synthesis_ensemble_cases import S2, classifiers, lite_models

P = 0x1000          # a non-null, 16-byte aligned "pointer": never dereferenced, every call below fails its checks first


# ---------------------------------------------------------------------------------------------- engine refusals
def test_engine_refuses_what_it_does_not_support(monkeypatch):
    from decode_tonal_langauge_amd import _lite_ensemble_engine as le
    from decode_tonal_langauge_amd.models.synthesis_models import SynthesisLite
    with pytest.raises(ValueError, match="no models"):
        le.check_supported([])
    with pytest.raises(ValueError, match="model Linear.*SynthesisLite models of equal constructor arguments"):
        le.check_supported([nn.Linear(4, 4)])
    a, b = SynthesisLite(80, 4, 64), SynthesisLite(80, 4, 64, conv_channels=16)
    with pytest.raises(ValueError, match="member 1 was built with"):
        le.check_supported([a, b])
    with pytest.raises(ValueError, match="member 1 was built with"):
        le.check_supported([a, SynthesisLite(80, 4, 64, dropout=0.5)])
    with pytest.raises(ValueError, match="on 'cpu'.*one CUDA device"):
        le.check_supported([a, SynthesisLite(80, 4, 64)])
    with pytest.raises(ValueError, match="dtype torch.float16.*fp32"):
        le.check_supported([SynthesisLite(80, 4, 64).half()])
    monkeypatch.setattr(le.parallel, "world", lambda: (0, 2))
    with pytest.raises(ValueError, match="a process group of 2 ranks.*single process"):
        le.check_supported([a])


def test_engine_refuses_layers_wider_than_the_member_gemm_takes():
    """The fc.1 / fc.3 weight gradients run on the short-reduction TN kernel (Mdim * Ndim <= 2^20) - the only one with a member
    dimension: 512 * ldf and r4(output_dim) * 512 must fit, and a model beyond that is refused when the group is formed."""
    from decode_tonal_langauge_amd import _lite_ensemble_engine as le
    from decode_tonal_langauge_amd.models.synthesis_models import SynthesisLite
    # the default model: 32 * (T // 4) + 64 <= 2048 up to T = 251
    with pytest.raises(ValueError, match=r"fc.1 with 2080 padded inputs.*n_timepoints 252.*at most 2048 padded inputs"):
        le.check_supported([SynthesisLite(80, 4, 252)])
    with pytest.raises(ValueError, match="fc.1 with 3264 padded inputs"):
        le.check_supported([SynthesisLite(80, 4, 400)])
    with pytest.raises(ValueError, match="on 'cpu'"):            # 2048 inputs pass this check and reach the next one
        le.check_supported([SynthesisLite(80, 4, 251)])
    with pytest.raises(ValueError, match="output_dim 2049.*output_dim <= 2048"):
        le.check_supported([SynthesisLite(2049, 4, 64)])
    with pytest.raises(ValueError, match="on 'cpu'"):
        le.check_supported([SynthesisLite(2048, 4, 64)])


def test_batch_limit_arithmetic():
    from decode_tonal_langauge_amd._lite_ensemble_engine import check_train_batch
    check_train_batch(102, 5)                       # 102 * 5 - 1 = 509
    check_train_batch(512, 1)
    with pytest.raises(ValueError, match=r"B = 103.*L = 5.*B \* L - 1 = 514.*B \* L - 1 <= 512"):
        check_train_batch(103, 5)
    with pytest.raises(ValueError, match="B = 513"):
        check_train_batch(513, 1)


def test_trainer_refusals(monkeypatch):
    from decode_tonal_langauge_amd import parallel
    from decode_tonal_langauge_amd.models.synthesis_ensemble_trainer import SynthesisEnsembleTrainer
    tone, syl = classifiers(S2[2])
    models = lite_models(S2)
    kw = dict(seeds=(1, 2, 3), verbose=False)
    with pytest.raises(ValueError, match="needs a CUDA device"):
        SynthesisEnsembleTrainer(models, tone, syl, gi.TONE_MAP, device=torch.device("cpu"), **kw)
    with pytest.raises(ValueError, match="train_classifiers=True is not supported"):
        SynthesisEnsembleTrainer(models, tone, syl, gi.TONE_MAP, device=torch.device("cuda"), train_classifiers=True, **kw)
    with pytest.raises(ValueError, match="expected 3 seeds"):
        SynthesisEnsembleTrainer(models, tone, syl, gi.TONE_MAP, device=torch.device("cuda"), seeds=(1,), verbose=False)
    monkeypatch.setattr(parallel, "active", lambda: True)
    with pytest.raises(ValueError, match="data parallelism is not supported"):
        SynthesisEnsembleTrainer(models, tone, syl, gi.TONE_MAP, device=torch.device("cuda"), **kw)


# ---------------------------------------------------------------------------------------------- entry point
def _flags(**kw):
    base = dict(ensemble=True, synthesis_model_name="SynthesisLite", tone_model_path="t.pt", syllable_model_path="s.pt",
                device="cuda:0")
    base.update(kw)
    return Namespace(**base)


def test_cli_flag_parses_and_defaults_to_off():
    from decode_tonal_langauge_amd import train_synthesizer as ts
    need = ['--sample_path', 'x', '--subject_id', '1', '--result_file', 'r', '--model_name', 'm', '--synthesis_model_name',
            'SynthesisLite', '--syllable_model_name', 'logistic', '--tone_model_name', 'logistic']
    assert ts.build_parser().parse_args(need).ensemble is False
    assert ts.build_parser().parse_args(need + ['--ensemble']).ensemble is True
    assert ts.check_ensemble(_flags(ensemble=False, synthesis_model_name="SynthesisFull")) is False      # off: nothing is asked
    assert ts.check_ensemble(Namespace(synthesis_model_name="SynthesisFull")) is False


def test_entry_point_states_the_conditions(monkeypatch):
    from decode_tonal_langauge_amd import train_synthesizer as ts
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    assert ts.check_ensemble(_flags()) is True
    for kw, what in ((dict(synthesis_model_name="SynthesisFull"), "synthesis_model_name is 'SynthesisFull'"),
                     (dict(tone_model_path=None), "a classifier checkpoint is missing"),
                     (dict(syllable_model_path=None), "a classifier checkpoint is missing"),
                     (dict(device="cpu"), "device is 'cpu'")):
        with pytest.raises(ValueError, match=what + ".*--ensemble needs --synthesis_model_name SynthesisLite"):
            ts.check_ensemble(_flags(**kw))
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(ValueError, match="more than one process.*single process"):
        ts.check_ensemble(_flags())


# ---------------------------------------------------------------------------------------------- C entries
# name -> (valid-looking arguments without active / stream, index of M, index of the stride of an output)
ENTRIES = {
    "tl_lite_conv_fwd_group": ([P, P, P, P, P, 2, 2, 3, 4, 8, 3, 1, 48, 36, 4, 64, 16], 5, 15),
    "tl_lite_bn_finalize_group": ([P, P, P, P, P, 2, 2, 4, 16, 8, 0.1, 1e-5, 1, P, 16, 4, 4, 1], 5, 15),
    "tl_lite_bn_act_pool_fwd_group": ([P, P, P, P, P, P, 2, 2, 4, 8, 0.01, 64, 4, 4, 32], 6, 14),
    "tl_lite_bn_act_pool_bwd_group": ([P] * 10 + [2, 2, 4, 8, 0.01, 1, 32, 64, 4, 4, 64, 4, 16], 10, 20),
    "tl_lite_conv_bwd_group": ([P] * 6 + [2, 2, 3, 4, 8, 3, 1, 64, 48, 36, 48, 72, 8], 6, 17),
    "tl_sum_slabs2_group": ([P, P, 8, P, P, 4, 2, 2, 16, 8, 8, 4], 7, 9),
    "tl_colsum_group": ([P, P, 1, 2, 4, 4, 1, 1, 2, 8, 4], 8, 10),
    "tl_lite_lstm_fwd_group": ([P] * 8 + [2, 2, 3, 4, 2, 12, 32, 64, 16, 96, 24], 8, 17),
    "tl_lite_lstm_bwd_group": ([P] * 5 + [2, 2, 3, 4, 4, 8, 64, 96, 24], 5, 12),
    "tl_lstm_ih_grad_group": ([P] * 5 + [2, 1, 6, 4, 2, 96, 12, 32, 16], 5, 12),
    "tl_lite_cat_group": ([P, P, P, 2, 2, 8, 4, 3, 12, 0.3, P, 16, 24, 24], 3, 13),
    "tl_lite_uncat_group": ([P, P, P, 2, 2, 8, 4, 12, 0.3, P, 24, 16, 8], 3, 11),
    "tl_splitk_bias_lrelu_group": ([P, P, P, 2, 16, 4, 0.01, 2, 16, 32, 4, 16], 7, 11),
    "tl_l1_mcd_group": ([P, P, P, P, 2, 2, 3, 4, 1, 1.0, 6, 6, 8], 4, 12),
}


@pytest.fixture(scope="module")
def lib():
    from decode_tonal_langauge_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_group_entry_argument_checks(lib, name):
    args, i_m, i_stride = ENTRIES[name]
    fn, err = getattr(lib, name), lib.tl_last_error
    short = name[3:]
    assert len(args) + 2 == len(fn.argtypes)
    null = list(args)
    null[0] = None
    assert fn(*null, None, None) == -1 and short.encode() in err(), err()
    none = list(args)
    none[i_m] = 0
    assert fn(*none, None, None) == -1 and b"number of members M must lie in [1, 65535]" in err(), err()
    many = list(args)
    many[i_m] = 65536
    assert fn(*many, None, None) == -1 and b"number of members" in err(), err()
    cut = list(args)
    cut[i_stride] = 0
    assert fn(*cut, None, None) == -1 and b"member stride" in err() and short.encode() in err(), err()


def test_splitk_group_entry_wants_the_slab_stride_for_every_m(lib):
    fn, err = lib.tl_splitk_bias_lrelu_group, lib.tl_last_error
    for M in (1, 2):
        assert fn(P, P, P, 2, 16, 4, 0.01, M, 0, 32, 4, 16, None, None) == -1 and b"slab stride is shorter" in err(), (M, err())
        assert fn(P, P, P, 2, 16, 4, 0.01, M, 15, 32, 4, 16, None, None) == -1 and b"slab stride is shorter" in err(), (M, err())


def test_lite_group_entries_need_the_seed_table(lib):
    for name in ("tl_lite_cat_group", "tl_lite_uncat_group"):
        args = list(ENTRIES[name][0])
        args[args.index(0.3) + 1] = None
        assert getattr(lib, name)(*args, None, None) == -1 and b"seed table is null" in lib.tl_last_error()


def _nt(**kw):
    from decode_tonal_langauge_amd._lib import NtParams
    f = dict(A=P, Bw=P, out=P, M=2, A_rows=2, N=8, K=8, lda=8, ldb=8, ldo=8, ldaux=8, J=1, Tp=1, loader=0, epilogue=0, splitk=1, bm=32)
    f.update(kw)
    return NtParams(**f)


def test_nt_group_fc_argument_checks(lib):
    fn, err = lib.tl_gemm_nt_window_group_fc, lib.tl_last_error

    def call(prm, M=2, s_A=16, s_Bw=64, s_bias=0, s_aux=0, s_out=16):
        return fn(C.byref(prm) if prm is not None else None, M, s_A, s_Bw, s_bias, s_aux, s_out, None, None)
    assert call(None) == -1 and b"null params" in err()
    assert call(_nt(A=None)) == -1 and b"null A/Bw/out" in err()
    assert call(_nt(), M=0) == -1 and b"number of members" in err()
    assert call(_nt(), s_out=15) == -1 and b"member stride of out" in err()
    assert call(_nt(splitk=2, slab_stride=16), s_out=31) == -1 and b"member stride of out" in err()
    assert call(_nt(splitk=2, slab_stride=15), s_out=64) == -1 and b"slab_stride shorter" in err()
    assert call(_nt(), s_A=6) == -1 and b"multiples of 4" in err()
    for kw, what in ((dict(J=3, A_rows=4), b"J = 1"), (dict(loader=1), b"DIRECT"), (dict(row_shift=-1, J=2), b"row_shift"),
                     (dict(bm=256), b"bm must be 32 or 128"), (dict(bm=0), b"bm must be 32 or 128"),
                     (dict(epilogue=1), b"STORE and MASK"), (dict(epilogue=3), b"MASK epilogue needs aux"),
                     (dict(aux=P), b"no member stride"), (dict(epilogue=3, aux=P, auxbits=P), b"no member stride"),
                     (dict(splitk=2, slab_stride=16, epilogue=3, aux=P), b"split-K needs the STORE epilogue")):
        assert call(_nt(**kw), s_out=64) == -1 and what in err(), (kw, err())


def _tn(**kw):
    from decode_tonal_langauge_amd._lib import TnParams
    f = dict(A=P, B=P, slab=P, Krows=2, A_rows=2, B_rows=2, Mdim=4, Ndim=4, lda=4, ldb=4, ldc=4, J=1, Tp=1, Tvalid=1, loader=0, splitk=1)
    f.update(kw)
    return TnParams(**f)


def test_tn_group_argument_checks(lib):
    fn, err = lib.tl_gemm_tn_window_group, lib.tl_last_error

    def call(prm, M=2, s_A=8, s_B=8, s_slab=16, s_colsum=4):
        return fn(C.byref(prm) if prm is not None else None, M, s_A, s_B, s_slab, s_colsum, None, None)
    assert call(None) == -1 and b"null params" in err()
    assert call(_tn(slab=None)) == -1 and b"null A/B/slab" in err()
    assert call(_tn(), M=0) == -1 and b"number of members" in err()
    assert call(_tn(), s_slab=12) == -1 and b"member stride of slab" in err()
    assert call(_tn(splitk=2, slab_stride=16), s_slab=16) == -1 and b"member stride of slab" in err()
    assert call(_tn(colsum=P), s_colsum=3) == -1 and b"member stride of colsum" in err()
    assert call(_tn(), s_A=6) == -1 and b"multiples of 4" in err()
    for kw in (dict(J=3), dict(loader=1, bbits=P, Tp=2, Tvalid=2, ld_bbits=1), dict(Krows=513, A_rows=513, B_rows=513),
               dict(splitk=9, slab_stride=16), dict(Mdim=2048, Ndim=1024, lda=2048, ldb=1024, ldc=1024), dict(ldc=6),
               dict(splitk=2, slab_stride=8)):
        assert call(_tn(**kw), s_slab=1 << 22) == -1 and b"only the short-reduction kernel has a group form" in err(), (kw, err())
    assert call(_tn(vd=P)) == -1 and b"no member stride" in err()
