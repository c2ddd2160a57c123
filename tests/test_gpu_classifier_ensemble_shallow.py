"""GPU: the ShallowNNClassifier ensemble - ``tl_gemm_nt_window_group`` and ``tl_head_bwd_act_group`` bit for bit against their
single launches (M = 1 and 3, every member on inputs of its own, a masked member's canaries untouched, member strides with
canaried padding), ``ClassifierEnsembleEngine`` against three ``SimpleClassifierEngine``s, the active mask, the 64-row limit of
training batches, ``ClassifierEnsembleTrainer`` against sequential ``ClassifierTrainer(fused=True)`` runs that stop at
different epochs, and the pipeline key against the sequential pipeline.

All comparisons are exact (``torch.equal`` on the raw buffers): a group kernel runs the single kernel's body with a member
dimension on the grid, and the single engine's own tests tie it to the float64 reference."""
import copy

import pytest
import torch

from tests import ensemble_cases as ec
from tests.ensemble_cases import CANARY, CASES, DEV, IDS
from tests.ensemble_cases import (canary as _canary, gen as _gen, lib as _lib, mask_words as _mask, on as _on, r4 as _r4,
                                  stream as _stream)

pytestmark = pytest.mark.gpu


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
@pytest.mark.parametrize("B,K,N", [(1, 4, 1), (7, 12, 3), (65, 260, 33), (70, 20, 9), (70, 12, 3)])
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
# (the bodies of the tests that also exist for logistic members are tests/ensemble_cases.py's)
SHALLOW = ("relu", "lrelu")


@pytest.mark.parametrize("kind", SHALLOW)
@pytest.mark.parametrize("sizes", ec.KINDS["relu"]["sizes"], ids=["b8_b8", "b64_b19", "b1"])
def test_engine_steps_equal_the_single_engine(kind, sizes):
    ec.engine_steps_equal_the_single_engine(kind, sizes)


def test_engine_refuses_training_batches_above_64_rows_and_evaluates_them():
    from decode_tonal_langauge_amd._classifier_ensemble_engine import ClassifierEnsembleEngine
    from decode_tonal_langauge_amd._simple_classifier_engine import SimpleClassifierEngine
    models = ec.member_models(3, "relu")
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
    ec.engine_mask_freezes_a_member("lrelu")


def test_engine_mask_freezes_a_relu_member():
    ec.engine_mask_freezes_a_member("relu")


# ---------------------------------------------------------------------------------------------- trainer
def test_trainer_equals_sequential_fused_runs_with_members_stopping_apart(tmp_path):
    ec.trainer_equals_sequential_fused_runs(tmp_path, "relu")


def test_trainer_with_leaky_relu_members_equals_sequential_fused_runs(tmp_path):
    ec.trainer_equals_sequential_fused_runs(tmp_path, "lrelu")


def test_trainer_refuses_training_loaders_above_64_rows_before_the_first_epoch():
    from decode_tonal_langauge_amd.data_loading.dataloaders import split_dataset
    from decode_tonal_langauge_amd.data_loading.resident import ResidentDataset
    from decode_tonal_langauge_amd.models.classifier_ensemble_trainer import ClassifierEnsembleTrainer
    rds = ResidentDataset.from_tensor_dataset(ec.planted(), device=DEV)
    models = ec.member_models(2, "relu")
    before = copy.deepcopy([m.state_dict() for m in models])
    loaders = [split_dataset(rds, [0.7, 0.1, 0.2], [True, False, False], batch_size=65, seed=s, resident=True, device=DEV)
               for s in (1, 2)]
    ens = ClassifierEnsembleTrainer(models, ec.KINDS["relu"]["lr"], ec.KINDS["relu"]["wd"])
    state = torch.get_rng_state()
    with pytest.raises(ValueError, match="65 rows.*at most 64 rows"):
        ens.fit([lo[0] for lo in loaders], [lo[1] for lo in loaders], max_epochs=2, patience=1)
    assert ens.history == [[], []] and torch.equal(torch.get_rng_state(), state)   # nothing was drawn, nothing trained
    for sd, m in zip(before, models):
        assert all(torch.equal(sd[k], v) for k, v in m.state_dict().items())


# ---------------------------------------------------------------------------------------------- pipeline
@pytest.mark.parametrize("separate", [False, True], ids=["joint", "separate"])
def test_pipeline_with_the_key_equals_the_sequential_pipeline(tmp_path, monkeypatch, separate):
    ec.pipeline_with_the_key_equals_the_sequential_pipeline(tmp_path, monkeypatch, "relu", separate)


@pytest.mark.parametrize("separate", [False, True], ids=["joint", "separate"])
def test_pipeline_with_leaky_relu_members_equals_the_sequential_pipeline(tmp_path, monkeypatch, separate):
    ec.pipeline_with_the_key_equals_the_sequential_pipeline(tmp_path, monkeypatch, "lrelu", separate)


def test_pipeline_refuses_a_batch_size_above_64_before_training_starts(tmp_path, monkeypatch):
    with pytest.raises(ValueError, match="128 rows.*at most 64 rows"):
        ec.run_pipeline(tmp_path, monkeypatch, "big", "relu", False, True, batch_size=128)
    assert not any(f.endswith("metrics.csv") or f.endswith(".pt") for f in ec.files(str(tmp_path / "logs_big")))
