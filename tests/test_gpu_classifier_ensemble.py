"""GPU: the classifier ensemble - every ``tl_*_group`` kernel bit for bit against its single-model launch (M = 1 and 3, every
member on inputs of its own), the active mask (a masked member's buffers, pre-filled with canaries, do not change by a bit),
``ClassifierEnsembleEngine`` against ``SimpleClassifierEngine`` on the low-rank, the dense and the mixed route,
``ClassifierEnsembleTrainer`` against sequential ``ClassifierTrainer(fused=True)`` runs with members that stop at different
epochs, and the pipeline key against the sequential pipeline.

All comparisons are exact (``torch.equal`` on the raw buffers): a group kernel IS the single kernel, launched with a member
dimension, and the single engine's own tests tie it to the float64 reference."""
import ctypes as C

import pytest
import torch
from torch.utils.data import TensorDataset

from tests import ensemble_cases as ec
from tests.ensemble_cases import CANARY, CASES, DEV, IDS
from tests.ensemble_cases import (canary as _canary, gen as _gen, lib as _lib, mask_words as _mask, on as _on, r4 as _r4,
                                  stream as _stream)

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------- forward and loss
@pytest.mark.parametrize("M,mask", CASES, ids=IDS)
@pytest.mark.parametrize("B,K,N", [(1, 4, 2), (7, 12, 3), (65, 260, 33)])
def test_linear_rows_and_ce_loss_group_equal_the_single_launches(M, mask, B, K, N):
    L, lib = _lib()
    g, ldd, words = _gen(B * 100 + N), _r4(N), 3 + N * N
    x = torch.randn(M, B, K, generator=g).to(DEV)
    W = (torch.randn(M, N, K, generator=g) * 0.3).to(DEV)
    bias = _canary(M, ldd)
    bias[:, :N] = torch.randn(M, N, generator=g).to(DEV)
    y = torch.randint(0, N, (M, B), generator=g).to(DEV)
    y[M - 1, 0] = N                                            # one label out of range, in one member only

    def stats_fill(rows):                                      # the statistics accumulate: start them from values of their own
        s = torch.arange(rows * words, dtype=torch.int64, device=DEV).reshape(rows, words) + 5
        s[:, 0] = torch.tensor([1.5], dtype=torch.float64).view(torch.int64).item()
        s[:, 2] = 0
        return s

    logits, dl, db, pred, stats = _canary(M, B, N), _canary(M, B, ldd), _canary(M, ldd), _canary(M, B, dtype=torch.int64), stats_fill(M)
    act = _mask(mask)
    L.check(lib.tl_linear_rows_group(x.data_ptr(), W.data_ptr(), bias.data_ptr(), logits.data_ptr(), M, B, K, N, K, 0, B * K, N * K,
                                     ldd, B * N, L.ptr(act), _stream()), "tl_linear_rows_group")
    base = stats.data_ptr()
    L.check(lib.tl_ce_loss_group(logits.data_ptr(), y.data_ptr(), dl.data_ptr(), db.data_ptr(), pred.data_ptr(), base, base + 8,
                                 base + 24, base + 16, M, B, N, N, ldd, 1.0 / B, B * N, B, B * ldd, ldd, B, words, L.ptr(act),
                                 _stream()), "tl_ce_loss_group")
    # prediction only (labels null): a second pred buffer, the statistics are not touched
    pred2, before = _canary(M, B, dtype=torch.int64), stats.clone()
    L.check(lib.tl_ce_loss_group(logits.data_ptr(), None, None, None, pred2.data_ptr(), None, None, None, None, M, B, N, N, ldd, 0.0,
                                 B * N, 0, 0, 0, B, 0, L.ptr(act), _stream()), "tl_ce_loss_group")
    torch.cuda.synchronize()
    assert torch.equal(stats, before)
    for m in range(M):
        if not _on(mask, m):
            assert torch.equal(logits[m], _canary(B, N)) and torch.equal(dl[m], _canary(B, ldd)) and torch.equal(db[m], _canary(ldd))
            assert torch.equal(pred[m], _canary(B, dtype=torch.int64)) and torch.equal(pred2[m], pred[m])
            assert torch.equal(stats[m], stats_fill(M)[m])
            continue
        s_logits, s_dl, s_db, s_pred, s_stats = _canary(B, N), _canary(B, ldd), _canary(N), _canary(B, dtype=torch.int64), stats_fill(M)[m]
        xm, wm, bm, ym = x[m].clone(), W[m].clone(), bias[m, :N].clone(), y[m].clone()
        L.check(lib.tl_linear_rows(xm.data_ptr(), wm.data_ptr(), bm.data_ptr(), s_logits.data_ptr(), B, K, N, K, 0, _stream()),
                "tl_linear_rows")
        sb = s_stats.data_ptr()
        L.check(lib.tl_ce_loss(s_logits.data_ptr(), ym.data_ptr(), s_dl.data_ptr(), s_db.data_ptr(), s_pred.data_ptr(), sb, sb + 8,
                               sb + 24, sb + 16, B, N, N, ldd, 1.0 / B, _stream()), "tl_ce_loss")
        torch.cuda.synchronize()
        assert torch.equal(logits[m], s_logits), m
        assert torch.equal(dl[m], s_dl) and torch.equal(db[m, :N], s_db) and torch.equal(db[m, N:], _canary(ldd - N)), m
        assert torch.equal(pred[m], s_pred) and torch.equal(pred2[m], s_pred), m
        assert torch.equal(stats[m], s_stats), m
        assert int(stats[m, 2]) == (1 if m == M - 1 else 0)                        # the range flag is the member's own


# ---------------------------------------------------------------------------------------------- updates
def _scalars(step, mu):
    from decode_tonal_langauge_amd.optim import nadam_scalars
    return nadam_scalars(step, mu, 0.01, 0.9, 0.999, 0.004)


@pytest.mark.parametrize("M,mask", CASES, ids=IDS)
@pytest.mark.parametrize("kr,rows,cols", [(1, 2, 4), (7, 3, 12), (64, 33, 260)])
def test_nadam_lowrank_group_equals_the_single_launch_over_two_steps(M, mask, kr, rows, cols):
    L, lib = _lib()
    g, ldfa = _gen(kr * 7 + rows), _r4(rows)
    p = torch.randn(M, rows, cols, generator=g).to(DEV)
    mo, vo = torch.zeros_like(p), torch.zeros_like(p)
    single = [(p[m].clone(), mo[m].clone(), vo[m].clone()) for m in range(M)]
    p0, act, mu = p.clone(), _mask(mask), 1.0
    for step in (1, 2):
        fa = torch.randn(M, kr, ldfa, generator=g).to(DEV)
        fb = torch.randn(M, kr, cols, generator=g).to(DEV)
        cg, cm, bc2, mu = _scalars(step, mu)
        args = (cg, cm, 0.9, 0.999, bc2, 1e-8, 0.01, 1.0)
        L.check(lib.tl_nadam_lowrank_group(p.data_ptr(), mo.data_ptr(), vo.data_ptr(), fa.data_ptr(), fb.data_ptr(), M, kr, rows, cols,
                                           ldfa, cols, rows * cols, kr * ldfa, kr * cols, *args, L.ptr(act), _stream()),
                "tl_nadam_lowrank_group")
        for m in range(M):
            sp, sm, sv = single[m]
            fam, fbm = fa[m].clone(), fb[m].clone()
            L.check(lib.tl_nadam_lowrank(sp.data_ptr(), sm.data_ptr(), sv.data_ptr(), fam.data_ptr(), fbm.data_ptr(), kr, rows, cols,
                                         ldfa, cols, *args, _stream()), "tl_nadam_lowrank")
        torch.cuda.synchronize()
    for m in range(M):
        if _on(mask, m):
            assert all(torch.equal(a[m], b) for a, b in zip((p, mo, vo), single[m])), m
            assert not torch.equal(p[m], p0[m])
        else:
            assert torch.equal(p[m], p0[m]) and not mo[m].any() and not vo[m].any()


@pytest.mark.parametrize("M,mask", CASES, ids=IDS)
@pytest.mark.parametrize("B,K,N", [(65, 260, 33), (70, 12, 3)])
def test_head_bwd_group_equals_the_single_launch(M, mask, B, K, N):
    L, lib = _lib()
    g, ldd = _gen(B + N), _r4(N)
    dl = torch.randn(M, B, ldd, generator=g).to(DEV)
    h = torch.randn(M, B, K, generator=g).to(DEV)
    W = torch.randn(M, N, K, generator=g).to(DEV)
    dw = _canary(M, N, K)
    L.check(lib.tl_head_bwd_group(dl.data_ptr(), h.data_ptr(), W.data_ptr(), dw.data_ptr(), M, B, K, N, ldd, B * ldd, B * K, N * K,
                                  N * K, L.ptr(_mask(mask)), _stream()), "tl_head_bwd_group")
    for m in range(M):
        if not _on(mask, m):
            assert torch.equal(dw[m], _canary(N, K))
            continue
        s_dw, dlm, hm, wm = _canary(N, K), dl[m].clone(), h[m].clone(), W[m].clone()
        L.check(lib.tl_head_bwd(dlm.data_ptr(), hm.data_ptr(), wm.data_ptr(), None, None, s_dw.data_ptr(), B, K, N, ldd, 0, 0.0,
                                _stream()), "tl_head_bwd")
        torch.cuda.synchronize()
        assert torch.equal(dw[m], s_dw), m


@pytest.mark.parametrize("M,mask", CASES, ids=IDS)
@pytest.mark.parametrize("n,stride", [(3, 4), (2, 4), (33, 36), (33 * 260, 33 * 260)])
def test_nadam_group_equals_the_single_launch(M, mask, n, stride):
    """The dense update: bias rows of N floats stored at row stride r4(N), and a whole weight gradient above rank 64."""
    L, lib = _lib()
    g = _gen(n)
    p = _canary(M, stride)
    p[:, :n] = torch.randn(M, n, generator=g).to(DEV)
    mo, vo = torch.zeros_like(p), torch.zeros_like(p)
    single = [(p[m].clone(), mo[m].clone(), vo[m].clone()) for m in range(M)]
    p0, act, mu = p.clone(), _mask(mask), 1.0
    for step in (1, 2):
        grad = _canary(M, stride)
        grad[:, :n] = torch.randn(M, n, generator=g).to(DEV)
        cg, cm, bc2, mu = _scalars(step, mu)
        args = (cg, cm, 0.9, 0.999, bc2, 1e-8, 0.0, 1.0)
        L.check(lib.tl_nadam_group(p.data_ptr(), grad.data_ptr(), mo.data_ptr(), vo.data_ptr(), M, n, stride, stride, *args,
                                   L.ptr(act), _stream()), "tl_nadam_group")
        for m in range(M):
            sp, sm, sv = single[m]
            gm = grad[m].clone()
            L.check(lib.tl_nadam(sp.data_ptr(), gm.data_ptr(), sm.data_ptr(), sv.data_ptr(), n, *args, _stream()), "tl_nadam")
        torch.cuda.synchronize()
    for m in range(M):
        if _on(mask, m):
            assert all(torch.equal(a[m], b) for a, b in zip((p, mo, vo), single[m])), m
            assert torch.equal(p[m, n:], _canary(stride - n)) and not mo[m, n:].any()      # the padding is nobody's
            assert not torch.equal(p[m, :n], p0[m, :n])
        else:
            assert torch.equal(p[m], p0[m]) and not mo[m].any() and not vo[m].any()


# ---------------------------------------------------------------------------------------------- gather
@pytest.mark.parametrize("M,mask", CASES, ids=IDS)
def test_gather_rows_group_against_torch_indexing(M, mask):
    """48-byte rows (16-byte accesses), 3-byte rows (byte accesses) and a channel list in one launch; repeated indices, a
    start offset into the table, canary rows behind every member's destination, one index out of range in one member."""
    L, lib = _lib()
    g, n, rows, pad, start, width = _gen(11), 29, 9, 2, 3, 16
    wide = torch.randn(n, 12, generator=g).to(DEV)
    small = torch.randint(0, 255, (n, 3), generator=g, dtype=torch.uint8).to(DEV)
    chans = torch.randn(n, 5, 4, generator=g).to(DEV)
    clist = torch.tensor([3, 0, 3], dtype=torch.int32, device=DEV)
    table = torch.randint(0, n, (M, width), generator=g)
    table[:, start + 2] = table[:, start + 1]                                  # a repeated index
    table[M - 1, start + 4] = n                                                # out of range: never read, never written
    table_dev = table.to(DEV)
    d_wide, d_small, d_chan = _canary(M, rows + pad, 12), torch.full((M, rows + pad, 3), 9, dtype=torch.uint8, device=DEV), \
        _canary(M, rows + pad, 3, 4)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    P4, L4 = C.c_void_p * 4, C.c_int64 * 4
    src = P4(wide.data_ptr(), small.data_ptr(), chans.data_ptr(), None)
    dst = P4(d_wide.data_ptr(), d_small.data_ptr(), d_chan.data_ptr(), None)
    stride = L4(*[t.stride(0) * t.element_size() for t in (d_wide, d_small, d_chan)], 0)
    L.check(lib.tl_gather_rows_group(src, dst, stride, L4(n, n, n, 0), L4(1, 1, 5, 0), L4(48, 3, 16, 0),
                                     P4(None, None, clist.data_ptr(), None), L4(0, 0, 3, 0), 3, table_dev.data_ptr() + 8 * start,
                                     width, rows, M, L.ptr(_mask(mask)), err.data_ptr(), _stream()), "tl_gather_rows_group")
    torch.cuda.synchronize()
    want_err = 1 if _on(mask, M - 1) else 0
    assert int(err.item()) == want_err
    for m in range(M):
        idx = table[m, start:start + rows]
        for got, source, fill in ((d_wide, wide, CANARY), (d_small, small, 9), (d_chan, chans[:, [3, 0, 3]], CANARY)):
            tail = torch.full_like(got[m, rows:], fill)
            assert torch.equal(got[m, rows:], tail), m                          # nothing behind the member's batch
            if not _on(mask, m):
                assert torch.equal(got[m, :rows], torch.full_like(got[m, :rows], fill)), m
                continue
            ok = (idx < n).to(DEV)
            assert torch.equal(got[m, :rows][ok], source[idx.to(DEV)[ok]]), m
            assert torch.equal(got[m, :rows][~ok], torch.full_like(got[m, :rows][~ok], fill)), m


def test_gather_group_of_the_resident_dataset():
    from decode_tonal_langauge_amd.data_loading.resident import ResidentDataset
    g = _gen(4)
    x, y = torch.randn(31, 2, 6, generator=g), torch.randint(0, 3, (31,), generator=g).float()
    rds = ResidentDataset.from_tensor_dataset(TensorDataset(x, y), device=DEV)
    table = torch.stack([torch.randperm(31, generator=g)[:20] for _ in range(3)])
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    gx, gy = rds.gather_group(table.to(DEV), 8, 13, err)
    assert gx.shape == (3, 5, 2, 6) and gy.shape == (3, 5) and int(err.item()) == 0
    for m in range(3):
        one = rds.gather(table[m].to(DEV), 8, 13, err)
        assert torch.equal(gx[m], one[0]) and torch.equal(gy[m], one[1])
        assert torch.equal(gx[m].cpu(), x[table[m, 8:13]])


# ---------------------------------------------------------------------------------------------- engine, trainer, pipeline
# (the bodies are tests/ensemble_cases.py's, shared with the shallow members' module)
@pytest.mark.parametrize("sizes", ec.KINDS["logistic"]["sizes"], ids=["lowrank", "dense", "dense_then_lowrank"])
def test_engine_steps_equal_the_single_engine(sizes):
    ec.engine_steps_equal_the_single_engine("logistic", sizes)


def test_engine_mask_freezes_a_member_and_names_the_member_with_a_bad_label():
    ec.engine_mask_freezes_a_member("logistic")


def test_trainer_equals_sequential_fused_runs_with_members_stopping_apart(tmp_path):
    ec.trainer_equals_sequential_fused_runs(tmp_path, "logistic")


@pytest.mark.parametrize("separate", [False, True], ids=["joint", "separate"])
def test_pipeline_with_the_key_equals_the_sequential_pipeline(tmp_path, monkeypatch, separate):
    ec.pipeline_with_the_key_equals_the_sequential_pipeline(tmp_path, monkeypatch, "logistic", separate)
