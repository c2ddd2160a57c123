"""GPU: data-parallel classifier training on the HIP path - ``tl_dropout_scale_at``, ``tl_pool3_fwd_shard`` /
``tl_pool3_bwd_shard``, the sharded ``SimpleClassifierEngine`` / ``CnnClassifierTrainEngine`` / ``CnnRnnClassifierTrainEngine``
and ``ClassifierTrainer(fused=True)`` under a process group.  Two ranks are spawned on the one test GPU over gloo
(``tests/dp_harness.spawn``); one spawn per model runs everything the tests of that model need.

How the bounds are formed.  Masks, predictions, counts, confusion matrices and the replica spread are compared exactly.  The
parameters of the 2-rank run after the three steps on global batches of 6, 5 (shards 2 + 3) and 1 (one rank on weight 0) are
compared with the single-process fused run on the same batches, one tensor at a time, as ``rel_l2`` of the two 3-step updates;
the bound of a tensor is 10 yardsticks, a yardstick being ``rel_l2`` between the float32 and the float64 CPU restatement of the
same three steps (autograd + ``torch.optim.NAdam`` with the two decay groups; the deep references run on the planes and keep
masks the HIP path took, read off the single-process engine).  A sharded sum differs from the whole one by its summation order
alone; a wrong 1 / N or shard weight moves the second and third update by order 1.  Every figure is printed and recorded
(``classifier_dp_*``) before it is asserted.

Which planes the deep restatements run on.  Two HIP runs are compared, and from the second step on their parameters differ in
their last bits, so a pre-activation that sits on a tie (a pool pair, a LeakyReLU input at 0) can fall either way in one of
them: over the three steps one or two of ~10^6 branches do.  Such a flip re-routes one element's gradient - at batch 1 a visible
part of a bias gradient - and is no error of either run.  So the two restatements mirror the two runs: the float64 one runs on
the planes the single process took, the float32 one on the planes the 2-rank run took (the shards' planes put together in
row order).  Where no branch differs these are the same planes and the yardstick is the plain float32-against-float64 distance;
where one does, the distance holds what the reference itself makes of that flip.  The planes are not trusted for this:
``_flips`` holds both runs' planes, step by step, to the decisions the float64 restatement takes on the parameters the step
started from, with ``branch_planes.check_flips`` - a branch may differ only within 1e-4 of the layer's scale of a tie, and only
a handful per plane - and step 1 must show no difference between the runs.  A shard weight or 1 / N that is wrong flips no planes and moves the updates by order 1 (checked once by
hand: a mean of local means in place of 1 / B_global).

Observed on an MI355X: ``profiles/parity_observed.json``, sections ``classifier_dp_*``."""
import copy
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import classifier_train_ref as ref
from tests import cnn_classifier_ref as cref
from tests import cnnrnn_classifier_ref as rref
from tests import dp_harness, parity_record

pytestmark = pytest.mark.gpu
DEV = "cuda"
LR, WD = 5e-3, 0.01
SIZES = (6, 5, 1)
_REC = {}


def _held(section, name, dev, yard):
    bound = ref.FACTOR * yard
    print(f"[{section}] {name}: 2-rank vs single {dev:.3e}  yardstick {yard:.3e}  bound {bound:.3e}")
    _REC.setdefault(section, {}).update({name + "_gpu": dev, name + "_bound": bound})
    parity_record.record("classifier_dp_" + section, _REC[section])
    return dev <= bound


def _lib():
    from decode_tonal_langauge_amd import _lib as L
    return L, L.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---------------------------------------------------------------------------------------------- 1. kernels
@pytest.mark.parametrize("n,index0", [(1000, 0), (777, 12345), (5, (1 << 33) + 3)])
def test_dropout_scale_at_is_a_slice_of_the_whole_mask(n, index0):
    L, lib = _lib()
    x = torch.randn(n, device=DEV)
    a, b = x.clone(), x.clone()
    L.check(lib.tl_dropout_scale(a.data_ptr(), n, 0.5, 99, _stream()), "tl_dropout_scale")
    L.check(lib.tl_dropout_scale_at(b.data_ptr(), n, 0.5, 99, 0, _stream()), "tl_dropout_scale_at")
    assert torch.equal(a, b)                                                               # zero offset: the same bits
    if index0 and index0 < (1 << 20):
        whole = torch.ones(index0 + n, device=DEV)
        part = torch.ones(n, device=DEV)
        L.check(lib.tl_dropout_scale(whole.data_ptr(), whole.numel(), 0.5, 99, _stream()), "tl_dropout_scale")
        L.check(lib.tl_dropout_scale_at(part.data_ptr(), n, 0.5, 99, index0, _stream()), "tl_dropout_scale_at")
        assert torch.equal(part, whole[index0:]) and 0 < int((part == 0).sum()) < n
    elif index0:                                                                           # past 2^32: a 64-bit index
        hi, lo = torch.ones(64, device=DEV), torch.ones(64, device=DEV)
        L.check(lib.tl_dropout_scale_at(hi.data_ptr(), 64, 0.5, 99, index0, _stream()), "tl_dropout_scale_at")
        L.check(lib.tl_dropout_scale_at(lo.data_ptr(), 64, 0.5, 99, index0 & 0xFFFFFFFF, _stream()), "tl_dropout_scale_at")
        assert not torch.equal(hi, lo) and 0 < int((hi == 0).sum()) < 64                   # the high word reaches the hash


def test_cnn_feature_rows_of_a_shard_draw_their_rows_of_the_mask():
    """The ``CNNClassifier`` layout: rows [(b * C + c) * tp + t][ld], a shard at b0 starts at b0 * C * tp * ld."""
    L, lib = _lib()
    B, C, tp, ld, b0, nb = 5, 3, 7, 12, 2, 3
    whole = torch.ones(B * C * tp, ld, device=DEV)
    part = torch.ones(nb * C * tp, ld, device=DEV)
    L.check(lib.tl_dropout_scale(whole.data_ptr(), whole.numel(), 0.3, 5, _stream()), "tl_dropout_scale")
    L.check(lib.tl_dropout_scale_at(part.data_ptr(), part.numel(), 0.3, 5, b0 * C * tp * ld, _stream()), "tl_dropout_scale_at")
    assert torch.equal(part, whole[b0 * C * tp:(b0 + nb) * C * tp])


def _pool3(fn, Y, B, w1, Cn, Cc, Tp, tq, p, seed, extra=(), dX=None, slope=0.1):
    L, lib = _lib()
    W = w1 + Cn
    if dX is None:
        X = torch.full((tq * B, Cc * W), float("nan"), device=DEV)
        L.check(getattr(lib, fn)(Y.data_ptr(), X.data_ptr(), B, w1, Cn, Cc, Tp, tq, Cc, 1, B, p, seed, *extra, _stream()), fn)
        return X
    dZ = torch.full((B * W * Tp, Cc), float("nan"), device=DEV)
    L.check(getattr(lib, fn)(Y.data_ptr(), dX.data_ptr(), dZ.data_ptr(), B, w1, Cn, Cc, Tp, tq, Cc, Cc, 1, B, p, seed, slope,
                             *extra, _stream()), fn)
    return dZ


def _shard_rows(t, B, w1, Cn, b0, nb):
    """Rows of the branch-major (B * (w1 + Cn), ...) tensor that belong to batch rows [b0, b0 + nb), in shard order."""
    return torch.cat((t[b0 * w1:(b0 + nb) * w1], t[B * w1 + b0 * Cn:B * w1 + (b0 + nb) * Cn]))


@pytest.mark.parametrize("w1,Cn", [(2, 3), (1, 2)])
def test_pool3_shard_draws_the_rows_of_the_single_process_mask(w1, Cn):
    B, Cc, Tp, tq, p, seed = 5, 256, 12, 3, 0.5, 4242
    b0, nb = 2, 2                                                                          # a shard that starts mid-batch
    W = w1 + Cn
    g = torch.Generator().manual_seed(3)
    Y = torch.randn(B * W * Tp, Cc, generator=g).to(DEV)
    dX = torch.randn(tq * B, Cc * W, generator=g).to(DEV)
    # zero offsets: the bits of the existing entry points
    X0 = _pool3("tl_pool3_fwd", Y, B, w1, Cn, Cc, Tp, tq, p, seed)
    assert torch.equal(X0, _pool3("tl_pool3_fwd_shard", Y, B, w1, Cn, Cc, Tp, tq, p, seed, extra=(0, B)))
    Z0 = _pool3("tl_pool3_bwd", Y, B, w1, Cn, Cc, Tp, tq, p, seed, dX=dX)
    assert torch.equal(Z0, _pool3("tl_pool3_bwd_shard", Y, B, w1, Cn, Cc, Tp, tq, p, seed, extra=(0, B), dX=dX))
    assert not bool(torch.isnan(X0).any()) and not bool(torch.isnan(Z0).any())
    # the mask: all-ones input (every row triple of a sequence pools to 1), whole batch against the shard
    ones = torch.ones(B * W * Tp, Cc, device=DEV)
    whole = _pool3("tl_pool3_fwd", ones, B, w1, Cn, Cc, Tp, tq, p, seed)                   # rows s * B + b
    Ys = _shard_rows(ones.view(B * W, Tp, Cc), B, w1, Cn, b0, nb).reshape(-1, Cc).contiguous()
    part = _pool3("tl_pool3_fwd_shard", Ys, nb, w1, Cn, Cc, Tp, tq, p, seed, extra=(b0, B))
    want = whole.view(tq, B, -1)[:, b0:b0 + nb].reshape(tq * nb, -1)
    assert torch.equal(part, want)
    dropped = float((part == 0).float().mean())
    assert abs(dropped - p) < 0.05, dropped
    # both branches of the column order took part: column % W < w1 is an LSTM-branch column, the rest are electrodes
    is_lstm = (torch.arange(Cc * W, device=DEV) % W) < w1
    for cols in (part[:, is_lstm], part[:, ~is_lstm]):
        assert 0 < int((cols == 0).sum()) < cols.numel()
    wrong = _pool3("tl_pool3_fwd_shard", Ys, nb, w1, Cn, Cc, Tp, tq, p, seed, extra=(0, nb))
    assert not torch.equal(wrong, want)                                                    # the local index draws another mask
    # backward: the same keep decisions, local dZ addressing
    Zs = _pool3("tl_pool3_bwd_shard", _shard_rows(Y.view(B * W, Tp, Cc), B, w1, Cn, b0, nb).reshape(-1, Cc).contiguous(), nb, w1,
                Cn, Cc, Tp, tq, p, seed, extra=(b0, B),
                dX=dX.view(tq, B, -1)[:, b0:b0 + nb].reshape(tq * nb, -1).contiguous())
    assert torch.equal(Zs.view(nb * W, Tp, Cc), _shard_rows(Z0.view(B * W, Tp, Cc), B, w1, Cn, b0, nb))


# ---------------------------------------------------------------------------------------------- the cases
def _case(kind, dropout):
    """(model on the CPU, [(x, y)] global batches of ``SIZES``) - the same in every process."""
    from decode_tonal_langauge_amd.models.simple_classifiers import LogisticRegressionClassifier, ShallowNNClassifier
    g = torch.Generator().manual_seed(77)
    if kind == "logistic":
        torch.manual_seed(5)
        model, shape, n = LogisticRegressionClassifier(1600, 3), (16, 100), 3
    elif kind == "shallow":
        torch.manual_seed(6)
        model, shape, n = ShallowNNClassifier(320, 3, 32, "LeakyReLU"), (8, 40), 3
    elif kind == "cnn":
        model, _, _ = cref.build((1, 8, 150, 3), 7, dropout)
        shape, n = (8, 150), 3
    else:
        model, _, _ = rref.build((1, 8, 48, 48, 3), 8, dropout)
        shape, n = (8, 48), 3
    data = [(torch.randn(B, *shape, generator=g), torch.randint(0, n, (B,), generator=g)) for B in SIZES]
    return model, data


def _engine(kind, model):
    if kind == "cnn":
        from decode_tonal_langauge_amd._cnn_classifier_train_engine import CnnClassifierTrainEngine as E
    elif kind == "cnnrnn":
        from decode_tonal_langauge_amd._cnnrnn_classifier_train_engine import CnnRnnClassifierTrainEngine as E
    else:
        from decode_tonal_langauge_amd._simple_classifier_engine import SimpleClassifierEngine as E
    return E(copy.deepcopy(model).to(DEV), LR, WD)


def _np(t):
    return t.detach().cpu().numpy()


def _factors(eng):
    names = {p: k for k, p in eng.model.named_parameters()}
    return {names.get(k, k): (_np(fa), _np(fb)) for k, (fa, fb) in getattr(eng, "last_lowrank", {}).items()}


def _run(kind, dropout, planes=False):
    """Three train steps, the epoch statistics, an evaluation pass and the predictions of one engine (any number of ranks)."""
    model, data = _case(kind, dropout)
    eng = _engine(kind, model)
    eng.model.train()
    out = {"planes": [], "keep": [], "grad_keys": None, "factors": None}
    eng.model.eval()                               # on the initial parameters: the same terms in every run
    for x, y in data:
        eng.eval_batch(x.to(DEV), y.to(DEV))
    ls, cnt, cm = eng.epoch_stats()
    out["eval0_stats"] = (ls, cnt, cm.numpy())
    out["pred0"] = [_np(eng.predict_batch(x.to(DEV))) for x, _ in data]
    eng.model.train()
    for i, (x, y) in enumerate(data):
        if planes:                                 # the parameters the step starts from: where ``_flips`` judges its branches
            out.setdefault("before", []).append({k: v.detach().cpu().clone() for k, v in eng.model.named_parameters()})
        eng.train_batch(x.to(DEV), y.to(DEV))
        torch.cuda.synchronize()
        if i == 0:
            names = {p: k for k, p in eng.model.named_parameters()}
            out["grad_keys"] = sorted(names.get(k, k) for k in eng.grads)
            out["factors"] = _factors(eng)
        if kind in ("cnn", "cnnrnn"):
            r = cref if kind == "cnn" else rref
            rows = eng._plan.rows                  # (the whole batch without a process group)
            out["planes"].append({k: v.numpy() for k, v in r.hip_planes(eng, rows).items()} if eng.dp else r.hip_planes(eng, rows))
            out["keep"].append(r.hip_keep_mask(eng, rows) if planes else None)
            out.setdefault("live", []).append(eng._plan.live)
    out["params"] = {k: _np(v) for k, v in eng.model.named_parameters()}
    ls, cnt, cm = eng.epoch_stats()
    out["train_stats"] = (ls, cnt, cm.numpy())
    eng.model.eval()
    for x, y in data:
        eng.eval_batch(x.to(DEV), y.to(DEV))
    ls, cnt, cm = eng.epoch_stats()
    out["eval_stats"] = (ls, cnt, cm.numpy())
    out["pred"] = [_np(eng.predict_batch(x.to(DEV))) for x, _ in data]
    if kind == "logistic":                         # one batch above LOWRANK_MAX: the dense path
        g = torch.Generator().manual_seed(78)
        x, y = torch.randn(65, 16, 100, generator=g), torch.randint(0, 3, (65,), generator=g)
        eng2 = _engine(kind, model)
        eng2.train_batch(x.to(DEV), y.to(DEV))
        eng2.train_batch(x.to(DEV)[:33], y.to(DEV)[:33])
        eng2.force_dense = True
        eng2.train_batch(x.to(DEV)[:33], y.to(DEV)[:33])
        torch.cuda.synchronize()
        out["dense_params"] = {k: _np(v) for k, v in eng2.model.named_parameters()}
        out["dense_grad_numel"] = int(sum(t.numel() for t in eng2.grads.values()))
    return out


def _worker(rank, world, port, q, kind="logistic", dropout=0.0):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    from decode_tonal_langauge_amd import parallel
    parallel.init_from_env(backend="gloo")
    out = _run(kind, dropout)
    q.put((rank, out))
    torch.distributed.destroy_process_group()


def _dense_case():
    model, _ = _case("logistic", 0.0)
    g = torch.Generator().manual_seed(78)
    x, y = torch.randn(65, 16, 100, generator=g), torch.randint(0, 3, (65,), generator=g)
    return model, [(x, y), (x[:33], y[:33]), (x[:33], y[:33])]


# ---------------------------------------------------------------------------------------------- CPU restatements
def _deep_updates(kind, dropout, single, dtype, planes=None):
    """theta_after - theta_before of the three steps on the CPU in ``dtype``, on the planes a HIP run took (``planes``: one dict
    per step; default the single-process run's) and the single-process run's keep masks (a shard draws its rows of the same
    mask: the kernel tests)."""
    r = cref if kind == "cnn" else rref
    model, data = _case(kind, dropout)
    p = r.leaves(model, dtype)
    before = {k: v.detach().clone() for k, v in p.items()}
    decay = [v for v in p.values() if v.ndim >= 2]
    rest = [v for v in p.values() if v.ndim < 2]
    opt = torch.optim.NAdam([{"params": decay, "weight_decay": WD}, {"params": rest, "weight_decay": 0.0}], lr=LR)
    first = None
    for (x, y), pl, keep in zip(data, planes or single["planes"], single["keep"]):
        _, _, g = r.loss_and_grads(model, p, x, y, planes=pl, keep=keep)
        first = first or {k: v.detach().clone() for k, v in g.items()}
        for k, v in p.items():
            v.grad = g[k]
        opt.step()
    return {k: v.detach() - before[k] for k, v in p.items()}, first


@functools.lru_cache(maxsize=None)
def _both(kind, dropout, port):
    """(single-process run, [rank 0's run, rank 1's run]) of a case: computed once, shared by the tests of the case."""
    single = _run(kind, dropout, planes=True)
    ranks = dp_harness.spawn(_worker, 2, dp_harness.port_base(port), kind=kind, dropout=dropout)
    return single, ranks


def _initial(kind, dropout):
    return {k: _np(v) for k, v in _case(kind, dropout)[0].named_parameters()}


def _check_common(kind, dropout, single, ranks, yards, tag):
    init = _initial(kind, dropout)
    ok = []
    for k in sorted(init):
        # replica spread 0: both ranks end with identical bits
        assert np.array_equal(ranks[0]["params"][k], ranks[1]["params"][k]), (tag, k)
        dev = ref.rel_l2(ranks[0]["params"][k] - init[k], single["params"][k] - init[k])
        ok.append(_held("steps", f"{tag}_{k}", dev, yards[k]))
    assert all(ok), tag
    n_all = sum(SIZES)
    for which in ("eval0_stats", "train_stats", "eval_stats"):
        assert single[which][1] == n_all
        for r in ranks:
            assert r[which][1] == n_all, (which, r[which][1])                               # the weight-0 duplicate is not counted
            assert r[which][0] == ranks[0][which][0] and np.array_equal(r[which][2], ranks[0][which][2])   # equal on both ranks
            assert int(r[which][2].sum()) == n_all
    # on the initial parameters the two runs evaluate the same terms: confusion matrix and predictions exactly, the fp64 loss sum
    # to 1e-12 relative
    ls1, _, cm1 = single["eval0_stats"]
    for r in ranks:
        ls2, _, cm2 = r["eval0_stats"]
        rel = abs(ls2 - ls1) / abs(ls1)
        print(f"[stats] {tag}: loss sum single {ls1!r} 2-rank {ls2!r} rel {rel:.3e}")
        _REC.setdefault("stats", {})[f"{tag}_loss_sum_rel"] = rel
        parity_record.record("classifier_dp_stats", _REC["stats"])
        assert np.array_equal(cm1, cm2), tag
        assert rel <= 1e-12, (tag, rel)
        assert [len(a) for a in r["pred0"]] == list(SIZES)
        assert all(np.array_equal(a, b) for a, b in zip(r["pred0"], single["pred0"])), tag
        assert all(np.array_equal(a, b) for a, b in zip(r["pred"], ranks[0]["pred"])), tag


@pytest.mark.parametrize("kind", ["logistic", "shallow"])
def test_simple_classifiers_two_ranks_match_the_single_process(kind):
    single, ranks = _both(kind, 0.0, 31100 + (kind == "shallow"))
    model, data = _case(kind, 0.0)
    m64, d64 = ref.as_double(model, data)
    u64, u32 = ref.updates_after(m64, d64, LR, WD), ref.updates_after(model, data, LR, WD)
    yards = {k: ref.rel_l2(u32[k], u64[k]) for k in u64}
    _check_common(kind, 0.0, single, ranks, yards, kind)
    # no dense weight gradient on any rank at B_global <= 64: the biases alone
    want = ["linear.bias"] if kind == "logistic" else ["hidden.bias", "output.bias"]
    assert single["grad_keys"] == want and all(r["grad_keys"] == want for r in ranks)
    # the gathered factors of the first step (identical parameters): B_global rows in global row order
    x, y = data[0]

    def cpu_factors(dtype):
        m = copy.deepcopy(model).to(dtype)
        xx = x.reshape(len(y), -1).to(dtype)
        if kind == "logistic":
            z = m.linear(xx)
            z.retain_grad()
            F.cross_entropy(z, y).backward()
            return {"linear.weight": (z.grad, xx)}
        pre = m.hidden(xx)
        pre.retain_grad()
        h = m.activation(pre)
        z = m.output(h)
        z.retain_grad()
        F.cross_entropy(z, y).backward()
        return {"output.weight": (z.grad, h.detach()), "hidden.weight": (pre.grad, xx)}
    f64, f32 = cpu_factors(torch.float64), cpu_factors(torch.float32)
    ok = []
    for r, run in enumerate(ranks):
        assert set(run["factors"]) == set(f64)
        for k in sorted(f64):
            for j, side in enumerate(("fa", "fb")):
                got, one = run["factors"][k][j], single["factors"][k][j]
                assert got.shape == one.shape == tuple(f64[k][j].shape), (k, side, got.shape)
                yard = max(ref.rel_l2(f32[k][j], f64[k][j]), 2.0 ** -24)                    # (x itself is exact in both)
                ok.append(_held("factors", f"{kind}_rank{r}_{k}_{side}", ref.rel_l2(got, one), yard))
    assert all(ok), kind
    if kind == "logistic":
        model, data = _dense_case()
        m64, d64 = ref.as_double(model, data)
        u64, u32 = ref.updates_after(m64, d64, LR, WD), ref.updates_after(model, data, LR, WD)
        init = _initial(kind, 0.0)
        ok = []
        for k in sorted(u64):
            assert np.array_equal(ranks[0]["dense_params"][k], ranks[1]["dense_params"][k])
            dev = ref.rel_l2(ranks[0]["dense_params"][k] - init[k], single["dense_params"][k] - init[k])
            ok.append(_held("steps", f"logistic_dense_B65_{k}", dev, ref.rel_l2(u32[k], u64[k])))
        assert all(ok)
        assert all(r["dense_grad_numel"] == model.get_nparams() for r in ranks)            # dW exists on the dense path


def _assembled_planes(ranks):
    """The planes of the 2-rank run per step, the live ranks' shards put together in global row order."""
    out = []
    for step in range(len(SIZES)):
        shards = [r["planes"][step] for r in ranks if r["live"][step]]
        out.append({k: torch.as_tensor(np.concatenate([sh[k] for sh in shards], axis=0)) for k in shards[0]})
    return out


def _flips(kind, dropout, tag, single, dp_planes):
    """How many discrete branches (pool arg-max, LeakyReLU sign) the 2-rank run took differently from the single process, per
    step - printed and recorded.  Step 1 starts from identical parameters and must show none.  Neither run's planes are
    trusted: each is held by ``branch_planes.check_flips`` to the decisions the float64 restatement takes for itself on the
    parameters the single-process step started from (the 2-rank run's differ from those in their last bits): a branch may
    differ only where the reference was within 1e-4 of its scale of flipping, and only a handful may, so a plane that differs
    for any reason but a near-tie fails here."""
    from tests import branch_planes
    r = cref if kind == "cnn" else rref
    model, data = _case(kind, dropout)
    for step, (whole, mine) in enumerate(zip(single["planes"], dp_planes)):
        own, margins = {}, {}
        with torch.no_grad():
            r.forward(model, {k: v.double() for k, v in single["before"][step].items()}, data[step][0],
                      keep=single["keep"][step], own=own, margins=margins)
        diff = {k: int((mine[k] != torch.as_tensor(v)).sum()) for k, v in whole.items()}
        diff = {k: n for k, n in diff.items() if n}
        worst = 0.0
        for name, planes in (("single", whole), ("2-rank", mine)):
            held = branch_planes.check_flips({k: torch.as_tensor(v) for k, v in planes.items()}, own, margins)
            worst = max([worst] + [w for _, w in held.values()])
        print(f"[flips] {tag} step {step + 1} (batch {SIZES[step]}): {sum(diff.values())} branches differ between the runs "
              f"{diff}; largest margin / scale of a branch either run took against the float64 restatement: {worst:.2e}")
        _REC.setdefault("flips", {}).update({f"{tag}_step{step + 1}": sum(diff.values()),
                                             f"{tag}_step{step + 1}_worst_margin": worst})
        parity_record.record("classifier_dp_flips", _REC["flips"])
        if step == 0:
            assert not diff, (tag, diff)


@pytest.mark.parametrize("dropout", [0.0, 0.5])
@pytest.mark.parametrize("kind", ["cnn", "cnnrnn"])
def test_deep_classifiers_two_ranks_match_the_single_process(kind, dropout):
    single, ranks = _both(kind, dropout, 31200 + 2 * (kind == "cnnrnn") + (dropout > 0))
    assert all((k is not None) == (dropout > 0) for k in single["keep"])
    # the two restatements mirror the two runs that are compared: float64 on the branches the single process took, float32 on
    # the branches the 2-rank run took (see the module docstring)
    dp_planes = _assembled_planes(ranks)
    u64, g64 = _deep_updates(kind, dropout, single, torch.float64)
    u32, g32 = _deep_updates(kind, dropout, single, torch.float32, planes=dp_planes)
    yards = {k: ref.rel_l2(u32[k], u64[k]) for k in u64}
    tag = f"{kind}_p{dropout}"
    _flips(kind, dropout, tag, single, dp_planes)
    _check_common(kind, dropout, single, ranks, yards, tag)
    if kind == "cnnrnn":
        return
    lin = ["classifier.1.weight", "classifier.3.weight"]
    ok = []
    for r, run in enumerate(ranks):
        assert not set(lin) & set(run["grad_keys"])                                         # no dense fc1 / fc2 buffer on any rank
        assert sorted(run["factors"]) == lin
        for k in lin:
            (fa, fb), (sa, sb) = run["factors"][k], single["factors"][k]
            assert fa.shape == sa.shape and fb.shape == sb.shape and fa.shape[0] == SIZES[0]
            prod = lambda a, b: torch.as_tensor(a).double().t() @ torch.as_tensor(b).double()
            ok.append(_held("factors", f"{tag}_rank{r}_{k}", ref.rel_l2(prod(fa, fb), prod(sa, sb)), ref.rel_l2(g32[k], g64[k])))
    assert all(ok), tag


# ---------------------------------------------------------------------------------------------- trainer
def _trainer_data():
    return tuple(ref.planted(n, seed=s) for n, s in ((70, 3), (21, 4), (9, 5)))


def _fit(log_dir, fused=True):
    from decode_tonal_langauge_amd.models.classifier_trainer import ClassifierTrainer
    from decode_tonal_langauge_amd.models.simple_classifiers import ShallowNNClassifier
    torch.manual_seed(9)
    model = ShallowNNClassifier(1600, 4, 32, "ReLU").to(DEV)
    (x, y), (vx, vy), (tx, ty) = _trainer_data()
    dev = lambda a, b: ref.batches(a.to(DEV), b.to(DEV), 32)
    tr = ClassifierTrainer(model, 0.02, WD, log_dir=log_dir, fused=fused)
    hist = tr.fit(dev(x, y), dev(vx, vy), max_epochs=12, patience=2)
    res = tr.test(dev(tx, ty))
    return hist, tr.stopped_epoch, res["confusion_matrix"].numpy(), _np(tr.predict(dev(tx, ty)))


def _trainer_worker(rank, world, port, q, log_dir=None):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    from decode_tonal_langauge_amd import parallel
    from decode_tonal_langauge_amd.models.classifier_trainer import ClassifierTrainer
    from decode_tonal_langauge_amd.models.simple_classifiers import LogisticRegressionClassifier
    parallel.init_from_env(backend="gloo")
    try:
        ClassifierTrainer(LogisticRegressionClassifier(16, 2).to(DEV), fused=False)
        refused = None
    except ValueError as e:
        refused = str(e)
    # every rank is given a directory of its own name: what exists afterwards shows who wrote
    out = _fit(os.path.join(log_dir, f"rank{rank}"))
    q.put((rank, out + (refused,)))
    torch.distributed.destroy_process_group()


def test_two_rank_trainer_stops_together_and_writes_once(tmp_path):
    from decode_tonal_langauge_amd.models.classifier_trainer import ClassifierTrainer
    from decode_tonal_langauge_amd.models.simple_classifiers import ShallowNNClassifier
    hist1, stop1, cm1, pred1 = _fit(str(tmp_path / "single"))
    ranks = dp_harness.spawn(_trainer_worker, 2, dp_harness.port_base(31300), log_dir=str(tmp_path))
    (h0, s0, cm0, p0, refused0), (h1, s1, cm1r, p1, refused1) = ranks
    assert h0 == h1 and s0 == s1 and np.array_equal(cm0, cm1r) and np.array_equal(p0, p1)   # the same values on every rank
    assert s0 == stop1 and len(h0) == len(hist1)
    assert refused0 and refused1 and "fused=True" in refused0
    assert sorted(os.listdir(tmp_path / "rank0")) == ["confusion_matrix_test.csv", "metrics.csv"]
    assert not os.path.exists(tmp_path / "rank1")                                          # rank 1 wrote nothing
    # the history against the single process: the yardstick is the float32 CPU loop against the float64 one
    (x, y), (vx, vy), _ = _trainer_data()
    torch.manual_seed(9)
    model = ShallowNNClassifier(1600, 4, 32, "ReLU")
    cpu = lambda a, b, dt=torch.float32: ref.batches(a.to(dt), b, 32)
    n = len(hist1)
    h32 = ref.parent_fit(copy.deepcopy(model), 0.02, WD, cpu(x, y), cpu(vx, vy), n)
    h64 = ref.parent_fit(copy.deepcopy(model).double(), 0.02, WD, cpu(x, y, torch.float64), cpu(vx, vy, torch.float64), n)
    ok = []
    for key in ("train/loss_epoch", "val/loss", "train/weight_norm"):
        rel = lambda h, base: max(abs(a[key] - b[key]) / abs(b[key]) for a, b in zip(h, base))
        ok.append(_held("trainer", key, rel(h0, hist1), rel(h32, h64)))
    assert all(ok)
    assert [r["val/accuracy"] for r in h0] == [r["val/accuracy"] for r in hist1]
    assert np.array_equal(cm0, cm1) and np.array_equal(p0, pred1)


# ---------------------------------------------------------------------------------------------- rehearsal
def _rehearsal_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0",
                      TONAL_DP_FORCE="1", TONAL_DIST_BACKEND="tl")
    from decode_tonal_langauge_amd import parallel
    parallel.init_from_env()
    assert parallel.active() and parallel.tl_active()
    out = {}
    for kind, dropout in (("logistic", 0.0), ("shallow", 0.0), ("cnn", 0.5), ("cnnrnn", 0.5)):
        model, data = _case(kind, dropout)
        eng = _engine(kind, model)
        assert eng.dp and eng.world == 1
        eng.model.train()
        eng.train_batch(data[0][0].to(DEV), data[0][1].to(DEV))
        torch.cuda.synchronize()
        out[kind] = ({k: _np(v) for k, v in eng.model.named_parameters()}, eng.epoch_stats()[1])
    parallel.tl_comm_destroy()
    q.put((0, out))
    torch.distributed.destroy_process_group()


def test_single_rank_rehearsal_over_the_c_abi_handle():
    got = dp_harness.spawn(_rehearsal_worker, 1, dp_harness.port_base(31400))[0]
    ok = []
    for kind, dropout in (("logistic", 0.0), ("shallow", 0.0), ("cnn", 0.5), ("cnnrnn", 0.5)):
        model, data = _case(kind, dropout)
        eng = _engine(kind, model)
        assert not eng.dp
        eng.model.train()
        eng.train_batch(data[0][0].to(DEV), data[0][1].to(DEV))
        torch.cuda.synchronize()
        init = _initial(kind, dropout)
        one = [data[0]]
        if kind in ("logistic", "shallow"):
            m64, d64 = ref.as_double(model, one)
            u64, u32 = ref.updates_after(m64, d64, LR, WD), ref.updates_after(model, one, LR, WD)
        else:
            r = cref if kind == "cnn" else rref
            single = {"planes": [r.hip_planes(eng, SIZES[0])], "keep": [r.hip_keep_mask(eng, SIZES[0])]}
            u64, u32 = (_deep_updates(kind, dropout, single, dt)[0] for dt in (torch.float64, torch.float32))
        params, count = got[kind]
        assert count == SIZES[0]
        for k, v in eng.model.named_parameters():
            ok.append(_held("rehearsal", f"{kind}_{k}", ref.rel_l2(params[k] - init[k], _np(v) - init[k]), ref.rel_l2(u32[k], u64[k])))
    assert all(ok)
