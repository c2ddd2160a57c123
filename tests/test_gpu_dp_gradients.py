"""GPU: the data-parallel step held at GRADIENT level against the float64 oracle.

tests/test_gpu_dp.py compares the parameters after NAdam with those of one process; NAdam divides by sqrt(v), so a gradient
that is a constant factor off (an output bias reduced twice, a W_hh gradient N times too large) moves the parameters by less
than those bounds.  Here ranks spawned on the one test GPU (gloo) report, for every step, the pre-step parameters, their row
shard, the inputs and labels they used, their branch planes and dropout mask, every exchanged gradient and the W_hh gradient
the optimiser consumed.  The parent re-assembles the global batch (tests/dp_harness.assemble), runs the float64 oracle's
backward on the ranks' branches (checked by branch_planes.check_flips) and holds every gradient to 5e-5 relative L2 - the
bound of the other decided-branch tests - the reduced ones bit-identical on every rank, the summed loss statistics to the
oracle's loss and MCD of the global batch, and each configuration to the exchange path it is there to cover."""
import os

import numpy as np
import pytest
import torch

from tests import dp_harness as dp
from tests.branch_planes import check_flips, flip_record, hip_decisions
from tests.parity_record import record

pytestmark = pytest.mark.gpu

GRAD_BOUND = 5e-5
STATS_BOUND = 1e-5
WHH = dp.WHH
OUTPUT_SPAN = 80 * 64 * 5 * 8 + 80          # output_layer.weight + .bias: the early bucket of the flat gradient buffer


def _trace(parallel, log):
    """Record the exchange calls of a step: (function, elements, extra) - the trainer and the engine look these up in the
    module at every call."""
    def wrap(name):
        fn = getattr(parallel, name)

        def run(t, *a, **k):
            if isinstance(t, (list, tuple)):
                log.append((name, sum(x.numel() for x in t), len(t)))
            elif name == "gather_lowrank":                 # (dg, h, keys): whether rows are de-duplicated by key
                log.append((name, t.numel(), (a[1] if len(a) > 1 else k.get("keys")) is not None))
            else:
                log.append((name, t.numel(), tuple(t.shape)))
            return fn(t, *a, **k)
        setattr(parallel, name, run)
    for name in ("all_reduce_", "all_reduce_async", "allreduce_bucketed", "gather_lowrank"):
        wrap(name)


def _grad_worker(rank, world, port, q, sizes=(8, 8), dropout=0.0, shard="1", tone_map=None, switch=None, n_syl=2):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK="0", TONAL_LSTM_SHARD=shard)
    from decode_tonal_langauge_amd import parallel
    parallel.init_from_env(backend="gloo")
    dev = torch.device("cuda:0")
    model, tr, batches = dp.build(dev, sizes, dropout, tone_map, n_syl)
    assert tr.world == world and tr.dp
    eng = model._engine
    log, seen = [], {}
    _trace(parallel, log)
    fused = tr._fused_step

    def fused_step(x, lab, tgt, graph=False):          # what the step consumed: this rank's shard and its labels
        seen.update(x=x.cpu().numpy(), labels=lab.cpu().numpy(), targets=tgt.cpu().numpy())
        return fused(x, lab, tgt, graph)
    tr._fused_step = fused_step
    model.train()
    steps = []
    for i, b in enumerate(batches):
        if switch is not None and i in switch:
            assert tr.set_lstm_shard(switch[i]) == switch[i]
        tr.sync_parameters()                          # the row-sharded W_hh is stale on the other ranks' rows without it
        torch.cuda.synchronize()
        pre = {k: v.detach().cpu().numpy() for k, v in model.named_parameters()}
        del log[:]
        tr.train_step(*b)
        torch.cuda.synchronize()
        nb = seen["x"].shape[0]
        form, whh, r0, kr = dp.whh_gradient(eng, tr._grads)
        s = dict(pre=pre, row0=int(tr._row0), rows=nb, weight=float(tr._weight), **seen,
                 dec={k: v.numpy() for k, v in hip_decisions(eng, nb, 8).items()},
                 mask=(dp.read_dropout_mask(eng, eng._seed_used, eng._p_drop_used, tr._row0, nb).cpu().numpy()
                       if eng._p_drop_used > 0 else None),
                 grads={k: v.detach().cpu().numpy() for k, v in tr._grads.items() if k != WHH},
                 whh=(form, whh, r0, kr), sh=eng._sh, table=bool(eng._table_labels), U=int(eng._U), L=int(eng._L),
                 calls=list(log), stats=tr._stats.cpu().numpy().copy())
        steps.append(s)
    torch.cuda.synchronize()
    q.put((rank, steps))
    torch.distributed.destroy_process_group()


def _uniq_rows(labels) -> set:
    return {tuple(r) for r in np.asarray(labels).reshape(len(labels), -1).tolist()}


def _check(res, name, expect):
    """``res``: per rank, per step.  ``expect(step, shards)`` asserts the path of one step."""
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    world, nsteps = len(res), len(res[0])
    worst, obs, loss_sum, mcd_sum = {}, {}, 0.0, 0.0
    for s in range(nsteps):
        shards = [r[s] for r in res]
        expect(s, shards)
        pre = shards[0]["pre"]
        for sh in shards[1:]:
            for k in pre:
                assert np.array_equal(sh["pre"][k], pre[k]), ("pre-step replicas differ", s, k)
        g = dp.assemble(shards)
        ref = dp.oracle_step(pre, g["x"], g["labels"], g["targets"], decisions=g["dec"], mask=g["mask"])
        flips = check_flips(g["dec"], ref["own"], ref["margins"])
        for k, v in flip_record(flips).items():
            obs[k] = max(obs.get(k, 0.0), v)
        rows = {}
        for rank, sh in enumerate(shards):
            for k, v in sh["grads"].items():
                e = dp.rel_l2(v, ref["grads"][k])
                worst[k] = max(worst.get(k, 0.0), e)
                assert e <= GRAD_BOUND, (name, s, rank, k, e)
            form, whh, r0, _kr = sh["whh"]
            e = dp.rel_l2(whh, ref["grads"][WHH][r0:r0 + whh.shape[0]])
            worst[WHH] = max(worst.get(WHH, 0.0), e)
            assert e <= GRAD_BOUND, (name, s, rank, WHH, form, e)
            rows[r0] = whh.shape[0]
        # every row of the W_hh gradient is held by some rank
        assert sum(rows.values()) == ref["grads"][WHH].shape[0] or set(rows) == {0}, rows
        # reduced gradients (and the LSTM gradients every rank forms from the global dgates) are the same bits everywhere
        for sh in shards[1:]:
            for k in shards[0]["grads"]:
                assert np.array_equal(sh["grads"][k], shards[0]["grads"][k]), (name, s, k)
            if shards[0]["whh"][0] != "shard":
                assert np.array_equal(sh["whh"][1], shards[0]["whh"][1]), (name, s, WHH)
        # the per-rank statistics carry the rank's weight: their sums are the global batch's loss / MCD
        loss_sum += ref["loss"]
        mcd_sum += ref["mcd"]
        st = np.sum([sh["stats"].astype(np.float64) for sh in shards], axis=0)
        for i, want in enumerate((loss_sum, mcd_sum, ref["loss"], ref["mcd"])):
            e = abs(st[i] - want) / abs(want)
            obs[f"stats{i}"] = max(obs.get(f"stats{i}", 0.0), e)
            assert e <= STATS_BOUND, (name, s, i, float(st[i]), want)
    print(name, "worst gradient rel L2", f"{max(worst.values()):.2e}", max(worst, key=worst.get))
    record(f"DP gradients vs float64 oracle on the ranks' branches: {name} ({world} ranks, {nsteps} steps)",
           dict({"grad." + k: v for k, v in worst.items()}, **obs))


def _sharded_step(shards, U=8, L=5):
    for sh in shards:
        assert sh["sh"] is not None and sh["table"], "the label LSTM must have run row-sharded"
        form, whh, r0, kr = sh["whh"]
        assert form == "shard" and kr == (L - 1) * U and sh["U"] == U and sh["L"] == L
        assert (r0, whh.shape[0]) == (sh["sh"][0], sh["sh"][1])
        asy = [c for c in sh["calls"] if c[0] == "all_reduce_async"]
        assert [c[1] for c in asy][:1] == [OUTPUT_SPAN] and len(asy) == 2, sh["calls"]      # early output-layer bucket
        assert not any(c[0] in ("allreduce_bucketed", "gather_lowrank") for c in sh["calls"]), sh["calls"]


def _reduce_rows_step(shards, U=8, L=5):
    for sh in shards:
        assert sh["sh"] is None and sh["table"], "whole LSTM per rank on the label table"
        form, _whh, _r0, kr = sh["whh"]
        assert form == "factors" and kr == (L - 1) * U
        assert ("all_reduce_", (L - 1) * U * 4 * 240, ((L - 1) * U, 4 * 240)) in sh["calls"], sh["calls"]   # reduce_rows(fa)
        asy = [c for c in sh["calls"] if c[0] == "all_reduce_async"]
        assert [c[1] for c in asy][:1] == [OUTPUT_SPAN] and len(asy) == 2, sh["calls"]
        assert not any(c[0] in ("allreduce_bucketed", "gather_lowrank") for c in sh["calls"]), sh["calls"]


def _run(base, **kw):
    world = kw.pop("world", 2)
    return dp.spawn(_grad_worker, world, dp.port_base(base), timeout=300, **kw)


def test_dp_gradients_even_shards_row_sharded_lstm():
    res = _run(40500)

    def expect(s, shards):
        assert [(sh["row0"], sh["rows"], sh["weight"]) for sh in shards] == [(0, 4, 0.5), (4, 4, 0.5)]
        _sharded_step(shards)
    _check(res, "a: 8 + 8, row-sharded LSTM", expect)


def test_dp_gradients_ragged_shards_weight_zero_rank_and_dropout():
    res = _run(41500, sizes=(7, 1, 8), dropout=0.5)

    def expect(s, shards):
        want = [[(0, 3, 3 / 7), (3, 4, 4 / 7)], [(0, 1, 1.0), (0, 1, 0.0)], [(0, 4, 0.5), (4, 4, 0.5)]][s]
        assert [(sh["row0"], sh["rows"], sh["weight"]) for sh in shards] == want
        assert all(sh["mask"] is not None for sh in shards)
        _sharded_step(shards)
    _check(res, "b: 7 (3 + 4), 1 (weight-0 rank), 8, dropout 0.5", expect)


def test_dp_gradients_unsharded_lstm_reduces_factor_rows():
    res = _run(42500, shard="0")

    def expect(s, shards):
        _reduce_rows_step(shards)
    _check(res, "c: 8 + 8, TONAL_LSTM_SHARD=0", expect)


def test_dp_gradients_sharded_lstm_fallback_dense_whh():
    res = _run(43500, tone_map=dp.LONG_TONE_MAP)

    def expect(s, shards):
        for sh in shards:
            assert sh["sh"] is None and sh["table"] and sh["L"] == 10 and sh["U"] == 8, "(L - 1) U = 72 > 64: fallback"
            assert sh["whh"][0] == "dense"
            assert ("all_reduce_", 72 * 960, (72, 960)) in sh["calls"], sh["calls"]
            asy = [c for c in sh["calls"] if c[0] == "all_reduce_async"]
            assert [c[1] for c in asy] == [OUTPUT_SPAN], sh["calls"]                # only the early bucket ...
            assert [c[0] for c in sh["calls"]].count("allreduce_bucketed") == 1      # ... and the fallback branch
    _check(res, "d: 8 + 8, 10-entry tone map (sharded LSTM falls back)", expect)


def test_dp_gradients_without_pair_table_gather_with_key_dedup():
    """Five syllable classes: 20 (tone, syllable) pairs > 16, so the trainer keeps no pair table; every rank runs the LSTM on
    its own distinct label rows and the W_hh factors are gathered, rows of equal (step, label sequence) summed."""
    res = _run(44500, n_syl=5)
    overlap = []

    def expect(s, shards):
        ranks_rows = [_uniq_rows(sh["labels"]) for sh in shards]
        union = set().union(*ranks_rows)
        overlap.append(len(union) < sum(len(r) for r in ranks_rows))
        pad = len({len(r) for r in ranks_rows}) > 1          # zero rows of the shorter factors share one key
        for sh, mine in zip(shards, ranks_rows):
            assert sh["sh"] is None and not sh["table"] and sh["U"] == len(mine)
            form, _whh, _r0, kr = sh["whh"]
            assert form == "factors" and kr == (sh["L"] - 1) * len(union) + pad, (kr, len(union), pad)
            assert [c for c in sh["calls"] if c[0] == "gather_lowrank"] == [("gather_lowrank", (sh["L"] - 1) * len(mine) * 960,
                                                                            True)], sh["calls"]
    _check(res, "e: 8 + 8, no pair table (gather with key de-duplication)", expect)
    assert any(overlap), "no label sequence was shared between the ranks: the de-duplication went untested"


def test_dp_gradients_three_ranks():
    res = _run(45500, world=3, sizes=(8, 7))
    sharded = (4 * 240) % (4 * 3) == 0

    def expect(s, shards):
        want = [[(0, 2), (2, 3), (5, 3)], [(0, 2), (2, 2), (4, 3)]][s]
        assert [(sh["row0"], sh["rows"]) for sh in shards] == want
        if sharded:
            _sharded_step(shards)
        else:
            assert all(sh["sh"] is None for sh in shards)
    _check(res, "f: 8 (2 + 3 + 3), 7 (2 + 2 + 3)", expect)


def test_dp_gradients_across_the_lstm_shard_switch():
    res = _run(46500, sizes=(8, 8, 8), switch={1: False, 2: True})

    def expect(s, shards):
        (_reduce_rows_step if s == 1 else _sharded_step)(shards)
    _check(res, "g: 8, 8, 8 with set_lstm_shard {1: False, 2: True}", expect)
