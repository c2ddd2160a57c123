"""The parent-side assembly of a data-parallel step (tests/dp_harness.py), checked on the CPU with the float64 oracle at the DP
tests' geometry: tests/test_gpu_dp_gradients.py trusts it to rebuild the global batch, branch planes and dropout mask from
the ranks' shards, so a wrong assembly must show up here rather than hide an error of the sharded step there."""
import pytest
import torch

from oracle import synthesis_oracle as so
from tests import dp_harness as dp
from tests import golden_inputs as gi
from tests.branch_planes import check_flips


@pytest.fixture(scope="module")
def step():
    """Seeded parameters of SynthesisModelCNN(80, 8, 100), a batch of 8 windows, a dropout mask of rate 0.5 and the oracle's
    own branches and gradients on it (no decisions supplied)."""
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
    torch.manual_seed(0)
    p = so.init_cnn_params(80, 8, 100)
    xs, tones, syls, labs, tg = gi.train_batches(1, 8, 8, 100, seed=77)
    g = torch.Generator().manual_seed(5)
    mask = 2.0 * (torch.rand(8, 64, so.latent_length(100), 8, generator=g) < 0.5).double()
    ref = dp.oracle_step(p, xs[0], labs[0], tg[0], mask=mask)
    return p, xs[0], labs[0], tg[0], mask, ref


def _shards(x, lab, tgt, mask, own, parts):
    """Rank shards of one batch: ``parts`` = [(row0, rows, weight)], each shard carrying its rows of every per-row array."""
    out = []
    for row0, rows, w in parts:
        sl = slice(row0, row0 + rows)
        out.append(dict(row0=row0, rows=rows, weight=w, x=x[sl], labels=lab[sl], targets=tgt[sl], mask=mask[sl],
                        dec={k: v[sl].clone() for k, v in own.items()}))
    return out


@pytest.mark.parametrize("n,parts", [(7, [(0, 3, 3 / 7), (3, 4, 4 / 7)]),             # uneven shards of a ragged batch
                                     (8, [(0, 8, 1.0), (0, 1, 0.0)]),                    # a weight-0 rank recomputing row 0
                                     (1, [(0, 1, 1.0), (0, 1, 0.0)])])                   # fewer rows than ranks
def test_assembled_shards_give_the_undecided_oracle_gradient_bit_for_bit(step, n, parts):
    p, x, lab, tgt, mask, ref = step
    if n < 8:
        x, lab, tgt, mask = x[:n], lab[:n], tgt[:n], mask[:n]
        ref = dp.oracle_step(p, x, lab, tgt, mask=mask)
    g = dp.assemble(_shards(x, lab, tgt, mask, ref["own"], parts))
    assert g["n"] == n
    assert torch.equal(g["x"], x) and torch.equal(g["labels"], lab) and torch.equal(g["targets"], tgt)
    assert torch.equal(g["mask"], mask)
    assert all(torch.equal(g["dec"][k], ref["own"][k]) for k in ref["own"])
    got = dp.oracle_step(p, g["x"], g["labels"], g["targets"], decisions=g["dec"], mask=g["mask"])
    check_flips(g["dec"], got["own"], got["margins"])
    assert got["loss"] == ref["loss"] and got["mcd"] == ref["mcd"]
    for k, v in ref["grads"].items():
        assert (got["grads"][k] == v).all(), k


def test_shards_assembled_in_the_wrong_order_are_rejected(step):
    """Rank 1's rows put first (each shard claiming the other's row offset): the shards still tile the batch, but the planes
    then belong to other windows, and check_flips rejects them against the oracle's own decisions on the inputs."""
    p, x, lab, tgt, mask, ref = step
    x, lab, tgt, mask = x[:7], lab[:7], tgt[:7], mask[:7]
    own = dp.oracle_step(p, x, lab, tgt, mask=mask)["own"]
    a, b = _shards(x, lab, tgt, mask, own, [(0, 3, 3 / 7), (3, 4, 4 / 7)])
    a["row0"], b["row0"] = 4, 0
    g = dp.assemble([a, b])
    got = dp.oracle_step(p, x, lab, tgt, decisions=g["dec"], mask=mask)
    with pytest.raises(AssertionError):
        check_flips(g["dec"], got["own"], got["margins"])


def test_assembly_refuses_shards_that_do_not_tile_the_batch(step):
    p, x, lab, tgt, mask, ref = step
    own = ref["own"]
    with pytest.raises(AssertionError):          # a gap
        dp.assemble(_shards(x, lab, tgt, mask, own, [(0, 3, 3 / 7), (4, 4, 4 / 7)]))
    with pytest.raises(AssertionError):          # a weight that is not rows / n (a weight-0 rank given 1 / n)
        dp.assemble(_shards(x, lab, tgt, mask, own, [(0, 1, 1.0), (0, 1, 1.0)]))
