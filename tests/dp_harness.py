"""The data-parallel test geometry and the parent-side view of a sharded step - TEST INFRASTRUCTURE.

``build`` is the model / trainer / batches of tests/test_gpu_dp.py and tests/test_gpu_dp_gradients.py (ranks spawned on the one
test GPU, gloo).  A rank reports its row shard of a step (``_row0``, rows, ``_weight``), the inputs and labels it used, its
branch planes (tests/branch_planes.hip_decisions) and its dropout keep mask (``read_dropout_mask``); ``assemble`` puts the
shards of the ranks back together in row order - the global batch, planes and mask of the step - and ``oracle_step`` runs the
float64 oracle's forward and backward on it with those branches.  ``assemble`` and ``oracle_step`` need no GPU: the same
functions are checked on the CPU (tests/test_dp_assembly.py), so a wrong assembly cannot hide an error of the sharded step."""
import math
import os

import numpy as np
import torch
import torch.multiprocessing as mp

WHH = "label_lstm.weight_hh_l0"
LONG_TONE_MAP = {"0": [3] * 10, "1": list(range(1, 11)), "2": [3, 2, 1, 2, 4, 3, 2, 1, 2, 4], "3": list(range(10, 0, -1))}


def batches(sizes=(8, 8)):
    """The global batches (ECoG, syllable-classifier input, tone-classifier input, targets) of the DP tests."""
    g = torch.Generator().manual_seed(11)
    return [(torch.randn(n, 8, 100, generator=g), torch.randn(n, 4, 100, generator=g),
             torch.randn(n, 4, 100, generator=g), 10 * torch.randn(n, 80, generator=g)) for n in sizes]


def build(dev, sizes=(8, 8), dropout=0.0, tone_map=None, n_syl=2):
    """``SynthesisModelCNN(80, 8, 100)`` (torch seed 0), its trainer and the batches.  ``n_syl`` syllable classes: with more
    than 16 (tone, syllable) pairs the trainer has no pair table (arbitrary label tensors)."""
    from decode_tonal_langauge_amd.models import LogisticRegressionClassifier, SynthesisModelCNN, SynthesisTrainer
    from tests import golden_inputs as gi
    torch.manual_seed(0)
    model = SynthesisModelCNN(80, 8, 100, dropout=dropout)
    tone = LogisticRegressionClassifier(4 * 100, 4)
    syl = LogisticRegressionClassifier(4 * 100, n_syl)
    tr = SynthesisTrainer(model, tone, syl, tone_map or gi.TONE_MAP, device=dev, verbose=False)
    return model, tr, batches(sizes)


def read_dropout_mask(eng, seed: int, p: float, row0: int, nb: int) -> torch.Tensor:
    """The keep mask * 1/(1-p) the concat kernel drew for windows [row0, row0 + nb) of the global batch with ``seed``: the
    kernel applied to an all-ones stage-5 activation.  (B, conv channels, latent, C), the layout of the reference's dropout
    input; the hash is indexed by the global element, so a rank's shard reads its own rows of the single-process mask."""
    from decode_tonal_langauge_amd._lib import check, ptr
    dev = eng._h[-1].device
    ones = torch.ones(nb * eng.C * eng.tp5, eng.ld5, device=dev)
    xc = torch.empty(nb * eng.C * eng.tp5, eng.ldx, device=dev)
    uid = torch.zeros(nb, dtype=torch.int32, device=dev)
    check(eng.lib.tl_concat_pack(ptr(ones), ptr(eng._h[-1]), ptr(uid), ptr(xc), nb, eng.C, eng.tp5, eng.lat, eng.Cc,
                                 eng.Lc, eng.ld5, eng.H, eng.ldx, p, seed, row0 * eng.C * eng.tp5,
                                 torch.cuda.current_stream().cuda_stream), "tl_concat_pack")
    return xc.view(nb, eng.C, eng.tp5, eng.ldx)[:, :, :eng.lat, :eng.Cc].permute(0, 3, 2, 1).contiguous()


def whh_gradient(eng, grads: dict, name: str = WHH):
    """The ``weight_hh_l0`` gradient the optimiser consumed after a backward pass, in float64 on the host, and its form:
    ("shard", rows r0 .. r0 + R of fa^T . fb), ("factors", fa^T . fb) or ("dense", the materialised gradient).  Returns
    (form, gradient rows, r0, factor rank or None)."""
    f = getattr(eng, "whh_factors", None)
    if f is None or f[0] is None:
        g = grads[name].detach().double().cpu()
        return "dense", g.numpy(), 0, None
    fa, fb = f[0].detach().double().cpu(), f[1].detach().double().cpu()
    g = (fa.t() @ fb).numpy()
    if len(f) == 4:
        assert g.shape[0] == f[3], (g.shape, f[3])
        return "shard", g, int(f[2]), int(fa.shape[0])
    return "factors", g, 0, int(fa.shape[0])


def spawn(target, world: int, port: int, timeout: float = 300, **kw) -> list:
    """``world`` ranks of ``target(rank, world, port, q, **kw)`` (spawned, one GPU over gloo); what each puts on the queue,
    in rank order (every rank puts ``(rank, result)``).  Every exit code is checked."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=target, args=(r, world, port, q), kwargs=kw) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=timeout) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0, p.exitcode
    return [r for _, r in sorted(res, key=lambda t: t[0])]


def port_base(base: int) -> int:
    return base + (os.getpid() % 1000)


def assemble(shards: list) -> dict:
    """The global batch of one step from the ranks' shards.  A shard: ``row0``, ``rows``, ``weight`` and per-row arrays
    (first axis = window) under ``x``, ``labels``, ``targets``, ``mask`` (or None) and ``dec`` (a dict of planes).  Ranks
    with weight 0 recomputed a row of a batch with fewer rows than ranks and are skipped; the others must tile the batch
    without gap or overlap, each with weight rows / n.  Returns the same keys for the whole batch, plus ``n``."""
    live = sorted((s for s in shards if s["weight"] != 0.0), key=lambda s: s["row0"])
    n = sum(s["rows"] for s in live)
    row = 0
    for s in live:
        assert s["row0"] == row, ("the shards do not tile the batch", [(t["row0"], t["rows"]) for t in live])
        assert math.isclose(s["weight"], s["rows"] / n, rel_tol=1e-12), (s["row0"], s["rows"], s["weight"], n)
        row += s["rows"]
    cat = lambda key: torch.cat([torch.as_tensor(s[key]) for s in live], dim=0)
    out = {"n": n, "x": cat("x"), "labels": cat("labels"), "targets": cat("targets")}
    out["mask"] = cat("mask") if live[0].get("mask") is not None else None
    out["dec"] = {k: torch.cat([torch.as_tensor(s["dec"][k]) for s in live], dim=0) for k in live[0]["dec"]}
    return out


def oracle_step(params: dict, x, labels, targets, decisions=None, mask=None) -> dict:
    """The float64 oracle on a global batch: forward (with ``mask``), backward on ``decisions`` (None: its own branches).
    ``targets`` are truncated like the trainer's (tl_l1_mcd).  Returns grads, loss, mcd, own, margins."""
    from oracle import synthesis_oracle as so
    leaves = {k: torch.as_tensor(v).double().clone().requires_grad_(True) for k, v in params.items()}
    own, margins = {}, {}
    out = so.cnn_forward(leaves, torch.as_tensor(x).double(), torch.as_tensor(labels).double(),
                         dropout_mask=None if mask is None else torch.as_tensor(mask).double(), decisions=decisions,
                         own=own, margins=margins)
    tgt = torch.as_tensor(targets).double().trunc()
    loss = so.l1_loss(out, tgt)
    grads = dict(zip(leaves, torch.autograd.grad(loss, list(leaves.values()))))
    with torch.no_grad():
        mcd = float((10.0 / math.log(10.0) * torch.sqrt(2.0 * ((out - tgt) ** 2).sum(dim=1))).mean())
    return {"grads": {k: v.numpy() for k, v in grads.items()}, "loss": float(loss.detach()), "mcd": mcd, "own": own,
            "margins": margins}


def rel_l2(a, b) -> float:
    a = np.asarray(a, dtype=np.float64).ravel()
    b = np.asarray(b, dtype=np.float64).ravel()
    return float(np.linalg.norm(a - b) / max(float(np.linalg.norm(b)), 1e-30))
