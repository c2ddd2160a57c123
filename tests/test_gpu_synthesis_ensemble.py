"""The SynthesisLite ensemble (all repeats of one experiment in one pass) against the single path, bit for bit.

1. every new ``tl_*_group`` entry against its single entry: M = 3 members with distinct weights and inputs, every output of
   member m ``torch.equal`` to the single launch on member m's inputs; again with ``active = [1, 0, 1]``: member 1's outputs,
   pre-filled with a sentinel, are untouched.  The two GEMM group entries in every form the engine uses, at S1 - S3.
2. ``LiteEnsembleEngine`` + ``SynthesisEnsembleTrainer`` against ``SynthesisTrainer`` runs of each member alone: loss / MCD
   words, parameters and BatchNorm buffers equal after every step; with the HIP graph on (replays reached) and off.
3. one member of the S1 group against the float64 oracle (the helper and bounds of tests/test_gpu_lite_shapes.py).
4. ``train_synthesizer.train`` with and without ``ensemble``: equal MCDs, losses and reconstructed mels; the label pass over
   M B rows against the per-member pass.
"""
import ctypes as C
import json
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

from tests import golden_inputs as gi
from tests.synthesis_ensemble_cases import M, S1, S2, SEEDS, SENTINEL, SHAPES, classifiers, dims, lite_models, step_batches

pytestmark = pytest.mark.gpu

# The bound tests/test_gpu_lite_shapes.py::test_lite_trainer_steps_follow_float64_oracle puts on a parameter's update vector
# after a trainer step (there a literal inside the test body, so it cannot be imported; the forward bound is imported below)
LITE_UPDATE_BOUND = 5e-4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    from decode_tonal_langauge_amd import _lib
    return _lib.load()


def _st():
    return torch.cuda.current_stream().cuda_stream


def p(t):
    return None if t is None else t.data_ptr()


# ---------------------------------------------------------------------------------------------- 1. group entry vs single entry
class Case:
    """Tensors of one kernel: ``ins`` / ``outs`` / ``inouts`` map a name to a per-member shape (dtype float32 unless given as
    (shape, dtype)); ``single(t)`` / ``group(t, s)`` return the argument lists (without active / stream), ``t`` the member's (or
    member 0's) tensors by name and ``s`` the member strides in elements."""

    def __init__(self, single_fn, group_fn, ins, outs, single, group, inouts=None, positive=()):
        self.single_fn, self.group_fn, self.ins, self.outs, self.inouts = single_fn, group_fn, ins, outs, inouts or {}
        self.single, self.group, self.positive = single, group, positive


def _alloc(spec, dev, gen, fill=None, positive=False):
    shape, dtype = spec if isinstance(spec[0], tuple) else (spec, torch.float32)
    full = (M,) + tuple(shape)
    if fill is not None:
        return torch.full(full, fill, dtype=dtype, device=dev)
    if dtype == torch.int64:
        return torch.randint(0, 1 << 40, full, generator=gen, dtype=dtype).to(dev)
    t = torch.randn(full, generator=gen)
    return (t.abs() + 0.5 if positive else t).to(dev)


def _run_case(lib, dev, case, active):
    gen = torch.Generator().manual_seed(17)
    t = {k: _alloc(v, dev, gen, positive=k in case.positive) for k, v in case.ins.items()}
    init = {k: _alloc(v, dev, gen, positive=k in case.positive) for k, v in case.inouts.items()}
    # the single launches, member by member, on the member's slices of the inputs
    want = []
    for m in range(M):
        tm = {k: v[m].contiguous() for k, v in t.items()}
        tm.update({k: v[m].clone() for k, v in init.items()})
        tm.update({k: _alloc(v, dev, gen, fill=SENTINEL)[0] for k, v in case.outs.items()})
        tm["_m"] = m
        rc = getattr(lib, case.single_fn)(*case.single(tm), _st())
        assert rc == 0, (case.single_fn, lib.tl_last_error())
        want.append(tm)
    tg = dict(t)
    tg.update({k: v.clone() for k, v in init.items()})
    tg.update({k: _alloc(v, dev, gen, fill=SENTINEL) for k, v in case.outs.items()})
    strides = {k: v.stride(0) for k, v in tg.items()}
    act = None if active is None else torch.tensor(active, dtype=torch.int32, device=dev)
    rc = getattr(lib, case.group_fn)(*case.group(tg, strides), p(act), _st())
    assert rc == 0, (case.group_fn, lib.tl_last_error())
    torch.cuda.synchronize()
    for m in range(M):
        on = active is None or active[m]
        for k in case.outs:
            if on:
                assert torch.equal(tg[k][m], want[m][k]), (case.group_fn, k, m)
            else:
                assert bool((tg[k][m] == SENTINEL).all()), (case.group_fn, k, m, "a masked member was written")
        for k in case.inouts:
            assert torch.equal(tg[k][m], want[m][k] if on else init[k][m]), (case.group_fn, k, m)


def _cases(cfg):
    d = dims(cfg)
    B, Cn, T, D, CC, H, ld, L, T1, T2, F, ldf, ldd, hid = (d[k] for k in ("B", "C", "T", "D", "CC", "H", "ld", "L", "T1", "T2", "F",
                                                                          "ldf", "ldd", "hid"))
    out = {}
    for tag, (cin, tt, k, pad) in {"1": (Cn, T, 5, 2), "2": (CC, T1, 3, 1)}.items():
        nt = (tt + 63) // 64
        out["conv_fwd" + tag] = Case(
            "tl_lite_conv_fwd", "tl_lite_conv_fwd_group",
            dict(x=(B, cin, tt), w=(CC, cin, k), b=(CC,)), dict(z=(B, CC, tt), part=(B * nt, CC, 2)),
            lambda t, cin=cin, tt=tt, k=k, pad=pad: [p(t["x"]), p(t["w"]), p(t["b"]), p(t["z"]), p(t["part"]), B, cin, CC, tt, k, pad],
            lambda t, s, cin=cin, tt=tt, k=k, pad=pad: [p(t["x"]), p(t["w"]), p(t["b"]), p(t["z"]), p(t["part"]), M, B, cin, CC, tt, k,
                                                        pad, s["x"], s["w"], s["b"], s["z"], s["part"]])
        out["bn_finalize" + tag] = Case(
            "tl_lite_bn_finalize", "tl_lite_bn_finalize_group",
            dict(part=(B * nt, CC, 2)), dict(mean=(CC,), rstd=(CC,)),
            lambda t, tt=tt, nt=nt: [p(t["part"]), p(t["mean"]), p(t["rstd"]), p(t["rm"]), p(t["rv"]), B * nt, CC, B * tt, tt, 0.1,
                                     1e-5, 1, p(t["n"])],
            lambda t, s, tt=tt, nt=nt: [p(t["part"]), p(t["mean"]), p(t["rstd"]), p(t["rm"]), p(t["rv"]), M, B * nt, CC, B * tt, tt,
                                        0.1, 1e-5, 1, p(t["n"]), s["part"], s["mean"], s["rm"], s["n"]],
            inouts=dict(rm=(CC,), rv=(CC,), n=((1,), torch.int64)), positive=("rv", "part"))
        out["bn_act_pool_fwd" + tag] = Case(
            "tl_lite_bn_act_pool_fwd", "tl_lite_bn_act_pool_fwd_group",
            dict(z=(B, CC, tt), mean=(CC,), rstd=(CC,), g=(CC,), b=(CC,)), dict(y=(B, CC, tt // 2)),
            lambda t, tt=tt: [p(t["z"]), p(t["mean"]), p(t["rstd"]), p(t["g"]), p(t["b"]), p(t["y"]), B, CC, tt, 0.01],
            lambda t, s, tt=tt: [p(t["z"]), p(t["mean"]), p(t["rstd"]), p(t["g"]), p(t["b"]), p(t["y"]), M, B, CC, tt, 0.01, s["z"],
                                 s["mean"], s["g"], s["y"]], positive=("rstd",))
        out["bn_act_pool_bwd" + tag] = Case(
            "tl_lite_bn_act_pool_bwd", "tl_lite_bn_act_pool_bwd_group",
            dict(dy=(B, CC, tt // 2), z=(B, CC, tt), mean=(CC,), rstd=(CC,), g=(CC,), b=(CC,)),
            dict(dz=(B, CC, tt), dg=(CC,), db=(CC,), work=(B * CC * 2,)),
            lambda t, tt=tt: [p(t["dy"]), p(t["z"]), p(t["mean"]), p(t["rstd"]), p(t["g"]), p(t["b"]), p(t["dz"]), p(t["dg"]),
                              p(t["db"]), p(t["work"]), B, CC, tt, 0.01, 1],
            lambda t, s, tt=tt: [p(t["dy"]), p(t["z"]), p(t["mean"]), p(t["rstd"]), p(t["g"]), p(t["b"]), p(t["dz"]), p(t["dg"]),
                                 p(t["db"]), p(t["work"]), M, B, CC, tt, 0.01, 1, s["dy"], s["z"], s["mean"], s["g"], s["dz"],
                                 s["dg"], s["work"]], positive=("rstd",))
        n = CC * cin * k
        out["conv_bwd" + tag] = Case(
            "tl_lite_conv_bwd", "tl_lite_conv_bwd_group",
            dict(dz=(B, CC, tt), x=(B, cin, tt), w=(CC, cin, k)), dict(dx=(B, cin, tt), dwp=(B, n), dbp=(B, CC)),
            lambda t, cin=cin, tt=tt, k=k, pad=pad: [p(t["dz"]), p(t["x"]), p(t["w"]), p(t["dx"]), p(t["dwp"]), p(t["dbp"]), B, cin,
                                                     CC, tt, k, pad],
            lambda t, s, cin=cin, tt=tt, k=k, pad=pad: [p(t["dz"]), p(t["x"]), p(t["w"]), p(t["dx"]), p(t["dwp"]), p(t["dbp"]), M, B,
                                                        cin, CC, tt, k, pad, s["dz"], s["x"], s["w"], s["dx"], s["dwp"], s["dbp"]])
        out["sum_slabs2" + tag] = Case(
            "tl_sum_slabs2", "tl_sum_slabs2_group",
            dict(a=(B, n), b=(B, CC)), dict(da=(n,), db=(CC,)),
            lambda t, n=n: [p(t["a"]), p(t["da"]), n, p(t["b"]), p(t["db"]), CC, B],
            lambda t, s, n=n: [p(t["a"]), p(t["da"]), n, p(t["b"]), p(t["db"]), CC, B, M, s["a"], s["da"], s["b"], s["db"]])
    out["lstm_fwd"] = Case(
        "tl_lite_lstm_fwd", "tl_lite_lstm_fwd_group",
        dict(xl=(B, L, ld), wih=(4 * H, ld), whh=(4 * H, H), bih=(4 * H,), bhh=(4 * H,)),
        dict(act=(B, L, 4 * H), cs=(B, L, H), hs=(B, L, H)),
        lambda t: [p(t["xl"]), p(t["wih"]), p(t["whh"]), p(t["bih"]), p(t["bhh"]), p(t["act"]), p(t["cs"]), p(t["hs"]), B, L, H, ld],
        lambda t, s: [p(t["xl"]), p(t["wih"]), p(t["whh"]), p(t["bih"]), p(t["bhh"]), p(t["act"]), p(t["cs"]), p(t["hs"]), M, B, L, H,
                      ld, s["xl"], s["wih"], s["whh"], s["bih"], s["act"], s["cs"]])
    out["lstm_bwd"] = Case(
        "tl_lite_lstm_bwd", "tl_lite_lstm_bwd_group",
        dict(dh=(B, H), whh=(4 * H, H), act=(B, L, 4 * H), cs=(B, L, H)), dict(dg=(B, L, 4 * H)),
        lambda t: [p(t["dh"]), p(t["whh"]), p(t["act"]), p(t["cs"]), p(t["dg"]), B, L, H, H],
        lambda t, s: [p(t["dh"]), p(t["whh"]), p(t["act"]), p(t["cs"]), p(t["dg"]), M, B, L, H, H, s["dh"], s["whh"], s["act"],
                      s["cs"]])
    out["lstm_ih_grad"] = Case(
        "tl_lstm_ih_grad", "tl_lstm_ih_grad_group",
        dict(dg=(B, L, 4 * H), xl=(B, L, ld)), dict(dw=(4 * H, ld), db=(4 * H,), db2=(4 * H,)),
        lambda t: [p(t["dg"]), p(t["xl"]), p(t["dw"]), p(t["db"]), p(t["db2"]), 1, B * L, H, ld],
        lambda t, s: [p(t["dg"]), p(t["xl"]), p(t["dw"]), p(t["db"]), p(t["db2"]), M, 1, B * L, H, ld, s["dg"], s["xl"], s["dw"],
                      s["db"]])
    # the dropout seed: the single launch reads the member's word, the group launch the table
    out["cat"] = Case(
        "tl_lite_cat_dev", "tl_lite_cat_group",
        dict(y2=(B, F), hs=(B, L, H), seed=((1,), torch.int64)), dict(feat=(B, ldf)),
        lambda t: [p(t["y2"]), p(t["hs"]), p(t["feat"]), B, F, H, L, ldf, 0.3, p(t["seed"])],
        lambda t, s: [p(t["y2"]), p(t["hs"]), p(t["feat"]), M, B, F, H, L, ldf, 0.3, p(t["seed"]), s["y2"], s["hs"], s["feat"]])
    out["uncat"] = Case(
        "tl_lite_uncat_dev", "tl_lite_uncat_group",
        dict(df=(B, ldf), seed=((1,), torch.int64)), dict(dy2=(B, F), dh=(B, H)),
        lambda t: [p(t["df"]), p(t["dy2"]), p(t["dh"]), B, F, H, ldf, 0.3, p(t["seed"])],
        lambda t, s: [p(t["df"]), p(t["dy2"]), p(t["dh"]), M, B, F, H, ldf, 0.3, p(t["seed"]), s["df"], s["dy2"], s["dh"]])
    sk, n = 4, B * hid
    out["splitk_bias_lrelu"] = Case(
        "tl_splitk_bias_lrelu", "tl_splitk_bias_lrelu_group",
        dict(slab=(sk, n), bias=(hid,)), dict(out=(n,)),
        lambda t: [p(t["slab"]), p(t["bias"]), p(t["out"]), sk, n, hid, 0.01],
        lambda t, s: [p(t["slab"]), p(t["bias"]), p(t["out"]), sk, n, hid, 0.01, M, n, s["slab"], s["bias"], s["out"]])
    out["l1_mcd"] = Case(
        "tl_l1_mcd", "tl_l1_mcd_group",
        dict(o=(B, D), tgt=(B, D)), dict(dout=(B, ldd)),
        lambda t: [p(t["o"]), p(t["tgt"]), p(t["dout"]), p(t["stats"]), B, D, ldd, 1, 1.0],
        lambda t, s: [p(t["o"]), p(t["tgt"]), p(t["dout"]), p(t["stats"]), M, B, D, ldd, 1, 1.0, s["o"], s["tgt"], s["dout"]],
        inouts=dict(stats=(4,)))
    nc4 = ldd
    rpb = max(1, 256 // (nc4 // 4))
    nblk = int(min(256, max(1, B // (rpb * 4))))
    out["colsum"] = Case(
        "tl_colsum", "tl_colsum_group",
        dict(g=(B, ldd)), dict(part=(nblk, nc4)),
        lambda t: [p(t["g"]), p(t["part"]), nblk, B, nc4, ldd, 1, 1],
        lambda t, s: [p(t["g"]), p(t["part"]), nblk, B, nc4, ldd, 1, 1, M, s["g"], s["part"]])
    return out


_KERNELS = sorted(_cases(S1))


@pytest.mark.parametrize("active", [None, [1, 0, 1]], ids=["all", "masked"])
@pytest.mark.parametrize("kernel", _KERNELS)
@pytest.mark.parametrize("shape", ["S1", "S2"])
def test_group_entry_matches_single_entry(dev, lib, shape, kernel, active):
    # (l1_mcd at S1: dout's padding column, ldd 8 > D 7, is written by neither launch and keeps the sentinel on both sides)
    _run_case(lib, dev, _cases(SHAPES[shape])[kernel], active)


def test_splitk_bias_lrelu_group_slab_major_layout(dev, lib):
    """The [nz][M][n] slab layout (zs = M n, member stride n) gives what [M][nz][n] gives."""
    sk, n, hid = 3, 5 * 512, 512
    gen = torch.Generator().manual_seed(2)
    slab = torch.randn(M, sk, n, generator=gen).to(dev)
    bias = torch.randn(M, hid, generator=gen).to(dev)
    a, b = torch.empty(M, n, device=dev), torch.empty(M, n, device=dev)
    assert lib.tl_splitk_bias_lrelu_group(p(slab), p(bias), p(a), sk, n, hid, 0.01, M, n, sk * n, hid, n, None, _st()) == 0
    zmajor = slab.permute(1, 0, 2).contiguous()
    assert lib.tl_splitk_bias_lrelu_group(p(zmajor), p(bias), p(b), sk, n, hid, 0.01, M, M * n, n, hid, n, None, _st()) == 0
    torch.cuda.synchronize()
    assert torch.equal(a, b)


# ---- the two GEMM group entries, in the forms LiteEnsembleEngine launches
def _nt_forms(cfg):
    d = dims(cfg)
    B, D, hid, ldf, ldd = d["B"], d["D"], d["hid"], d["ldf"], d["ldd"]
    bm = 32 if B <= 64 else 128
    sk1 = int(max(1, min((ldf + 31) // 32, 256 // (((B + bm - 1) // bm) * ((hid + 127) // 128)))))
    sk3 = int(max(1, min((hid + 31) // 32, 64 // (((B + bm - 1) // bm) * ((D + 127) // 128)))))
    skd = int(max(1, min((hid + 31) // 32, 256 // (((B + bm - 1) // bm) * ((ldf + 127) // 128)))))
    # name: (N, K, splitk, epilogue, bias?)
    return bm, {"fc1 forward (STORE, split-K)": (hid, ldf, sk1, 0, False),
                "fc3 forward (STORE, split-K)": (D, hid, sk3, 0, False),
                "fc3 forward (STORE, bias)": (D, hid, 1, 0, True),
                "fc1 input gradient (STORE, split-K)": (ldf, hid, skd, 0, False),
                "fc3 input gradient (MASK with aux)": (hid, ldd, 1, 3, False)}


@pytest.mark.parametrize("active", [None, [1, 0, 1]], ids=["all", "masked"])
@pytest.mark.parametrize("shape", ["S1", "S2", "S3"])
def test_nt_group_fc_matches_single(dev, lib, shape, active):
    from decode_tonal_langauge_amd._lib import NtParams
    cfg = SHAPES[shape]
    B = cfg[0]
    bm, forms = _nt_forms(cfg)
    gen = torch.Generator().manual_seed(9)
    act = None if active is None else torch.tensor(active, dtype=torch.int32, device=dev)
    for name, (N, K, sk, epi, with_bias) in forms.items():
        A = torch.randn(M, B, K, generator=gen).to(dev)
        W = torch.randn(M, N, K, generator=gen).to(dev)
        bias = torch.randn(M, N, generator=gen).to(dev) if with_bias else None
        aux = torch.randn(M, B, N, generator=gen).to(dev) if epi == 3 else None
        got = torch.full((M, sk, B, N), SENTINEL, device=dev)
        want = torch.full((M, sk, B, N), SENTINEL, device=dev)

        def params(m, out):
            return NtParams(A=p(A[m]), Bw=p(W[m]), bias=p(bias[m]) if with_bias else None, aux=p(aux[m]) if aux is not None else None,
                            out=p(out), M=B, A_rows=B, N=N, K=K, lda=K, ldb=K, ldo=N, ldaux=N, J=1, Tp=1, slope=0.01, loader=0,
                            epilogue=epi, splitk=sk, slab_stride=B * N, bm=bm)
        for m in range(M):
            prm = params(m, want[m])
            assert lib.tl_gemm_nt_window(C.byref(prm), _st()) == 0, (name, lib.tl_last_error())
        prm = params(0, got)
        rc = lib.tl_gemm_nt_window_group_fc(C.byref(prm), M, B * K, N * K, N if with_bias else 0, B * N if aux is not None else 0,
                                            sk * B * N, p(act), _st())
        assert rc == 0, (name, lib.tl_last_error())
        torch.cuda.synchronize()
        for m in range(M):
            if active is None or active[m]:
                assert torch.equal(got[m], want[m]), (shape, name, m)
                assert not bool((got[m] == SENTINEL).any()), (shape, name, m)
            else:
                assert bool((got[m] == SENTINEL).all()), (shape, name, m)


@pytest.mark.parametrize("active", [None, [1, 0, 1]], ids=["all", "masked"])
@pytest.mark.parametrize("shape", ["S1", "S2", "S3"])
def test_tn_group_matches_single(dev, lib, shape, active):
    from decode_tonal_langauge_amd._lib import TnParams
    cfg = SHAPES[shape]
    d = dims(cfg)
    B, D, H, L, hid, ldf, ldd = d["B"], d["D"], d["H"], d["L"], d["hid"], d["ldf"], d["ldd"]
    gen = torch.Generator().manual_seed(10)
    act = None if active is None else torch.tensor(active, dtype=torch.int32, device=dev)
    # name: (Krows, Mdim, Ndim, A row offset, Tp, Tvalid, splitk, colsum?)
    forms = {"fc3 weight gradient (tn_short with colsum)": (B, ldd, hid, 0, 1, 1, 1, True),
             "fc1 weight gradient (tn_short with colsum)": (B, hid, ldf, 0, 1, 1, 1, True),
             "fc3 weight gradient (no colsum)": (B, ldd, hid, 0, 1, 1, 1, False)}
    if L > 1:
        kr = B * L - 1
        forms["W_hh gradient (Tp / Tvalid, split-K)"] = (kr, 4 * H, H, 1, L, L - 1, max(1, min(8, (kr + 63) // 64)), False)
    for name, (kr, Md, Nd, off, Tp, Tv, sk, with_cs) in forms.items():
        rows = kr + off
        A = torch.randn(M, rows, Md, generator=gen).to(dev)
        Bm = torch.randn(M, rows, Nd, generator=gen).to(dev)
        got, want = (torch.full((M, sk, Md, Nd), SENTINEL, device=dev) for _ in range(2))
        gcs, wcs = (torch.full((M, Md), SENTINEL, device=dev) for _ in range(2))

        def params(m, slab, cs):
            return TnParams(A=A[m].data_ptr() + 4 * off * Md, B=p(Bm[m]), slab=p(slab), Krows=kr, A_rows=kr, B_rows=kr, Mdim=Md,
                            Ndim=Nd, lda=Md, ldb=Nd, ldc=Nd, J=1, Tp=Tp, Tvalid=Tv, loader=0, splitk=sk, slab_stride=Md * Nd,
                            colsum=p(cs) if with_cs else None)
        for m in range(M):
            prm = params(m, want[m], wcs[m])
            assert lib.tl_gemm_tn_window(C.byref(prm), _st()) == 0, (name, lib.tl_last_error())
        prm = params(0, got, gcs)
        rc = lib.tl_gemm_tn_window_group(C.byref(prm), M, rows * Md, rows * Nd, sk * Md * Nd, Md, p(act), _st())
        assert rc == 0, (name, lib.tl_last_error())
        torch.cuda.synchronize()
        for m in range(M):
            if active is None or active[m]:
                assert torch.equal(got[m], want[m]) and torch.equal(gcs[m], wcs[m]), (shape, name, m)
                assert not bool((got[m] == SENTINEL).any()), (shape, name, m)
                assert with_cs == (not bool((gcs[m] == SENTINEL).any())), (shape, name, m)
            else:
                assert bool((got[m] == SENTINEL).all()) and bool((gcs[m] == SENTINEL).all()), (shape, name, m)


# ---------------------------------------------------------------------------------------------- 2. engine + trainer vs single path
def _state(model):
    out = {k: v.detach().clone() for k, v in model.named_parameters()}
    out.update({k: v.detach().clone() for k, v in model.named_buffers()})
    return out


def _single_runs(dev, cfg, models, batches, step):
    """[member][step] -> (stats (4), state) of a SynthesisTrainer run of that member alone."""
    from decode_tonal_langauge_amd.models.synthesis_trainer import SynthesisTrainer
    tone, syl = classifiers(cfg[2])
    runs = []
    for m, model in enumerate(models):
        torch.manual_seed(SEEDS[m])                  # SynthesisLite._next_seed reads torch.initial_seed()
        tr = SynthesisTrainer(model, tone, syl, gi.TONE_MAP, device=dev, verbose=False)
        model.train()
        snaps = []
        for s in range(len(batches)):
            step(tr, *batches[s][m])
            torch.cuda.synchronize()
            snaps.append((tr._stats.clone(), _state(model)))
        runs.append(snaps)
    return runs


def _assert_members_equal(ens, runs, s):
    for m, model in enumerate(ens.models):
        stats, state = runs[m][s]
        assert torch.equal(ens._stats[m], stats), ("loss / MCD words", m, s, ens._stats[m].tolist(), stats.tolist())
        now = _state(model)
        assert set(now) == set(state)
        for k in state:
            assert torch.equal(now[k], state[k]), (k, m, s)


@pytest.mark.parametrize("shape", ["S1", "S2", "S3"])
def test_ensemble_steps_equal_single_runs(dev, shape, monkeypatch):
    """Three train steps of M = 3 members (dropout 0.3) on fixed batches and given labels."""
    from decode_tonal_langauge_amd.models.synthesis_ensemble_trainer import SynthesisEnsembleTrainer
    monkeypatch.setenv("TONAL_GRAPH", "0")
    cfg = SHAPES[shape]
    models = lite_models(cfg)
    batches = step_batches(cfg, M, 3)

    def single_step(tr, x, lab, tgt):
        tr._fused_step(x.to(dev), lab.to(dev), tgt.to(dev).float().contiguous())
    runs = _single_runs(dev, cfg, lite_models(cfg), batches, single_step)         # the same seeds: the same initial weights
    tone, syl = classifiers(cfg[2])
    ens = SynthesisEnsembleTrainer(models, tone, syl, gi.TONE_MAP, seeds=SEEDS, device=dev, verbose=False)
    for s in range(3):
        x, lab, tgt = (torch.stack([batches[s][m][i] for m in range(M)]).to(dev) for i in range(3))
        ens._step(x, lab, tgt.float().contiguous())
        torch.cuda.synchronize()
        _assert_members_equal(ens, runs, s)
    # the members' modules hold views of the stacks: the single path keeps working on them
    m1 = ens.models[1].eval()
    with torch.no_grad():
        out = m1(batches[0][1][0].to(dev), batches[0][1][1].to(dev))
    assert out.shape == (cfg[0], cfg[3]) and bool(torch.isfinite(out).all())
    assert set(m1.state_dict()) == set(lite_models(cfg)[0].state_dict())


@pytest.mark.parametrize("graph", ["1", "0"])
def test_ensemble_train_step_with_graph_equal_single_runs(dev, graph, monkeypatch):
    """S2 through ``train_step`` (labels from the classifiers): six steps - three eager, the capture, two replays."""
    from decode_tonal_langauge_amd.models.synthesis_ensemble_trainer import SynthesisEnsembleTrainer
    monkeypatch.setenv("TONAL_GRAPH", graph)
    cfg = S2
    B, Cn, T, D = cfg[:4]
    models = lite_models(cfg)
    g = torch.Generator().manual_seed(6)
    batches = [[(torch.randn(B, Cn, T, generator=g), torch.randn(B, 8, T, generator=g), torch.randn(B, 8, T, generator=g),
                 10 * torch.randn(B, D, generator=g)) for _ in range(M)] for _ in range(6)]
    runs = _single_runs(dev, cfg, lite_models(cfg), batches, lambda tr, *b: tr.train_step(*b))
    tone, syl = classifiers(T)
    ens = SynthesisEnsembleTrainer(models, tone, syl, gi.TONE_MAP, seeds=SEEDS, device=dev, verbose=False)
    for s in range(6):
        ens.train_step(*(torch.stack([batches[s][m][i] for m in range(M)]) for i in range(4)))
        torch.cuda.synchronize()
        _assert_members_equal(ens, runs, s)
    captured = sum(1 for v in ens._graphs.values() if v["graph"] is not None)
    assert captured == (1 if graph == "1" else 0)


def test_ensemble_hip_graph_is_dropped_when_what_it_froze_is_replaced(dev, monkeypatch):
    """The events of ``test_lite_hip_graph_is_dropped_when_what_it_froze_is_replaced`` (tests/test_gpu_parity.py) on the S2 group:
    ``optimizer.load_state_dict`` (new moment tensors), an edited ``weight_decay`` and a tone classifier re-loaded in place must
    each invalidate the captured group step; the run keeps the bits of the same run with TONAL_GRAPH=0."""
    import copy
    from decode_tonal_langauge_amd.models.simple_classifiers import LogisticRegressionClassifier
    from decode_tonal_langauge_amd.models.synthesis_ensemble_trainer import SynthesisEnsembleTrainer
    cfg = S2
    B, Cn, T, D = cfg[:4]
    g = torch.Generator().manual_seed(8)
    batches = [tuple(torch.stack([f(g) for _ in range(M)]) for f in (
        lambda g: torch.randn(B, Cn, T, generator=g), lambda g: torch.randn(B, 8, T, generator=g),
        lambda g: torch.randn(B, 8, T, generator=g), lambda g: 10 * torch.randn(B, D, generator=g))) for _ in range(20)]
    torch.manual_seed(5)
    other_tone = LogisticRegressionClassifier(8 * T, 4).state_dict()
    res = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("TONAL_GRAPH", mode)
        tone, syl = classifiers(T)
        ens = SynthesisEnsembleTrainer(lite_models(cfg), tone, syl, gi.TONE_MAP, seeds=SEEDS, device=dev, verbose=False)
        captures = []
        for i, b in enumerate(batches):
            if i == 6:                                            # moments move to freshly allocated tensors
                ens.optimizer.load_state_dict(copy.deepcopy(ens.optimizer.state_dict()))
            if i == 11:                                           # a launch scalar the capture passed by value
                for gparam in ens.optimizer.param_groups:
                    gparam["weight_decay"] = 0.01
            if i == 16:                                           # classifier weights re-loaded in place (version bump)
                ens.tone_model.load_state_dict({k: v.to(dev) for k, v in other_tone.items()})
            ens.train_step(*b)
            captures.append(sum(1 for v in ens._graphs.values() if v["graph"] is not None))
        torch.cuda.synchronize()
        if mode == "1":
            assert captures[5] == 1 and captures[6] == 0 and captures[10] == 1 and captures[11] == 0 and captures[16] == 0 \
                and captures[-1] == 1, captures
        else:
            assert captures == [0] * 20
        res[mode] = (ens._stats.clone(), [_state(m) for m in ens.models])
    assert torch.equal(res["1"][0], res["0"][0]), (res["1"][0].tolist(), res["0"][0].tolist())
    for m in range(M):
        assert set(res["1"][1][m]) == set(res["0"][1][m])
        for k, v in res["1"][1][m].items():
            assert torch.equal(v, res["0"][1][m][k]), (m, k)


def test_train_step_after_a_forward_through_a_member_module(dev, monkeypatch):
    """A forward through a member's module between two ``train_step`` calls (evaluation, inference) advances that member's
    dropout call counter on the host only; the next ``train_step`` still draws the masks of the sequential run."""
    from decode_tonal_langauge_amd.models.synthesis_ensemble_trainer import SynthesisEnsembleTrainer
    monkeypatch.setenv("TONAL_GRAPH", "0")
    cfg = S2
    B, Cn, T, D = cfg[:4]
    g = torch.Generator().manual_seed(7)
    batches = [[(torch.randn(B, Cn, T, generator=g), torch.randn(B, 8, T, generator=g), torch.randn(B, 8, T, generator=g),
                 10 * torch.randn(B, D, generator=g)) for _ in range(M)] for _ in range(2)]
    lab = torch.randn(B, 2, 5, generator=g).to(dev)

    def peek(model, times):
        model.eval()
        with torch.no_grad():
            for _ in range(times):
                model(batches[0][0][0].to(dev), lab)
        model.train()

    def single_step(tr, *b):
        tr.train_step(*b)
        peek(tr.model, 1 + SEEDS.index(torch.initial_seed()))          # member m: m + 1 forwards, so the counters part
    runs = _single_runs(dev, cfg, lite_models(cfg), batches, single_step)
    tone, syl = classifiers(T)
    ens = SynthesisEnsembleTrainer(lite_models(cfg), tone, syl, gi.TONE_MAP, seeds=SEEDS, device=dev, verbose=False)
    for s in range(2):
        ens.train_step(*(torch.stack([batches[s][m][i] for m in range(M)]) for i in range(4)))
        torch.cuda.synchronize()
        _assert_members_equal(ens, runs, s)
        for m, model in enumerate(ens.models):
            peek(model, 1 + m)


# ---------------------------------------------------------------------------------------------- 3. float64 oracle
def test_ensemble_member_follows_float64_oracle(dev, monkeypatch):
    """One step of the S1 group (dropout 0): member 1's loss, MCD and update against ``oracle.train_step("lite")`` in float64,
    with the bounds tests/test_gpu_lite_shapes.py applies to the single model."""
    from decode_tonal_langauge_amd.models.synthesis_ensemble_trainer import SynthesisEnsembleTrainer
    from oracle import synthesis_oracle as so
    from tests.test_gpu_lite_shapes import FWD_BOUND, _assert_no_ties, _f64, nearest_ties
    monkeypatch.setenv("TONAL_GRAPH", "0")
    cfg, m = S1, 1
    models = lite_models(cfg, dropout=0.0)
    x, lab, tgt = step_batches(cfg, M, 1)[0][m]
    pr, b = _f64(models[m])
    _assert_no_ties(nearest_ties(pr, {k: v.clone() for k, v in b.items()}, x.double(), lab.double(), True), "train")
    init = {k: v.clone() for k, v in pr.items()}
    loss, mcd = so.train_step("lite", pr, b, so.NAdamState(pr), x.double(), lab.double(), tgt.double())
    tone, syl = classifiers(cfg[2])
    ens = SynthesisEnsembleTrainer(models, tone, syl, gi.TONE_MAP, seeds=SEEDS, device=dev, verbose=False)
    batch = step_batches(cfg, M, 1)[0]
    xs, labs, tgts = (torch.stack([batch[k][i] for k in range(M)]).to(dev) for i in range(3))
    ens._step(xs, labs, tgts.float().contiguous())
    torch.cuda.synchronize()
    stats = ens._stats[m].cpu().double().numpy()
    assert abs(stats[2] - loss) / loss < FWD_BOUND and abs(stats[3] - mcd) / mcd < FWD_BOUND, (stats, loss, mcd)
    for k, q in ens.models[m].named_parameters():
        assert gi.update_rel_l2(q.detach().cpu().numpy(), pr[k].numpy(), init[k].numpy()) < LITE_UPDATE_BOUND, k
    for k, v in ens.models[m].named_buffers():
        if v.dtype == torch.long:
            assert int(v) == 1, k


# ---------------------------------------------------------------------------------------------- 4. entry point
N_TRIALS, N_CH, N_T, N_MEL = 23, 12, 64, 16


@pytest.fixture(scope="module")
def experiment(tmp_path_factory):
    from decode_tonal_langauge_amd.models.simple_classifiers import LogisticRegressionClassifier
    root = tmp_path_factory.mktemp("synthesis_ensemble")
    rng = np.random.default_rng(4)
    np.savez(root / "samples.npz", ecog=rng.standard_normal((N_TRIALS, N_CH, N_T)).astype(np.float32),
             mel=(10 * rng.standard_normal((N_TRIALS, N_MEL))).astype(np.float32))
    chans = {"active_channels": list(range(N_CH)), "tone_discriminative": [0, 1, 2], "syllable_discriminative": [3, 4]}
    (root / "channels.json").write_text(json.dumps(chans))
    config = {"mel_kwargs": {"n_mels": N_MEL}, "tone_dynamic_mapping": gi.TONE_MAP, "n_syllables": 2, "n_tones": 4}
    (root / "config.json").write_text(json.dumps(config))
    torch.manual_seed(8)
    torch.save(LogisticRegressionClassifier(3 * N_T, 4).state_dict(), root / "tone.pt")
    torch.save(LogisticRegressionClassifier(2 * N_T, 2).state_dict(), root / "syl.pt")
    return root


def _params(root, tag, ensemble):
    out = root / tag
    return Namespace(sample_path=str(root / "samples.npz"), subject_id="1", result_file=str(out / "results.csv"), figure_dir=None,
                     audio_dir=str(out / "audio"), channel_file=str(root / "channels.json"), config_file=str(root / "config.json"),
                     model_name="lite", syllable_model_path=str(root / "syl.pt"), tone_model_path=str(root / "tone.pt"),
                     synthesis_model_name="SynthesisLite", syllable_model_name="logistic", tone_model_name="logistic",
                     audio_sampling_rate=16000, seed=42, repeat=3, verbose=0, train_ratio=0.8, device="cuda:0", batch_size=4, epochs=2,
                     lr=0.0005, resident=True, ensemble=ensemble, n_audio_samples=0)


def test_train_synthesizer_ensemble_equals_the_sequential_loop(dev, experiment):
    """23 trials at train_ratio 0.8: 18 training samples, so at batch size 4 every epoch ends on a ragged batch of 2 (and the
    whole batches reach the HIP-graph replay in the first epoch); 5 evaluation trials; --repeat 3 --epochs 2 --resident."""
    from decode_tonal_langauge_amd import train_synthesizer as ts
    seq = ts.train(_params(experiment, "sequential", False))
    ens = ts.train(_params(experiment, "ensemble", True))
    assert seq["all_mcds"] == ens["all_mcds"]
    assert seq["losses"] == ens["losses"] and len(seq["losses"]) == 3 and len(seq["losses"][0]) == 2
    a = np.load(os.path.join(experiment, "sequential", "audio", "mels.npz"))
    b = np.load(os.path.join(experiment, "ensemble", "audio", "mels.npz"))
    assert np.array_equal(a["recon"], b["recon"]) and np.array_equal(a["origin"], b["origin"])
    assert seq["seeds"] == ens["seeds"] and seq["model_size"] == ens["model_size"]


def test_label_pass_over_all_members_rows(dev):
    """The one label pass over M B rows against the per-member pass: integer equality."""
    from decode_tonal_langauge_amd.models.synthesis_ensemble_trainer import SynthesisEnsembleTrainer
    cfg = S2
    B, T = cfg[0], cfg[2]
    tone, syl = classifiers(T)
    ens = SynthesisEnsembleTrainer(lite_models(cfg), tone, syl, gi.TONE_MAP, seeds=SEEDS, device=dev, verbose=False)
    g = torch.Generator().manual_seed(12)
    xt, xs = torch.randn(M, B, 8, T, generator=g).to(dev), torch.randn(M, B, 8, T, generator=g).to(dev)
    with torch.no_grad():
        group = ens._labels(xt, xs)
        assert group.shape == (M, B, 2, 5)
        for m in range(M):
            one = ens.single._labels(xt[m], xs[m])
            assert torch.equal(group[m].to(torch.int64), one.to(torch.int64)) and torch.equal(group[m], one), m
    assert len({tuple(group[m].flatten().tolist()) for m in range(M)}) > 1          # the members' labels do differ
