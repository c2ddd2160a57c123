"""tests/gemm_ref.py (the float64 restatement the GPU test of the windowed GEMMs stands on) against stock torch, and the case list
of tests/gemm_forms_cases.py against the matrix it promises.  CPU only."""
import collections

import pytest
import torch
import torch.nn.functional as F

from tests import gemm_forms_cases as gc
from tests import gemm_ref as gr

F64 = torch.float64


def _words(g, rows, ncols):
    return torch.randint(-2 ** 31, 2 ** 31, (rows, (ncols + 31) // 32), generator=g, dtype=torch.int64).to(torch.int32)


def test_bit_words_round_trip():
    g = torch.Generator().manual_seed(1)
    m = torch.rand(5, 70, generator=g) > 0.5
    w = gr.pack(m)
    assert w.dtype == torch.int32 and w.shape == (5, 3) and torch.equal(gr.bits(w, 70), m)
    assert int(w[0, 0]) & 1 == int(m[0, 0]) and (int(w[0, 1]) >> 3) & 1 == int(m[0, 35])


@pytest.mark.parametrize("J", [1, 2, 3, 5, 7])
def test_nt_ref_is_conv1d_per_sequence(J):
    """row_shift 0 on zero-padded sequences is the correlation; row_shift -(J-1) with the taps flipped and the channels swapped
    is conv_transpose1d (the input gradient)."""
    g = torch.Generator().manual_seed(J)
    S, Tp, K, N = 3, 11, 8, 5
    x = torch.zeros(S, Tp, K, dtype=F64)
    x[:, :Tp - (J - 1)] = torch.randn(S, Tp - (J - 1), K, generator=g, dtype=F64)      # J - 1 zero rows close every sequence
    w = torch.randn(N, K, J, generator=g, dtype=F64)                                   # conv1d weight [out][in][tap]
    Bw = torch.zeros(J, N, K + 4, dtype=F64)
    Bw[:, :, :K] = w.permute(2, 0, 1)
    M = S * Tp
    y = gr.nt_ref(x.reshape(M, K), Bw, M=M, N=N, K=K, J=J, row_shift=0, A_rows=M)
    ref = F.conv1d(F.pad(x.transpose(1, 2), (0, J - 1)), w).transpose(1, 2)            # [S][Tp][N]
    keep = Tp - (J - 1)                               # (the rows behind look into the next sequence: the rows are one flat run)
    assert torch.allclose(y.view(S, Tp, N)[:, :keep], ref[:, :keep], rtol=0, atol=1e-12)
    assert torch.allclose(y.view(S, Tp, N)[-1], ref[-1], rtol=0, atol=1e-12)           # behind the last one: zero, as padded
    # transposed form: dx[t] = sum_j dz[t - j] . w[:, :, j]  =  sum_j' dz[t - (J-1) + j'] . w[:, :, J-1-j']
    dz = torch.zeros(S, Tp, N, dtype=F64)
    dz[:, :Tp - (J - 1)] = torch.randn(S, Tp - (J - 1), N, generator=g, dtype=F64)
    Bt = w.flip(2).permute(2, 1, 0).contiguous()                                       # [J][K][N]
    dx = gr.nt_ref(dz.reshape(M, N), Bt, M=M, N=K, K=N, J=J, row_shift=-(J - 1), A_rows=M)
    ref = F.conv_transpose1d(dz[:, :Tp - (J - 1)].transpose(1, 2), w).transpose(1, 2)
    assert torch.allclose(dx.view(S, Tp, K), ref, rtol=0, atol=1e-12)


def test_nt_ref_reads_zero_outside_a_rows():
    g = torch.Generator().manual_seed(3)
    A = torch.randn(12, 4, generator=g, dtype=F64)
    Bw = torch.randn(3, 2, 4, generator=g, dtype=F64)
    full = gr.nt_ref(A, Bw, M=10, N=2, K=4, J=3, row_shift=0, A_rows=12)
    cut = gr.nt_ref(A, Bw, M=10, N=2, K=4, J=3, row_shift=0, A_rows=10)
    assert torch.equal(full[:8], cut[:8]) and not torch.equal(full[8:], cut[8:])
    assert torch.allclose(cut[9], A[9] @ Bw[0].t())


def test_pool_ref_is_max_pool1d_with_indices():
    g = torch.Generator().manual_seed(4)
    S, Tp, Tv, N = 4, 12, 8, 40
    y = torch.randn(S * Tp, N, generator=g, dtype=F64)
    bias = torch.randn(N, generator=g, dtype=F64)
    out, ob, osg, m_arg, m_sign = gr.pool_ref(y, bias, 0.1, Tp, Tv)
    a = F.leaky_relu(y + bias, 0.1).view(S, Tp, N).transpose(1, 2)
    ref, idx = F.max_pool1d(a, 2, return_indices=True)                 # [S][N][Tp / 2]
    ref, idx = ref.transpose(1, 2), idx.transpose(1, 2)
    valid = (torch.arange(Tp // 2) * 2 < Tv)[None, :, None]
    assert torch.equal(out.view(S, Tp // 2, N), torch.where(valid, ref, torch.zeros((), dtype=F64)))
    assert torch.equal(ob.view(S, Tp // 2, N), ((idx & 1) == 1) & valid)
    assert torch.equal(osg, out > 0) and not bool(osg.view(S, Tp // 2, N)[:, Tv // 2:].any())
    assert torch.equal(m_sign, out.abs())
    assert torch.equal(m_arg.view(S, Tp // 2, N), (a[:, :, 0::2] - a[:, :, 1::2]).abs().transpose(1, 2))


def test_unpool_ref_is_max_unpool1d():
    g = torch.Generator().manual_seed(5)
    S, Tp, Tv, K = 3, 12, 8, 70
    P = S * Tp // 2
    G = torch.randn(P, K, generator=g, dtype=F64)
    ab = _words(g, P, K)
    out = gr.unpool_ref(G, ab, Tp, Tv)
    odd = gr.bits(ab, K).view(S, Tp // 2, K).transpose(1, 2)           # [S][K][Tp / 2]
    idx = 2 * torch.arange(Tp // 2)[None, None, :] + odd.long()
    valid = (torch.arange(Tp // 2) * 2 < Tv)[None, None, :]
    ref = F.max_unpool1d(torch.where(valid, G.view(S, Tp // 2, K).transpose(1, 2), torch.zeros((), dtype=F64)), idx, 2)
    assert torch.equal(out.view(S, Tp, K), ref.transpose(1, 2))


@pytest.mark.parametrize("splitk", [1, 3])
def test_tn_ref_is_the_weight_gradient_of_conv1d(splitk):
    g = torch.Generator().manual_seed(6)
    S, Tp, Tv, Cin, Cout, J = 4, 12, 10, 8, 4, 3
    x = torch.zeros(S, Tp, Cin, dtype=F64)
    x[:, :Tv + J - 1] = torch.randn(S, Tv + J - 1, Cin, generator=g, dtype=F64)
    w = torch.randn(Cout, Cin, J, generator=g, dtype=F64, requires_grad=True)
    dz = torch.randn(S, Tp, Cout, generator=g, dtype=F64)              # rows t >= Tv hold numbers the mask must drop
    z = F.conv1d(x.transpose(1, 2), w)[:, :, :Tv]                      # [S][Cout][Tv]
    gw, = torch.autograd.grad(z, w, dz[:, :Tv].transpose(1, 2))
    rows = S * Tp
    slabs = gr.tn_ref(x.reshape(rows, Cin), dz.reshape(rows, Cout), Krows=rows, A_rows=rows, B_rows=rows, Mdim=Cin, Ndim=Cout,
                      J=J, Tp=Tp, Tvalid=Tv, splitk=splitk, step=32)
    assert slabs.shape == (splitk, J * Cin, Cout)
    assert torch.allclose(slabs.sum(0).view(J, Cin, Cout), gw.permute(2, 1, 0), rtol=0, atol=1e-12)
    if splitk == 3:                                                    # 2 K-steps of 32 rows over 3 splits: the last is empty
        assert bool((slabs[2] == 0).all()) and bool((slabs[:2] != 0).any(2).any(1).all())


def test_tn_ref_unpools_b_and_splits_like_the_kernels():
    g = torch.Generator().manual_seed(7)
    Kr, Md, Nd, Tp, Tv = 48, 4, 40, 12, 8
    A = torch.randn(Kr + 2, Md, generator=g, dtype=F64)
    Bp = torch.randn(Kr // 2, Nd, generator=g, dtype=F64)
    bb = _words(g, Kr // 2, Nd)
    kw = dict(Krows=Kr, A_rows=Kr + 2, Mdim=Md, Ndim=Nd, J=3, Tp=Tp, Tvalid=Tv, splitk=1, step=32)
    pooled = gr.tn_ref(A, Bp, B_rows=Kr // 2, bbits=bb, **kw)
    plain = gr.tn_ref(A, gr.unpool_ref(Bp, bb, Tp, Tv), B_rows=Kr, **kw)
    assert torch.equal(pooled, plain)
    assert gr.tn_split_ranges(Krows=70, A_rows=70, B_rows=70, splitk=2, step=32) == [(0, 64), (64, 70)]
    assert gr.tn_split_ranges(Krows=70, A_rows=70, B_rows=70, splitk=7, step=16)[4:] == [(64, 70), (70, 70), (70, 70)]
    assert gr.tn_split_ranges(Krows=300, A_rows=300, B_rows=290, splitk=3, step=64, chunked=True) == [(0, 128), (128, 256), (256, 290)]
    cs = gr.tn_colsum_a_ref(A, Krows=Kr, A_rows=Kr + 2, B_rows=40, Mdim=Md, Tp=Tp, Tvalid=Tv)
    keep = [r for r in range(40) if r % Tp < Tv]
    assert torch.allclose(cs, A[keep].sum(0))


# ------------------------------------------------------------------------------------------------------------------------
# the case list of the GPU test
# ------------------------------------------------------------------------------------------------------------------------
NT_CASES, TN_CASES = gc.nt_cases(), gc.tn_cases()


def _moved(a, b):
    return float((a - b).abs().max()) / float(a.abs().max())


@pytest.mark.parametrize("c", NT_CASES, ids=[c["id"] for c in NT_CASES])
def test_nt_shapes_tell_a_wrong_kernel_from_a_right_one(c):
    """Reversed taps, a validity mask one pooled row late and swapped un-pooling each move the float64 result by more than 100
    times the GPU tolerance; and the share of each bit plane too close to compare stays under the cap."""
    t = gc.nt_operands(c)
    ref = gc.nt_reference(c, t)
    assert bool(torch.isfinite(ref["out"]).all())
    need = 100 * gc.NT_TOL
    if c["J"] > 1:
        assert _moved(ref["out"], gc.nt_reference(c, t, "taps")["out"]) > need
    if c["loader"] == gc.UNPOOL:
        assert _moved(ref["out"], gc.nt_reference(c, t, "oddeven")["out"]) > need
    if c["loader"] == gc.UNPOOL or c["epi"] == gc.POOL:
        assert _moved(ref["out"], gc.nt_reference(c, t, "tvalid")["out"]) > need
    if c["epi"] == gc.POOL:
        for skip in gc.plane_skips(ref):
            assert float(skip.double().mean()) <= gc.BIT_SKIP_CAP
        assert bool(ref["obits"].any()) and bool((~ref["obits"]).any()) and bool(ref["osign"].any())


@pytest.mark.parametrize("c", TN_CASES, ids=[c["id"] for c in TN_CASES])
def test_tn_shapes_tell_a_wrong_kernel_from_a_right_one(c):
    t = gc.tn_operands(c)
    ref = gc.tn_reference(c, t).sum(0)
    assert bool(torch.isfinite(ref).all())
    need = 100 * gc.tn_tol(c["Krows"])
    if c["J"] > 1:
        assert _moved(ref, gc.tn_reference(c, t, "taps").sum(0)) > need
    if c["loader"] == gc.UNPOOL:
        assert _moved(ref, gc.tn_reference(c, t, "oddeven").sum(0)) > need
    if c["Tvalid"] < c["Tp"] and c["Krows"] > c["Tvalid"]:
        assert _moved(ref, gc.tn_reference(c, t, "tvalid").sum(0)) > need


def test_every_value_of_the_matrix_meets_every_form_it_is_legal_for():
    seen = collections.defaultdict(lambda: collections.defaultdict(set))
    for c in NT_CASES:
        f = gc.nt_form(c)
        for k in ("M", "N", "K", "J", "sk_kind", "osign", "maskfrom", "bias"):
            seen[f][k].add(c[k])
        seen[f]["geo"].add((c["Tp"], c["Tvalid_in"] if c["loader"] == gc.UNPOOL else c["Tvalid"]))
        seen[f]["shift"].add("neg" if c["row_shift"] < 0 else "zero")
        if c["J"] > 1:
            seen[f]["A_rows"].add("M" if c["extra"] == 0 else "M+J-1")
    assert all(c["id"].rsplit("-", 1)[0] == gc.nt_form(c) for c in NT_CASES if not c["id"].startswith("tail128"))
    direct = [f"win{bm}-direct-{e}" for bm in (32, 128, 256) for e in ("store", "lrelu", "pool", "mask")]
    unpool = [f"win{bm}-unpool-{e}" for bm in (128, 256) for e in ("store", "mask")]
    glds = [f"glds{ni}-{e}" for ni in (1, 2) for e in ("store", "lrelu", "pool", "mask")]
    assert set(seen) == set(direct + unpool + glds)
    geo = set(gc.GEO)
    for f in direct:
        bm, s = int(f[3:].split("-")[0]), seen[f]
        assert s["K"] == {36, 48, 96} and s["J"] == {1, 2, 3, 5, 7} and s["shift"] == {"neg", "zero"}, f
        assert s["A_rows"] == {"M", "M+J-1"}, f
        if f.endswith("pool"):
            assert s["N"] == set(gc.N_BITS) and s["geo"] == geo and s["osign"] == {False, True}, f
            assert s["M"] >= {gc.GEO_M[bm][tp] for tp, _ in gc.GEO} | {m for m in gc.NT_M[bm] if m % 2 == 0}, f
        else:
            assert s["M"] == set(gc.NT_M[bm]), f
            assert s["N"] >= set(gc.N_PLAIN), f
        if f.endswith("mask"):
            assert s["maskfrom"] == {"aux", "bits"} and s["N"] >= set(gc.N_BITS), f
        if f.endswith("store"):
            assert s["sk_kind"] == {1, 2, "all"} and s["bias"] == {False, True}, f
    for f in unpool:
        s = seen[f]
        assert s["K"] == {64, 96} and s["J"] == {1, 3, 5, 7} and s["shift"] == {"neg", "zero"} and s["geo"] == geo, f
        assert s["A_rows"] == {"M", "M+J-1"} and s["N"] >= set(gc.N_PLAIN), f
        if f.endswith("mask"):
            assert s["maskfrom"] == {"aux", "bits"}, f
        else:
            assert s["sk_kind"] == {1, 2, "all"}, f
    for f in glds:
        s = seen[f]
        assert s["K"] == {48, 96} and s["J"] == ({1} if f.startswith("glds1") else {1, 2, 3}) and s["shift"] == {"zero"}, f
        assert max(s["N"]) <= 64 if f.startswith("glds1") else (min(s["N"]) <= 64 and max(s["N"]) > 128), f
    assert any(gc.nt_form(c).startswith("glds2") and c["J"] == 3 and c["N"] <= 64 for c in NT_CASES)
    # shapes the direct-to-LDS kernel would take but for the rows behind the end: the register-staged kernel, default dispatch
    assert all(gc.nt_form(c).startswith("win128-direct") and c["glds"] == "1" for c in NT_CASES if c["id"].startswith("tail128"))

    tn = collections.defaultdict(lambda: collections.defaultdict(set))
    for c in TN_CASES:
        name = c["id"].rsplit("-", 1)[0]
        for k in ("Krows", "Mdim", "Ndim", "J", "splitk", "Tp", "kernel", "short", "colsum"):
            tn[name][k].add(c[k])
    for name, kernel in (("short", "short"), ("skinny", "skinny"), ("tn3-direct", "tn3"), ("tn3-unpool", "tn3"),
                         ("window-direct", "window"), ("window-unpool", "window")):
        assert tn[name]["kernel"] == {kernel}, name
    s = tn["short"]
    assert s["Krows"] == {1, 63, 64, 65, 300, 512} and s["Mdim"] == {4, 36, 72} and s["Ndim"] == {4, 132, 260}
    assert s["splitk"] == {1, 3, 8} and s["Tp"] == {1, 7, 100} and s["short"] == {None, "A", "B"} and s["colsum"] == {False, True}
    assert any(c["colsum"] and c["splitk"] == 1 for c in TN_CASES) and any(c["colsum"] and c["splitk"] > 1 for c in TN_CASES)
    s = tn["skinny"]
    assert s["Krows"] == {513, 530, 1037} and s["Mdim"] == {4, 8, 32} and s["Ndim"] == {8, 516, 1100}
    assert s["splitk"] == {1, 5, 40} and s["Tp"] == {1, 11}
    for name in ("tn3-direct", "tn3-unpool"):
        s = tn[name]
        assert s["Mdim"] == {20, 132} and s["Ndim"] == {32, 64, 96} and s["Krows"] == {60, 114, 70} and s["splitk"] == {1, 2, 7}, name
    assert tn["window-direct"]["J"] == {2, 5, 7} and tn["window-unpool"]["J"] == {1, 2, 5}
    for name in ("window-direct", "window-unpool"):
        s = tn[name]
        assert s["Mdim"] == {36, 132} and s["Ndim"] == {32, 160} and s["Krows"] == {60, 114, 70} and s["splitk"] == {1, 2, 7}, name
    bound = {c["id"]: c["kernel"] for c in TN_CASES if c["id"].startswith("bound-")}
    assert bound == {"bound-krows-lo": "short", "bound-krows-hi": "window", "bound-krows-skinny-lo": "short",
                     "bound-krows-skinny-hi": "skinny", "bound-mdim-lo": "skinny", "bound-mdim-hi": "window",
                     "bound-splitk-lo": "short", "bound-splitk-hi": "window", "bound-area-lo": "short",
                     "bound-area-hi": "window", "bound-ldc-lo": "short", "bound-ldc-hi": "window",
                     "bound-ldc-skinny-lo": "short", "bound-ldc-skinny-hi": "skinny"}
