"""Every kernel form behind ``tl_gemm_nt_window`` and ``tl_gemm_tn_window`` (csrc/tonal_gemm.hip) against the float64 restatement
of tests/gemm_ref.py, launched through ``_launch.launch_nt`` / ``launch_tn`` as the engines launch them.

Every output is NaN beforehand (bit planes: a sentinel word), every leading dimension is wider than the logical width, the pad
columns of A / Bw / B and the rows from A_rows / B_rows on are NaN: a form that reads or writes outside its operands fails.
Every launch runs twice and the two results are bit-identical (no atomics).  Values: |got - ref| < 2e-6 max|ref| (NT), times
max(1, rows / 1000) for the TN reductions - the bound of the one-tap tests in tests/test_gpu_parity.py; no form needed more.
Bit planes: exact wherever the float64 margin exceeds 1e-4 max|ref| (tests/test_gemm_ref_host.py caps the rest at 0.5 %); MASK
decisions come from inputs and are exact.  Observed figures go to tests/parity_record under "gemm forms ...".

What this test found: tail128-0..2 (J = 2 / 3, bm 128, DIRECT, row_shift 0, K % 16 == 0, A_rows = M; STORE and LRELU) came back
0.63 .. 0.66 max|ref| off in rows M - J + 1 .. M - 1: the direct-to-LDS kernel reads a row from A_rows on as row A_rows - 1, not
as zero.  tl_gemm_nt_window now takes that kernel at J > 1 only where A_rows >= M + J - 1; bm = 256 needed no change.

The matrix (tests/gemm_forms_cases.py builds it, tests/test_gemm_ref_host.py asserts it).  A case id is <form>-<n>; TONAL_GLDS=0
keeps the bm = 128 DIRECT cases on the register-staged kernel, everything else runs on the default dispatch.

  NT form (kernel instantiation)                      cases            values met by the form
  nt_window_kernel<32,  DIRECT, STORE>                win32-direct-store-0..11    M 1/33/70, N 20/72/136, K 36/48/96, J 1/2/3/5/7,
  nt_window_kernel<32,  DIRECT, LRELU>                win32-direct-lrelu-0..9     row_shift 0 and -(J-1), A_rows M and M+J-1;
  nt_window_kernel<32,  DIRECT, POOL>                 win32-direct-pool-0..9      STORE: bias at splitk 1, splitk 2 and one K-chunk
  nt_window_kernel<32,  DIRECT, MASK>                 win32-direct-mask-0..9      per split; POOL: N 32/96/160, (Tp, Tvalid) (6,4)
  nt_window_kernel<128, DIRECT, STORE>                win128-direct-store-0..11   (12,8) (38,30) at M = S Tp past a row tile and the
  nt_window_kernel<128, DIRECT, LRELU>                win128-direct-lrelu-0..9    even M of the list, with and without osign and
  nt_window_kernel<128, DIRECT, POOL>                 win128-direct-pool-0..9     bias; MASK: from aux (N 20/72/136) and from
  nt_window_kernel<128, DIRECT, MASK>                 win128-direct-mask-0..9     auxbits (N 32/96/160).  bm 128: M 130/257 and
  nt_window_kernel<256, DIRECT, STORE>                win256-direct-store-0..11   tail128-0..3 (below); bm 256: M 300
  nt_window_kernel<256, DIRECT, LRELU>                win256-direct-lrelu-0..9
  nt_window_kernel<256, DIRECT, POOL>                 win256-direct-pool-0..9
  nt_window_kernel<256, DIRECT, MASK>                 win256-direct-mask-0..9
  nt_window_kernel<128, UNPOOL, STORE>                win128-unpool-store-0..7    K 64/96, J 1/3/5/7 (even shift), row_shift 0 and
  nt_window_kernel<128, UNPOOL, MASK>                 win128-unpool-mask-0..7     -(J-1), the three (Tp, Tvalid_in), pooled A_rows
  nt_window_kernel<256, UNPOOL, STORE>                win256-unpool-store-0..7    M/2 and (M+J-1)/2, N as above, splitk as above
  nt_window_kernel<256, UNPOOL, MASK>                 win256-unpool-mask-0..7
  nt_glds_kernel<STORE, 1>                            glds1-store-0..5            the narrow form: J 1, N 20 / 32, K 48/96
  nt_glds_kernel<LRELU, 1>                            glds1-lrelu-0..5
  nt_glds_kernel<POOL, 1>                             glds1-pool-0..5
  nt_glds_kernel<MASK, 1>                             glds1-mask-0..5
  nt_glds_kernel<STORE, 2>                            glds2-store-0..5            J 1/2/3, every N; at J = 3 also N 20 / 32, which
  nt_glds_kernel<LRELU, 2>                            glds2-lrelu-0..5            the wide form must run; A_rows = M + J - 1 (with
  nt_glds_kernel<POOL, 2>                             glds2-pool-0..5             A_rows = M and J > 1 the dispatch keeps the
  nt_glds_kernel<MASK, 2>                             glds2-mask-0..5             register-staged kernel: tail128-0..3)

  TN kernel                    cases                                  values
  tn_short_kernel              short-0..17, bound-*-lo                Krows 1/63/64/65/300/512, Mdim 4/36/72, Ndim 4/132/260, splitk
                                                                      1/3/8, (Tp, Tvalid) (1,1) (7,5) (100,3), A_rows / B_rows
                                                                      short of Krows, colsum (written at splitk 1 only)
  tn_skinny_kernel             skinny-0..10, bound-krows-skinny-hi,   Mdim 4/8/32, Ndim 8/516/1100, Krows 513/530/1037, splitk
                               bound-mdim-lo, bound-ldc-skinny-hi     1/5/40 (40: empty slabs at 513 and 530), Tp 1/11
  tn3_kernel<DIRECT>           tn3-direct-0..8                        Mdim 20/132, Ndim 32/64/96, (S, Tp, Tvalid) (5,12,10)
  tn3_kernel<UNPOOL>           tn3-unpool-0..8                        (3,38,30) (1,70,64) x splitk 1/2/7 (7: empty splits)
  tn_window_kernel<DIRECT>     window-direct-0..8, bound-*-hi         J 2/5/7; Mdim 36/132, Ndim 32/160, geometry x splitk as tn3
  tn_window_kernel<UNPOOL>     window-unpool-0..8                     J 1/2/5 (J = 1 at Mdim 36 exists under UNPOOL only)
  dispatch boundaries          bound-krows, -krows-skinny, -mdim, -splitk, -area (1024 x 1024 / 1028), -ldc, -ldc-skinny: the same
                               operands either side; and the colsum refusal (test_tn_colsum_refusal)
"""
import ctypes as C

import pytest
import torch

from tests import gemm_forms_cases as gc
from tests import gemm_ref as gr
from tests import parity_record

pytestmark = pytest.mark.gpu

NAN = float("nan")
SENTINEL = 0x5A5A5A5A
NT_CASES, TN_CASES = gc.nt_cases(), gc.tn_cases()
_REC = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    from decode_tonal_langauge_amd import _lib
    return _lib.load()


def _record(section, **vals):
    """Worst figures of a form so far (a section per form; every case of the form updates it)."""
    rec = _REC.setdefault(section, {"cases": 0})
    rec["cases"] += 1
    for k, v in vals.items():
        rec[k] = max(rec.get(k, 0.0), float(v))
    parity_record.record("gemm forms " + section, rec)


def _same_bits(a, b):
    return a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))


# ------------------------------------------------------------------------------------------------------------------------
# NT
# ------------------------------------------------------------------------------------------------------------------------
def _launch_nt(lib, c, t, d, dev):
    """One launch of case ``c`` on fresh outputs; returns them on the CPU."""
    from decode_tonal_langauge_amd._launch import launch_nt
    from decode_tonal_langauge_amd._lib import ptr
    M, N = c["M"], c["N"]
    rows = M // 2 if c["epi"] == gc.POOL else M
    ldo = N + 4
    out = torch.full((c["splitk"], rows + 2, ldo), NAN, device=dev)
    kw = dict(A=ptr(d["A"]), Bw=ptr(d["Bw"]), out=ptr(out), M=M, A_rows=t["A_rows"], N=N, K=c["K"], lda=t["lda"], ldb=t["ldb"],
              ldo=ldo, J=c["J"], row_shift=c["row_shift"], Tp=c["Tp"], Tvalid=c["Tvalid"], Tvalid_in=c["Tvalid_in"],
              slope=gc.SLOPE, loader=c["loader"], epilogue=c["epi"], splitk=c["splitk"], slab_stride=(rows + 2) * ldo, bm=c["bm"])
    if "bias" in d:
        kw.update(bias=ptr(d["bias"]))
    if "abits" in d:
        kw.update(abits=ptr(d["abits"]), ld_abits=d["abits"].shape[1])
    if "aux" in d:
        kw.update(aux=ptr(d["aux"]), ldaux=d["aux"].shape[1])
    if "auxbits" in d:
        kw.update(auxbits=ptr(d["auxbits"]), ld_auxbits=d["auxbits"].shape[1])
    got = {}
    if c["epi"] == gc.POOL:
        planes = ["obits", "osign"] if c["osign"] else ["obits"]
        for name in planes:
            got[name] = torch.full((rows + 2, N // 32 + 1), SENTINEL, dtype=torch.int32, device=dev)
            kw[name] = ptr(got[name])
        kw["ld_obits"] = N // 32 + 1
    launch_nt(lib, **kw)
    torch.cuda.synchronize()
    got["out"] = out
    return {k: v.cpu() for k, v in got.items()}


@pytest.mark.parametrize("c", NT_CASES, ids=[c["id"] for c in NT_CASES])
def test_nt_form_matches_float64(dev, lib, c, monkeypatch):
    monkeypatch.setenv("TONAL_GLDS", c["glds"])
    t = gc.nt_operands(c)
    ref = gc.nt_reference(c, t)
    d = {k: v.to(dev) for k, v in t.items() if torch.is_tensor(v)}
    got = _launch_nt(lib, c, t, d, dev)
    again = _launch_nt(lib, c, t, d, dev)
    assert all(_same_bits(got[k], again[k]) for k in got), "two launches differ"

    M, N = c["M"], c["N"]
    rows = M // 2 if c["epi"] == gc.POOL else M
    out = got["out"]
    assert bool(torch.isnan(out[:, :, N:]).all()), "pad columns written"
    assert bool(torch.isnan(out[:, rows:]).all()), "rows past M written"
    body = out[:, :rows, :N].double()
    assert bool(torch.isfinite(body).all()), "an output (or a split's slab) is not fully written"
    scale = float(ref["out"].abs().max())
    err = float((body.sum(0) - ref["out"]).abs().max()) / scale
    fig = dict(worst_rel=err)
    print(f"{c['id']} [{gc.nt_form(c)}]: worst |got - ref| / max|ref| = {err:.3e}")
    if c["epi"] == gc.POOL:
        for name, skip in zip(("obits", "osign"), gc.plane_skips(ref)):
            if name not in got:
                continue
            words = got[name]
            assert bool((words[rows:] == SENTINEL).all()) and bool((words[:, N // 32:] == SENTINEL).all()), name + ": pad words written"
            wrong = (gr.bits(words[:rows], N) != ref[name]) & ~skip
            fig["skipped_share_" + name] = float(skip.double().mean())
            assert not bool(wrong.any()), f"{name}: {int(wrong.sum())} decided bits differ"
        masked = ref["m_sign"] == 0
        assert bool((body[0][masked] == 0).all()), "masked pairs are not exact zeros"
    _record("nt/" + gc.nt_form(c), **fig)
    assert err < gc.NT_TOL, (c["id"], err)


# ------------------------------------------------------------------------------------------------------------------------
# TN
# ------------------------------------------------------------------------------------------------------------------------
def _launch_tn(lib, c, t, d, dev):
    from decode_tonal_langauge_amd._launch import launch_tn
    from decode_tonal_langauge_amd._lib import ptr
    JM, ldc = c["J"] * c["Mdim"], c["ldc"]
    slab = torch.full((c["splitk"], JM + 2, ldc), NAN, device=dev)
    kw = dict(A=ptr(d["A"]), B=ptr(d["B"]), slab=ptr(slab), Krows=c["Krows"], A_rows=t["A_rows"], B_rows=t["B_rows"],
              Mdim=c["Mdim"], Ndim=c["Ndim"], lda=t["lda"], ldb=t["ldb"], ldc=ldc, J=c["J"], Tp=c["Tp"], Tvalid=c["Tvalid"],
              loader=c["loader"], splitk=c["splitk"], slab_stride=(JM + 2) * ldc)
    got = {"slab": slab}
    if "bbits" in d:
        kw.update(bbits=ptr(d["bbits"]), ld_bbits=d["bbits"].shape[1])
    if c["colsum"]:
        assert c["kernel"] == "short"             # (tn_window's colsum is another quantity: [splitk][Ndim] sums of B)
        got["colsum"] = torch.full((c["Mdim"] + 2,), NAN, device=dev)
        kw["colsum"] = ptr(got["colsum"])
    launch_tn(lib, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in got.items()}


@pytest.mark.parametrize("c", TN_CASES, ids=[c["id"] for c in TN_CASES])
def test_tn_kernel_matches_float64(dev, lib, c):
    t = gc.tn_operands(c)
    ref = gc.tn_reference(c, t)
    d = {k: v.to(dev) for k, v in t.items() if torch.is_tensor(v)}
    got = _launch_tn(lib, c, t, d, dev)
    again = _launch_tn(lib, c, t, d, dev)
    assert all(_same_bits(got[k], again[k]) for k in got), "two launches differ"

    JM, Nd = c["J"] * c["Mdim"], c["Ndim"]
    slab = got["slab"]
    assert bool(torch.isnan(slab[:, :, Nd:]).all()), "pad columns written"
    assert bool(torch.isnan(slab[:, JM:]).all()), "rows past J * Mdim written"
    body = slab[:, :JM, :Nd].double()
    assert bool(torch.isfinite(body).all()), "a slab is not fully written"
    ranges = gr.tn_split_ranges(Krows=c["Krows"], A_rows=t["A_rows"], B_rows=t["B_rows"] * (2 if "bbits" in t else 1),
                                splitk=c["splitk"], step=gc.TN_STEP[c["kernel"]], chunked=c["kernel"] == "short")
    for z, (r0, r1) in enumerate(ranges):
        if r0 == r1:
            assert bool((body[z] == 0).all()), f"empty split {z} is not zeros"
    total = ref.sum(0)
    scale = float(total.abs().max())
    tol = gc.tn_tol(c["Krows"])
    err = float((body.sum(0) - total).abs().max()) / scale
    err_slab = float((body - ref).abs().max()) / scale
    fig = dict(worst_rel=err, worst_rel_per_slab=err_slab)
    print(f"{c['id']} [tn_{c['kernel']}]: sum over slabs {err:.3e}, worst slab {err_slab:.3e} of max|ref| (bound {tol:.1e})")
    if c["colsum"]:
        cs = got["colsum"]
        if c["splitk"] == 1 and c["kernel"] == "short":
            cref = gr.tn_colsum_a_ref(t["A"], Krows=c["Krows"], A_rows=t["A_rows"], B_rows=t["B_rows"], Mdim=c["Mdim"], Tp=c["Tp"],
                                      Tvalid=c["Tvalid"])
            fig["worst_rel_colsum"] = float((cs[:c["Mdim"]].double() - cref).abs().max()) / float(cref.abs().max())
            assert bool(torch.isnan(cs[c["Mdim"]:]).all()), "colsum written past Mdim"
        else:
            assert bool(torch.isnan(cs).all()), "colsum written at splitk > 1"
    _record("tn/" + c["kernel"] + ("-unpool" if c["loader"] == gc.UNPOOL else ""), **fig)
    assert err < tol and err_slab < tol, (c["id"], err, err_slab)
    assert fig.get("worst_rel_colsum", 0.0) < tol, (c["id"], fig)


def test_tn_colsum_refusal(dev, lib):
    """``colsum`` with Mdim <= 32 past the short kernel's reach (Krows 513): no kernel sums it - the entry point says so."""
    from decode_tonal_langauge_amd._lib import TnParams
    A = torch.zeros(520, 32, device=dev)
    B = torch.zeros(520, 8, device=dev)
    slab = torch.full((32, 8), NAN, device=dev)
    cs = torch.full((32,), NAN, device=dev)
    p = TnParams(A=A.data_ptr(), B=B.data_ptr(), slab=slab.data_ptr(), colsum=cs.data_ptr(), Krows=513, A_rows=513, B_rows=513,
                 Mdim=32, Ndim=8, lda=32, ldb=8, ldc=8, J=1, Tp=1, Tvalid=1, loader=gc.DIRECT, splitk=1)
    assert lib.tl_gemm_tn_window(C.byref(p), torch.cuda.current_stream().cuda_stream) == -1
    assert b"colsum comes from the short-reduction kernel" in lib.tl_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(slab).all()) and bool(torch.isnan(cs).all())
