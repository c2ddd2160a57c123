"""The cases of tests/test_gpu_gemm_forms.py, their operands and their float64 references - TEST INFRASTRUCTURE.

Kept apart from the GPU test so that tests/test_gemm_ref_host.py can walk the same list without a GPU: that every shape tells a
wrong kernel from a right one (tap order, validity mask, odd / even rows of the un-pooling), that the undecidable share of every
bit plane stays under its cap, and that every value of the matrix is met by every kernel form it is legal for.

A parameter of a form takes its values in turn from shuffled rounds of its list (``_rr``), each parameter with a shuffle of its
own: any ``len(list)`` consecutive cases of a form hold every value, and the pairings differ from form to form."""
import random

import torch

from tests import gemm_ref as gr

STORE, LRELU, POOL, MASK = 0, 1, 2, 3            # (the ABI's numbers: include/tonal_hip.h)
DIRECT, UNPOOL = 0, 1
EPI_NAME = {STORE: "store", LRELU: "lrelu", POOL: "pool", MASK: "mask"}

NT_TOL = 2e-6                                     # |got - ref| < NT_TOL * max|ref|: the bound of the one-tap tests
BIT_MARGIN = 1e-4                                 # bit planes are compared where the float64 margin exceeds this * max|ref|
BIT_SKIP_CAP = 0.005
SLOPE = 0.1                                       # (not 0: under ReLU a quarter of the arg-max pairs would tie at 0)

NT_M = {32: (1, 33, 70), 128: (130, 257), 256: (300,)}
GEO = ((6, 4), (12, 8), (38, 30))                 # (Tp, Tvalid): shorter than the epilogue's 8-row stride; even; divides no tile
GEO_M = {32: {6: 36, 12: 36, 38: 76}, 128: {6: 132, 12: 132, 38: 152}, 256: {6: 258, 12: 264, 38: 266}}   # S * Tp past a row tile
N_PLAIN, N_BITS = (20, 72, 136), (32, 96, 160)


def tn_tol(rows):
    return NT_TOL * max(1.0, rows / 1000.0)


def _rr(values, n, seed):
    rng = random.Random(seed)
    out = []
    while len(out) < n:
        rnd = list(values)
        rng.shuffle(rnd)
        out += rnd
    return out[:n]


def _seed(name):
    return sum((i + 1) * ord(c) for i, c in enumerate(name))


# ------------------------------------------------------------------------------------------------------------------------
# NT cases
# ------------------------------------------------------------------------------------------------------------------------
def nt_takes_glds(c):
    """The dispatch rule of tl_gemm_nt_window, restated for the matrix: which cases run on the direct-to-LDS kernel."""
    return (c["glds"] == "1" and c["J"] <= 3 and c["bm"] == 128 and c["loader"] == DIRECT and c["row_shift"] == 0
            and c["K"] % 16 == 0 and (c["J"] == 1 or c["extra"] >= c["J"] - 1))


def nt_form(c):
    if nt_takes_glds(c):
        return f"glds{1 if c['N'] <= 64 and c['J'] == 1 else 2}-{EPI_NAME[c['epi']]}"
    return f"win{c['bm']}-{'unpool' if c['loader'] == UNPOOL else 'direct'}-{EPI_NAME[c['epi']]}"


def _nt_case(name, i, **kw):
    c = dict(bm=128, loader=DIRECT, epi=STORE, J=1, row_shift=0, extra=0, Tp=1, Tvalid=1, Tvalid_in=0, splitk=1, bias=False,
             osign=False, maskfrom="aux", glds="1")
    c.update(kw)
    c["id"] = f"{name}-{i}"
    c["seed"] = _seed(c["id"])
    c["sk_kind"] = c["splitk"]                    # 1, 2 or "all" (one K-chunk per split)
    if c["splitk"] == "all":
        c["splitk"] = c["K"] // 16 if nt_takes_glds({**c, "splitk": 1}) else -(-c["K"] // 32)
    return c


def _nt_direct(bm, epi, n=10):
    name = f"win{bm}-direct-{EPI_NAME[epi]}"
    s = _seed(name)
    Js, Ks = _rr((1, 2, 3, 5, 7), n, s), _rr((36, 48, 96), n, s + 1)
    neg, extra = _rr((False, True), n, s + 2), _rr((False, True), n, s + 3)
    Ms, geo = _rr(NT_M[bm], n, s + 4), _rr(GEO, n, s + 5)
    Np, Nb = _rr(N_PLAIN, n, s + 6), _rr(N_BITS, n, s + 7)
    sk, osign, mfrom = _rr((1, 2, "all"), n, s + 8), _rr((False, True), n, s + 9), _rr(("aux", "bits"), n, s + 10)
    out = []
    for i in range(n):
        J = Js[i]
        kw = dict(bm=bm, epi=epi, J=J, K=Ks[i], row_shift=-(J - 1) if neg[i] else 0, extra=J - 1 if extra[i] else 0, M=Ms[i],
                  N=Np[i], glds="0" if bm == 128 else "1")
        if epi == STORE:
            kw.update(splitk=sk[i], bias=sk[i] == 1)
        elif epi == LRELU:
            kw.update(bias=True)
        elif epi == POOL:
            Tp, Tv = geo[i]
            even = [m for m in NT_M[bm] if m % 2 == 0]                # every fourth case: the even M of the plain list, whose
            M = even[0] if i % 4 == 0 and even else GEO_M[bm][Tp]     # last sequence is cut short
            kw.update(M=M, Tp=Tp, Tvalid=Tv, N=Nb[i], osign=osign[i], bias=i % 3 != 0)
        else:
            kw.update(maskfrom=mfrom[i], N=(Nb if mfrom[i] == "bits" else Np)[mfrom[:i].count(mfrom[i])])   # every N with both
        out.append(_nt_case(name, i, **kw))
    return out


def _nt_unpool(bm, epi, n=8):
    name = f"win{bm}-unpool-{EPI_NAME[epi]}"
    s = _seed(name)
    Js, Ks = _rr((1, 3, 5, 7), n, s), _rr((64, 96), n, s + 1)       # J - 1 even: the loader needs an even shift
    neg, extra, geo = _rr((False, True), n, s + 2), _rr((False, True), n, s + 3), _rr(GEO, n, s + 5)
    Np, Nb = _rr(N_PLAIN, n, s + 6), _rr(N_BITS, n, s + 7)
    sk, mfrom = _rr((1, 2, "all"), n, s + 8), _rr(("aux", "bits"), n, s + 10)
    out = []
    for i in range(n):
        J = Js[i]
        Tp, Tv = geo[i]
        kw = dict(bm=bm, loader=UNPOOL, epi=epi, J=J, K=Ks[i], row_shift=-(J - 1) if neg[i] else 0,
                  extra=J - 1 if extra[i] else 0, M=GEO_M[bm][Tp], Tp=Tp, Tvalid_in=Tv, N=Np[i])
        if epi == STORE:
            kw.update(splitk=sk[i], bias=sk[i] == 1)
        else:
            kw.update(maskfrom=mfrom[i], N=(Nb if mfrom[i] == "bits" else Np)[mfrom[:i].count(mfrom[i])])   # every N with both
        out.append(_nt_case(name, i, **kw))
    return out


def _nt_glds(epi, ni, n=6):
    name = f"glds{ni}-{EPI_NAME[epi]}"
    s = _seed(name)
    Ks, Ms, geo = _rr((48, 96), n, s + 1), _rr(NT_M[128], n, s + 4), _rr(GEO, n, s + 5)
    sk, osign, mfrom = _rr((1, 2, "all"), n, s + 8), _rr((False, True), n, s + 9), _rr(("aux", "bits"), n, s + 10)
    if ni == 1:                                   # the narrow form: N <= 64 and one tap
        Js, Np, Nb = [1] * n, [20] * n, [32] * n
    else:                                         # the wide form: every N, and N <= 64 where J > 1
        Js = _rr((1, 2, 3), n, s)
        Np, Nb = _rr(N_PLAIN, n, s + 6), _rr(N_BITS, n, s + 7)
        for i in range(n):
            if Js[i] == 1 and Np[i] <= 64:
                Np[i] = 72
            if Js[i] == 1 and Nb[i] <= 64:
                Nb[i] = 96
        three = Js.index(3)
        Np[three], Nb[three] = 20, 32             # at J = 3 the wide form is what runs for N <= 64
    out = []
    for i in range(n):
        J = Js[i]
        kw = dict(epi=epi, J=J, K=Ks[i], extra=J - 1, M=Ms[i], N=Np[i])      # (rows behind the end exist: see nt_takes_glds)
        if epi == STORE:
            kw.update(splitk=sk[i], bias=sk[i] == 1)
        elif epi == LRELU:
            kw.update(bias=True)
        elif epi == POOL:
            Tp, Tv = geo[i]
            kw.update(M=GEO_M[128][Tp] if i % 3 else 130, Tp=Tp, Tvalid=Tv, N=Nb[i], osign=osign[i], bias=i % 2 == 0)
        else:
            kw.update(maskfrom=mfrom[i], N=(Nb if mfrom[i] == "bits" else Np)[mfrom[:i].count(mfrom[i])])   # every N with both
        if ni == 2 and J == 1 and kw["N"] <= 64:  # (one tap at N <= 64 is the narrow form's)
            kw["N"] = {20: 72, 32: 96}[kw["N"]]
        out.append(_nt_case(name, i, **kw))
    return out


def nt_cases():
    out = []
    for bm in (32, 128, 256):
        for epi in (STORE, LRELU, POOL, MASK):
            out += _nt_direct(bm, epi, 12 if epi == STORE else 10)
    for bm in (128, 256):
        for epi in (STORE, MASK):
            out += _nt_unpool(bm, epi)
    for ni in (1, 2):
        for epi in (STORE, LRELU, POOL, MASK):
            out += _nt_glds(epi, ni)
    # window rows behind A_rows = M read zero on the default dispatch too, at shapes the direct-to-LDS kernel would take if
    # rows behind the end existed
    for i, (J, epi) in enumerate(((2, STORE), (3, STORE), (3, LRELU), (3, POOL))):
        kw = dict(Tp=12, Tvalid=8, M=132, N=96) if epi == POOL else dict(M=130, N=72)
        out.append(_nt_case("tail128", i, epi=epi, J=J, K=48, extra=0, bias=True, **kw))
    return out


def nt_operands(c):
    """CPU operands of an NT case.  Everything a kernel must not read is NaN: the pad columns of A and Bw, A rows from A_rows on."""
    g = torch.Generator().manual_seed(c["seed"])
    M, N, K, J = c["M"], c["N"], c["K"], c["J"]
    lda, ldb = K + 4, K + 8
    nan = float("nan")
    t = {}
    if c["loader"] == UNPOOL:
        a_rows = (M + c["extra"]) // 2            # pooled rows
        t["abits"] = torch.randint(-2 ** 31, 2 ** 31, (a_rows + 2, K // 32 + 1), generator=g, dtype=torch.int64).to(torch.int32)
    else:
        a_rows = M + c["extra"]
    A = torch.full((a_rows + 3, lda), nan)
    A[:a_rows, :K] = torch.randn(a_rows, K, generator=g)
    Bw = torch.full((J, N, ldb), nan)
    Bw[:, :, :K] = torch.randn(J, N, K, generator=g)
    t.update(A=A, Bw=Bw, A_rows=a_rows, lda=lda, ldb=ldb)
    if c["bias"]:
        t["bias"] = torch.randn(N, generator=g)
    if c["epi"] == MASK:
        if c["maskfrom"] == "bits":
            t["auxbits"] = torch.randint(-2 ** 31, 2 ** 31, (M + 1, (N + 31) // 32 + 1), generator=g, dtype=torch.int64).to(torch.int32)
        else:
            aux = torch.full((M + 1, N + 4), nan)
            aux[:M, :N] = torch.randn(M, N, generator=g)
            t["aux"] = aux
    return t


def nt_reference(c, t, variant=None):
    """float64 result of an NT case: dict(y = the rows before the epilogue, out, and for POOL obits / osign / their margins).
    ``variant``: "taps" (tap order reversed), "tvalid" (validity mask one pooled row later), "oddeven" (un-pooling swapped)."""
    A, a_rows, Bw = t["A"], t["A_rows"], t["Bw"]
    shift = 2 if variant == "tvalid" else 0
    if variant == "taps":
        Bw = Bw.flip(0)
    if c["loader"] == UNPOOL:
        ab = ~t["abits"] if variant == "oddeven" else t["abits"]
        A = gr.unpool_ref(A[:a_rows, :c["K"]], ab, c["Tp"], c["Tvalid_in"], shift)
        a_rows *= 2
    y = gr.nt_ref(A, Bw, M=c["M"], N=c["N"], K=c["K"], J=c["J"], row_shift=c["row_shift"], A_rows=a_rows)
    r = dict(y=y)
    bias = t.get("bias")
    if c["epi"] == STORE:
        r["out"] = y + bias.double() if bias is not None else y
    elif c["epi"] == LRELU:
        r["out"] = gr.lrelu(y + bias.double(), SLOPE)
    elif c["epi"] == POOL:
        r["out"], r["obits"], r["osign"], r["m_arg"], r["m_sign"] = gr.pool_ref(y, bias, SLOPE, c["Tp"], c["Tvalid"], shift)
    else:
        r["out"] = gr.mask_ref(y, SLOPE, aux=t.get("aux"), auxbits=t["auxbits"][:c["M"]] if "auxbits" in t else None)
    return r


def plane_skips(r):
    """The entries of the two bit planes of a POOL reference that are too close to call, as bool masks (arg-max, sign)."""
    lim = BIT_MARGIN * float(r["out"].abs().max())
    valid = r["m_sign"] > 0                      # masked pairs (and exact zeros) carry a clear bit whichever way rounding goes
    return (r["m_arg"] <= lim) & valid, (r["m_sign"] <= lim) & valid


# ------------------------------------------------------------------------------------------------------------------------
# TN cases
# ------------------------------------------------------------------------------------------------------------------------
TN_GEO = ((5, 12, 10), (3, 38, 30), (1, 70, 64))  # (S, Tp, Tvalid): Krows = 60, 114, 70 - 2, 4, 3 K-steps of 32 rows
TN_STEP = {"short": 64, "skinny": 16, "tn3": 32, "window": 32}


def tn_kernel(c):
    """The dispatch rule of tl_gemm_tn_window, restated for the matrix."""
    direct = c["loader"] == DIRECT
    if (c["J"] == 1 and direct and c["Krows"] <= 512 and c["splitk"] <= 8 and c["Mdim"] * c["Ndim"] <= 2 ** 20
            and c["ldc"] % 4 == 0):
        return "short"
    if c["Mdim"] <= 32 and c["J"] == 1 and direct:
        return "skinny"
    return "tn3" if c["J"] == 3 else "window"


def _tn_case(name, i, **kw):
    c = dict(loader=DIRECT, J=1, Tp=1, Tvalid=1, splitk=1, short=None, colsum=False, ldc_pad=4)
    c.update(kw)
    c["id"] = f"{name}-{i}"
    c["seed"] = _seed(c["id"])
    c["ldc"] = c["Ndim"] + c["ldc_pad"]
    c["kernel"] = tn_kernel(c)
    return c


def _tn_short(n=18):
    s = _seed("tn-short")
    Kr, Md, Nd = _rr((1, 63, 64, 65, 300, 512), n, s), _rr((4, 36, 72), n, s + 1), _rr((4, 132, 260), n, s + 2)
    sk, geo = _rr((1, 3, 8), n, s + 3), _rr(((1, 1), (7, 5), (100, 3)), n, s + 4)
    short, cs = _rr((None, "A", "B"), n, s + 5), _rr((True, True, False), n, s + 6)
    return [_tn_case("short", i, Krows=Kr[i], Mdim=Md[i], Ndim=Nd[i], splitk=sk[i], Tp=geo[i][0], Tvalid=geo[i][1],
                     short=short[i], colsum=cs[i]) for i in range(n)]


def _tn_skinny(n=9):
    s = _seed("tn-skinny")
    Kr, Md, Nd = _rr((513, 530, 1037), n, s), _rr((4, 8, 32), n, s + 1), _rr((8, 516, 1100), n, s + 2)
    sk, geo, short = _rr((1, 5, 40), n, s + 3), _rr(((1, 1), (11, 7)), n, s + 4), _rr((None, "A", "B"), n, s + 5)
    out = [_tn_case("skinny", i, Krows=Kr[i], Mdim=Md[i], Ndim=Nd[i], splitk=sk[i], Tp=geo[i][0], Tvalid=geo[i][1],
                    short=short[i]) for i in range(n)]
    # 40 splits of 33 / 34 16-row steps: the last slabs are empty and must come back as zeros
    out.append(_tn_case("skinny", n, Krows=513, Mdim=8, Ndim=516, splitk=40, Tp=11, Tvalid=7))
    out.append(_tn_case("skinny", n + 1, Krows=530, Mdim=32, Ndim=8, splitk=40))
    return out


def _tn_taps(name, Js, loader, Mds):
    s = _seed(name)
    n = 9
    Md, Nd = _rr(Mds, n, s + 1), _rr((32, 64, 96) if name.startswith("tn3") else (32, 160), n, s + 2)
    Jl, short = _rr(Js, n, s + 3), _rr((None, "A", "B"), n, s + 5)
    out = []
    for i in range(n):                            # every geometry with every split count (7 leaves the last splits empty)
        S, Tp, Tv = TN_GEO[i % 3]
        out.append(_tn_case(name, i, loader=loader, J=Jl[i], Krows=S * Tp, Mdim=Md[i], Ndim=Nd[i], splitk=(1, 2, 7)[i // 3],
                            Tp=Tp, Tvalid=Tv, short=short[i]))
    return out


def _tn_boundaries():
    """The same operands (seed) either side of each dispatch threshold."""
    out = []
    def pair(name, a, b, **common):
        sd = _seed("bound-" + name)
        for side, kw in (("lo", a), ("hi", b)):
            c = _tn_case("bound-" + name, side, **{**common, **kw})
            c["seed"] = sd
            out.append(c)
    pair("krows", dict(Krows=512), dict(Krows=513), Mdim=36, Ndim=132, alloc_rows=513)
    pair("krows-skinny", dict(Krows=512), dict(Krows=513), Mdim=32, Ndim=132, alloc_rows=513)
    pair("mdim", dict(Mdim=32), dict(Mdim=36), Krows=600, Ndim=132, alloc_cols=36)
    pair("splitk", dict(splitk=8), dict(splitk=9), Krows=300, Mdim=36, Ndim=132)
    pair("area", dict(Ndim=1024), dict(Ndim=1028), Krows=64, Mdim=1024, alloc_colsB=1028)
    pair("ldc", dict(ldc_pad=4), dict(ldc_pad=6), Krows=64, Mdim=36, Ndim=132)
    pair("ldc-skinny", dict(ldc_pad=4), dict(ldc_pad=6), Krows=64, Mdim=32, Ndim=132)
    return out


def tn_cases():
    return (_tn_short() + _tn_skinny() + _tn_taps("tn3-direct", (3,), DIRECT, (20, 132))
            + _tn_taps("tn3-unpool", (3,), UNPOOL, (20, 132)) + _tn_taps("window-direct", (2, 5, 7), DIRECT, (36, 132))
            + _tn_taps("window-unpool", (1, 2, 5), UNPOOL, (36, 132)) + _tn_boundaries())


def tn_operands(c):
    """CPU operands of a TN case: A [rows][lda], B [rows][ldb] (pooled rows under UNPOOL), NaN in the pad columns and in the rows
    from A_rows / B_rows on."""
    g = torch.Generator().manual_seed(c["seed"])
    Kr, J, Md, Nd = c["Krows"], c["J"], c["Mdim"], c["Ndim"]
    rows = c.get("alloc_rows", Kr)
    ca, cb = c.get("alloc_cols", Md), c.get("alloc_colsB", Nd)
    unpool = c["loader"] == UNPOOL
    a_rows = rows + J - 1 if c["short"] != "A" else max(1, rows - 3)
    b_full = rows // 2 if unpool else rows
    b_rows = b_full if c["short"] != "B" else max(1, b_full - 3)
    nan = float("nan")
    Afull = torch.randn(rows + J - 1, ca, generator=g)          # drawn whole, so both sides of a threshold see the same numbers
    Bfull = torch.randn(b_full, cb, generator=g)
    A = torch.full((rows + J + 1, ca + 4), nan)
    A[:a_rows, :Md] = Afull[:a_rows, :Md]
    B = torch.full((b_full + 2, cb + 8), nan)
    B[:b_rows, :Nd] = Bfull[:b_rows, :Nd]
    t = dict(A=A, B=B, A_rows=min(a_rows, Kr + J - 1), B_rows=min(b_rows, Kr // 2 if unpool else Kr), lda=ca + 4, ldb=cb + 8)
    if unpool:
        t["bbits"] = torch.randint(-2 ** 31, 2 ** 31, (b_full + 2, (Nd + 31) // 32 + 1), generator=g, dtype=torch.int64).to(torch.int32)
    return t


def tn_reference(c, t, variant=None):
    """float64 slabs [splitk][J * Mdim][Ndim] of a TN case (``variant`` as in nt_reference; "tvalid": the mask one row later)."""
    A, bb = t["A"], t.get("bbits")
    shift = 0
    if variant == "taps":                         # tap j reads A rows R + (J - 1 - j)
        s = tn_reference(c, t)
        return s.view(c["splitk"], c["J"], c["Mdim"], c["Ndim"]).flip(1).reshape(s.shape)
    if variant == "tvalid":
        shift = 2 if bb is not None else 1
    if variant == "oddeven":
        bb = ~bb
    return gr.tn_ref(A, t["B"], Krows=c["Krows"], A_rows=t["A_rows"], B_rows=t["B_rows"], Mdim=c["Mdim"], Ndim=c["Ndim"],
                     J=c["J"], Tp=c["Tp"], Tvalid=c["Tvalid"], splitk=c["splitk"], step=TN_STEP[c["kernel"]], bbits=bb,
                     chunked=c["kernel"] == "short", t_shift=shift)
