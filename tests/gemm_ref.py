"""The windowed NT / TN GEMMs of csrc/tonal_gemm.hip restated in float64 - TEST INFRASTRUCTURE.

Plain torch on CPU tensors, written from the entry points' contract (include/tonal_hip.h, the comments of tonal_gemm.hip) and
sharing no code with the engines or the oracle.  tests/test_gemm_ref_host.py holds every function here against stock torch
(conv1d, max_pool1d, max_unpool1d, autograd), so a mistake in this file cannot hide a mistake in a kernel.

Bit planes are ``int32`` words, bit ``k & 31`` of word ``k >> 5`` belongs to column ``k``; ``bits`` / ``pack`` convert.
``t_shift`` (0 everywhere in the kernels' contract) moves the time index the validity masks are taken on: the host test uses it
to show that a mask moved by one row changes the result at every tested shape."""
import torch

F64 = torch.float64


def bits(words, ncols):
    """int32 words [R][W] -> bool [R][ncols]."""
    w = words.to(torch.int64) & 0xFFFFFFFF
    k = torch.arange(ncols)
    return ((w[:, k >> 5] >> (k & 31)) & 1).bool()


def pack(mask):
    """bool [R][C] -> int32 words [R][ceil(C / 32)] (pad bits 0)."""
    R, Cn = mask.shape
    W = (Cn + 31) // 32
    m = torch.zeros(R, W * 32, dtype=torch.int64)
    m[:, :Cn] = mask.to(torch.int64)
    w = (m.view(R, W, 32) << torch.arange(32)).sum(2)
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)


def lrelu(z, slope):
    return torch.where(z > 0, z, slope * z)


def nt_ref(A, Bw, *, M, N, K, J, row_shift, A_rows):
    """y[R][n] = sum_{j < J} sum_{k < K} A[R + row_shift + j][k] * Bw[j][n][k]; A rows outside [0, A_rows) are zero.
    ``Bw``: [J][N][ldb] (tap stride N * ldb)."""
    y = torch.zeros(M, N, dtype=F64)
    R = torch.arange(M)
    for j in range(J):
        rows = R + row_shift + j
        ok = (rows >= 0) & (rows < A_rows)
        a = torch.zeros(M, K, dtype=F64)
        a[ok] = A[rows[ok], :K].to(F64)
        y += a @ Bw[j, :N, :K].to(F64).t()
    return y


def unpool_ref(G, abits, Tp, Tvalid_in, t_shift=0):
    """Pooled rows G [P][K] -> conv rows [2 P][K]: column k of pooled row r goes to row 2r + 1 if its bit is set, else to row 2r;
    the pair is zero where (2r % Tp) >= Tvalid_in."""
    P, K = G.shape
    odd = bits(abits[:P], K)
    valid = ((2 * torch.arange(P) + t_shift) % Tp) < Tvalid_in
    g = torch.where(valid[:, None], G.to(F64), torch.zeros((), dtype=F64))
    out = torch.zeros(2 * P, K, dtype=F64)
    out[0::2] = torch.where(odd, torch.zeros((), dtype=F64), g)
    out[1::2] = torch.where(odd, g, torch.zeros((), dtype=F64))
    return out


def pool_ref(y, bias, slope, Tp, Tvalid, t_shift=0):
    """LeakyReLU(y + bias), then the max of rows 2r, 2r + 1 -> pooled row r.  Returns (out, obits, osign, margin_arg, margin_sign):
    obits = (y1 > y0) on valid pairs, osign = out > 0, both bool [M / 2][N]; pairs with (2r % Tp) >= Tvalid give 0 and clear bits.
    The margins |y1 - y0| and |out| say how far each decision is from flipping."""
    z = y.to(F64) if bias is None else y.to(F64) + bias.to(F64)
    a = lrelu(z, slope)
    y0, y1 = a[0::2], a[1::2]
    valid = (((2 * torch.arange(y0.shape[0]) + t_shift) % Tp) < Tvalid)[:, None]
    sel = (y1 > y0) & valid
    out = torch.where(valid, torch.where(sel, y1, y0), torch.zeros((), dtype=F64))
    return out, sel, out > 0, (y1 - y0).abs(), out.abs()


def mask_ref(y, slope, aux=None, auxbits=None):
    """y where aux > 0 (or where the sign bit of ``auxbits`` is set), slope * y elsewhere."""
    pos = bits(auxbits, y.shape[1]) if auxbits is not None else aux[:y.shape[0], :y.shape[1]] > 0
    return torch.where(pos, y, slope * y)


def tn_valid_rows(Krows, Tp, Tvalid, unpool=False, t_shift=0):
    R = torch.arange(Krows)
    if unpool:
        R = R - (R & 1)                                   # validity is taken on the even conv row of a pooled pair
    return ((R + t_shift) % Tp) < Tvalid


def tn_split_ranges(*, Krows, A_rows, B_rows, splitk, step, chunked=False):
    """Row range [r0, r1) of every split.  Whole ``step``-row K-steps dealt out evenly (tn_window / tn3: 32, tn_skinny: 16); with
    ``chunked`` (tn_short, step 64) the rows that exist in A and B are dealt out evenly and each share is rounded up to whole
    chunks."""
    if chunked:
        kall = min(Krows, A_rows, B_rows)
        per = -(-(-(-kall // splitk)) // step) * step
        return [(min(z * per, kall), min(z * per + per, kall)) for z in range(splitk)]
    nsteps = -(-Krows // step)
    per = -(-nsteps // splitk) * step
    return [(min(z * per, Krows), min(z * per + per, Krows)) for z in range(splitk)]


def tn_ref(A, B, *, Krows, A_rows, B_rows, Mdim, Ndim, J, Tp, Tvalid, splitk, step, bbits=None, chunked=False, t_shift=0):
    """slab[z][j * Mdim + m][n] = sum_R A[R + j][m] * B[R][n] over split z's rows with R < min(Krows, B_rows) and (R % Tp) < Tvalid;
    A rows >= min(A_rows, Krows + j) are zero.  With ``bbits`` B holds pooled rows (B_rows of them) and is un-pooled first."""
    if bbits is not None:
        Bc = unpool_ref(B[:B_rows, :Ndim], bbits[:B_rows], Tp, Tvalid, t_shift)
        b_rows = 2 * B_rows
    else:
        Bc, b_rows = B[:, :Ndim].to(F64), B_rows
    b_lim = min(Krows, b_rows)
    Bm = torch.zeros(Krows, Ndim, dtype=F64)
    Bm[:b_lim] = Bc[:b_lim]
    Bm[~tn_valid_rows(Krows, Tp, Tvalid, bbits is not None, t_shift)] = 0
    slabs = torch.zeros(splitk, J * Mdim, Ndim, dtype=F64)
    ranges = tn_split_ranges(Krows=Krows, A_rows=A_rows, B_rows=b_rows, splitk=splitk, step=step, chunked=chunked)
    for j in range(J):
        Aj = torch.zeros(Krows, Mdim, dtype=F64)
        n = max(0, min(A_rows, Krows + j) - j)            # rows R with R + j inside A
        Aj[:n] = A[j:j + n, :Mdim].to(F64)
        for z, (r0, r1) in enumerate(ranges):
            slabs[z, j * Mdim:(j + 1) * Mdim] = Aj[r0:r1].t() @ Bm[r0:r1]
    return slabs


def tn_colsum_a_ref(A, *, Krows, A_rows, B_rows, Mdim, Tp, Tvalid):
    """tn_short's ``colsum``: the column sums of A over the rows that take part in the product."""
    kall = min(Krows, A_rows, B_rows)
    keep = tn_valid_rows(kall, Tp, Tvalid)
    return A[:kall, :Mdim].to(F64)[keep].sum(0)
