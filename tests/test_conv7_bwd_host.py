"""CPU: the host side of ``TONAL_KERNELS conv7=wino63bwd`` (the F(6,3) backward of the CNN-RNN classifier's 7-tap stages) - the
setting, the exported symbols, the two appended struct fields and the argument checks that run without a GPU."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("tl_wino63_ydz", "tl_wino63_xform2s", "tl_conv7_wino63v_dgrad_nt")


def test_conv7_takes_wino63bwd_and_refuses_unknown_values(monkeypatch):
    from decode_tonal_langauge_amd import _kernels
    monkeypatch.delenv("TONAL_CONV7", raising=False)
    monkeypatch.setenv("TONAL_KERNELS", "conv7=wino63bwd")
    assert _kernels.get("conv7") == "wino63bwd" and _kernels.conv7_forward() == "wino63"
    _kernels.validate()
    monkeypatch.setenv("TONAL_KERNELS", "conv7=direct")
    assert _kernels.conv7_forward() == "direct"
    monkeypatch.setenv("TONAL_KERNELS", "")
    assert _kernels.get("conv7") == "wino63" and _kernels.conv7_forward() == "wino63"      # the default stays
    for bad in ("conv7=wino63fwd", "conv7=wino63bwd2", "conv7="):
        monkeypatch.setenv("TONAL_KERNELS", bad)
        with pytest.raises(ValueError, match="conv7"):
            _kernels.get("conv7")
    assert len(_kernels.KEYS) <= 12


def test_new_symbols_are_exported_and_declared():
    from decode_tonal_langauge_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "tonal_hip.h")).read()
    declared = set(re.findall(r"\b(tl_[a-z0-9_]+)\s*\(", header))
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name


def test_appended_struct_fields_match_the_library():
    from decode_tonal_langauge_amd import _lib
    lib = _lib.load()
    nt, tn = _lib.NtParams, _lib.TnParams
    assert C.sizeof(nt) == lib.tl_sizeof_nt_params() and C.sizeof(tn) == lib.tl_sizeof_tn_params()
    # appended, in this order, behind the fields the parent had last
    assert [f[0] for f in nt._fields_][-3:] == ["vout2", "mask", "ld_mask"]
    assert nt.mask.offset == nt.vout2.offset + 8 and nt.ld_mask.offset == nt.mask.offset + 8
    assert [f[0] for f in tn._fields_][-2:] == ["g_tp", "a_hex"] and tn.a_hex.offset == tn.g_tp.offset + 4


def test_bad_arguments_are_refused_without_a_gpu():
    from decode_tonal_langauge_amd import _lib
    lib = _lib.load()
    err = lambda: lib.tl_last_error()
    assert lib.tl_wino63_ydz(None, None, 24, 12, 6, 8, 8, 8, None) == -1 and b"null" in err()
    assert lib.tl_wino63_ydz(16, 16, 24, 12, 13, 8, 8, 8, None) == -1 and b"Tvalid" in err()
    assert lib.tl_wino63_ydz(16, 16, 24, 10, 6, 8, 8, 8, None) == -1
    assert lib.tl_wino63_ydz(16, 16, 24, 12, 6, 8, 8, 12, None) == -1 and b"ldv" in err()
    assert lib.tl_wino63_xform2s(16, 16, 16, 24, 12, 6, 7, 8, 8, 8, None) == -1 and b"shift" in err()
    assert lib.tl_wino63_xform2s(16, 16, None, 24, 12, 6, 6, 8, 8, 8, None) == -1 and b"null" in err()
    assert lib.tl_conv7_wino63v_dgrad_nt(None, None) == -1
    p = _lib.NtParams()
    p.A = p.aux = p.Bw = p.out = 16
    p.M, p.A_rows, p.N, p.K, p.lda, p.ldb, p.ldo = 24, 128, 32, 16, 16, 48, 32
    p.J, p.Tp, p.Tvalid, p.slope, p.loader, p.epilogue, p.splitk = 7, 12, 12, 0.1, _lib.LOAD_V, _lib.EPI_MASK, 1
    assert lib.tl_conv7_wino63v_dgrad_nt(C.byref(p), None) == -1 and b"mask source" in err()       # neither
    p.auxbits, p.ld_auxbits, p.mask, p.ld_mask = 16, 1, 16, 32
    assert lib.tl_conv7_wino63v_dgrad_nt(C.byref(p), None) == -1 and b"mask source" in err()       # both
    p.auxbits = None
    p.ld_mask = 16
    assert lib.tl_conv7_wino63v_dgrad_nt(C.byref(p), None) == -1 and b"ld_mask" in err()
    p.ld_mask, p.epilogue = 32, _lib.EPI_LRELU
    assert lib.tl_conv7_wino63v_dgrad_nt(C.byref(p), None) == -1 and b"MASK" in err()
    p.epilogue, p.J = _lib.EPI_MASK, 3
    assert lib.tl_conv7_wino63v_dgrad_nt(C.byref(p), None) == -1 and b"7 taps" in err()
    p.J, p.ldb = 7, 40
    assert lib.tl_conv7_wino63v_dgrad_nt(C.byref(p), None) == -1 and b"leading" in err()
    # the hex offset of the transform-free weight-gradient kernel: 0 or 1, and only with both operands pre-transformed
    t = _lib.TnParams()
    t.A = t.B = t.slab = 16
    t.Krows, t.A_rows, t.B_rows, t.Mdim, t.Ndim, t.lda, t.ldb, t.ldc = 24, 128, 128, 256, 64, 256, 64, 64
    t.J, t.Tp, t.Tvalid, t.loader, t.splitk, t.a_hex = 3, 12, 6, _lib.LOAD_Y, 1, 2
    assert lib.tl_conv3_wino63v_tn(C.byref(t), None) == -1 and b"a_hex" in err()
    t.loader, t.a_hex, t.bbits = _lib.LOAD_UNPOOL, 1, 16
    assert lib.tl_conv3_wino63v_tn(C.byref(t), None) == -1 and b"a_hex" in err()
