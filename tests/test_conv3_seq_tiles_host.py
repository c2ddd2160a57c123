"""CPU: conv3 on whole-sequence tiles - the host side of the compact-M mode of ``tl_conv3_wino63v_nt`` (``a_hps_extra``), the
Y-only forms of epilogues 6 and 7, and the engine's decision where the path engages (no kernel is launched without a GPU)."""
import ctypes as C

import pytest


def _params(**kw):
    """A parameter set that passes every check in front of the compact-M block: 3 sequences of 16 computed hexes, 17 stored"""
    from decode_tonal_langauge_amd import _lib
    p = _lib.NtParams()
    for k in ("A", "Bw", "out", "obits"):
        setattr(p, k, 16)
    p.loader, p.J, p.epilogue, p.splitk = _lib.LOAD_V, 3, _lib.EPI_POOL, 1
    p.M, p.Tp, p.Tvalid, p.N, p.K, p.lda, p.ldb, p.ldo, p.ld_obits = 3 * 96, 96, 92, 64, 48, 48, 48, 64, 2
    p.A_rows, p.a_hps_extra, p.slope = 136, 1, 0.01
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _refused(fn, p, word):
    from decode_tonal_langauge_amd import _lib
    lib = _lib.load()
    rc = getattr(lib, fn)(C.byref(p), None)
    err = lib.tl_last_error()
    assert rc == -1 and word in err, (rc, err)


def test_the_new_field_fills_padding_and_moves_nothing():
    from decode_tonal_langauge_amd import _lib
    lib = _lib.load()
    nt = _lib.NtParams
    assert C.sizeof(nt) == lib.tl_sizeof_nt_params()
    assert nt.a_hps_extra.offset == nt.bm.offset + 4 and nt.osign.offset == nt.bm.offset + 8


def test_compact_m_refuses_a_bad_hex_pair_tiles_off_sequences_and_a_short_operand():
    _refused("tl_conv3_wino63v_nt", _params(a_hps_extra=-1), b"a_hps_extra must lie in")
    _refused("tl_conv3_wino63v_nt", _params(a_hps_extra=17), b"a_hps_extra must lie in")
    # 17 computed hexes per sequence: a 128-hex tile would start inside a sequence
    _refused("tl_conv3_wino63v_nt", _params(Tp=102, M=3 * 102), b"sequence boundaries")
    # 8 computed hexes: tiles start on sequences, but a lane would own two of them
    _refused("tl_conv3_wino63v_nt", _params(Tp=48, M=3 * 48, Tvalid=46), b"16 computed hexes")
    # one tile reads 8 stored sequences = 136 hexes; two tiles 272
    _refused("tl_conv3_wino63v_nt", _params(A_rows=134), b"8 (16 + a_hps_extra) hexes")
    _refused("tl_conv3_wino63v_nt", _params(M=9 * 96, A_rows=270), b"8 (16 + a_hps_extra) hexes")
    _refused("tl_conv3_wino63v_nt", _params(a_hps_extra=2, A_rows=142), b"8 (16 + a_hps_extra) hexes")
    # the other epilogues and the other entry points of the kernel keep the stored geometry
    from decode_tonal_langauge_amd import _lib
    _refused("tl_conv3_wino63v_nt", _params(epilogue=_lib.EPI_MASK, row_shift=-2, auxbits=16), b"POOL epilogue or epilogue 6")
    _refused("tl_conv3_wino63v_nt", _params(epilogue=_lib.EPI_POOLV), b"POOL epilogue or epilogue 6")


def test_the_other_entry_points_refuse_the_mode():
    from decode_tonal_langauge_amd import _lib
    p = _params(epilogue=_lib.EPI_LRELU, J=7, aux=16, ldb=144, A_rows=128)
    _refused("tl_conv7_wino63v_nt", p, b"a_hps_extra must be 0")
    p = _params(epilogue=_lib.EPI_MASK, J=7, aux=16, ldb=144, A_rows=128, auxbits=16, ld_auxbits=2)
    _refused("tl_conv7_wino63v_dgrad_nt", p, b"a_hps_extra must be 0")
    p = _params(epilogue=_lib.EPI_GY, J=1, A_rows=128, auxbits=16, abits=16)
    _refused("tl_conv1_wino63v_dgrad_nt", p, b"a_hps_extra must be 0")


def _masky(**kw):
    from decode_tonal_langauge_amd import _lib
    base = dict(epilogue=_lib.EPI_MASKY, out=None, obits=None, row_shift=0, auxbits=16, abits=16, ld_auxbits=2, ld_abits=2,
                Tvalid_in=196, vout=16, ld_vout=64, vout_quads=3 * 34)
    base.update(kw)
    return _params(**base)


def test_epilogue_6_on_whole_sequence_tiles_checks_its_operands():
    _refused("tl_conv3_wino63v_nt", _masky(row_shift=-2), b"row_shift 0")
    _refused("tl_conv3_wino63v_nt", _masky(abits=None), b"auxbits and abits")
    _refused("tl_conv3_wino63v_nt", _masky(Tvalid_in=198), b"Tvalid_in")        # rows 98.. of a sequence have no hex to go to
    _refused("tl_conv3_wino63v_nt", _masky(ld_abits=1), b"abits")
    _refused("tl_conv3_wino63v_nt", _masky(vout_quads=3 * 34 - 2), b"hexes per sequence")
    _refused("tl_conv3_wino63v_nt", _masky(vout2=16, vhalo=16), b"Y only")


def test_epilogue_7_takes_vout2_and_vhalo_together_or_neither():
    from decode_tonal_langauge_amd import _lib
    p = _params(epilogue=_lib.EPI_GY, J=1, a_hps_extra=0, M=3 * 51, Tp=51, A_rows=128, out=None, obits=None, auxbits=16, abits=16,
                ld_auxbits=2, ld_abits=2, out_tp=50, Tvalid_in=96, vout=16, ld_vout=64, vout_quads=52, vout2=16, vhalo=None)
    _refused("tl_conv1_wino63v_dgrad_nt", p, b"together")
    p.vout2, p.vhalo = None, 16
    _refused("tl_conv1_wino63v_dgrad_nt", p, b"together")


NARROW = [(128, 3, True), (128, 3, True), (64, 3, True), (64, 1, True), (8, 1, False)]
WIDE = [(256, 3, True), (256, 3, True), (128, 3, True), (64, 1, True), (8, 1, False)]


def _engine(T, defs=WIDE, n_ch=3):
    from decode_tonal_langauge_amd._cnn_engine import CnnEngine
    return CnnEngine(80, n_ch, T, 4, 8, 0.0, 0.01, defs, [16, 8])


def test_the_engine_engages_where_the_valid_rows_fit_16_of_more_stored_hexes(monkeypatch):
    e = _engine(400)
    s3 = e.stages[1]
    assert (s3.tc, s3.tp_in) == (96, 102) and e.f63_yprod and e.f63_yprod3 and e.gy4 and e.f63_seq16
    # 388 samples: 93 valid conv rows in the same 17 stored hexes - a lane's last hex is half padding
    e = _engine(388)
    s3 = e.stages[1]
    assert (s3.tc, s3.tp_in) == (93, 102) and e.f63_seq16
    # 17 hexes of valid rows: the path must not engage
    e = _engine(412)
    s3 = e.stages[1]
    assert s3.tc > 96 and s3.tp_in // 6 > 16 and not e.f63_seq16
    # nothing stored beyond 16 hexes: nothing to skip
    e = _engine(376)
    s3 = e.stages[1]
    assert s3.tp_in == 96 and not e.f63_seq16
    # C_in of conv2 not a multiple of 256: conv2 does not run on Y2, the chain of Y operands is not there
    assert not _engine(400, NARROW).f63_seq16
    monkeypatch.setenv("TONAL_KERNELS", "f63_yprod=vd3")
    assert not _engine(400).f63_seq16
    monkeypatch.setenv("TONAL_KERNELS", "conv4_dgrad=gemm")
    assert not _engine(400).f63_seq16
    monkeypatch.setenv("TONAL_KERNELS", "f63_yprod=2")
    with pytest.raises(ValueError):
        _engine(400)


def test_issue_factors_and_family_labels_report_what_is_issued(monkeypatch):
    e = _engine(400)
    s2, s3 = e.stages[0], e.stages[1]
    assert abs(e.f63_issue_factor(s3) - 16 * 8 / (96 * 3)) < 1e-12
    assert abs(e.f63_issue_factor(s3, wgrad=True) - 17 * 8 / (96 * 3)) < 1e-12 and e.wgrad_issue_factor(s3) == e.f63_issue_factor(s3, wgrad=True)
    assert abs(e.f63_issue_factor(s2) - 34 * 8 / (197 * 3)) < 1e-12 and e.wgrad_issue_factor(s2) == e.f63_issue_factor(s2)
    fams, issued = e.kernel_families()
    by_tag = {tags[0]: k for k, tags in fams.items()}
    assert "16 of the 17 stored hexes" in by_tag["conv3_fwd"] and "16 of the 17 stored hexes" in by_tag["conv3_dgrad"]
    assert "on Y3" in by_tag["conv3_dgrad"] and "Vd3" not in by_tag["conv3_wgrad"]
    assert issued[by_tag["conv3_fwd"]] == issued[by_tag["conv3_dgrad"]] == e.f63_issue_factor(s3)
    assert issued[by_tag["conv3_wgrad"]] == e.f63_issue_factor(s3, wgrad=True)
    assert all(issued[by_tag[t]] == e.f63_issue_factor(s2) for t in ("conv2_fwd", "conv2_dgrad", "conv2_wgrad"))
    monkeypatch.setenv("TONAL_KERNELS", "f63_yprod=vd3")
    e = _engine(400)
    fams, issued = e.kernel_families()
    assert all("16 of" not in k for k in fams) and e.f63_issue_factor(e.stages[1]) == 17 * 8 / (96 * 3)


def test_the_operand_buffers_cover_eight_stored_sequences_per_row_tile():
    """``_v_hex_buffer`` appends zero hexes to whole 128-hex tiles and by at least 24; the whole-sequence launches read 8 stored
    sequences (136 hexes) per row tile: S = 3 would hold 128 hexes, S = 17 384 of the 408 its three tiles read.  Their two
    operands (V2, Y3) are sized for it; every other buffer, and every sequence count that is a multiple of 8, as before."""
    import torch
    e = _engine(400)
    e._dev, e.V, e.Yt, e.Vd = torch.device("cpu"), {}, {}, {}
    for S, want, plain in ((3, 256, 128), (8, 256, 256), (17, 512, 384), (768, 13184, 13184)):
        e.S = S
        assert want >= -(-S // 8) * 136 and plain == (S * 17 + 24 + 127) // 128 * 128
        assert e._v_hex_buffer(e.V, 2, S * 102, 8).shape == (want, 8, 8)
        assert e._v_hex_buffer(e.Yt, 3, S * 102, 8).shape == (want, 8, 8)
        assert e._v_hex_buffer(e.Vd, 3, S * 102, 8).shape == (plain, 8, 8)
        assert e._v_hex_buffer(e.Yt, 2, S * 102, 8).shape == (plain, 8, 8)
    assert e._seq16(e.stages[1]) and not e._seq16(e.stages[0])
