"""CPU: the shared launch helpers (``_launch.py``) fill the parameter structs exactly as documented and refuse unknown
field names; the classifier engine is a conv stack without the synthesis model's parts.  No GPU, no kernel launch."""
import ctypes as C

import pytest

from decode_tonal_langauge_amd import _launch
from decode_tonal_langauge_amd._lib import NtParams, TnParams

NT_DEFAULTS = dict(splitk=1, bm=128, J=1, Tp=1, slope=0.0)          # everything else 0 / NULL: Tvalid stays 0
TN_DEFAULTS = dict(splitk=1, J=1, Tp=1, Tvalid=1)


class StandInLib:
    """Every entry point copies the struct it is handed and reports success."""

    def __init__(self, struct):
        self.struct, self.calls = struct, []

    def __getattr__(self, name):
        def entry(ref, stream):
            p = self.struct()
            C.memmove(C.byref(p), ref, C.sizeof(p))
            self.calls.append((name, p, stream))
            return 0
        return entry


def fields_of(p):
    return {name: getattr(p, name) or 0 for name, _ in p._fields_}       # (a NULL c_void_p reads as None)


@pytest.fixture(autouse=True)
def stream(monkeypatch):
    monkeypatch.setattr(_launch, "_stream", lambda: 77)


@pytest.mark.parametrize("launch,struct,defaults,entry", [
    (_launch.launch_nt, NtParams, NT_DEFAULTS, "tl_gemm_nt_window"), (_launch.launch_tn, TnParams, TN_DEFAULTS, "tl_gemm_tn_window")])
def test_launch_defaults_fields_and_entry_point(launch, struct, defaults, entry):
    lib = StandInLib(struct)
    launch(lib)
    name, p, stream = lib.calls[0]
    assert (name, stream) == (entry, 77)
    want = {n: 0 for n, _ in struct._fields_}
    want.update(defaults)
    assert fields_of(p) == want
    blank = struct(**defaults)
    assert bytes(p) == bytes(blank)
    # given fields arrive unchanged, on top of the defaults; fn= selects the entry point
    given = dict(A=0x1000, lda=36, Tp=50, Tvalid=48, splitk=7, slab_stride=1 << 40, loader=2)
    launch(lib, fn="tl_other_entry", **given)
    name, p, _ = lib.calls[1]
    assert name == "tl_other_entry" and len(lib.calls) == 2
    want.update(given)
    assert fields_of(p) == want


def test_unknown_field_raises_and_launches_nothing():
    lib = StandInLib(NtParams)
    with pytest.raises(TypeError, match="ld_obit"):
        _launch.launch_nt(lib, A=16, ld_obit=1)
    lib_t = StandInLib(TnParams)
    with pytest.raises(TypeError, match="Tvalidd"):
        _launch.launch_tn(lib_t, Tvalidd=1)
    assert lib.calls == [] and lib_t.calls == []
    assert _launch.r4(5) == 8 and _launch.r4(8) == 8


def test_classifier_engine_is_a_conv_stack_without_the_synthesis_parts(monkeypatch):
    """At the stage list of CNNClassifier (tests/test_gpu_pipeline.py): the same stack geometry as a CnnEngine that keeps the
    F(4,3) geometry, and none of the LSTM / concat / output-layer attributes or passes."""
    from decode_tonal_langauge_amd._classifier_engine import CnnClassifierEngine
    from decode_tonal_langauge_amd._cnn_engine import CnnEngine
    from decode_tonal_langauge_amd._conv_stack import ConvStack
    defs = [(512, 3, True), (512, 3, True), (512, 3, True), (512, 3, True), (512, 3, False), (256, 3, True)]
    for Cn, T in ((8, 400), (3, 401)):
        clf = CnnClassifierEngine(Cn, T, defs, 1024, 4, 0.01)
        with monkeypatch.context() as m:
            m.setattr(CnnEngine, "F63_CAPABLE", False)
            syn = CnnEngine(4, Cn, T, 2, defs[-1][0], 0.0, 0.01, defs, [16, 8])
        assert not clf.wino63 and not syn.wino63 and len(clf.stages) == len(syn.stages) == 5
        for a, b in zip(clf.stages, syn.stages):
            assert (a.tp_in, a.tp_out, a.tout, a.tin) == (b.tp_in, b.tp_out, b.tout, b.tin)
        assert (clf.tp1, clf.lat, clf.tp5, clf.ld5) == (syn.tp1, syn.lat, syn.tp5, syn.ld5)
        assert clf.n63 == 3 and clf.tp63[0] % 24 == 0 and clf.tp63[0] >= clf.tout1       # the F(6,3) prefix: its own rows
        for name in ("concat_dims", "kflat", "ldx", "lowrank_param", "backward", "forward", "grad_order", "_lstm_forward"):
            assert hasattr(syn, name) and not hasattr(clf, name), name
    assert CnnEngine not in CnnClassifierEngine.__mro__ and ConvStack in CnnClassifierEngine.__mro__
    assert issubclass(CnnEngine, ConvStack)
