"""CPU: the shared launch helpers (``_launch.py``) fill the parameter structs exactly as documented and refuse unknown
field names, the group helpers hand member count, strides, mask and stream on unchanged; the classifier engine is a conv stack
without the synthesis model's parts.  No GPU, no kernel launch."""
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
    launch(lib, stream=55, **given)                       # a stream the caller has read already; it is no field
    name, p, stream = lib.calls[2]
    assert (name, stream) == (entry, 55) and fields_of(p) == want


def test_unknown_field_raises_and_launches_nothing():
    lib = StandInLib(NtParams)
    with pytest.raises(TypeError, match="ld_obit"):
        _launch.launch_nt(lib, A=16, ld_obit=1)
    lib_t = StandInLib(TnParams)
    with pytest.raises(TypeError, match="Tvalidd"):
        _launch.launch_tn(lib_t, Tvalidd=1)
    assert lib.calls == [] and lib_t.calls == []
    assert _launch.r4(5) == 8 and _launch.r4(8) == 8


class StandInGroupLib(StandInLib):
    """... and keeps what a ``_group`` entry is handed between the struct and the stream: member count, strides, ``active``."""

    def __getattr__(self, name):
        def entry(ref, *rest):
            p = self.struct()
            C.memmove(C.byref(p), ref, C.sizeof(p))
            self.calls.append((name, p, rest))
            return 0
        return entry


class Words:
    """A stand-in for the device tensor of mask words: the helpers pass its ``data_ptr()``."""

    def data_ptr(self):
        return 0x7000


GROUP_LAUNCHES = [
    (_launch.launch_nt_group_fc, NtParams, NT_DEFAULTS, "tl_gemm_nt_window_group_fc", (3, 640, 1280, 8, 320, 5120),
     dict(A=0x1000, aux=0x3000, ldaux=512, M=5, slope=0.25, epilogue=3, splitk=7, slab_stride=1 << 40, bm=32)),
    (_launch.launch_tn_group, TnParams, TN_DEFAULTS, "tl_gemm_tn_window_group", (3, 640, 1280, 1 << 33, 512),
     dict(A=0x1000, colsum=0x3000, Krows=511, Tp=5, Tvalid=4, splitk=8, slab_stride=1 << 40)),
]


@pytest.mark.parametrize("launch,struct,defaults,entry,group,given", GROUP_LAUNCHES)
def test_group_launch_defaults_fields_members_strides_active_and_stream(launch, struct, defaults, entry, group, given):
    lib = StandInGroupLib(struct)
    launch(lib, *group, None)
    name, p, rest = lib.calls[0]
    assert name == entry and rest == (*group, None, 77)                   # members, strides; active None -> NULL; the stream
    want = {n: 0 for n, _ in struct._fields_}
    want.update(defaults)
    assert fields_of(p) == want and bytes(p) == bytes(struct(**defaults))
    # given fields arrive unchanged on top of the defaults (M is a field: the member count is positional); the mask's pointer
    launch(lib, *group, Words(), **given)
    name, p, rest = lib.calls[1]
    assert name == entry and rest == (*group, 0x7000, 77) and len(lib.calls) == 2
    want.update(given)
    assert fields_of(p) == want
    # a stream the caller has read already is the one launched on; it is no field
    launch(lib, *group, None, stream=55, **given)
    name, p, rest = lib.calls[2]
    assert name == entry and rest == (*group, None, 55) and fields_of(p) == want


@pytest.mark.parametrize("launch,struct,defaults,entry,group,given", GROUP_LAUNCHES)
def test_group_launch_unknown_field_raises_and_launches_nothing(launch, struct, defaults, entry, group, given):
    lib = StandInGroupLib(struct)
    with pytest.raises(TypeError, match=f"{struct.__name__} has no field slab_strid"):
        launch(lib, *group, None, slab_strid=16, **given)
    with pytest.raises(TypeError):                                          # the strides and the mask are positional only
        launch(lib, *group, active=None)
    assert lib.calls == []


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


def test_pack_cache_rebuilds_when_a_tensor_it_was_built_from_changed():
    """``PackCache``: one build while every ``(_version, data_ptr())`` stands; a bumped version of any one tensor of a tuple, or
    a tensor at another address in its place, is a rebuild; with ``into`` the rebuild lands in the previous pack's storage."""
    import torch
    bump = torch.autograd.graph.increment_version
    cache, builds = _launch.PackCache(), []

    def pack_of(*ts):
        def build():
            builds.append(len(builds))
            return sum(t.detach().sum() for t in ts).reshape(1)
        return build

    a, b, c = (torch.nn.Parameter(torch.full((4,), float(i))) for i in (1, 2, 3))
    first = cache.get("abc", (a, b, c), pack_of(a, b, c))
    assert cache.get("abc", (a, b, c), pack_of(a, b, c)) is first and builds == [0]
    assert cache.get("abc", (a, b.detach(), c), pack_of(a, b, c)) is first and builds == [0]     # .detach() shares the counter
    for n, p in enumerate((a, b, c), start=1):                    # any one of the tuple
        bump(p)
        assert cache.get("abc", (a, b, c), pack_of(a, b, c)) is not first and builds == list(range(n + 1))
        assert cache.get("abc", (a, b, c), pack_of(a, b, c)) is cache.get("abc", (a, b, c), pack_of(a, b, c))
        assert builds == list(range(n + 1))
    # a single tensor is its own tuple; another key is another pack
    one = cache.get("a", a, pack_of(a))
    assert float(one) == 4.0 and cache.get("a", a, pack_of(a)) is one and len(builds) == 5
    # the parameter replaced by a tensor at another address (same version: both fresh)
    a2 = torch.nn.Parameter(a.detach().clone() * 2)
    torch.autograd.graph.increment_version([a2] * a._version)
    assert a2._version == a._version and a2.data_ptr() != a.data_ptr()
    two = cache.get("a", a2, pack_of(a2))
    assert float(two) == 8.0 and two is not one and len(builds) == 6
    # into: build() allocates once, into(pack) fills - the first time and every rebuild, in the same storage
    fills = []

    def fill(pack):
        fills.append(pack.data_ptr())
        pack.copy_(a2.detach() + 1)

    alloc = lambda: builds.append("alloc") or torch.empty(4)
    p0 = cache.get("into", a2, alloc, into=fill)
    assert builds.count("alloc") == 1 and len(fills) == 1 and torch.equal(p0, a2.detach() + 1)
    assert cache.get("into", a2, alloc, into=fill) is p0 and len(fills) == 1
    with torch.no_grad():
        a2.add_(1.0)                                              # torch's own in-place write moves the version too
    p1 = cache.get("into", a2, alloc, into=fill)
    assert p1.data_ptr() == p0.data_ptr() and builds.count("alloc") == 1 and len(fills) == 2
    assert torch.equal(p1, a2.detach() + 1)


def test_rejected_lowrank_update_leaves_schedule_and_version_alone():
    """Factors of the wrong shape are refused by the shape check, which stands before the device check - so this runs on the
    CPU - and before the schedule moves: no advanced ``step``, the parameter's ``_version`` as it was."""
    import torch
    from decode_tonal_langauge_amd.optim import FusedNAdam
    p = torch.nn.Parameter(torch.ones(6, 8))
    opt = FusedNAdam([p])
    version, value = p._version, p.detach().clone()
    for call in (lambda: opt.step(lowrank={p: (torch.ones(2, 5), torch.ones(2, 8))}),         # fa: 5 columns for 6 rows
                 lambda: opt.step_lowrank({p: (torch.ones(2, 6), torch.ones(3, 8))})):         # fb: another rank
        with pytest.raises(RuntimeError, match="do not match the parameter"):
            call()
        assert opt.state[p].get("step", 0) == 0 and opt.state[p].get("mu_product", 1.0) == 1.0
        assert p._version == version and torch.equal(p.detach(), value)
