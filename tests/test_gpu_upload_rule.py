"""GPU: the input rule of ``_lib.to_gpu`` at the sites whose own tests do not hold it (mel, Welch and YIN have theirs): the same
recording given as a read-only array, a Fortran-ordered array, an int16 array, a row-strided CUDA view and a transposed CUDA
view gives, bit for bit, what its contiguous float64 copy gives, and the result's container follows the input's."""
import warnings
from argparse import Namespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

STARTS, LENGTH = [0, 13, 450], 250


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch.device("cuda:0")


def _sites():
    from decode_tonal_langauge_amd.channel_selection.utils import anova_oneway
    from decode_tonal_langauge_amd.data_loading.epoching import extract_windows
    from decode_tonal_langauge_amd.preprocess.signal import car_rereference, channel_zscore, frequency_filter
    return {
        "car_rereference": lambda x: car_rereference.run(x, Namespace()),
        "channel_zscore": lambda x: channel_zscore.run(x, Namespace()),
        "hilbert_filter": lambda x: frequency_filter.hilbert_filter(x, 400, [(70.0, 150.0)]),
        "anova_oneway": lambda x: anova_oneway(x, np.array([0, 0, 1])),
        "extract_windows": lambda x: extract_windows(x, STARTS, LENGTH),
    }


@pytest.fixture(scope="module")
def recording():
    rec = np.random.default_rng(20240607).standard_normal((3, 700))
    rec.setflags(write=False)
    return rec


@pytest.fixture(scope="module")
def expected(dev, recording):
    """Per site: the result on the contiguous float64 array, on the float64 copy of its int16 form and (``extract_windows``
    moves elements of any size) on the int16 array itself - computed once, as NumPy."""
    as_i16 = (recording * 1000.0).astype(np.int16)
    out = {}
    for name, site in _sites().items():
        out[name] = {"f64": _host(site(np.array(recording))),
                     "i16": _host(site(as_i16.copy() if name == "extract_windows" else as_i16.astype(np.float64)))}
    return out


def _host(result):
    parts = result if isinstance(result, tuple) else (result,)
    return tuple(p.cpu().numpy() if isinstance(p, torch.Tensor) else np.asarray(p) for p in parts)


def _forms(recording, dev):
    as_i16 = (recording * 1000.0).astype(np.int16)
    wide = torch.zeros(3, 900, dtype=torch.float64, device=dev)
    wide[:, :700] = torch.from_numpy(np.array(recording)).to(dev)
    tall = torch.from_numpy(np.ascontiguousarray(recording.T)).to(dev)
    return {"read_only": (recording, "f64"), "fortran": (np.asfortranarray(recording), "f64"), "int16": (as_i16, "i16"),
            "row_strided_view": (wide[:, :700], "f64"), "transposed_view": (tall.t(), "f64")}


@pytest.mark.parametrize("form", ["read_only", "fortran", "int16", "row_strided_view", "transposed_view"])
@pytest.mark.parametrize("site", ["car_rereference", "channel_zscore", "hilbert_filter", "anova_oneway", "extract_windows"])
def test_every_form_of_the_recording_gives_the_bits_of_its_contiguous_copy(dev, recording, expected, site, form):
    x, key = _forms(recording, dev)[form]
    if form == "read_only":
        assert not x.flags.writeable
    if form == "fortran":
        assert not x.flags.c_contiguous
    if form == "row_strided_view":
        assert x.stride() == (900, 1) and not x.is_contiguous()
    if form == "transposed_view":
        assert x.stride() == (1, 3)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                       # a read-only array must not draw torch's non-writable warning
        got = _sites()[site](x)
    parts = got if isinstance(got, tuple) else (got,)
    # the container follows the input; extract_windows hands the device tensor to its caller whatever it was given
    on_device = isinstance(x, torch.Tensor) or site == "extract_windows"
    for p in parts:
        if on_device:
            assert isinstance(p, torch.Tensor) and p.device == dev
        else:
            assert isinstance(p, np.ndarray)
    want = expected[site][key]
    assert len(parts) == len(want)
    for p, w in zip(_host(got), want):
        assert p.dtype == w.dtype and p.shape == w.shape
        assert np.array_equal(p, w, equal_nan=p.dtype.kind == "f")
