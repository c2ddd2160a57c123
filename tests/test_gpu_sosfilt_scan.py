"""GPU: the time-parallel causal Butterworth filter (``TONAL_KERNELS=butter=scan`` with ``causal=True``, tl_sosfilt_scan_f64)
against the sequential kernel, which stands in for scipy (tests/test_gpu_signal_steps.py holds it at 0 from ``sosfilt``).

Bound per case, relative to the largest output sample: 3 x the largest ratio the host test recorded for the restated scan
(profiles/parity_observed.json, section ``sosfilt_scan_restated``) x the case's own yardstick - |scipy - the same loop in long
double| on three channels and the first min(T, 16 384) samples (the filter is causal: an output prefix depends on the input
prefix only) - with a floor of 16 eps.  Exact properties: the first two blocks of every channel, and so a whole recording of up to
two blocks, carry the sequential kernel's bits; a longer one does not (it really is the other kernel); two runs agree bit for bit.

Observed on the MI355X (profiles/parity_observed.json, sections ``sosfilt_scan_*``): the recorded restatement ratio is 1.81, so
the bound is 5.4 x the yardstick; the scan stands 0 - 2.4 x the yardstick from the sequential kernel (worst: 70 x 16 385,
3.1e-14 against a yardstick of 1.3e-14)."""
import json
import os

import numpy as np
import pytest
import scipy.signal as sps
import torch

from tests import sosfilt_scan_ref as R
from tests.parity_record import record

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = float(np.finfo(np.float64).eps)
L = 128                                                      # frequency_filter._SCAN_L: no case here has > 65 535 blocks


def _restated_ratio():
    with open(os.path.join(ROOT, "profiles", "parity_observed.json")) as f:
        sec = json.load(f)["sosfilt_scan_restated"]
    return max(float(v) for k, v in sec.items() if k.endswith("ratio"))


def _both(x, freqs, fs, **kw):
    from decode_tonal_langauge_amd.preprocess.signal import frequency_filter as ff
    seq = ff.butter_filter(x, freqs, fs, causal=True, **kw)
    os.environ["TONAL_BUTTER"] = "scan"                      # (A/B switch; the product setting is TONAL_KERNELS=butter=scan)
    try:
        scan = ff.butter_filter(x, freqs, fs, causal=True, **kw)
    finally:
        os.environ.pop("TONAL_BUTTER", None)
    return seq, scan


def _judge(tag, x, seq, scan, order, freqs, fs, ftype):
    """deviation and bound of one case, both relative to the largest output sample; recorded, printed, then asserted"""
    sos = R.design(order, freqs, fs, ftype)
    assert scan.dtype == np.float64 and scan.shape == seq.shape == x.shape and np.isfinite(scan).all()
    n = min(x.shape[1], 16384)
    head = np.asarray(x[:3, :n], dtype=np.float64)
    ref = sps.sosfilt(sos, head, axis=-1)
    scale = float(np.abs(seq).max())
    assert np.abs(seq[:3, :n] - ref).max() <= 1e-13 * scale  # the stand-in is scipy (observed: 0), as test_gpu_signal_steps holds it
    yard = float(np.abs(R.sosfilt_loop(sos, head, np.longdouble).astype(np.float64) - ref).max()) / scale
    dev = float(np.abs(scan - seq).max()) / scale
    bound = max(3.0 * _restated_ratio() * yard, 16 * EPS)
    print(f"{tag}: scan vs sequential {dev:.3e}, scipy vs long double {yard:.3e}, bound {bound:.3e}")
    record(f"sosfilt_scan_{tag}", {"scan vs sequential": dev, "scipy vs long double (prefix)": yard, "bound": bound})
    assert dev <= bound, (tag, dev, bound)
    return dev


@pytest.mark.parametrize("C,T,dtype", [(3, 60, np.float64), (65, 129, np.float32), (70, 16385, np.float64), (1, 300007, np.float64),
                                       (256, 24000, np.float32)])
def test_scan_sosfilt_sizes(C, T, dtype):
    """one block; a block edge + 1 with 64 + 1 channels; across a chunk of the prefix (129 blocks: past 64 and past 128); many
    chunks; the C5 size"""
    assert R.has_long_double()
    x = np.random.default_rng(C * 7 + T).standard_normal((C, T)).astype(dtype)
    seq, scan = _both(x, [2.0, 60.0], 400.0)
    _judge(f"{C}x{T}_{np.dtype(dtype).name}", x, seq, scan, 4, [2.0, 60.0], 400.0, "bandpass")
    # the first block runs the same statements from a zero state, and the state it ends in IS the second block's start state
    # (A^L . 0 + s_0, exact): two blocks carry the sequential kernel's bits, so (65, 129) - one sample into the second block -
    # is bit-equal as a whole; from the third block on the states come out of the scan
    assert np.array_equal(scan[:, :2 * L], seq[:, :2 * L])
    if T <= 2 * L:
        assert np.array_equal(scan, seq)
    else:
        assert not np.array_equal(scan, seq)                 # really the other kernel
    _seq2, scan2 = _both(x, [2.0, 60.0], 400.0)
    assert np.array_equal(scan2, scan)                       # two runs, the same bits


@pytest.mark.parametrize("name,order,freqs,fs,ftype,dc", [
    ("lp1", 1, 60.0, 400.0, "lowpass", 0.0), ("lp2", 2, 60.0, 400.0, "lowpass", 0.0), ("lp16", 16, 60.0, 400.0, "lowpass", 0.0),
    ("bp8", 8, [70.0, 150.0], 400.0, "bandpass", 0.0), ("hp4_dc1000", 4, 0.5, 400.0, "highpass", 1000.0),
    ("bp4_24414", 4, [1.0, 50.0], 24414.0, "bandpass", 0.0)])
def test_scan_sosfilt_designs(name, order, freqs, fs, ftype, dc):
    """1, 1 and 8 sections of a low-pass, 8 of a band-pass, a high-pass on a DC level, a very low band at a raw rate"""
    assert R.has_long_double()
    x = np.random.default_rng(order).standard_normal((5, 5000)) + dc
    assert R.design(order, freqs, fs, ftype).shape[0] == {"lp1": 1, "lp2": 1, "lp16": 8, "bp8": 8, "hp4_dc1000": 2, "bp4_24414": 4}[name]
    seq, scan = _both(x, freqs, fs, order=order, filter_type=ftype)
    _judge(f"design_{name}", x, seq, scan, order, freqs, fs, ftype)
    assert np.array_equal(scan[:, :L], seq[:, :L])


def test_scan_sosfilt_doubles_the_block_length_past_65535_blocks():
    """one channel of 65 535 x 128 + 1 samples: one block too many at L = 128, so the route takes L = 256 and the matrices of
    that length.  Against scipy itself (the sequential kernel would walk 8.4 M samples one by one); the same bound."""
    from decode_tonal_langauge_amd.preprocess.signal import frequency_filter as ff
    assert R.has_long_double()
    T = 65535 * L + 1
    x = np.random.default_rng(77).standard_normal((1, T)).astype(np.float32)
    sos = R.design(4, [2.0, 60.0], 400.0, "bandpass")
    os.environ["TONAL_BUTTER"] = "scan"
    try:
        scan = ff.butter_filter(x, [2.0, 60.0], 400.0, causal=True)
        mats = [c[3] for c in ff._BUTTER_CACHE.values() if len(c) == 4 and isinstance(c[3], dict)]
    finally:
        os.environ.pop("TONAL_BUTTER", None)
    assert any(2 * L in m for m in mats)                     # the longer block's matrices, cached beside the first
    ref = sps.sosfilt(sos, x.astype(np.float64), axis=-1)
    scale = float(np.abs(ref).max())
    n = 16384
    yard = float(np.abs(R.sosfilt_loop(sos, x[:, :n], np.longdouble).astype(np.float64) - ref[:, :n]).max()) / scale
    dev = float(np.abs(scan - ref).max()) / scale
    bound = max(3.0 * _restated_ratio() * yard, 16 * EPS)
    print(f"1x{T}: scan vs scipy {dev:.3e}, scipy vs long double {yard:.3e}, bound {bound:.3e}")
    record("sosfilt_scan_long_blocks", {"scan vs scipy": dev, "scipy vs long double (prefix)": yard, "bound": bound})
    assert scan.shape == x.shape and dev <= bound, (dev, bound)


def test_scan_sosfilt_device_tensor_linearity_and_1d():
    from decode_tonal_langauge_amd.preprocess.signal import frequency_filter as ff
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(3)
    a = torch.randn(70, 16385, device=dev, generator=g, dtype=torch.float64)
    b = torch.randn(70, 16385, device=dev, generator=g, dtype=torch.float64)
    x1 = np.random.default_rng(5).standard_normal(1000)
    os.environ["TONAL_BUTTER"] = "scan"
    try:
        fa, fb = (ff.butter_filter(v, [2.0, 60.0], 400.0, causal=True) for v in (a, b))
        fab = ff.butter_filter(2.0 * a - 3.0 * b, [2.0, 60.0], 400.0, causal=True)
        y1 = ff.butter_filter(x1, [2.0, 60.0], 400.0, causal=True)
    finally:
        os.environ.pop("TONAL_BUTTER", None)
    assert isinstance(fab, torch.Tensor) and fab.is_cuda and fab.dtype == torch.float64 and fab.shape == a.shape
    scale = float(fab.abs().max())
    d = float((fab - (2.0 * fa - 3.0 * fb)).abs().max()) / scale
    record("sosfilt_scan_linearity", {"f(2a - 3b) vs 2 f(a) - 3 f(b)": d})
    assert d < 1e-9, d
    assert isinstance(y1, np.ndarray) and y1.shape == (1000,) and y1.dtype == np.float64
    sos = R.design(4, [2.0, 60.0], 400.0, "bandpass")
    assert np.abs(y1 - sps.sosfilt(sos, x1)).max() <= 1e-12 * np.abs(y1).max()


def test_scan_route_refuses_nine_sections_like_the_sequential_route():
    from decode_tonal_langauge_amd.preprocess.signal import frequency_filter as ff
    x = np.random.default_rng(2).standard_normal((2, 4000))
    with pytest.raises(RuntimeError, match=r"1\.\.8") as want:
        ff.butter_filter(x, [2.0, 60.0], 400.0, order=9, causal=True)
    os.environ["TONAL_BUTTER"] = "scan"
    try:
        with pytest.raises(RuntimeError, match=r"1\.\.8") as got:
            ff.butter_filter(x, [2.0, 60.0], 400.0, order=9, causal=True)
    finally:
        os.environ.pop("TONAL_BUTTER", None)
    assert str(got.value) == str(want.value)


def test_default_causal_route_is_the_sequential_entry_bit_for_bit():
    from decode_tonal_langauge_amd import _lib
    from decode_tonal_langauge_amd.preprocess.signal import frequency_filter as ff
    assert "TONAL_BUTTER" not in os.environ and "butter" not in os.environ.get("TONAL_KERNELS", "")
    dev = torch.device("cuda:0")
    x = torch.randn(65, 5001, device=dev, dtype=torch.float32, generator=torch.Generator(device=dev).manual_seed(9))
    out = ff.butter_filter(x, [2.0, 60.0], 400.0, causal=True)
    sos = torch.from_numpy(R.design(4, [2.0, 60.0], 400.0, "bandpass")).to(dev)
    y = torch.empty(65, 5001, dtype=torch.float64, device=dev)
    _lib.check(_lib.load().tl_sosfilt_f64(_lib.ptr(x), 0, _lib.ptr(sos), _lib.ptr(y), 65, 5001, 4, torch.cuda.current_stream().cuda_stream),
               "tl_sosfilt_f64")
    torch.cuda.synchronize()
    assert torch.equal(out, y)
