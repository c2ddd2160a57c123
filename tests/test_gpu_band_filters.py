"""GPU: the band extraction - ``hilbert_filter`` and ``fir_bandpass_filter`` - on every kernel form and bank, against plain
CPU references: the float64 oracle of the Gaussian Hilbert bank (``oracle.signal_oracle.hilbert_filter``, pinned to G6 / G15
and, by tests/test_oracle_golden.py, to 1e-12 of its ``np.longdouble`` statement in tests/signal_refs.py) and
``scipy.signal.lfilter`` per band for the FIR bank.

Which kernel runs is decided on the host from the band count, the kernels' half-width, the recording length and the
band-limited check.  Every case therefore also asserts WHICH entry point of the library ran (``spy``): the table ``ROWS`` is
written down here, not derived from the module, so a change of dispatch cannot move a case onto a kernel that another case
covers already.

Bounds (the project's): 1e-9 of max |y| for float64 recordings and for float32 recordings on the default fp64-math path
(against the float64 statement of the same float32 samples); 1e-5 for ``hilbert_f32=1`` and for float32 FIR output.  Each test
collects every miss before it fails and records its worst observed deviations with ``tests.parity_record``."""
from argparse import Namespace

import numpy as np
import pytest
import torch

from oracle import signal_oracle as sg
from tests.parity_record import record
from tests.signal_refs import band_cases, hilbert_filter_longdouble, scipy_fir_bank

pytestmark = pytest.mark.gpu

BAND_ENTRIES = ("tl_gauss_envelope", "tl_gauss_envelope_sym", "tl_hilbert_ols", "tl_hilbert_ols_bl", "tl_hilbert_fft",
                "tl_fir_bank", "tl_fir_bank_ols")
BL, OLS, SYM, FFT = "tl_hilbert_ols_bl", "tl_hilbert_ols", "tl_gauss_envelope_sym", "tl_hilbert_fft"
TAPS8, GEN = "tl_gauss_envelope[8]", "tl_gauss_envelope[generic]"
HG = [70., 150.]
LENGTHS = (300, 1000, 1023, 1024, 1025, 5003, 7169, 7170, 24000)


def _by_length(*steps):
    """{T: entry} from (first length, entry) steps in rising order."""
    return {T: [e for t0, e in steps if T >= t0][-1] for T in LENGTHS}


# (rate, range) -> (band count, {T: the entry point ``auto`` must reach}).  Overlap-save needs T >= 1024 and a half-width of
# at most 256; a kernel that does not decay inside the recording is used whole (``ntap == T``) in the time domain up to 7169
# taps (the LDS window), in the DFT domain beyond; banks of other than 8 bands take the generic time-domain kernel.
ROWS = {
    (400, (70., 150.)): (8, _by_length((0, SYM), (1024, BL))),                       # half 104, segments of 816
    (500, (70., 150.)): (8, _by_length((0, SYM), (1024, BL))),                       # half 130, segments of 764
    (512, (70., 150.)): (8, _by_length((0, SYM), (1024, BL))),                       # half 133, segments of 758
    (1000, (70., 150.)): (8, _by_length((0, TAPS8), (1000, SYM))),                   # half 260 > 256: no overlap-save
    (2000, (70., 150.)): (8, _by_length((0, TAPS8), (5003, SYM))),                   # half 520: whole up to T = 1041
    (400, (30., 70.)): (9, _by_length((0, GEN))),                                    # half 162
    (400, (100., 150.)): (4, _by_length((0, GEN))),                                  # half 85
    (1000, (150., 300.)): (7, _by_length((0, GEN))),                                 # half 174
    (400, (70., 170.)): (9, _by_length((0, GEN), (7170, FFT))),                      # Gaussians cut by Nyquist: no decay
    (400, (70., 199.)): (11, _by_length((0, GEN), (7170, FFT))),
    (400, (4., 8.)): (7, _by_length((0, GEN), (7170, FFT))),
    (400, (8., 13.)): (5, _by_length((0, GEN), (7170, FFT))),
    (400, (13., 30.)): (8, _by_length((0, TAPS8), (7170, FFT))),
    (400, (1., 4.)): (14, _by_length((0, GEN), (7170, FFT))),
}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch.device("cuda:0")


class _Spy:
    """The loaded library with every call of a band entry point noted (name; the 8-band and the generic time-domain kernels
    behind ``tl_gauss_envelope`` told apart by its band-count argument)."""

    def __init__(self, lib):
        self._lib = lib
        self.calls = []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name not in BAND_ENTRIES:
            return fn

        def noted(*args):
            self.calls.append(f"{name}[{'8' if args[6] == 8 else 'generic'}]" if name == "tl_gauss_envelope" else name)
            return fn(*args)
        return noted

    def take(self):
        out, self.calls = sorted(set(self.calls)), []
        return out


@pytest.fixture
def spy(monkeypatch, dev):
    from decode_tonal_langauge_amd import _lib
    s = _Spy(_lib.load())
    monkeypatch.setattr(_lib, "load", lambda: s)
    monkeypatch.delenv("TONAL_KERNELS", raising=False)
    for k in ("TONAL_HILBERT", "TONAL_HILBERT_F32"):
        monkeypatch.delenv(k, raising=False)
    return s


def rel(a, b):
    a = np.asarray(a, dtype=np.longdouble)
    b = np.asarray(b, dtype=np.longdouble)
    return float(np.max(np.abs(a - b)) / max(float(np.max(np.abs(b))), 1e-30))


def _ff():
    from decode_tonal_langauge_amd.preprocess.signal import frequency_filter as ff
    return ff


class _Tally:
    """Worst deviation per key, every miss of a bound or of an expected entry point; ``close`` records and asserts."""

    def __init__(self):
        self.obs, self.bad = {}, []

    def value(self, key, case, got, ref, bound):
        d = rel(got, ref) if np.all(np.isfinite(np.asarray(got, dtype=np.float64))) else float("inf")
        self.obs[key] = max(self.obs.get(key, 0.0), d)
        if not d < bound:
            self.bad.append((key, case, d, bound))
        return d

    def expect(self, case, got, want):
        if got != want:
            self.bad.append((case, "ran", got, "expected", want))

    def close(self, section):
        record(section, self.obs)
        print(section, {k: f"{v:.2e}" for k, v in sorted(self.obs.items())})
        assert not self.bad, f"{len(self.bad)} misses: {self.bad[:40]}"


def _hilbert_both(ff, x, fs, fr, env, dev):
    """NumPy in / NumPy out and resident tensor in / resident tensor out; the two must agree bit for bit."""
    out = ff.hilbert_filter(x, fs, freq_ranges=fr, envelope=env)
    assert isinstance(out, np.ndarray) and out.dtype == np.float64 and out.shape == x.shape
    res = ff.hilbert_filter(torch.from_numpy(x).to(dev), fs, freq_ranges=fr, envelope=env)
    assert isinstance(res, torch.Tensor) and res.is_cuda and res.dtype == torch.float64
    assert np.array_equal(out, res.cpu().numpy(), equal_nan=True)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# 1. every decision of hilbert = auto
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fs,fr", list(ROWS), ids=[f"{fs}Hz-{int(a)}-{int(b)}" for fs, (a, b) in ROWS])
def test_hilbert_auto_reaches_each_kernel_and_matches_oracle(dev, spy, fs, fr):
    """One row of the decision table at the lengths that cross the overlap-save threshold (1024), the whole-kernel limit
    ``ntap == T``, the LDS window (7169 / 7170) and the 1024-sample tile edge; envelope and real part, NumPy and resident
    input, a silent channel (exactly 0) and one that starts constant."""
    ff = _ff()
    nb, by_len = ROWS[(fs, fr)]
    assert len(sg.gaussian_bank(list(fr), fs)[0]) == nb
    tal = _Tally()
    for T in LENGTHS:
        x = band_cases(np.random.default_rng(1000 + T), 3, T, scale=30.0)
        for env in (True, False):
            ref = sg.hilbert_filter(x, fs, list(fr), envelope=env)
            out = _hilbert_both(ff, x, fs, list(fr), env, dev)
            tal.expect((T, env), spy.take(), [by_len[T]])
            tal.value(f"{by_len[T]} {'env' if env else 'real'}", (T, env), out, ref, 1e-9)
            if out[-1].any():
                tal.bad.append(("silent channel not 0", T, env))
    tal.close(f"band_filters_auto.{fs}Hz {int(fr[0])}-{int(fr[1])}")


FULL = [((400, (70., 150.)), "auto", BL), ((400, (70., 150.)), "ols_full", OLS), ((400, (70., 150.)), "taps", TAPS8),
        ((400, (70., 150.)), "sym", SYM), ((400, (70., 150.)), "fft", FFT), ((1000, (70., 150.)), "auto", SYM),
        ((400, (30., 70.)), "auto", GEN), ((400, (1., 4.)), "auto", FFT)]


def test_hilbert_recording_size_every_form(dev, spy, monkeypatch):
    """256 channels x 24 000 samples (float32, as the pipeline holds them) once per kernel form, values against the float64
    oracle of the same samples."""
    ff = _ff()
    x = band_cases(np.random.default_rng(24), 256, 24000, scale=30.0).astype(np.float32)
    xd = torch.from_numpy(x).to(dev)
    tal, refs = _Tally(), {}
    for (fs, fr), mode, entry in FULL:
        if (fs, fr) not in refs:
            refs = {(fs, fr): sg.hilbert_filter(x.astype(np.float64), fs, list(fr))}      # (one at a time: 49 MB each)
        monkeypatch.setenv("TONAL_HILBERT", mode)
        out = ff.hilbert_filter(xd, fs, freq_ranges=list(fr)).cpu().numpy()
        tal.expect((fs, fr, mode), spy.take(), [entry])
        tal.value(f"{entry} {fs}Hz {mode}", (fs, fr), out, refs[(fs, fr)], 1e-9)
    tal.close("band_filters_full_size")


# ---------------------------------------------------------------------------------------------------------------------
# 2. forced forms on the 8-band banks
# ---------------------------------------------------------------------------------------------------------------------

EIGHT = [(400, HG), (500, HG), (512, HG), (1000, HG), (2000, HG), (400, [13., 30.])]


def _forced_entry(fs, fr, T, mode):
    """What a forced form reaches: ``ols`` / ``ols_full`` / ``sym`` fall through to the next form the bank allows."""
    if mode == "fft":
        return FFT
    auto = ROWS[(fs, tuple(fr))][1][T]
    if auto == FFT:
        return FFT if mode in ("ols", "ols_full") else None           # taps / sym refuse
    if mode == "taps" or auto == TAPS8:
        return TAPS8
    if mode == "sym" or auto == SYM:
        return SYM
    return BL if mode == "ols" else OLS


def test_hilbert_forced_forms_match_oracle(dev, spy, monkeypatch):
    ff = _ff()
    tal = _Tally()
    for fs, fr in EIGHT:
        for T in (1000, 5003, 7170):
            x = band_cases(np.random.default_rng(T + fs), 3, T, scale=2.0)
            refs = {env: sg.hilbert_filter(x, fs, fr, envelope=env) for env in (True, False)}
            for mode in ("ols", "ols_full", "sym", "taps", "fft"):
                monkeypatch.setenv("TONAL_HILBERT", mode)
                want = _forced_entry(fs, fr, T, mode)
                if want is None:
                    with pytest.raises(ValueError, match=rf"need {T} taps .* supports up to 7169 .*hilbert={mode} forbids"):
                        ff.hilbert_filter(x, fs, freq_ranges=fr)
                    assert spy.take() == []
                    continue
                for env in (True, False):
                    out = _hilbert_both(ff, x, fs, fr, env, dev)
                    tal.expect((fs, fr, T, mode, env), spy.take(), [want])
                    tal.value(f"{mode}->{want}", (fs, fr, T, env), out, refs[env], 1e-9)
    tal.close("band_filters_forced")


# ---------------------------------------------------------------------------------------------------------------------
# 3. overlap-save geometry at other segment lengths
# ---------------------------------------------------------------------------------------------------------------------

def test_hilbert_overlap_save_geometry_at_other_half_widths(dev, spy, monkeypatch):
    """500 Hz (half 130, segments of 764) and 512 Hz (half 133, segments of 758): the last segment holds 1 sample, ``half``
    samples, exactly a full segment, one more than a full one; and T = 1024, where one window wraps the whole recording."""
    ff = _ff()
    tal = _Tally()
    for fs, half in ((500, 130), (512, 133)):
        cfs, sds = sg.gaussian_bank(HG, fs)
        seg = 1024 - 2 * half
        for T in (1024, 2 * seg + 1, 2 * seg + half, 3 * seg, 3 * seg + 1):
            assert ff.analytic_taps(T, fs, cfs, sds)[1] == half
            x64 = band_cases(np.random.default_rng(T), 3, T)
            for dt in (np.float64, np.float32):
                x = x64.astype(dt)
                for env in (True, False):
                    ref = sg.hilbert_filter(x.astype(np.float64), fs, HG, envelope=env)
                    for mode, want in (("ols", BL), ("ols_full", OLS)):
                        monkeypatch.setenv("TONAL_HILBERT", mode)
                        out = _hilbert_both(ff, x, fs, HG, env, dev)
                        tal.expect((fs, T, mode), spy.take(), [want])
                        tal.value(f"{want} {np.dtype(dt).name}", (fs, T, env), out, ref, 1e-9)
    tal.close("band_filters_ols_geometry")


# ---------------------------------------------------------------------------------------------------------------------
# 4. / 5. DC offset, scale and float32 recordings on every form
# ---------------------------------------------------------------------------------------------------------------------

FORMS = [(400, HG, 2449, "auto", BL), (400, HG, 2449, "ols_full", OLS), (400, HG, 2449, "sym", SYM),
         (400, HG, 2449, "taps", TAPS8), (400, HG, 2449, "fft", FFT), (400, HG, 1000, "auto", SYM),
         (512, HG, 1517, "auto", BL), (1000, HG, 2449, "auto", SYM), (2000, HG, 1024, "auto", TAPS8),
         (400, [30., 70.], 2449, "auto", GEN), (400, [100., 150.], 1025, "auto", GEN), (400, [1., 4.], 2449, "auto", GEN),
         (400, [70., 199.], 1500, "auto", GEN), (400, [1., 4.], 7170, "auto", FFT)]
OFFSETS = (0.0, 1e3, 1e5)


def test_hilbert_dc_offset_and_scale_on_every_form(dev, spy, monkeypatch):
    """x = (offset + noise) * 40 with offset in {0, 1e3, 1e5} standard deviations - raw ECoG carries one; the reference
    zeroes H[0] exactly, the time-domain and overlap-save forms convolve TRUNCATED kernels whose taps do not sum to 0
    exactly, and the band-limited form drops spectrum bins.  One channel starts with a constant stretch, one is silent.

    Reference: the np.longdouble statement (tests/signal_refs.py), since at an offset the float64 oracle's own rounding
    grows with it - measured on the CPU over nine (rate, range, T) cases of the table: 7.6e-16 at offset 0, 6.7e-13 at 1e3,
    6.8e-12 at 1e4, 6.1e-11 at 1e5 and 6.1e-10 at 1e6 standard deviations.  1e6 leaves the 1e-10 that a 1e-9 bound can
    afford its reference, so the largest offset is 1e5.  The bound stays 1e-9 of max |y|."""
    ff = _ff()
    tal = _Tally()
    for fs, fr, T, mode, want in FORMS:
        monkeypatch.setenv("TONAL_HILBERT", mode)
        for off in OFFSETS:
            x = band_cases(np.random.default_rng(int(T + off) % 9973), 4, T, offset=off, scale=40.0)
            for env in (True, False):
                ref = hilbert_filter_longdouble(x, fs, fr, envelope=env)
                out = _hilbert_both(ff, x, fs, fr, env, dev)
                tal.expect((fs, fr, T, mode), spy.take(), [want])
                tal.value(f"{want} {mode} offset {off:g}", (fs, fr, T, env), out, ref, 1e-9)
                if out[-1].any():
                    tal.bad.append(("silent channel not 0", fs, fr, T, mode, off, env))
    tal.close("band_filters_dc_offset")


def test_hilbert_float32_recordings_on_every_form(dev, spy, monkeypatch):
    """float32 in, float64 out; the default path does fp64 math on the float32 samples: 1e-9 of the float64 oracle of the
    same samples.  ``hilbert_f32=1`` (fp32 transforms in the band-limited overlap-save form): 1e-5, zero-mean input."""
    ff = _ff()
    tal = _Tally()
    for fs, fr, T, mode, want in FORMS:
        monkeypatch.setenv("TONAL_HILBERT", mode)
        x = band_cases(np.random.default_rng(T + 32), 4, T, scale=40.0).astype(np.float32)
        for env in (True, False):
            ref = sg.hilbert_filter(x.astype(np.float64), fs, fr, envelope=env)
            out = _hilbert_both(ff, x, fs, fr, env, dev)
            tal.expect((fs, fr, T, mode), spy.take(), [want])
            tal.value(f"{want} {mode}", (fs, fr, T, env), out, ref, 1e-9)
            if want == BL:
                monkeypatch.setenv("TONAL_HILBERT_F32", "1")
                out32 = _hilbert_both(ff, x, fs, fr, env, dev)
                monkeypatch.delenv("TONAL_HILBERT_F32")
                tal.expect((fs, fr, T, "hilbert_f32"), spy.take(), [BL])
                tal.value(f"{want} hilbert_f32=1", (fs, fr, T, env), out32, ref, 1e-5)
                assert not np.array_equal(out, out32)                    # (the switch really selects other arithmetic)
    tal.close("band_filters_float32")


# ---------------------------------------------------------------------------------------------------------------------
# 6. argument normalisation
# ---------------------------------------------------------------------------------------------------------------------

def test_hilbert_argument_edges(dev, spy):
    ff = _ff()
    tal = _Tally()
    x = band_cases(np.random.default_rng(6), 3, 2000)
    ref = sg.hilbert_filter(x, 400, HG)
    tal.value("tuple", None, ff.hilbert_filter(x, 400, freq_ranges=(70., 150.)), ref, 1e-9)
    tal.expect("tuple", spy.take(), [BL])
    two = [(70., 110.), (100., 150.)]                                    # overlapping ranges: 5 + 4 bands
    assert len(sg.gaussian_bank(two, 400)[0]) == 9
    tal.value("two ranges", None, ff.hilbert_filter(x, 400, freq_ranges=two), sg.hilbert_filter(x, 400, two), 1e-9)
    tal.expect("two ranges", spy.take(), [GEN])
    x1 = x[:1]
    tal.value("C=1", None, _hilbert_both(ff, x1, 400, HG, True, dev), ref[:1], 1e-9)
    tal.expect("C=1", spy.take(), [BL])
    # an empty bank: the reference's mean over no bands is NaN, float64, whatever the input
    empty = [(150., 70.)]
    assert len(sg.gaussian_bank(empty, 400)[0]) == 0
    for inp in (x, x.astype(np.float32), torch.from_numpy(x).to(dev)):
        out = ff.hilbert_filter(inp, 400, freq_ranges=empty)
        assert type(out) is type(inp) and tuple(out.shape) == (3, 2000)
        out = out.cpu().numpy() if isinstance(out, torch.Tensor) else out
        assert out.dtype == np.float64 and np.isnan(out).all()
    assert spy.take() == []
    # more rows than the kernels' grids take: refused on the host, nothing launched
    for T in (300, 1024):
        big = torch.zeros(65536, T, dtype=torch.float32, device=dev)
        with pytest.raises(ValueError, match="65535"):
            ff.hilbert_filter(big, 400, freq_ranges=HG)
        with pytest.raises(ValueError, match="65535"):
            ff.fir_bandpass_filter(big, 400, 64, [100.])
        assert spy.take() == []
    tal.close("band_filters_arguments")


# ---------------------------------------------------------------------------------------------------------------------
# instantiations that only the C ABI reaches: run-time band counts of the overlap-save kernels, float64 -> float32 FIR
# ---------------------------------------------------------------------------------------------------------------------

def _ols_operands(ff, dev, T, fs, fr):
    cfs, sds = ff.gaussian_bank(fr, fs)
    taps, half = ff.analytic_taps(T, fs, cfs, sds)
    nb = len(cfs)
    assert taps.shape == (nb, 2 * half + 1) and 0 < half <= 256
    g = np.zeros((nb, 1024), dtype=np.complex128)
    g[:, :2 * half + 1] = taps
    G = np.fft.fft(g, axis=1) / 1024
    Gd = torch.from_numpy(np.ascontiguousarray(np.stack([G.real, G.imag], axis=-1))).to(dev)
    bl = ff._band_limited(G, dev)
    assert bl is not None, "the Gaussian bank must fit the band-limited windows"
    return nb, half, Gd, bl, ff._ols_twiddles(dev)


def test_overlap_save_kernels_with_other_band_counts_through_the_c_abi(dev, spy):
    """``ols_bank_kernel<., double, 0>`` in Hilbert mode and ``ols_bank_bl_kernel<., 0, .>``: the host builds overlap-save
    operands for 8 bands only, so banks of 4 bands ([100, 150] at 400 Hz, half 85) and 7 ([150, 300] at 1 kHz, half 174)
    are launched directly, operands from the module's own helpers; all three ``x_is_f64`` modes of the band-limited form."""
    ff = _ff()
    from decode_tonal_langauge_amd._lib import ptr
    st = torch.cuda.current_stream().cuda_stream
    tal = _Tally()
    for fs, fr, nb_, half_ in ((400, [100., 150.], 4, 85), (1000, [150., 300.], 7, 174)):
        for T in (1024, 2449, 24000):
            nb, half, Gd, (Gp, k0), tw = _ols_operands(ff, dev, T, fs, fr)
            assert (nb, half) == (nb_, half_)
            x64 = band_cases(np.random.default_rng(T + nb), 5, T, scale=3.0)
            for dt in (np.float64, np.float32):
                x = x64.astype(dt)
                xd = torch.from_numpy(x).to(dev)
                is64 = int(dt == np.float64)
                for env in (1, 0):
                    ref = sg.hilbert_filter(x.astype(np.float64), fs, fr, envelope=bool(env))
                    y = torch.full((5, T), float("nan"), dtype=torch.float64, device=dev)
                    rc = spy.tl_hilbert_ols(ptr(xd), is64, ptr(Gd), ptr(tw), ptr(y), 5, T, nb, half, 1024, env, st)
                    assert rc == 0, spy.tl_last_error()
                    tal.value(f"tl_hilbert_ols nb{nb} {np.dtype(dt).name}", (T, env), y.cpu().numpy(), ref, 1e-9)
                    for mode_x, bound in ((1, 1e-9),) if is64 else ((2, 1e-9), (0, 1e-5)):
                        y = torch.full((5, T), float("nan"), dtype=torch.float64, device=dev)
                        rc = spy.tl_hilbert_ols_bl(ptr(xd), mode_x, ptr(Gp), ptr(k0), ptr(tw), ptr(y), 5, T, nb, half, 1024,
                                                   env, st)
                        assert rc == 0, spy.tl_last_error()
                        tal.value(f"tl_hilbert_ols_bl nb{nb} mode {mode_x}", (T, env), y.cpu().numpy(), ref, bound)
    assert spy.take() == [OLS, BL]
    # refusals: nothing is launched, the message names the limit
    nb, half, Gd, (Gp, k0), tw = _ols_operands(ff, dev, 1024, 400, [100., 150.])
    xd = torch.zeros(2, 1024, dtype=torch.float64, device=dev)
    y = torch.zeros(2, 1024, dtype=torch.float64, device=dev)
    for fn, lead in ((spy.tl_hilbert_ols, (ptr(Gd),)), (spy.tl_hilbert_ols_bl, (ptr(Gp), ptr(k0)))):
        assert fn(ptr(xd), 1, *lead, ptr(tw), ptr(y), 2, 1024, 65, half, 1024, 1, st) != 0
        assert b"1..64 bands" in spy.tl_last_error()
        assert fn(ptr(xd), 1, *lead, ptr(tw), ptr(y), 2, 1024, nb, 257, 1024, 1, st) != 0
        assert b"at most 513 taps" in spy.tl_last_error()
    assert spy.tl_hilbert_ols_bl(ptr(xd), 1, ptr(Gp), ptr(k0), ptr(tw), ptr(y), 2, 1023, nb, half, 1024, 1, st) != 0
    assert b"at least 1024 samples" in spy.tl_last_error()
    torch.cuda.synchronize()
    assert not y.any()
    tal.close("band_filters_c_abi_ols")


def test_fir_kernels_float64_in_float32_out_through_the_c_abi(dev, spy):
    """``fir_bank_kernel<double, float>`` and ``ols_bank_kernel<double, float, 0>``: the module's output dtype follows its
    input, so float64 samples with a float32 result exist only behind the C ABI."""
    from decode_tonal_langauge_amd._lib import ptr
    ff = _ff()
    st = torch.cuda.current_stream().cuda_stream
    tal = _Tally()
    for order, cfs in ((390, [100.]), (64, [60., 120., 35.])):
        taps = sg.fir_taps(400, order, cfs)
        nb, ntap = taps.shape
        g = np.zeros((nb, 1024))
        g[:, :ntap] = taps
        G = np.fft.fft(g, axis=1) / 1024
        Gd = torch.from_numpy(np.ascontiguousarray(np.stack([G.real, G.imag], axis=-1))).to(dev)
        td = torch.from_numpy(np.ascontiguousarray(taps)).to(dev)
        for T in (700, 1024, 5003):
            x = band_cases(np.random.default_rng(T), 3, T, offset=2.0, scale=5.0)
            xd = torch.from_numpy(x).to(dev)
            ref = scipy_fir_bank(x, taps)
            y = torch.full((3, T), float("nan"), dtype=torch.float32, device=dev)
            assert spy.tl_fir_bank(ptr(xd), 1, ptr(td), ptr(y), 0, 3, T, nb, ntap, st) == 0, spy.tl_last_error()
            tal.value("tl_fir_bank f64->f32", (order, T), y.cpu().numpy(), ref, 1e-5)
            y = torch.full((3, T), float("nan"), dtype=torch.float32, device=dev)
            assert spy.tl_fir_bank_ols(ptr(xd), 1, ptr(Gd), ptr(ff._ols_twiddles(dev)), ptr(y), 0, 3, T, nb, ntap,
                                       st) == 0, spy.tl_last_error()
            tal.value("tl_fir_bank_ols f64->f32", (order, T), y.cpu().numpy(), ref, 1e-5)
    assert spy.take() == ["tl_fir_bank", "tl_fir_bank_ols"]
    tal.close("band_filters_c_abi_fir")


# ---------------------------------------------------------------------------------------------------------------------
# FIR bank
# ---------------------------------------------------------------------------------------------------------------------

FIR_ORDERS = (2, 64, 390, 511, 512, 513, 514, 1000, 7168)
FIR_LENGTHS = (1, 63, 1023, 1024, 1025, 5003, 24000)
FIR_CFS = [100., 60., 120., 35., 150.]


def _fir_entry(order, T):
    """Overlap-save for recordings of at least one transform (1024) and up to 513 taps; the time-domain kernel otherwise."""
    return "tl_fir_bank_ols" if T >= 1024 and order <= 512 else "tl_fir_bank"


def _fir_both(ff, x, fs, order, cfs, dev):
    out = ff.fir_bandpass_filter(x, fs, order, cfs)
    assert isinstance(out, np.ndarray) and out.dtype == x.dtype and out.shape == x.shape
    res = ff.fir_bandpass_filter(torch.from_numpy(x).to(dev), fs, order, cfs)
    assert isinstance(res, torch.Tensor) and res.is_cuda and res.dtype == torch.from_numpy(x).dtype
    assert np.array_equal(out, res.cpu().numpy())
    return out


@pytest.mark.parametrize("order", FIR_ORDERS)
def test_fir_bank_orders_lengths_and_band_counts_against_scipy(dev, spy, order):
    """512 is the last overlap-save order, 7168 the last the LDS window takes; lengths below, at and past one transform and
    the tile edge, shorter than the taps included; 1, 2 and 5 bands at 400 Hz and 1 kHz; float64 and float32; NumPy and
    resident input; zero-mean and on a DC level of 1000 standard deviations - a causal FIR with zero initial state starts
    with a transient of the offset's size, which puts the overlap-save form's first segment (zero history) to the test."""
    ff = _ff()
    tal = _Tally()
    for T in FIR_LENGTHS:
        for nb in (1, 2, 5):
            for fs in (400, 1000):
                cfs = FIR_CFS[:nb]
                taps = sg.fir_taps(fs, order, cfs)
                for off in (0.0, 1e3):
                    x64 = band_cases(np.random.default_rng(order + T + nb), 2, T, offset=off, scale=7.0)
                    ref = scipy_fir_bank(x64, taps)
                    out = _fir_both(ff, x64, fs, order, cfs, dev)
                    tal.expect((T, nb, fs), spy.take(), [_fir_entry(order, T)])
                    tal.value(f"{_fir_entry(order, T)} float64 offset {off:g}", (T, nb, fs), out, ref, 1e-9)
                    x32 = x64.astype(np.float32)
                    out = _fir_both(ff, x32, fs, order, cfs, dev)
                    tal.expect((T, nb, fs, "float32"), spy.take(), [_fir_entry(order, T)])
                    tal.value(f"{_fir_entry(order, T)} float32 offset {off:g}", (T, nb, fs), out,
                              scipy_fir_bank(x32.astype(np.float64), taps), 1e-5)
    tal.close(f"band_filters_fir.order {order}")


def test_fir_bank_recording_size_squeeze_and_refusal(dev, spy):
    ff = _ff()
    tal = _Tally()
    x = band_cases(np.random.default_rng(77), 256, 24000, offset=0.5, scale=30.0)
    for order, cfs in ((390, [100.]), (1000, [60., 120.])):
        taps = sg.fir_taps(400, order, cfs)
        ref = scipy_fir_bank(x, taps)
        tal.value(f"{_fir_entry(order, 24000)} 256x24000 float64", order, _fir_both(ff, x, 400, order, cfs, dev), ref, 1e-9)
        tal.expect(order, spy.take(), [_fir_entry(order, 24000)])
        x32 = x.astype(np.float32)
        tal.value(f"{_fir_entry(order, 24000)} 256x24000 float32", order, _fir_both(ff, x32, 400, order, cfs, dev),
                  scipy_fir_bank(x32.astype(np.float64), taps), 1e-5)
        tal.expect((order, "float32"), spy.take(), [_fir_entry(order, 24000)])
    for T in (700, 3000):                                                # 1-D input: a 1-D result
        v = x[3, :T].copy()
        out = ff.fir_bandpass_filter(v, 400, 64, [60., 120.])
        assert out.shape == (T,) and out.dtype == np.float64
        tal.value("1-D", T, out, scipy_fir_bank(v[None], sg.fir_taps(400, 64, [60., 120.]))[0], 1e-9)
        tal.expect(T, spy.take(), [_fir_entry(64, T)])
    with pytest.raises(ValueError, match="order 7169 exceeds the kernel limit 7168"):
        ff.fir_bandpass_filter(x[:2, :3000], 400, 7169, [100.])
    assert spy.take() == []
    tal.close("band_filters_fir.full_size")


# ---------------------------------------------------------------------------------------------------------------------
# the plugin entry on a resident tensor
# ---------------------------------------------------------------------------------------------------------------------

def test_run_on_a_resident_tensor_matches_the_oracle(dev, spy):
    ff = _ff()
    x = band_cases(np.random.default_rng(9), 3, 1500, offset=0.3, scale=20.0)
    bands = [{"method": "hilbert", "params": {"freq_ranges": [70., 150.], "envelope": True}},
             {"method": "butter", "params": {"freqs": [0.3, 100], "filter_type": "bandpass"}},
             {"method": "fir", "params": {"order": 390, "center_frequencies": [100.]}}]
    ref = sg.run(x, Namespace(signal_freq=400, bands=bands))
    out = ff.run(torch.from_numpy(x).to(dev), Namespace(signal_freq=400, bands=bands))
    assert isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float64 and tuple(out.shape) == (9, 1500)
    assert spy.take() == ["tl_fir_bank_ols", BL]
    tal = _Tally()
    for i, name in enumerate(("hilbert", "butter", "fir")):
        tal.value(name, None, out[3 * i:3 * i + 3].cpu().numpy(), ref[3 * i:3 * i + 3], 1e-9)
    tal.close("band_filters_run")
