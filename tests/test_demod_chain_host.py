"""CPU: the demodulator's host half -- band-pass design, the mode table, the
device-less error path -- and the sanity of the restated chain
(tests/demod_chain_ref.py) that the GPU tests compare against.  There are no
reference vectors for this stage, so the restatement is pinned by properties of
the signal it must produce."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import demod_chain_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
_fp = ctypes.POINTER(ctypes.c_float)


@pytest.fixture(scope="module")
def lib():
    import rfanalyzer_amd
    rfanalyzer_amd.build()
    return rfanalyzer_amd.lib()


def same_bits(a, b):
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


# (rate, low, high) of the USB, LSB and CW designs at their default widths, then at the limits
DESIGNS = [(96000, 200.0, 2800.0), (96000, -2800.0, -200.0), (48000, 750 - 300 / 2.0, 750 + 300 / 2.0),
           (96000, 200.0, 5000.0), (96000, -1500.0, -200.0), (48000, 750 - 151 / 2.0, 750 + 151 / 2.0),
           (48000, 350.0, 1150.0)]


@pytest.mark.parametrize("rate,lo,hi", DESIGNS)
def test_bandpass_taps_bit_identical_to_restatement(lib, rate, lo, hi):
    from rfanalyzer_amd import demod
    tw = float(F32(rate) * F32(0.01))
    got = demod.create_band_pass_taps(1.0, rate, lo, hi, tw, 40.0)
    want = ref.band_pass_taps(1.0, rate, lo, hi, tw, 40.0)
    assert got is not None and want is not None
    assert len(got[0]) == len(got[1]) == 181
    assert same_bits(got[0], want[0]) and same_bits(got[1], want[1])


@pytest.mark.parametrize("args", [(1, 96000, 200, 200, 960, 40), (1, 96000, 300, 200, 960, 40),
                                  (1, 96000, -48001, 200, 960, 40), (1, 96000, 200, 48001, 960, 40),
                                  (1, 96000, 200, 2800, 0, 40), (1, 96000, 200, 2800, -5, 40),
                                  (1, 0, 200, 2800, 960, 40)])
def test_bandpass_taps_rejects_what_the_reference_rejects(lib, args):
    from rfanalyzer_amd import demod
    assert ref.band_pass_taps(*args) is None
    assert demod.create_band_pass_taps(*map(float, args)) is None
    n = ctypes.c_int32(7)
    assert lib.rfa_bandpass_taps(*map(float, args), None, None, 0, ctypes.byref(n)) == -1 and n.value == 0


def test_bandpass_taps_capacity(lib):
    n = ctypes.c_int32(0)
    buf = np.full(181, 7.0, F32)
    rc = lib.rfa_bandpass_taps(1.0, 96000.0, 200.0, 2800.0, 960.0, 40.0, buf.ctypes.data_as(_fp), None, 180,
                               ctypes.byref(n))
    assert rc == -2 and n.value == 181 and np.all(buf == 7.0)


def test_mode_info_and_width_coercion(lib):
    from rfanalyzer_amd import demod
    for name, mode in demod.MODES.items():
        assert demod.mode_info(name) == ref.MODE_INFO[mode], name
    v = ctypes.c_int32(0)
    for bad in (-1, 7, 100):
        assert lib.rfa_demod_mode_info(bad, ctypes.byref(v), None, None, None) == -1
    # the restatement coerces per mode, as channelWidth's setter does
    for mode, (_, lo, hi, dflt) in ref.MODE_INFO.items():
        c = ref.DemodChain(mode)
        assert c.width == dflt
        c.set_width(10 ** 7)
        assert c.width == hi
        c.set_width(-5)
        assert c.width == lo


def test_create_without_device(lib):
    import torch
    h = ctypes.c_void_p(1)
    assert lib.rfa_demod_create(0, 9, ctypes.byref(h)) == -1 and not h.value      # bad mode, checked first
    h = ctypes.c_void_p(1)
    rc = lib.rfa_demod_create(0, ref.AM, ctypes.byref(h))
    if not torch.cuda.is_available():
        assert rc == -4 and not h.value                                           # RFA_ERR_NODEVICE, nothing leaked
        from rfanalyzer_amd import RfaError, demod
        with pytest.raises(RfaError):
            demod.Demodulator("am")
    elif rc == 0:
        assert lib.rfa_demod_destroy(h) == 0
    assert lib.rfa_demod_destroy(None) == -1
    n = ctypes.c_size_t(3)
    assert lib.rfa_demod_process(None, None, None, 0, 0, None, 0, ctypes.byref(n)) == -1


def test_filter_lengths_of_the_restatement():
    c = ref.DemodChain(ref.NFM)
    c.process(np.zeros(4, F32), np.zeros(4, F32))
    assert len(c.user.taps) == 27 and len(c.sink.f1.taps) == 9 and len(c.sink.f2.taps) == 13
    for mode in (ref.USB, ref.LSB, ref.CW):
        c = ref.DemodChain(mode)
        c.process(np.zeros(4, F32), np.zeros(4, F32))
        assert len(c.band.tr) == 181 and c.band.d == (1 if mode == ref.CW else 2)


@pytest.mark.parametrize("dec", [1, 2])
def test_complex_fir_closed_form_equals_the_literal_loop(dec):
    rng = np.random.Generator(np.random.PCG64(5))
    tr, ti = ref.band_pass_taps(1, 96000, 200, 2800, 960, 40)
    a, b = ref.ComplexFir(tr, ti, dec), ref.ComplexFir(tr, ti, dec)
    for n in (1, 0, 2, 181, 50, 7):
        re = (0.3 * rng.standard_normal(n)).astype(F32)
        im = (0.3 * rng.standard_normal(n)).astype(F32)
        got, want = a.filter(re, im), b.filter_literal(re, im)
        assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]), n


def test_first_packet_after_a_build_is_one_short():
    c = ref.DemodChain(ref.NFM, audio_sink=False)
    z = np.ones(100, F32)
    assert len(c.process(z, z)) == 99
    assert len(c.process(z, z)) == 100
    c.set_width(5000)
    assert len(c.process(z, z)) == 99


def test_nfm_of_a_tone_is_its_frequency_over_the_deviation():
    c = ref.DemodChain(ref.NFM, audio_sink=False)
    df, rate = 2000.0, 96000
    t = np.arange(4000)
    x = 0.5 * np.exp(2j * np.pi * df * t / rate)
    re, im = x.real.astype(F32), x.imag.astype(F32)
    want = df / (0.75 * c.width)
    # the discriminator alone: its first sample is measured against the zero carry-over, the rest is constant
    step = ref.DemodChain(ref.NFM)._fm(re, im, 0.75)
    assert np.max(np.abs(step[1:] - want)) < 2e-4 * want + 1e-5
    # the whole chain: the same once the 27-tap user filter has filled
    out = c.process(re, im)
    assert len(out) == len(re) - 1
    assert np.max(np.abs(out[27:] - want)) < 2e-4 * want + 1e-5


def test_am_recovers_the_modulating_tone():
    c = ref.DemodChain(ref.AM)
    rate = 96000
    t = np.arange(9600)
    tone = np.cos(2 * np.pi * 1000.0 * t / rate)
    x = 0.4 * (1 + 0.5 * tone) * np.exp(1j * 0.3)
    out = c.process(x.real.astype(F32), x.imag.astype(F32), packet_samples=2400)
    # audio at 48 kHz; compare against the tone at every delay of one period, skip the start-up
    out = out[200:].astype(np.float64)
    k = np.arange(len(out))
    best = max(abs(np.corrcoef(out, np.cos(2 * np.pi * 1000.0 * (k - d) / 48000))[0, 1]) for d in range(48))
    assert best > 0.99, best


def _tone_power_db(mode):
    c = ref.DemodChain(mode)
    rate = 96000
    t = np.arange(9600)
    x = 0.3 * np.exp(2j * np.pi * 1000.0 * t / rate)
    c.process(x.real.astype(F32), x.imag.astype(F32))
    # before the AGC's gain: pre_sink / gain; the gain is 0.75 / lastMax
    pre = c.pre_sink[400:].astype(np.float64) * float(c.last_max) / 0.75
    return 10 * np.log10(np.mean(pre ** 2) + 1e-30)


def test_usb_passes_and_lsb_rejects_an_upper_tone():
    usb, lsb = _tone_power_db(ref.USB), _tone_power_db(ref.LSB)
    assert usb > 10 * np.log10(0.3 ** 2 / 2) - 1.0       # the real part of a unit-gain pass band
    assert usb - lsb >= 30.0, (usb, lsb)                  # the design is 40 dB


def test_silent_first_am_packet_is_nan():
    c = ref.DemodChain(ref.AM, audio_sink=False)
    out = c.process(np.zeros(8, F32), np.zeros(8, F32))
    assert len(out) == 7 and np.all(np.isnan(out))


def test_host_check_program_passes_under_sanitizers(lib):
    """tools/demod_host_check: demod.hip's host side built with -fsanitize=address,undefined
    into a stand-alone program that walks the host-only entries and the error paths."""
    exe = os.path.join(ROOT, "tools", "demod_host_check")
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tools"), exe], capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "demod_host_check ok" in r.stdout
