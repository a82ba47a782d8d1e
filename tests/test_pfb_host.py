"""CPU: the polyphase channelizer's restatement (tests/pfb_ref.py) pinned by properties -- the
reference holds no vectors for this stage -- and the host-only side of rfa_pfb_*: the length
rule, the argument checks that come before the device is looked for, and tools/pfb_host_check
(the same paths with the host code under ASan + UBSan)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import pfb_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS, SPACING, QRATE = 2_400_000, 25_000, 96_000      # the app case: 96 channels, decimation 25


@pytest.fixture(scope="module")
def lib():
    import rfanalyzer_amd
    rfanalyzer_amd.build()
    return rfanalyzer_amd.lib()


def _noise(n, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)


# ------------------------------------------------------------------ the restatement

@pytest.mark.parametrize("M,T,D", [(16, 61, 5), (60, 120, 60)])
def test_direct_and_folded_forms_agree(M, T, D):
    rng = np.random.default_rng(M + T)
    h = rng.uniform(-1, 1, T)
    x = _noise(6 * max(T, M) + 3, D)
    a = pfb_ref.direct(x, h, M, D)
    b = pfb_ref.folded(x, h, M, D)
    assert a.shape == b.shape == (M, len(x) // D)
    assert np.abs(a - b).max() <= 1e-12


def test_tone_lands_in_its_channel_with_the_prototype_gain(lib):
    """A tone at +k0 * Fs / M + delta is a tone at delta in channel k0 with the prototype's gain at
    delta, at least 55 dB down two channels away, and absent from channel M - k0 (the sign)."""
    from rfanalyzer_amd import demod
    h = demod.create_low_pass_taps(1, FS, 0.375 * SPACING, 0.25 * SPACING, 60).astype(np.float64)
    M, D, k0, delta = FS // SPACING, FS // QRATE, 7, 3000.0
    assert M == 96 and D == 25 and 10.5 * M < len(h) < 11.5 * M      # about 10.9 taps per channel
    j = np.arange(4 * len(h))
    x = np.exp(2j * np.pi * (k0 / M + delta / FS) * j)
    n0 = len(h) // D + 1                                                # windows past the zero prefix
    y = pfb_ref.folded(x, h, M, D, n0)
    i_n = (n0 + np.arange(y.shape[1])) * D + D - 1
    gain = (h * np.exp(-2j * np.pi * delta * np.arange(len(h)) / FS)).sum()
    assert abs(abs(gain) - 1.0) < 0.01                                   # 3 kHz is inside the pass band
    want = gain * np.exp(2j * np.pi * delta * i_n / FS)
    assert np.abs(y[k0] - want).max() < 1e-10
    level = lambda k: 20 * np.log10(np.abs(y[k % M]).max() / abs(gain))  # noqa: E731
    assert level(k0 + 2) <= -55 and level(k0 - 2) <= -55, (level(k0 + 2), level(k0 - 2))
    assert level(M - k0) <= -55, level(M - k0)
    assert np.abs(pfb_ref.direct(x, h, M, D, n0, n0 + 2) - y[:, :2]).max() < 1e-10


@pytest.mark.parametrize("form", [pfb_ref.direct, pfb_ref.folded])
def test_output_count_rule_over_random_splits(form):
    M, T, D = 16, 61, 5
    rng = np.random.default_rng(99)
    h = rng.uniform(-1, 1, T)
    x = _noise(403, 5)
    whole = form(x, h, M, D)
    for trial in range(5):
        s = pfb_ref.Stream(M, D, h, form)
        cuts = np.sort(rng.integers(0, len(x) + 1, 12))
        parts, c0 = [], 0
        for c1 in list(cuts) + [len(x)]:
            out = s.process(x[c0:c1])
            assert out.shape == (M, pfb_ref.output_count(c0, c1, D)) == (M, c1 // D - c0 // D)
            parts.append(out)
            c0 = c1
        np.testing.assert_array_equal(np.concatenate(parts, axis=1), whole)


def test_conversion_formulas():
    raw = np.array([0, 255, 128, 127], np.uint8)
    np.testing.assert_array_equal(pfb_ref.convert(raw, "s8"), [0 - 1j / 128, -1 + 127j / 128])
    u = lambda b: float((np.float32(b) - np.float32(127.4)) / np.float32(128))  # noqa: E731
    np.testing.assert_array_equal(pfb_ref.convert(raw, "u8"), [u(0) + 1j * u(255), u(128) + 1j * u(127)])
    s = np.array([-32768, 32767], "<i2")
    np.testing.assert_array_equal(pfb_ref.convert(s, "s16"), [-1 + 1j * (32767 / 32768)])
    f = np.array([0.1, -2.5], "<f4")
    np.testing.assert_array_equal(pfb_ref.convert(f, "f32"), [float(f[0]) + 1j * float(f[1])])


# ------------------------------------------------------------------ host side of the C-ABI

def _smooth(n):
    if n < 8 or n > 4096:
        return False
    for f in (2, 3, 5):
        while n % f == 0:
            n //= f
    return n == 1


def test_supported_is_the_2_3_5_rule(lib):
    bad = [n for n in range(1, 5001) if bool(lib.rfa_pfb_supported(n)) != _smooth(n)]
    assert not bad, bad[:10]
    assert all(lib.rfa_pfb_supported(n) for n in (96, 100, 400, 4096))


def _create(lib, fmt, M, D, taps, T=None):
    h = ctypes.c_void_p(1)
    taps = None if taps is None else np.ascontiguousarray(taps, np.float32)
    ptr = None if taps is None else taps.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    rc = lib.rfa_pfb_create(0, fmt, M, D, ptr, (0 if taps is None else taps.size) if T is None else T,
                            ctypes.byref(h))
    if rc == 0:
        lib.rfa_pfb_destroy(h)
    return rc, h.value


def test_argument_errors_come_before_the_device(lib):
    taps = np.ones(16 * 4096 + 1, np.float32)
    inv, uns = -1, -3
    assert lib.rfa_pfb_create(0, 0, 16, 4, taps.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), 16, None) == inv
    for args in [(-1, 16, 4, taps, 16), (4, 16, 4, taps, 16),           # format (4: planar floats)
                 (0, 0, 1, taps, 16), (0, -16, 1, taps, 16),            # channels
                 (0, 16, 0, taps, 16), (0, 16, -1, taps, 16), (0, 16, 17, taps, 16),   # decimation
                 (0, 16, 4, None, 16), (0, 16, 4, taps, 0), (0, 16, 4, taps, -5),
                 (0, 16, 4, taps, 257), (0, 4096, 64, taps, 16 * 4096 + 1),             # more than 16 phases
                 (0, 7, 0, taps, 8)]:                                                    # invalid before unsupported
        assert _create(lib, *args) == (inv, None), args
    for M in (1, 7, 14, 22, 4097, 8192):
        assert _create(lib, 1, M, 1, taps, 8) == (uns, None), M


def test_valid_request_without_a_device_is_nodevice(lib):
    import torch
    taps = np.ones(1047, np.float32)
    for fmt in range(4):
        rc, h = _create(lib, fmt, 96, 25, taps)
        if not torch.cuda.is_available():
            assert (rc, h) == (-4, None)                                # RFA_ERR_NODEVICE, *out NULL
        else:
            assert rc == 0


def test_for_raster_rejects_fractional_ratios(lib):
    from rfanalyzer_amd import demod
    with pytest.raises(ValueError):
        demod.Channelizer.for_raster("u8", FS, 25_001, QRATE)
    with pytest.raises(ValueError):
        demod.Channelizer.for_raster("u8", FS, SPACING, 95_000)
    with pytest.raises(ValueError):
        demod.Channelizer("u9", 96, 25, np.ones(8, np.float32))


def test_host_check_program_passes_under_sanitizers(lib):
    """tools/pfb_host_check: channelizer.hip's host side built with -fsanitize=address,undefined
    into a stand-alone program that walks the host-only entries and the error paths."""
    exe = os.path.join(ROOT, "tools", "pfb_host_check")
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tools"), exe], capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "pfb_host_check ok" in r.stdout
