"""CPU: the rational-rate channelizer's restatement (tests/pfb_rational_ref.py) pinned by
properties, and the host-only side of the new rfa_pfb_* entries: the count rule
(rfa_pfb_rational_outputs), the argument checks of rfa_pfb_create_rational that come before the
device is looked for, the raster arithmetic of Channelizer.for_raster_resampled, and
tools/pfb_rational_host_check (the same paths with the host code under ASan + UBSan).

20 Msps to 96 kHz is 3 / 625 in lowest terms (gcd(96000, 20000000) = 32000): the definition asks
gcd(L, D) = 1, so the raster is (M, L, D) = (800, 3, 625), and the unreduced (800, 6, 1250) is an
RFA_ERR_INVALID request."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import pfb_rational_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(16, 3, 7, 61), (20, 4, 9, 203), (16, 5, 64, 400)]           # (M, L, D, T)
INV, UNS, NODEV = -1, -3, -4


@pytest.fixture(scope="module")
def lib():
    import rfanalyzer_amd
    rfanalyzer_amd.build()
    return rfanalyzer_amd.lib()


def _noise(n, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)


# ------------------------------------------------------------------ the restatement

@pytest.mark.parametrize("M,L,D,T", SHAPES)
def test_direct_and_folded_forms_agree(M, L, D, T):
    g = np.random.default_rng(M + T).uniform(-1, 1, T)
    x = _noise(4 * max(-(-T // L), M, D) + 3, D)
    a = ref.direct(x, g, M, L, D)
    b = ref.folded(x, g, M, L, D)
    assert a.shape == b.shape == (M, -(-len(x) * L // D))
    assert np.abs(a - b).max() <= 1e-12


@pytest.mark.parametrize("M,L,D,T", SHAPES + [(60, 1, 7, 100)])
def test_channel_0_is_the_sequential_resampler(M, L, D, T):
    g = np.random.default_rng(L + T).uniform(-1, 1, T)
    x = _noise(3 * max(-(-T // L), D) + 5, T)
    seq = ref.sequential(x, g, L, D)
    assert seq.size == ref.count(len(x), L, D) == -(-len(x) * L // D)   # exactly ceil(c L / D) outputs
    assert np.abs(ref.direct(x, g, M, L, D)[0] - seq).max() <= 1e-12
    assert np.abs(ref.folded(x, g, M, L, D)[0] - seq).max() <= 1e-12
    for c in range(0, 40):                                               # the loop's own count, any length
        assert ref.sequential(x[:c], g, L, D).size == -(-c * L // D)


def test_l_equal_1_samples_at_n_d_not_at_the_integer_entry_s_index():
    """L = 1: m_n = n * D; the integer entry's i_n = n * D + D - 1 is the same filter D - 1 samples later."""
    import pfb_ref
    M, D, T = 16, 5, 61
    g = np.random.default_rng(3).uniform(-1, 1, T)
    x = _noise(200, 4)
    a = ref.folded(x, g, M, 1, D)
    assert a.shape == (M, 40)
    b = pfb_ref.folded(np.concatenate([np.zeros(D - 1), x]), g, M, D)   # delayed by D - 1: i_n - (D-1) = n * D
    rot = np.exp(2j * np.pi * np.arange(M) * (D - 1) / M)[:, None]       # the NCO runs on the delayed index
    assert np.abs(a - b[:, :40] * rot).max() <= 1e-12


@pytest.mark.parametrize("form", [ref.direct, ref.folded])
def test_output_count_rule_over_random_splits(form):
    M, L, D, T = 16, 3, 7, 61
    rng = np.random.default_rng(99)
    g = rng.uniform(-1, 1, T)
    x = _noise(403, 5)
    whole = form(x, g, M, L, D)
    assert whole.shape == (M, 173)                                       # ceil(403 * 3 / 7)
    for trial in range(5):
        s = ref.Stream(M, L, D, g, form)
        cuts = np.sort(rng.integers(0, len(x) + 1, 12))
        parts, c0 = [], 0
        for c1 in [int(c) for c in cuts] + [len(x)]:
            out = s.process(x[c0:c1])
            assert out.shape == (M, ref.output_count(c0, c1, L, D)) == (M, -(-c1 * L // D) - -(-c0 * L // D))
            parts.append(out)
            c0 = c1
        np.testing.assert_array_equal(np.concatenate(parts, axis=1), whole)


def _blackman_lowpass(L, fs, cutoff, transition):
    """A stand-in prototype in float64 (windowed sinc, Blackman, gain L at rate L * fs)."""
    rate = L * fs
    n = int(round(5.5 * rate / transition)) | 1
    k = np.arange(n) - (n - 1) / 2
    h = 2 * cutoff / rate * np.sinc(2 * cutoff / rate * k) * np.blackman(n)
    return L * h / h.sum()


@pytest.mark.parametrize("M,L,D,fs", [(80, 12, 125, 1_000_000), (32, 3, 64, 256_000)])
def test_tone_lands_in_its_channel_with_the_prototype_gain(M, L, D, fs):
    """A tone at k0 * Fs / M + delta comes out of channel k0 as G * exp(2 pi j delta (n D / L) / Fs),
    G = sum g[s] exp(-2 pi j delta s / (L Fs)) / L, to within the prototype's own image leakage
    sum_{i=1..L-1} |G(delta + i Fs)| plus 1e-9; channels k0 +- 2 and M - k0 are at least 55 dB down."""
    spacing = fs // M
    g = _blackman_lowpass(L, fs, 0.375 * spacing, 0.25 * spacing)
    k0, delta = 7, 0.12 * spacing
    s = np.arange(len(g))
    G = lambda f: (g * np.exp(-2j * np.pi * f * s / (L * fs))).sum() / L  # noqa: E731
    assert abs(abs(G(delta)) - 1.0) < 0.01                                # inside the pass band
    leak = sum(abs(G(delta + i * fs)) for i in range(1, L))
    Tp = -(-len(g) // L)
    j = np.arange(2 * Tp + 40 * D // L)
    x = np.exp(2j * np.pi * (k0 / M + delta / fs) * j)
    n0 = -(-Tp * L // D) + 1                                              # windows past the zero prefix
    y = ref.folded(x, g, M, L, D, n0)
    n = n0 + np.arange(y.shape[1])
    assert y.shape[1] >= 30
    want = G(delta) * np.exp(2j * np.pi * delta * (n * D / L) / fs)
    err = np.abs(y[k0] - want).max()
    print(f"tone M={M} L={L} D={D}: err {err:.3e}, image leakage {leak:.3e}")
    assert err <= leak + 1e-9, (err, leak)
    level = lambda k: 20 * np.log10(np.abs(y[k % M]).max() / abs(G(delta)))  # noqa: E731
    assert level(k0 + 2) <= -55 and level(k0 - 2) <= -55, (level(k0 + 2), level(k0 - 2))
    assert level(M - k0) <= -55, level(M - k0)
    assert np.abs(ref.direct(x, g, M, L, D, n0, n0 + 2) - y[:, :2]).max() < 1e-10


def test_phase_major_table():
    g = np.arange(1, 12, dtype=np.float64)                               # T = 11, L = 4: Tp = 3
    gp = ref.phases(g, 4)
    np.testing.assert_array_equal(gp, [[1, 5, 9], [2, 6, 10], [3, 7, 11], [4, 8, 0]])


# ------------------------------------------------------------------ host side of the C-ABI

def _outputs(lib, L, D, consumed, n):
    out = ctypes.c_size_t(12345)
    rc = lib.rfa_pfb_rational_outputs(L, D, consumed, n, ctypes.byref(out))
    return rc, out.value


def test_rational_outputs_is_the_count_rule(lib):
    rng = np.random.default_rng(7)
    for L, D in [(1, 1), (1, 7), (3, 7), (4, 9), (3, 64), (12, 125), (3, 625), (48, 125), (64, 65), (63, 64)]:
        assert _outputs(lib, L, D, 0, 0) == (0, 0)
        assert _outputs(lib, L, D, 0, 1) == (0, 1)                       # output 0 is due with sample 0
        c = 0
        for n in [int(v) for v in rng.integers(0, 3 * D + 2, 40)] + [1 << 24, (1 << 40) + 3]:
            assert _outputs(lib, L, D, c, n) == (0, -(-(c + n) * L // D) - -(-c * L // D)), (L, D, c, n)
            c += n
        for c in [(1 << 52) - 3, (1 << 52) + 12345, (1 << 53) - 2000]:   # consumed near 2^52 and below 2^53
            for n in (0, 1, D, 1999):
                assert _outputs(lib, L, D, c, n) == (0, -(-(c + n) * L // D) - -(-c * L // D)), (L, D, c, n)
    assert _outputs(lib, 64, 65, (1 << 53) - 2, 1)[0] == 0               # total 2^53 - 1: the last valid one
    assert _outputs(lib, 64, 65, (1 << 53) - 1, 1) == (INV, 12345)       # total 2^53
    assert _outputs(lib, 64, 65, 1 << 53, 0) == (INV, 12345)
    assert _outputs(lib, 3, 7, (1 << 64) - 1, 2) == (INV, 12345)         # no wrap-around
    for L, D in [(0, 7), (-3, 7), (7, 3), (2, 2), (4, 6), (6, 1250), (3, 0), (65, 66)]:
        assert _outputs(lib, L, D, 0, 10) == (INV, 12345), (L, D)
    assert lib.rfa_pfb_rational_outputs(3, 7, 0, 10, None) == INV


def _create(lib, fmt, M, L, D, taps, T=None):
    h = ctypes.c_void_p(1)
    taps = None if taps is None else np.ascontiguousarray(taps, np.float32)
    ptr = None if taps is None else taps.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    rc = lib.rfa_pfb_create_rational(0, fmt, M, L, D, ptr, (0 if taps is None else taps.size) if T is None else T,
                                     ctypes.byref(h))
    if rc == 0:
        lib.rfa_pfb_destroy(h)
    return rc, h.value


def test_argument_errors_come_before_the_device(lib):
    taps = np.ones(16 * 16 * 64 + 1, np.float32)
    assert lib.rfa_pfb_create_rational(0, 0, 16, 3, 7, taps.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), 61,
                                       None) == INV
    outside = [(-1, 16, 3, 7, taps, 61), (4, 16, 3, 7, taps, 61),        # format (4: planar floats)
               (0, 0, 3, 7, taps, 61), (0, -16, 3, 7, taps, 61),         # channels
               (0, 16, 0, 7, taps, 61), (0, 16, -1, 7, taps, 61),        # 1 <= L
               (0, 16, 65, 66, taps, 61),                                # L <= 64
               (0, 16, 8, 7, taps, 61), (0, 16, 3, 0, taps, 61),         # L <= D
               (0, 16, 3, 49, taps, 61), (0, 16, 1, 17, taps, 61),       # D <= L * M
               (0, 16, 3, 9, taps, 61), (0, 16, 4, 6, taps, 61), (0, 16, 2, 2, taps, 61),   # gcd
               (0, 800, 6, 1250, taps, 8000),                            # 20 Msps to 96 kHz, not reduced
               (0, 16, 3, 7, None, 61), (0, 16, 3, 7, taps, 0), (0, 16, 3, 7, taps, -5),
               (0, 16, 3, 7, taps, 16 * 16 * 3 + 1), (0, 16, 64, 65, taps, 16 * 16 * 64 + 1),   # more than 16 M L
               (0, 7, 3, 9, taps, 8)]                                    # invalid before unsupported
    for args in outside:
        assert _create(lib, *args) == (INV, None), args
    for M in (1, 7, 14, 22, 4097, 8192):
        assert _create(lib, 1, M, 1, 1, taps, 8) == (UNS, None), M
    import torch
    want = (0,) if torch.cuda.is_available() else (NODEV,)
    inside = [(0, 16, 1, 7, taps, 61), (0, 16, 64, 65, taps, 61), (0, 16, 7, 8, taps, 61), (0, 16, 1, 1, taps, 61),
              (0, 16, 3, 47, taps, 61), (0, 16, 1, 16, taps, 61), (0, 16, 3, 7, taps, 1),
              (0, 16, 3, 7, taps, 16 * 16 * 3), (0, 16, 64, 65, taps, 16 * 16 * 64),
              (1, 256, 3, 64, taps, 8000), (2, 80, 12, 125, taps, 10000), (3, 800, 3, 625, taps, 16000)]
    for args in inside:                                                  # each limit one step inside
        rc, h = _create(lib, *args)
        assert rc in want and (rc == 0 or h is None), (args, rc)


def test_for_raster_resampled_ratios(lib):
    from rfanalyzer_amd import demod
    rr = demod.Channelizer.raster_ratio
    assert rr(2_048_000, 8_000, 96_000) == (256, 3, 64)
    assert rr(1_000_000, 12_500, 96_000) == (80, 12, 125)
    assert rr(20_000_000, 25_000, 96_000) == (800, 3, 625)               # 6 / 1250 in lowest terms
    assert rr(10_000_000, 25_000, 96_000) == (400, 6, 625)
    assert rr(2_500_000, 12_500, 96_000) == (200, 24, 625)
    assert rr(2_400_000, 25_000, 96_000) == (96, 1, 25)
    assert rr(1_000_000, 12_500, 48_000) == (80, 6, 125)                 # CW's quadrature rate
    assert rr(2_500_000, 12_500, 48_000) == (200, 12, 625)
    for bad in [(2_048_000, 8_001, 96_000),                              # M not whole
                (1_000_000, 12_500, 1_000_001),                          # L > D
                (1_000_000, 12_500, 96_001),                             # L = 96001 > 64
                (1_000_000, 100_000, 50_000),                            # D = 20 > L * M = 10
                (1_100_000, 100_000, 100_000),                           # M = 11
                (0, 8_000, 96_000), (2_048_000, 0, 96_000), (2_048_000, 8_000, -1)]:
        with pytest.raises(ValueError):
            rr(*bad)
        with pytest.raises(ValueError):
            demod.Channelizer.for_raster_resampled("u8", *bad)
    with pytest.raises(ValueError):
        demod.Channelizer.rational("u9", 16, 3, 7, np.ones(8, np.float32))
    # the prototype: the for_raster design at the interpolated rate, gain L, about 10.9 * M * L taps
    for fs, sp in [(2_048_000, 8_000), (1_000_000, 12_500), (20_000_000, 25_000)]:
        M, L, D = rr(fs, sp, 96_000)
        g = demod.create_low_pass_taps(L, L * fs, 0.375 * sp, 0.25 * sp, 60)
        assert 10.5 * M * L < g.size < 11.5 * M * L and g.size <= 16 * M * L, (M, L, g.size)
        assert abs(float(g.astype(np.float64).sum()) - L) < 0.01 * L


def test_host_check_program_passes_under_sanitizers(lib):
    """tools/pfb_rational_host_check: channelizer.hip's host side built with
    -fsanitize=address,undefined into a stand-alone program that walks the new host-only entries
    and the error paths."""
    exe = os.path.join(ROOT, "tools", "pfb_rational_host_check")
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tools"), exe], capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "pfb_rational_host_check ok" in r.stdout
