"""CPU: the host-only side of the channelizer's fine tuning (include/rfa.h, rfa_pfb_set_tuning;
DESIGN.md §5.7j): the table index the kernel itself computes (rfa_pfb_tuning_index) against
Python integers, the table (rfa_pfb_tuning_table) against float64, the raster and offset
arithmetic of demod.Channelizer (nearest_channel, offsets_tuning, channels_design), and
tools/pfb_tune_host_check (the same entries with the host code under ASan + UBSan)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INV, SIZE = -1, -2
QS = [1, 2, 7, 96, 3840, 96_000, 1 << 20]
LIM = 1 << 53


@pytest.fixture(scope="module")
def lib():
    import rfanalyzer_amd
    rfanalyzer_amd.build()
    return rfanalyzer_amd.lib()


def _index(lib, q, m, n):
    i = ctypes.c_int32(-99)
    rc = lib.rfa_pfb_tuning_index(q, m, n, ctypes.byref(i))
    return rc, i.value


# ------------------------------------------------------------------ rfa_pfb_tuning_index

def test_tuning_index_equals_python_integers(lib):
    rng = np.random.default_rng(20)
    bad = []
    for trial in range(10_000):
        q = QS[trial % len(QS)]
        m = int(rng.integers(-(q - 1), q))
        n = int(rng.integers(0, LIM)) >> int(rng.integers(0, 53))       # every magnitude up to 2^53 - 1
        if _index(lib, q, m, n) != (0, (n * m) % q):
            bad.append((q, m, n))
    assert not bad, bad[:5]
    for q in QS:
        for m in {0, q - 1, -(q - 1), (q - 1) // 2, -((q - 1) // 2)}:
            for n in (0, 1, q, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, LIM - 1):
                assert _index(lib, q, m, n) == (0, (n * m) % q), (q, m, n)


def test_tuning_index_argument_errors(lib):
    for q, m, n in [(0, 0, 1), (-1, 0, 1), ((1 << 20) + 1, 1, 1), (7, 7, 1), (7, -7, 1), (1, 1, 0), (96, 96, 5),
                    (96, -(1 << 31), 5), (7, 3, LIM), (7, 3, (1 << 64) - 1)]:
        assert _index(lib, q, m, n) == (INV, -99), (q, m, n)
    assert lib.rfa_pfb_tuning_index(7, 3, 5, None) == INV
    assert _index(lib, 1 << 20, (1 << 20) - 1, LIM - 1) == (0, ((LIM - 1) * ((1 << 20) - 1)) % (1 << 20))


# ------------------------------------------------------------------ rfa_pfb_tuning_table

def _table(lib, q, cap=None):
    cap = q if cap is None else cap
    c, s = np.full(max(cap, 1), 9, np.float32), np.full(max(cap, 1), 9, np.float32)
    fp = ctypes.POINTER(ctypes.c_float)
    return lib.rfa_pfb_tuning_table(q, c.ctypes.data_as(fp), s.ctypes.data_as(fp), cap), c, s


@pytest.mark.parametrize("q", QS)
def test_tuning_table_is_the_rounded_float64_circle(lib, q):
    rc, c, s = _table(lib, q)
    assert rc == 0
    ang = 2 * np.pi * np.arange(q) / q
    err = max(np.abs(c.astype(np.float64) - np.cos(ang)).max(), np.abs(s.astype(np.float64) - np.sin(ang)).max())
    print(f"tuning table q={q}: max |W - float64| = {err:.3e}")
    assert err <= 2.0 ** -23
    assert (c[0], s[0]) == (1.0, 0.0)
    if q % 4 == 0:
        assert (c[q // 4], s[q // 4]) == (0.0, 1.0)
        assert (c[q // 2], s[q // 2]) == (-1.0, 0.0)
        assert (c[3 * q // 4], s[3 * q // 4]) == (0.0, -1.0)
    if q > 1:
        rc, c2, s2 = _table(lib, q, q - 1)
        assert rc == SIZE and np.all(c2 == 9) and np.all(s2 == 9)


def test_tuning_table_argument_errors(lib):
    fp = ctypes.POINTER(ctypes.c_float)
    buf = np.zeros(4, np.float32)
    p = buf.ctypes.data_as(fp)
    for q in (0, -5, (1 << 20) + 1):
        assert lib.rfa_pfb_tuning_table(q, p, p, 4) == INV
    assert lib.rfa_pfb_tuning_table(4, None, p, 4) == INV
    assert lib.rfa_pfb_tuning_table(4, p, None, 4) == INV
    assert lib.rfa_pfb_tuning_table(4, p, p, 3) == SIZE
    assert lib.rfa_pfb_set_tuning(None, 7, None, 0) == INV
    assert lib.rfa_pfb_get_tuning(None, None, None, 0, None) == INV


# ------------------------------------------------------------------ Python helpers

def test_nearest_channel(lib):
    from rfanalyzer_amd.demod import Channelizer
    near = lambda f, cf: Channelizer.nearest_raster_channel(96, f, cf, 2_400_000)     # noqa: E731
    f0 = 100_000_000
    assert near(f0, f0) == (0, 0)
    assert near(f0, f0 + 7 * 25_000 + 5_000) == (7, 5_000)
    assert near(f0, f0 + 7 * 25_000 - 5_000) == (7, -5_000)
    assert near(f0, f0 + 7 * 25_000 + 12_499) == (7, 12_499)
    assert near(f0, f0 + 7 * 25_000 + 12_500) == (8, -12_500)            # the tie goes up: delta in [-s/2, s/2)
    assert near(f0, f0 + 7 * 25_000 - 12_500) == (7, -12_500)            # the edge, k one lower than + 12 500 gives
    assert near(f0, f0 - 3_000) == (0, -3_000)                           # negative offsets
    assert near(f0, f0 - 13_000) == (95, 12_000)                         # wrap to k >= M / 2
    assert near(f0, f0 - 25_000 * 10 - 1) == (86, -1)
    assert near(f0, f0 + 1_200_000) == (48, 0) and near(f0, f0 - 1_200_000) == (48, 0)   # +- Fs / 2: one channel
    assert near(f0, f0 + 1_199_999) == (48, -1)
    for bad in (f0 + 1_200_001, f0 - 1_200_001, f0 + 5_000_000):         # beyond Fs / 2
        with pytest.raises(ValueError):
            near(f0, bad)
    with pytest.raises(ValueError):
        Channelizer.nearest_raster_channel(7, f0, f0, 2_400_000)         # spacing not a whole number of Hz
    # an odd spacing: floor((offset + spacing / 2) / spacing) without a half
    assert Channelizer.nearest_raster_channel(8, 0, 62, 1000) == (0, 62)      # spacing 125: 62 < 62.5
    assert Channelizer.nearest_raster_channel(8, 0, 63, 1000) == (1, -62)
    assert Channelizer.nearest_raster_channel(8, 0, -63, 1000) == (7, 62)


def test_offsets_tuning(lib):
    from rfanalyzer_amd.demod import Channelizer
    ot = Channelizer.offsets_tuning
    assert ot([5000, -12_500, 1, 0], 96_000) == (96_000, [5000, -12_500, 1, 0])
    assert ot([5000], 96_000) == (96, [5])
    assert ot([5000, -12_500], 96_000) == (192, [10, -25])
    assert ot([0, 0], 96_000) == (1, [0, 0])
    assert ot([-47_999], 96_000) == (96_000, [-47_999])
    assert ot([3], 1 << 20) == (1 << 20, [3])
    for bad in [([1], (1 << 20) + 1), ([96_000], 96_000), ([-96_001], 96_000), ([0.5], 96_000), ([1], 0)]:
        with pytest.raises(ValueError):
            ot(*bad)


def test_for_channels_design(lib):
    from rfanalyzer_amd import demod
    cd = demod.Channelizer.channels_design
    (M, L, D), taps = cd(2_400_000, 25_000, 96_000, 22_500)
    assert (M, L, D) == (96, 1, 25)
    want = demod.create_low_pass_taps(1, 2_400_000, (22_500 + 48_000) / 2, 48_000 - 22_500, 60)
    np.testing.assert_array_equal(taps, want)
    assert taps.size < 0.4 * demod.create_low_pass_taps(1, 2_400_000, 0.375 * 25_000, 0.25 * 25_000, 60).size
    (M, L, D), taps = cd(2_048_000, 8_000, 96_000, 20_000, resample=True)
    assert (M, L, D) == (256, 3, 64)
    want = demod.create_low_pass_taps(3, 3 * 2_048_000, (20_000 + 48_000) / 2, 48_000 - 20_000, 60)
    np.testing.assert_array_equal(taps, want)
    assert abs(float(taps.astype(np.float64).sum()) - 3) < 0.03
    for bad in [(2_400_000, 25_000, 96_000, 48_000), (2_400_000, 25_000, 96_000, 50_000),     # fp >= fs
                (2_400_000, 25_000, 96_000, 0), (2_400_000, 25_000, 96_000, -1),
                (2_048_000, 8_000, 96_000, 20_000),                                             # needs resample
                (2_400_000, 25_001, 96_000, 20_000), (1_100_000, 100_000, 100_000, 20_000)]:    # a channelizer limit
        with pytest.raises(ValueError):
            cd(*bad)
        with pytest.raises(ValueError):
            demod.Channelizer.for_channels("u8", *bad)
    with pytest.raises(ValueError):
        cd(1_000_000, 12_500, 96_001, 20_000, resample=True)                                    # L above 64


# ------------------------------------------------------------------ the sanitizer build

def test_host_check_program_passes_under_sanitizers(lib):
    """tools/pfb_tune_host_check: channelizer.hip's host side built with
    -fsanitize=address,undefined into a stand-alone program that walks the host-only tuning
    entries, their argument errors and the null-handle answers."""
    exe = os.path.join(ROOT, "tools", "pfb_tune_host_check")
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tools"), exe], capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "pfb_tune_host_check ok" in r.stdout
