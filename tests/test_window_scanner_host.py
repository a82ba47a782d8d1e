"""CPU: the scanner mirrors added with the batch window statistics -- the AirComm window
arithmetic and group_signals against the restatement in tests/scanner_ref.py and hand-checked
cases, the batch scanner functions over a fake engine that serves numpy rows, and the new
C-ABI entries declared on both sides."""
import math
import os
import re

import numpy as np
import pytest

import scanner_ref as ref
from oracle import scanner as osc
from rfanalyzer_amd import scanner as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F0, SR, N = 433_000_000, 2_400_000, 4096


class FakeEngine:
    """Duck-typed SpectrumEngine: rows come from numpy, reductions from the restatement."""

    def __init__(self, n):
        self.n = n
        self._win = None
        self._rows = np.empty((0, n), np.float32)

    def set_windows(self, lo, hi):
        lo, hi = np.asarray(lo, np.int32), np.asarray(hi, np.int32)
        self._win = (lo, hi) if lo.size else None

    def windows(self):
        return self._win

    def process(self, rows):
        self._rows = np.asarray(rows, np.float32)

    def window_stats(self):
        if self._win is None:
            return np.empty((0, 0), np.float32), np.empty((0, 0), np.float32)
        st = [osc.window_stats(r, *self._win) for r in self._rows]
        return np.array([s[0] for s in st], np.float32), np.array([s[1] for s in st], np.float32)

    def row_window_stats(self, lo, hi):
        return osc.window_stats(self._rows[-1], lo, hi)


def _rows(frames, n, seed):
    rng = np.random.default_rng(seed)
    rows = (-80 + 5 * rng.standard_normal((frames, n))).astype(np.float32)
    for f in range(frames):
        rows[f, (300 + 411 * f) % n] = -20.0 - f  # a carrier that moves from frame to frame
        rows[f, 2048 + 171 * (f % 3)] = -30.0
    return rows


# ---------------------------------------------------------------- AirComm windows
def test_air_comm_windows_hand_checked():
    # 2.4 MHz / 4096 = 585.9375 Hz per bin; 12500 / 585.9375 = 21.33 -> 21
    assert sc.air_comm_half_window(SR, N) == 21
    assert sc.air_comm_window(SR, N) == (2027, 2069)
    # 2.4 MHz / 64 = 37.5 kHz per bin: 0.33 -> 0, at least 3
    assert sc.air_comm_half_window(SR, 64) == 3 and sc.air_comm_window(SR, 64) == (29, 35)
    # the row starts at 431.8 MHz; 1.7 MHz / 585.9375 = 2901.33 -> bin 2901
    assert sc.air_comm_window_at(433_500_000, F0, SR, N) == (2880, 2922)
    assert sc.air_comm_window_at(431_800_000, F0, SR, N) == (0, 21)           # bin 0, clamped
    assert sc.air_comm_window_at(431_800_000 - 500, F0, SR, N) == (0, 21)     # -0.85 truncates to bin 0
    assert sc.air_comm_window_at(431_800_000 - 586, F0, SR, N) is None        # bin -1
    assert sc.air_comm_window_at(434_199_999, F0, SR, N) == (4074, 4095)      # bin 4095, clamped
    assert sc.air_comm_window_at(434_200_000, F0, SR, N) is None              # bin 4096: outside
    assert sc.air_comm_window_at(500_000_000, F0, SR, N) is None


@pytest.mark.parametrize("n", [64, 1024, 4096, 65536, 1048576])
@pytest.mark.parametrize("sr", [250_000, 2_400_000, 20_000_000, 61_440_000])
def test_air_comm_windows_match_the_restatement(n, sr):
    assert sc.air_comm_window(sr, n) == ref.air_comm_window(sr, n)
    rng = np.random.default_rng(n + sr)
    for t in [F0 - sr // 2, F0 + sr // 2 - 1, F0 + sr // 2, F0] + list(rng.integers(F0 - sr, F0 + sr, 200)):
        assert sc.air_comm_window_at(int(t), F0, sr, n) == ref.air_comm_window_at(int(t), F0, sr, n), t


def test_air_comm_detection_over_a_fake_engine():
    e = FakeEngine(N)
    rows = _rows(3, N, 4)
    rows[2, 2050] = np.nan  # NaN wins the peak
    e.process(rows[:2])
    assert sc.detect_air_comm_signal(e, SR) == ref.air_comm_peak(rows[1], ref.air_comm_window(SR, N))
    for t in (433_500_000, 431_800_000, 434_199_999):
        assert sc.detect_air_comm_signal_at_frequency(e, t, F0, SR) == \
            ref.air_comm_peak(rows[1], ref.air_comm_window_at(t, F0, SR, N))
    assert sc.detect_air_comm_signal_at_frequency(e, 500_000_000, F0, SR) is None
    e.process(rows)
    assert math.isnan(sc.detect_air_comm_signal(e, SR))


# ---------------------------------------------------------------- group_signals
S = sc.DiscoveredSignal


def _as_ref(signals):
    return [ref.Signal(s.frequency, s.peak_strength, s.average_strength, s.bandwidth, s.is_grouped) for s in signals]


def test_group_signals_hand_checked():
    assert sc.group_signals([], 12_500, 2) == []
    one = S(100_000_000, -40.0, -50.0)
    assert sc.group_signals([one], 12_500, 2) == [one]  # a single signal is returned as it is
    # a gap of exactly stepSize * minimumGap still groups; one hertz more does not
    a, b, c = S(100_000_000, -40.0, -50.0), S(100_025_000, -35.5, -52.0), S(100_050_001, -60.0, -61.0)
    got = sc.group_signals([a, b, c], 12_500, 2)
    assert got == [S(100_012_500, -35.5, -51.0, 25_000, True), c]
    # unsorted input is sorted by frequency first
    assert sc.group_signals([c, b, a], 12_500, 2) == got
    # odd sums: Long division truncates; the averages are summed in double and rounded once
    got = sc.group_signals([S(7, -1.0, 0.1), S(10, -2.0, 0.2), S(12, -3.0, 0.4)], 1, 3)
    assert got == [S(9, -1.0, float(np.float32((float(np.float32(0.1)) + float(np.float32(0.2)) +
                                                 float(np.float32(0.4))) / 3)), 5, True)]
    # NaN wins the peak
    got = sc.group_signals([S(1, float("nan"), 0.0), S(2, -3.0, 0.0)], 1, 1)
    assert len(got) == 1 and math.isnan(got[0].peak_strength)


def test_group_signals_match_the_restatement():
    rng = np.random.default_rng(8)
    for trial in range(50):
        k = int(rng.integers(1, 40))
        freqs = rng.choice(np.arange(0, 400) * 12_500 + 88_000_000, size=k, replace=False)
        sig = [S(int(f), float(np.float32(rng.normal(-50, 10))), float(np.float32(rng.normal(-60, 10)))) for f in freqs]
        gap = int(rng.integers(0, 5))
        got, exp = _as_ref(sc.group_signals(sig, 12_500, gap)), ref.group_signals(_as_ref(sig), 12_500, gap)
        assert got == exp, (trial, gap)


# ---------------------------------------------------------------- batch forms
def test_batch_functions_equal_the_single_row_ones_frame_by_frame():
    rows = _rows(5, N, 1)
    scan = (F0, SR, 2_000_000, 12_500, -45.0, sc.PEAK_OR_AVERAGE, -90.0, 6.0, 0, 10 ** 12)
    chans = [F0 + k * 100_000 for k in range(-14, 15)]
    batch, one = FakeEngine(N), FakeEngine(N)
    single = {"level": [], "scan": [], "iem": []}
    for f in range(len(rows)):
        one.process(rows[f:f + 1])
        single["level"].append(sc.average_signal_level(one))
        single["scan"].append(sc.detect_signals_in_fft(one, *scan))
        single["iem"].append(sc.detect_iem_channels(one, chans, F0, SR, -45.0))
    assert any(single["scan"]) and any(single["iem"])
    assert len({tuple(s.frequency for s in fr) for fr in single["scan"]}) > 1  # the frames differ
    sc.watch_average_level(batch)
    batch.process(rows)
    assert sc.average_signal_levels(batch).tolist() == single["level"]
    sc.watch_scan(batch, F0, SR, 2_000_000, 12_500, 0, 10 ** 12)
    batch.process(rows)
    assert sc.detect_signals_in_batch(batch, *scan) == single["scan"]
    sc.watch_iem_channels(batch, chans, F0, SR)
    batch.process(rows)
    assert sc.detect_iem_channels_in_batch(batch, chans, F0, SR, -45.0) == single["iem"]


def test_batch_functions_need_their_own_window_list():
    e = FakeEngine(N)
    with pytest.raises(ValueError):
        sc.average_signal_levels(e)  # no list at all
    sc.watch_average_level(e)
    e.process(_rows(2, N, 2))
    with pytest.raises(ValueError):
        sc.detect_signals_in_batch(e, F0, SR, 2_000_000, 12_500, -45.0, sc.PEAK_ONLY, -90.0, 6.0, 0, 10 ** 12)
    assert sc.average_signal_levels(e).shape == (2,)


# ---------------------------------------------------------------- declarations
NEW = ("rfa_set_windows", "rfa_get_window_stats", "rfa_get_window_stats_device", "rfa_ring_window_stats")


def test_new_entries_declared_in_header_and_bindings():
    header = open(os.path.join(ROOT, "include", "rfa.h")).read()
    bindings = open(os.path.join(ROOT, "rfanalyzer_amd", "_lib.py")).read()
    for name in NEW:
        assert re.search(r"RFA_API int %s\(" % name, header), name
        assert '"%s"' % name in bindings, name
    from rfanalyzer_amd import SpectrumEngine
    for method in ("set_windows", "window_stats", "window_stats_device", "ring_window_stats"):
        assert callable(getattr(SpectrumEngine, method))
