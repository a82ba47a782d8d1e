"""Scanner and squelch reductions of the newest waterfall row.

Host mirror of the reference's scanner helpers in ui/MainViewModel.kt (paths
relative to app/src/main/java/com/mantz_it/rfanalyzer/): the window arithmetic
and detection rules stay on the host in the reference's types (Long, Float,
Kotlin ``toInt()``), the reductions over the fft-shifted newest ring row run on
the device (``rfa_row_window_stats``) instead of on a JVM copy of the row.

* ``average_signal_level``   -- getAverageSignalLevel, MainViewModel.kt:1391-1413
* ``detect_signal``          -- detectSignal, MainViewModel.kt:1415-1457
* ``detect_signals_in_fft``  -- detectSignalsInFFT, MainViewModel.kt:1462-1540
* ``detect_iem_channels``    -- detectIEMChannelsInFFT, MainViewModel.kt:861-929
* ``detect_air_comm_signal`` / ``detect_air_comm_signal_at_frequency``
                             -- detectAirCommSignal(AtFrequency), MainViewModel.kt:1151-1250
* ``group_signals``          -- groupSignals / finalizeGroup, MainViewModel.kt:1552-1607 (host only)

Batch forms, for every frame of a ``process`` call instead of the newest row
(``rfa_set_windows``): ``watch_average_level`` / ``watch_scan`` /
``watch_iem_channels`` put the function's windows on the engine BEFORE the
caller's ``process``; ``average_signal_levels`` / ``detect_signals_in_batch`` /
``detect_iem_channels_in_batch`` read the [frames][windows] matrices after it
and apply the single-row rule frame by frame.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

F32 = np.float32
PEAK_ONLY, AVERAGE_ONLY, PEAK_OR_AVERAGE = "PEAK_ONLY", "AVERAGE_ONLY", "PEAK_OR_AVERAGE"  # ScanDetectionMode


def kotlin_float_to_int(x: np.float32) -> int:
    """Kotlin Float.toInt(): truncation toward zero, NaN -> 0, saturating."""
    if np.isnan(x):
        return 0
    if x >= 2 ** 31 - 1:
        return 2 ** 31 - 1
    if x <= -(2 ** 31):
        return -(2 ** 31)
    return int(x)


@dataclass
class DiscoveredSignal:
    frequency: int
    peak_strength: float
    average_strength: float
    bandwidth: int = 0         # Hz, 0: a single frequency (ScanDao.kt:70)
    is_grouped: bool = False   # built by group_signals from several detections (ScanDao.kt:71)


@dataclass
class IEMDetectedChannel:
    channel_frequency: int
    peak_strength: float
    average_strength: float


def _detected(mode: str, peak: np.float32, avg: np.float32, thr: np.float32) -> bool:
    if mode == PEAK_ONLY:
        return bool(peak > thr)
    if mode == AVERAGE_ONLY:
        return bool(avg > thr)
    return bool(peak > thr or avg > thr)


def effective_threshold(threshold: float, noise_floor: float, margin: float) -> np.float32:
    """maxOf(threshold, noiseFloor + noiseFloorMargin) in Float."""
    s = F32(F32(noise_floor) + F32(margin))
    t = F32(threshold)
    return t if t >= s else s


def bin_index(frequency: int, start_frequency: int, resolution: np.float32) -> int:
    """((f - startFrequency) / frequencyResolution).toInt(): Long / Float is a Float division."""
    return kotlin_float_to_int(F32(F32(frequency - start_frequency) / resolution))


def resolution(sample_rate: int, n: int) -> np.float32:
    return F32(F32(sample_rate) / F32(n))  # sampleRate.toFloat() / fftSize


def scan_windows(center: int, sample_rate: int, n: int, usable_bandwidth: int, step: int, scan_start: int,
                 scan_end: int):
    """detectSignalsInFFT's loop (MainViewModel.kt:1490-1512): frequencies and +-2-bin windows."""
    res = resolution(sample_rate, n)
    start_frequency = center - sample_rate // 2
    usable_start = (sample_rate - usable_bandwidth) // 2
    usable_end = usable_start + usable_bandwidth
    f = max(scan_start, start_frequency + usable_start)
    end = min(scan_end, start_frequency + usable_end)
    freqs, lo, hi = [], [], []
    while f <= end:
        b = bin_index(f, start_frequency, res)
        if 0 <= b < n:
            freqs.append(f)
            lo.append(max(0, b - 2))
            hi.append(min(n - 1, b + 2))
        f += step
    return freqs, np.array(lo, np.int32), np.array(hi, np.int32)


def iem_windows(center: int, sample_rate: int, n: int, channel_frequencies):
    """detectIEMChannelsInFFT windows (MainViewModel.kt:884-898): +-max(5, (100000/res).toInt()) bins."""
    res = resolution(sample_rate, n)
    start_frequency = center - sample_rate // 2
    half = max(5, kotlin_float_to_int(F32(F32(100000) / res)))
    freqs, lo, hi = [], [], []
    for cf in channel_frequencies:
        b = bin_index(cf, start_frequency, res)
        if 0 <= b < n:
            freqs.append(cf)
            lo.append(max(0, b - half))
            hi.append(min(n - 1, b + half))
    return freqs, np.array(lo, np.int32), np.array(hi, np.int32)


def average_signal_level(engine) -> float:
    """Mean dB of the newest row (MainViewModel.kt:1391-1413)."""
    _, av = engine.row_window_stats([0], [engine.n - 1])
    return float(av[0])


def detect_signal(engine, threshold: float, mode: str, noise_floor: float, margin: float):
    """(peak, avg) of the newest row if detected, else None (MainViewModel.kt:1415-1457)."""
    pk, av = engine.row_window_stats([0], [engine.n - 1])
    thr = effective_threshold(threshold, noise_floor, margin)
    return (float(pk[0]), float(av[0])) if _detected(mode, pk[0], av[0], thr) else None


def detect_signals_in_fft(engine, center: int, sample_rate: int, usable_bandwidth: int, step: int, threshold: float,
                          mode: str, noise_floor: float, margin: float, scan_start: int, scan_end: int):
    """MainViewModel.kt:1462-1540 with the window reductions on the device."""
    freqs, lo, hi = scan_windows(center, sample_rate, engine.n, usable_bandwidth, step, scan_start, scan_end)
    if not freqs:
        return []
    pk, av = engine.row_window_stats(lo, hi)
    thr = effective_threshold(threshold, noise_floor, margin)
    return [DiscoveredSignal(f, float(p), float(a)) for f, p, a in zip(freqs, pk, av) if _detected(mode, p, a, thr)]


def detect_iem_channels(engine, channel_frequencies, center: int, sample_rate: int, threshold: float):
    """MainViewModel.kt:861-929: a channel is detected when its window peak exceeds the threshold."""
    freqs, lo, hi = iem_windows(center, sample_rate, engine.n, channel_frequencies)
    if not freqs:
        return []
    pk, av = engine.row_window_stats(lo, hi)
    return [IEMDetectedChannel(f, float(p), float(a)) for f, p, a in zip(freqs, pk, av) if p > F32(threshold)]


# ---------------------------------------------------------------------------------------
# AirComm (MainViewModel.kt:1151-1250): the peak of a +-12.5 kHz window of the newest row.

def air_comm_half_window(sample_rate: int, n: int) -> int:
    """(12500 / frequencyResolution).toInt().coerceAtLeast(3): Int / Float is a Float division."""
    return max(3, kotlin_float_to_int(F32(F32(12500) / resolution(sample_rate, n))))


def air_comm_window(sample_rate: int, n: int):
    """detectAirCommSignal's window around the centre bin (MainViewModel.kt:1169-1179)."""
    half, center = air_comm_half_window(sample_rate, n), n // 2
    return max(0, center - half), min(n - 1, center + half)


def air_comm_window_at(target_frequency: int, batch_center: int, sample_rate: int, n: int):
    """detectAirCommSignalAtFrequency's window (MainViewModel.kt:1221-1237), None outside the row."""
    res = resolution(sample_rate, n)
    b = bin_index(target_frequency, batch_center - sample_rate // 2, res)
    if not 0 <= b < n:
        return None
    half = air_comm_half_window(sample_rate, n)
    return max(0, b - half), min(n - 1, b + half)


def detect_air_comm_signal(engine, sample_rate: int):
    """Peak dB of the centre window of the newest row (MainViewModel.kt:1151-1191)."""
    lo, hi = air_comm_window(sample_rate, engine.n)
    pk, _ = engine.row_window_stats([lo], [hi])
    return float(pk[0])


def detect_air_comm_signal_at_frequency(engine, target_frequency: int, batch_center: int, sample_rate: int):
    """Peak dB around target_frequency while tuned to batch_center, None when it lies outside the
    row (MainViewModel.kt:1203-1250)."""
    w = air_comm_window_at(target_frequency, batch_center, sample_rate, engine.n)
    if w is None:
        return None
    pk, _ = engine.row_window_stats([w[0]], [w[1]])
    return float(pk[0])


# ---------------------------------------------------------------------------------------
# groupSignals / finalizeGroup (MainViewModel.kt:1552-1607): host only.

def _finalize_group(group):
    if len(group) == 1:
        return group[0]
    lo, hi = min(s.frequency for s in group), max(s.frequency for s in group)
    total = lo + hi
    center = total // 2 if total >= 0 else -((-total) // 2)  # Long division truncates
    peak = F32(group[0].peak_strength)
    for s in group[1:]:  # maxOf on Float: NaN wins
        x = F32(s.peak_strength)
        peak = F32(np.nan) if np.isnan(x) or np.isnan(peak) else (x if x > peak else peak)
    acc = 0.0
    for s in group:  # Iterable<Float>.average(): double sum / count
        acc += float(F32(s.average_strength))
    return DiscoveredSignal(center, float(peak), float(F32(acc / len(group))), hi - lo, True)


def group_signals(signals, step_size: int, minimum_gap: int):
    """Neighbouring detections at most stepSize * minimumGap apart become one signal."""
    if not signals:
        return []
    srt = sorted(signals, key=lambda s: s.frequency)
    gap_threshold = step_size * minimum_gap
    out, cur = [], [srt[0]]
    for prev, sig in zip(srt, srt[1:]):
        if sig.frequency - prev.frequency <= gap_threshold:
            cur.append(sig)
        else:
            out.append(_finalize_group(cur))
            cur = [sig]
    out.append(_finalize_group(cur))
    return out


# ---------------------------------------------------------------------------------------
# Batch forms: every frame of the caller's process call (rfa_set_windows).

def watch_average_level(engine) -> None:
    """Before process: the whole row, for average_signal_levels."""
    engine.set_windows([0], [engine.n - 1])


def watch_scan(engine, center: int, sample_rate: int, usable_bandwidth: int, step: int, scan_start: int,
               scan_end: int) -> None:
    """Before process: detectSignalsInFFT's +-2-bin windows, for detect_signals_in_batch."""
    _, lo, hi = scan_windows(center, sample_rate, engine.n, usable_bandwidth, step, scan_start, scan_end)
    engine.set_windows(lo, hi)


def watch_iem_channels(engine, channel_frequencies, center: int, sample_rate: int) -> None:
    """Before process: detectIEMChannelsInFFT's windows, for detect_iem_channels_in_batch."""
    _, lo, hi = iem_windows(center, sample_rate, engine.n, channel_frequencies)
    engine.set_windows(lo, hi)


def _batch_stats(engine, lo, hi):
    cur = engine.windows()
    if cur is None or not (np.array_equal(cur[0], lo) and np.array_equal(cur[1], hi)):
        raise ValueError("the engine holds another window list: call the matching watch_* before process")
    return engine.window_stats()


def average_signal_levels(engine) -> np.ndarray:
    """average_signal_level of every frame of the last process call, float32 [frames]."""
    _, av = _batch_stats(engine, [0], [engine.n - 1])
    return av[:, 0].copy() if av.size else np.empty(0, np.float32)


def detect_signals_in_batch(engine, center: int, sample_rate: int, usable_bandwidth: int, step: int, threshold: float,
                            mode: str, noise_floor: float, margin: float, scan_start: int, scan_end: int):
    """detect_signals_in_fft for every frame of the last process call: a list per frame."""
    freqs, lo, hi = scan_windows(center, sample_rate, engine.n, usable_bandwidth, step, scan_start, scan_end)
    pk, av = _batch_stats(engine, lo, hi)
    thr = effective_threshold(threshold, noise_floor, margin)
    return [[DiscoveredSignal(f, float(p), float(a)) for f, p, a in zip(freqs, rp, ra) if _detected(mode, p, a, thr)]
            for rp, ra in zip(pk, av)]


def detect_iem_channels_in_batch(engine, channel_frequencies, center: int, sample_rate: int, threshold: float):
    """detect_iem_channels for every frame of the last process call: a list per frame."""
    freqs, lo, hi = iem_windows(center, sample_rate, engine.n, channel_frequencies)
    pk, av = _batch_stats(engine, lo, hi)
    return [[IEMDetectedChannel(f, float(p), float(a)) for f, p, a in zip(freqs, rp, ra) if p > F32(threshold)]
            for rp, ra in zip(pk, av)]
