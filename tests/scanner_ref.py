"""TEST INFRASTRUCTURE ONLY -- restatement of the reference's remaining row-window consumers,
written from the Kotlin semantics of ui/MainViewModel.kt (app/src/main/java/com/mantz_it/rfanalyzer/):

* detectAirCommSignal (:1151-1191) and detectAirCommSignalAtFrequency (:1203-1250): the peak
  (FloatArray.maxOrNull) of the window +-max(3, (12500 / frequencyResolution).toInt()) bins
  around the centre bin / around ((targetFreq - startFrequency) / frequencyResolution).toInt(),
  clamped to the row; null when that bin is outside the row.
* groupSignals / finalizeGroup (:1552-1607).

Kotlin types are kept: sampleRate.toFloat() / fftSize is a Float, Int / Float and Long / Float
are Float divisions, Float.toInt() truncates toward zero (NaN -> 0, saturating), Long / 2
truncates toward zero, maxOf on Floats is Math.max (NaN wins), Iterable<Float>.average() is a
double sum divided by the count.
"""
from __future__ import annotations

import math
import struct
from typing import NamedTuple, Optional


def f32(x: float) -> float:
    """Round a Python float to the nearest Float, kept as a Python float."""
    return struct.unpack("f", struct.pack("f", x))[0]


def float_to_int(x: float) -> int:
    if math.isnan(x):
        return 0
    return max(-(2 ** 31), min(2 ** 31 - 1, math.trunc(x)))


def half_window(sample_rate: int, fft_size: int) -> int:
    resolution = f32(f32(float(sample_rate)) / float(fft_size))
    return max(3, float_to_int(f32(12500.0 / resolution)))


def air_comm_window(sample_rate: int, fft_size: int):
    half, center = half_window(sample_rate, fft_size), fft_size // 2
    return max(center - half, 0), min(center + half, fft_size - 1)


def air_comm_window_at(target: int, batch_center: int, sample_rate: int, fft_size: int):
    resolution = f32(f32(float(sample_rate)) / float(fft_size))
    start = batch_center - sample_rate // 2
    b = float_to_int(f32(f32(float(target - start)) / resolution))
    if b < 0 or b >= fft_size:
        return None
    half = half_window(sample_rate, fft_size)
    return max(b - half, 0), min(b + half, fft_size - 1)


def air_comm_peak(row, window) -> Optional[float]:
    if window is None:
        return None
    m = float(row[window[0]])
    for x in row[window[0] + 1:window[1] + 1]:
        x = float(x)
        m = math.nan if math.isnan(x) or math.isnan(m) else max(m, x)
    return m


class Signal(NamedTuple):
    frequency: int
    peak: float
    average: float
    bandwidth: int = 0
    grouped: bool = False


def group_signals(signals, step_size: int, minimum_gap: int):
    if not signals:
        return []
    ordered = sorted(signals, key=lambda s: s.frequency)
    groups, threshold = [[ordered[0]]], step_size * minimum_gap
    for i in range(1, len(ordered)):
        if ordered[i].frequency - ordered[i - 1].frequency <= threshold:
            groups[-1].append(ordered[i])
        else:
            groups.append([ordered[i]])
    out = []
    for g in groups:
        if len(g) == 1:
            out.append(g[0])
            continue
        lo, hi = g[0].frequency, g[-1].frequency  # sorted: the group's min and max
        peak = g[0].peak
        for s in g[1:]:
            peak = math.nan if math.isnan(peak) or math.isnan(s.peak) else max(peak, s.peak)
        total = 0.0
        for s in g:
            total += f32(s.average)
        center = abs(lo + hi) // 2 * (1 if lo + hi >= 0 else -1)  # Long / 2 truncates toward zero
        out.append(Signal(center, peak, f32(total / len(g)), hi - lo, True))
    return out
