"""Restatement of the tone meter and the tone squelch rule (rfanalyzer_amd/csrc/tone.hip,
demod.ToneRule) in numpy and plain Python, written from the design and not from the code: the phasor
index, the eight terms per sample, the quality, the guards and the rule, plus the signals of the
device tests.  The order of the additions is tests/slot_sum_plan.plan_sum's.

Audio at ``rate`` Hz, M = 10 * rate.  A probe is f10 tenths of a hertz (0: unused).  Sample i of a call
whose slot counter is ``base`` meets W[(f10 * (base + i)) mod M], W[p] = (cos, sin)(2 pi p / M).  Per
slot and call, in double with every product rounded once:
    [2j] Sc_j = sum a[i] * W.cos   [2j+1] Ss_j = sum a[i] * W.sin   (j = 0, 1, 2; +0.0 where unused)
    [6] P = sum a[i] * a[i]        [7] S1 = sum a[i]"""
import functools
import math

import numpy as np

import slot_sum_plan as plan

SUMS = 8
PROBES = 3
CTCSS = (67.0, 69.3, 71.9, 74.4, 77.0, 79.7, 82.5, 85.4, 88.5, 91.5, 94.8, 97.4, 100.0, 103.5, 107.2, 110.9, 114.8,
         118.8, 123.0, 127.3, 131.8, 136.5, 141.3, 146.2, 151.4, 156.7, 159.8, 162.2, 165.5, 167.9, 171.3, 173.8,
         177.3, 179.9, 183.5, 186.2, 189.9, 192.8, 196.6, 199.5, 203.5, 206.5, 210.7, 218.1, 225.7, 229.1, 233.6,
         241.8, 250.3, 254.1)


def modulus(rate: int) -> int:
    return 10 * int(rate)


def numpy_table(rate: int) -> np.ndarray:
    """W as [M, 2] from numpy: the angle is ((2 pi) * p) / M in double."""
    M = modulus(rate)
    th = (2.0 * np.pi * np.arange(M, dtype=np.float64)) / float(M)
    return np.stack([np.cos(th), np.sin(th)], axis=1)


@functools.lru_cache(maxsize=None)
def library_table(rate: int) -> np.ndarray:
    """W as [M, 2] through rfa_tone_phasor, the function that fills the device's table: its own values."""
    import ctypes

    import rfanalyzer_amd
    fn = rfanalyzer_amd.lib().rfa_tone_phasor
    M = modulus(rate)
    out = np.empty((M, 2), np.float64)
    c, s = ctypes.c_double(0), ctypes.c_double(0)
    rc, rs = ctypes.byref(c), ctypes.byref(s)
    for p in range(M):
        if fn(rate, p, rc, rs) != 0:
            raise RuntimeError(f"rfa_tone_phasor({rate}, {p}) failed")
        out[p, 0], out[p, 1] = c.value, s.value
    out.setflags(write=False)
    return out


def indices(f10: int, base: int, n: int, rate: int) -> np.ndarray:
    """p(i) for i = 0 ... n-1, in 64-bit integers (f10 < 5 * rate < 2^21, base + i < 2^37)."""
    return (np.int64(f10) * (np.int64(base) + np.arange(n, dtype=np.int64))) % np.int64(modulus(rate))


def terms(a, f10s, base: int, rate: int, table: np.ndarray):
    """The eight term arrays of one slot and call; None for the two of an unused probe."""
    a = np.asarray(a, np.float32).astype(np.float64)
    out = []
    with np.errstate(all="ignore"):
        for f10 in f10s:
            if f10 == 0:
                out += [None, None]
                continue
            w = table[indices(f10, base, a.size, rate)]
            out += [a * w[:, 0], a * w[:, 1]]
        out += [a * a, a.copy()]
    return out


def sums(a, f10s, base: int, rate: int, table: np.ndarray) -> np.ndarray:
    """The plan's eight sums of one slot and call."""
    return np.array([0.0 if t is None else plan.plan_sum(t) for t in terms(a, f10s, base, rate, table)])


def quality(sc: float, ss: float, p: float, s1: float, n: int) -> float:
    if not all(math.isfinite(v) for v in (sc, ss, p, s1)):
        return math.nan
    den = float(n) * p - s1 * s1
    if not den > 0.0:
        return 0.0
    return 2.0 * (sc * sc + ss * ss) / den


def guards(hz: float):
    for i in range(1, len(CTCSS) - 1):
        if abs(CTCSS[i] - hz) <= 0.05:
            return CTCSS[i - 1], CTCSS[i + 1]
    return round(hz * 0.965 * 10) / 10, round(hz * 1.035 * 10) / 10


class Rule:
    """The tone squelch rule, one slot at a time in plain Python."""

    def __init__(self, n_channels, rate, window_s=0.5, threshold=0.01, guard_ratio=4.0, hang=2, used=None):
        self.K, self.need = n_channels, window_s * rate
        self.threshold, self.guard_ratio, self.hang = threshold, guard_ratio, hang
        self.used = [[True] * PROBES for _ in range(n_channels)] if used is None else [list(u) for u in used]
        self.acc = [[0.0] * SUMS for _ in range(n_channels)]
        self.n = [0] * n_channels
        self.gate = [False] * n_channels
        self.misses = [0] * n_channels
        self.q = [math.nan] * n_channels

    def update(self, sums_, n, active=None):
        for k in range(self.K):
            if not self.used[k][0]:
                continue
            if (active is not None and not active[k]) or n[k] == 0:
                self.acc[k], self.n[k], self.gate[k], self.misses[k], self.q[k] = [0.0] * SUMS, 0, False, 0, math.nan
                continue
            self.acc[k] = [float(x) + float(sums_[c][k]) for c, x in enumerate(self.acc[k])]
            self.n[k] += int(n[k])
            if self.n[k] < self.need:
                continue
            a, cnt = self.acc[k], self.n[k]
            self.acc[k], self.n[k] = [0.0] * SUMS, 0
            q = self.q[k] = quality(a[0], a[1], a[6], a[7], cnt)
            power = [a[2 * j] * a[2 * j] + a[2 * j + 1] * a[2 * j + 1] for j in range(PROBES)]
            hit = math.isfinite(q) and q > self.threshold and all(
                power[0] > self.guard_ratio * power[j] for j in (1, 2) if self.used[k][j])
            if hit:
                self.gate[k], self.misses[k] = True, 0
            else:
                self.misses[k] += 1
                if self.misses[k] >= self.hang:
                    self.gate[k] = False
        return [g or not u[0] for g, u in zip(self.gate, self.used)]


# ------------------------------------------------------------------ signals of the device tests

def voice(rng, n: int, fs: float, rms: float, lo: float = 300.0, hi: float = 3000.0) -> np.ndarray:
    """Band-limited Gaussian noise of the given RMS: the stand-in for speech."""
    spec = np.fft.rfft(rng.standard_normal(n))
    f = np.fft.rfftfreq(n, 1.0 / fs)
    spec[(f < lo) | (f > hi)] = 0.0
    x = np.fft.irfft(spec, n)
    return x * (rms / np.sqrt(np.mean(x * x)))


def fm(deviation_hz: np.ndarray, fs: float, amplitude: float = 0.5) -> np.ndarray:
    """Complex baseband FM of an instantaneous-deviation track in Hz."""
    return amplitude * np.exp(2j * np.pi * np.cumsum(deviation_hz) / fs)


def four_signals(n: int, fs: float, seed: int = 77):
    """The four slots of the chain tests as complex baseband at ``fs``: a 100.0 Hz tone (600 Hz deviation)
    under voice (RMS 1500 Hz deviation), a 103.5 Hz tone under voice, voice alone, noise alone."""
    rng = np.random.Generator(np.random.PCG64(seed))
    t = np.arange(n) / fs
    out = [fm(600.0 * np.sin(2 * np.pi * 100.0 * t + 0.7) + voice(rng, n, fs, 1500.0), fs),
           fm(600.0 * np.sin(2 * np.pi * 103.5 * t + 1.9) + voice(rng, n, fs, 1500.0), fs),
           fm(voice(rng, n, fs, 1500.0), fs),
           0.2 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))]
    return out
