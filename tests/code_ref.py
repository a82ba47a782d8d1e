"""Restatement of the code meter and the DCS code squelch rule (rfanalyzer_amd/csrc/code.hip,
demod.CodeRule) in numpy and plain Python, written from the design and not from the code: the word, the
sub-cell index, the quantised sample, the sub-cell sums, the carry between calls and the rule, plus the
signals of the device tests.

Audio at ``rate`` Hz, P = 8 sub-cells to the 134.4 bit/s bit.  Sample g of a slot's stream, counted from
its last break, belongs to sub-cell s(g) = floor(672 P g / (5 rate)); it contributes q(a) = rint(a * 2^24)
(ties to even) or, where a is not finite or |a| >= 2^15, 0 and one to the call's bad count.  All int64:
nothing here has a tolerance."""
import math

import numpy as np

P = 8
BITS = 23
NUM = 672 * P
GENERATOR = 0xC75
CODES = tuple(int(c, 8) for c in (
    "023 025 026 031 032 036 043 047 051 053 054 065 071 072 073 074 114 115 116 122 125 131 132 134 143 145 152 "
    "155 156 162 165 172 174 205 212 223 225 226 243 244 245 246 251 252 255 261 263 265 266 271 274 306 311 315 "
    "325 331 332 343 346 351 356 364 365 371 411 412 413 423 431 432 445 446 452 454 455 462 464 465 466 503 506 "
    "516 523 526 532 546 565 606 612 624 627 631 632 654 662 664 703 712 723 731 732 734 743 754").split())


# ------------------------------------------------------------------ the word

def gf2_remainder(value: int, generator: int) -> int:
    """value modulo generator, both polynomials over GF(2) as bit masks."""
    top = generator.bit_length()
    while value.bit_length() >= top:
        value ^= generator << (value.bit_length() - top)
    return value


def word(code: int, generator: int = GENERATOR) -> int:
    d = 0x800 | code
    return d | gf2_remainder(d << 11, generator) << 12


def rotations(w: int) -> set:
    return {((w >> r) | (w << (BITS - r))) & 0x7FFFFF for r in range(BITS)}


# ------------------------------------------------------------------ the sums

def subcell(g, rate: int):
    """s(g); Python integers or int64 arrays (672 P g < 2^61 for g <= 2^48)."""
    return NUM * g // (5 * rate)


def quantise(a):
    """(q int64, bad bool) of float32 samples."""
    a = np.asarray(a, np.float32)
    bad = ~(np.abs(a) < np.float32(32768.0))                 # NaN compares false: bad
    with np.errstate(all="ignore"):
        q = np.rint(np.where(bad, np.float32(0), a).astype(np.float64) * 2.0 ** 24)
    return q.astype(np.int64), bad


def sums(a, g0: int, rate: int):
    """One slot and call: (j0, int64 sums of the touched sub-cells j0 ... , bad count); no samples: (s(g0), [], 0)."""
    a = np.asarray(a, np.float32)
    j0 = subcell(int(g0), rate)
    if a.size == 0:
        return j0, np.zeros(0, np.int64), 0
    q, bad = quantise(a)
    j = subcell(np.int64(g0) + np.arange(a.size, dtype=np.int64), rate)
    out = np.zeros(int(j[-1]) - j0 + 1, np.int64)
    np.add.at(out, j - j0, q)
    return j0, out, int(bad.sum())


def sums_literal(a, g0: int, rate: int):
    """The same, one sample at a time in Python integers."""
    out, bad = {}, 0
    for i, v in enumerate(np.asarray(a, np.float32)):
        j = (672 * P * (g0 + i)) // (5 * rate)
        out.setdefault(j, 0)
        x = float(v)
        if math.isnan(x) or math.isinf(x) or abs(x) >= 32768.0:
            bad += 1
            continue
        y = x * 16777216.0                                   # exact: a power of two
        f = math.floor(y)
        r = f + 1 if y - f > 0.5 or (y - f == 0.5 and f % 2) else f
        out[j] += int(r)
    j0 = (672 * P * g0) // (5 * rate)
    return j0, [out[j] for j in sorted(out)], bad


def completed(a, rate: int):
    """The completed sub-cells of a whole stream from sample 0: every touched one but the last where the
    next sample would still fall into it."""
    _, s, _ = sums(a, 0, rate)
    n = len(a)
    if n and subcell(n, rate) == len(s) - 1:
        s = s[:-1]
    return s


class Carry:
    """The host half of a slot: counter, carried partial, merge."""

    def __init__(self, rate: int):
        self.rate, self.g, self.carry = rate, 0, None        # carry: (index, sum)

    def call(self, a):
        """One call's samples -> (first completed index, completed int64 sums, bad)."""
        j0, s, bad = sums(a, self.g, self.rate)
        self.g += len(a)
        if len(s) == 0:
            return j0, s, bad
        s = s.copy()
        if self.carry is not None:
            assert self.carry[0] == j0
            s[0] += self.carry[1]
        last = j0 + len(s) - 1
        if subcell(self.g, self.rate) == last:
            self.carry = (last, int(s[-1]))
            s = s[:-1]
        else:
            self.carry = None
        return j0, s, bad


# ------------------------------------------------------------------ the rule

def pattern(w: int, rot: int, words: int) -> np.ndarray:
    return np.array([1.0 if w >> ((i + rot) % BITS) & 1 else -1.0 for i in range(BITS * words)])


def score(sub, w: int, words: int) -> float:
    """The largest signed normalised correlation over the P phases and the 23 rotations."""
    sub = np.asarray(sub, np.float64)
    n = BITS * words
    best = -2.0
    for p in range(P):
        x = np.array([sub[p + P * i:p + P * i + P].sum() for i in range(n)])
        x = x - x.mean()
        nx = math.sqrt(float(x @ x))
        for r in range(BITS):
            b = pattern(w, r, words)
            b = b - b.mean()
            rho = 0.0 if nx == 0.0 else float(x @ b) / (nx * math.sqrt(float(b @ b)))
            best = max(best, rho)
    return best


class Rule:
    """The code squelch rule, one slot at a time in plain Python."""

    def __init__(self, words_, threshold, hang, wanted):
        """wanted: per slot None or the 23-bit word as it is on the air (complemented for an inverted code)."""
        self.words, self.threshold, self.hang, self.wanted = words_, threshold, hang, list(wanted)
        K = len(self.wanted)
        self.need = P * (BITS * words_ + 1)
        self.buf = [[] for _ in range(K)]
        self.next = [None] * K
        self.gate, self.misses, self.score = [False] * K, [0] * K, [math.nan] * K

    def _reset(self, k):
        self.buf[k], self.next[k], self.gate[k], self.misses[k], self.score[k] = [], None, False, 0, math.nan

    def update(self, first, cells, bad, n, active=None):
        for k, w in enumerate(self.wanted):
            if w is None:
                continue
            if (active is not None and not active[k]) or n[k] == 0 or bad[k] > 0:
                self._reset(k)
                continue
            if len(cells[k]) == 0:
                continue
            if self.next[k] is not None and self.next[k] != first[k]:
                self._reset(k)
            self.buf[k] += [int(v) for v in cells[k]]
            self.next[k] = int(first[k]) + len(cells[k])
            while len(self.buf[k]) >= self.need:
                rho = self.score[k] = score(self.buf[k][:self.need], w, self.words)
                self.buf[k] = self.buf[k][self.need:]
                if rho > self.threshold:
                    self.gate[k], self.misses[k] = True, 0
                else:
                    self.misses[k] += 1
                    if self.misses[k] >= self.hang:
                        self.gate[k] = False
        return [g or w is None for g, w in zip(self.gate, self.wanted)]


# ------------------------------------------------------------------ signals of the device tests

def nrz(w: int, n: int, fs: float, start_bit: float = 0.0) -> np.ndarray:
    """+-1 per sample: the word sent over and over at 134.4 bit/s, bit 0 first, 1 as +1."""
    bit = np.floor(start_bit + np.arange(n) * (134.4 / fs)).astype(np.int64) % BITS
    return np.where((w >> bit) & 1, 1.0, -1.0)


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


def four_signals(n: int, fs: float, seed: int = 91):
    """The four slots of the chain tests as complex baseband at ``fs``: code 023 (600 Hz deviation) under
    voice (RMS 1500 Hz deviation), code 047 -- the inverse of 023 -- alone, code 025 under voice, voice alone."""
    rng = np.random.Generator(np.random.PCG64(seed))
    return [fm(600.0 * nrz(word(0o023), n, fs, 3.3) + voice(rng, n, fs, 1500.0), fs),
            fm(600.0 * nrz(word(0o047), n, fs, 11.7), fs),
            fm(600.0 * nrz(word(0o025), n, fs, 7.1) + voice(rng, n, fs, 1500.0), fs),
            fm(voice(rng, n, fs, 1500.0), fs)]
