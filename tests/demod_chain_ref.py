"""TEST INFRASTRUCTURE ONLY -- restatement of the reference's demodulator chain.

Not a test.  Written from the algorithm of analyzer/Demodulator.kt:151-187 and
:215-403, dsp/ComplexFirFilter.java:123-262 and analyzer/AudioSink.java:94-97,
215-237 (paths relative to app/src/main/java/com/mantz_it/rfanalyzer/): per packet
the user filter, the mode's demodulator, the volume, then the AudioSink's
decimating filters on the real stream.

Float32 semantics are kept per operation with numpy float32 scalars and arrays
(every product and sum rounds; no fused multiply-add).  ``math.sin``/``cos`` are
the platform libm, as in oracle/demod.py; ``np.arctan2`` in float64 cast to
float32 stands in for the JVM's ``Math.atan2``.
"""
from __future__ import annotations

import math

import numpy as np

from oracle.demod import F32, FirDecimator, _jtoint, blackman, low_pass_taps

OFF, AM, NFM, WFM, LSB, USB, CW = range(7)
MODE_NAMES = {OFF: "OFF", AM: "AM", NFM: "NFM", WFM: "WFM", LSB: "LSB", USB: "USB", CW: "CW"}
AUDIO_RATE = 48000
CW_OFFSET_FREQUENCY = 750
# mode: (quadrature rate, min width, max width, default width)
MODE_INFO = {
    OFF: (96000, 0, 50000, 0),
    AM: (96000, 3000, 15000, 8000),
    NFM: (96000, 3000, 15000, 10000),
    WFM: (384000, 30000, 150000, 100000),
    LSB: (96000, 1500, 5000, 2800),
    USB: (96000, 1500, 5000, 2800),
    CW: (48000, 150, 800, 300),
}


def band_pass_taps(gain, sample_rate, low, high, transition, attenuation):
    """ComplexFirFilter.createBandPass: (re, im) float32 taps, None where it returns null."""
    g, fs, lo, hi, tw, att = (F32(v) for v in (gain, sample_rate, low, high, transition, attenuation))
    if not fs > 0.0:
        return None
    if float(lo) < float(fs) * -0.5 or float(hi) > float(fs) * 0.5:
        return None
    if not lo < hi:
        return None
    if not tw > 0:
        return None
    ntaps = _jtoint(float(F32(att * fs)) / (22.0 * float(tw)))
    if ntaps & 1 == 0:
        ntaps += 1
    cut = F32(F32(hi - lo) / F32(2))
    pi = F32(math.pi)
    M = (ntaps - 1) // 2
    lp = np.empty(ntaps, F32)
    fwt0 = F32(F32(F32(F32(2) * pi) * cut) / fs)
    for n in range(-M, M + 1):
        w = blackman(n + M, ntaps)
        if n == 0:
            lp[n + M] = F32(F32(fwt0 / pi) * w)
        else:
            lp[n + M] = F32(F32(F32(math.sin(float(F32(F32(n) * fwt0)))) / F32(F32(n) * pi)) * w)
    fmax = lp[M]
    for n in range(1, M + 1):
        fmax = F32(fmax + F32(F32(2) * lp[n + M]))
    lp = (lp * F32(g / fmax)).astype(F32)
    freq = F32(F32(pi * F32(hi + lo)) / fs)
    phase = F32(F32(-freq) * F32(ntaps // 2))
    re = np.empty(ntaps, F32)
    im = np.empty(ntaps, F32)
    for i in range(ntaps):
        re[i] = F32(lp[i] * F32(math.cos(float(phase))))
        im[i] = F32(lp[i] * F32(math.sin(float(phase))))
        phase = F32(phase + freq)
    return re, im


class ComplexFir:
    """ComplexFirFilter.filter: delay line of zeros, decimationCounter 1, per output
    re += tr*dr - ti*di; im += ti*dr + tr*di, newest sample first."""

    def __init__(self, taps_re, taps_im, decimation, low=0.0, high=0.0):
        self.tr = np.asarray(taps_re, F32)
        self.ti = np.asarray(taps_im, F32)
        self.d = int(decimation)
        self.low, self.high = F32(low), F32(high)
        T = len(self.tr)
        self.hist_re = np.zeros(T - 1, F32)
        self.hist_im = np.zeros(T - 1, F32)
        self.counter = 1

    def filter(self, re, im):
        re, im = np.asarray(re, F32), np.asarray(im, F32)
        T, S, D = len(self.tr), len(re), self.d
        if S == 0:
            return np.zeros(0, F32), np.zeros(0, F32)
        xre = np.concatenate([self.hist_re, re])
        xim = np.concatenate([self.hist_im, im])
        first = 1 if (D == 1 and self.counter == 1) else (D - self.counter) % D
        js = np.arange(first, S, D)
        # one row per output, one column per tap; the running sums start at 0 and take the
        # per-tap terms left to right (accumulate is sequential, every step rounds to float32)
        idx = T - 1 + js[:, None] - np.arange(T)[None, :]
        dr, di = xre[idx], xim[idx]
        zero = np.zeros((len(js), 1), F32)
        tre = np.concatenate([zero, self.tr * dr - self.ti * di], axis=1).astype(F32)
        tim = np.concatenate([zero, self.ti * dr + self.tr * di], axis=1).astype(F32)
        ore = np.add.accumulate(tre, axis=1, dtype=F32)[:, -1]
        oim = np.add.accumulate(tim, axis=1, dtype=F32)[:, -1]
        self.hist_re = xre[len(xre) - (T - 1):].copy()
        self.hist_im = xim[len(xim) - (T - 1):].copy()
        self.counter = (self.counter + S) % D
        return ore.astype(F32), oim.astype(F32)

    def filter_literal(self, re, im):
        """The per-sample loop, for small cases (checks the closed form above)."""
        T = len(self.tr)
        if not hasattr(self, "_dre"):
            self._dre, self._dim, self._tap, self._ctr = np.zeros(T, F32), np.zeros(T, F32), 0, 1
        out_re, out_im = [], []
        for x, y in zip(np.asarray(re, F32), np.asarray(im, F32)):
            self._dre[self._tap], self._dim[self._tap] = x, y
            if self._ctr == 0:
                a, b, i = F32(0), F32(0), self._tap
                for tr, ti in zip(self.tr, self.ti):
                    a = F32(a + F32(F32(tr * self._dre[i]) - F32(ti * self._dim[i])))
                    b = F32(b + F32(F32(ti * self._dre[i]) + F32(tr * self._dim[i])))
                    i = i - 1 if i > 0 else T - 1
                out_re.append(a)
                out_im.append(b)
            self._ctr += 1
            if self._ctr >= self.d:
                self._ctr = 0
            self._tap = self._tap + 1 if self._tap + 1 < T else 0
        return np.array(out_re, F32), np.array(out_im, F32)


class RealFir:
    """FirFilter.filterReal: the real delay line and the counters of a FirFilter."""

    def __init__(self, taps, decimation):
        self.fir = FirDecimator(taps, decimation)
        self.taps = self.fir.taps

    def filter(self, x):
        x = np.asarray(x, F32)
        if len(x) == 0:                      # an empty packet moves no counter
            return np.zeros(0, F32)
        return self.fir.filter(x, np.zeros(len(x), F32))[0]


class ComplexLowPass:
    """FirFilter.filter of a complex packet, with the cut-off the rebuild rule reads."""

    def __init__(self, taps, cutoff):
        self.fir = FirDecimator(taps, 1)
        self.taps = self.fir.taps
        self.cutoff = F32(cutoff)

    def filter(self, re, im):
        if len(re) == 0:
            return np.zeros(0, F32), np.zeros(0, F32)
        return self.fir.filter(re, im)


class AudioSinkRef:
    """AudioSink's two filters and applyAudioFilter, keyed by the packet's sample rate."""

    def __init__(self):
        self.f1 = RealFir(low_pass_taps(1, 1, 0.1, 0.15, 30), 2)
        self.f2 = RealFir(low_pass_taps(1, 1, 0.1, 0.1, 30), 4)

    def play(self, x, rate):
        if rate <= AUDIO_RATE:
            return np.asarray(x, F32)
        if rate // AUDIO_RATE == 8:
            return self.f2.filter(self.f1.filter(x))
        if rate // AUDIO_RATE == 2:
            return self.f1.filter(x)
        raise ValueError(rate)

    def taps_in_use(self, rate):
        r = rate // AUDIO_RATE
        return [self.f1.taps, self.f2.taps] if r == 8 else ([self.f1.taps] if r == 2 else [])


class DemodChain:
    """Demodulator + AudioSink, one packet at a time."""

    def __init__(self, mode, audio_sink=True):
        self.user = None
        self.band = None
        self.carry_re = F32(0)
        self.carry_im = F32(0)
        self.last_max = F32(0)
        self.volume = F32(1)
        self.sink = AudioSinkRef()
        self.sink_enabled = audio_sink
        self.mode = OFF
        self.width = 0
        self.set_mode(mode)
        self.pre_sink = np.zeros(0, F32)     # what the last process() handed to the AudioSink
        self.packet_rate = AUDIO_RATE

    # -- settings
    def set_mode(self, mode):
        self.mode = mode
        self.set_width(MODE_INFO[mode][3])

    def set_width(self, w):
        _, lo, hi, _ = MODE_INFO[self.mode]
        self.width = min(max(int(w), lo), hi)

    @property
    def rate(self):
        return MODE_INFO[self.mode][0]

    def reset(self):
        mode, width, vol, en = self.mode, self.width, self.volume, self.sink_enabled
        self.__init__(mode, en)
        self.width, self.volume = width, vol

    def state(self):
        return self.last_max, self.carry_re, self.carry_im

    # -- per packet
    def _user_filter(self, re, im):
        if self.user is None or _jtoint(float(self.user.cutoff)) != self.width:
            rate = F32(self.rate)
            taps = low_pass_taps(1, rate, F32(self.width), F32(rate * F32(0.10)), 60)
            assert taps is not None
            self.user = ComplexLowPass(taps, self.width)
        return self.user.filter(re, im)

    def _agc(self, x):
        self.last_max = F32(self.last_max * F32(0.95))
        live = x[~np.isnan(x)]
        if len(live) and live.max() > self.last_max:
            self.last_max = F32(live.max())
        with np.errstate(divide="ignore"):
            return F32(F32(0.75) / self.last_max)

    def _fm(self, re, im, dev_factor):
        max_dev = F32(F32(self.width) * F32(dev_factor))
        qgain = F32(F32(self.rate) / F32(2 * math.pi * float(max_dev)))
        if len(re) == 0:
            return np.zeros(0, F32)
        pre = np.concatenate([[self.carry_re], re[:-1]]).astype(F32)
        pim = np.concatenate([[self.carry_im], im[:-1]]).astype(F32)
        cr = re * pre + im * pim
        ci = im * pre - re * pim
        ang = np.arctan2(ci.astype(np.float64), cr.astype(np.float64)).astype(F32)
        self.carry_re, self.carry_im = F32(re[-1]), F32(im[-1])
        return (qgain * ang).astype(F32)

    def _am(self, re, im):
        x = (re * re + im * im).astype(F32)
        gain = self._agc(x)
        if len(x) == 0:
            return x
        avg = F32(np.add.accumulate(x, dtype=F32)[-1] / F32(len(x)))   # sequential, index order
        with np.errstate(invalid="ignore", over="ignore"):
            return ((x - avg) * gain).astype(F32)

    def _band(self, re, im):
        w = self.width
        if self.mode == CW:
            stale = self.band is None or _jtoint(float(self.band.high)) != CW_OFFSET_FREQUENCY + w // 2
            if stale:
                lo = F32(F32(CW_OFFSET_FREQUENCY) - F32(w) / F32(2.0))
                hi = F32(F32(CW_OFFSET_FREQUENCY) + F32(w) / F32(2.0))
                dec = 1
        else:
            upper = self.mode == USB
            stale = (self.band is None or (upper and _jtoint(float(self.band.high)) != w)
                     or (not upper and _jtoint(float(self.band.low)) != -w))
            if stale:
                lo, hi = (F32(200), F32(w)) if upper else (F32(-w), F32(-200))
                dec = 2
        if stale:
            rate = F32(self.rate)
            tr, ti = band_pass_taps(1, rate, lo, hi, F32(rate * F32(0.01)), 40)
            self.band = ComplexFir(tr, ti, dec, lo, hi)
        out, _ = self.band.filter(re, im)
        gain = self._agc(out)
        with np.errstate(invalid="ignore", over="ignore"):
            return (out * gain).astype(F32), self.rate // self.band.d

    def packet(self, re, im):
        """One input packet -> (audioBuffer after the volume, its sample rate)."""
        if self.mode == OFF:
            return np.zeros(0, F32), self.rate
        fre, fim = self._user_filter(np.asarray(re, F32), np.asarray(im, F32))
        rate = self.rate
        if self.mode == AM:
            out = self._am(fre, fim)
        elif self.mode == NFM:
            out = self._fm(fre, fim, 0.75)
        elif self.mode == WFM:
            out = self._fm(fre, fim, 0.85)
        else:
            out, rate = self._band(fre, fim)
        with np.errstate(invalid="ignore", over="ignore"):
            return (out * self.volume).astype(F32), rate

    def process(self, re, im, packet_samples=0):
        """A call of the device library: packets of packet_samples (0: one packet; no
        samples: one empty packet), each through the chain and the AudioSink."""
        re, im = np.asarray(re, F32), np.asarray(im, F32)
        n = len(re)
        if self.mode == OFF:
            return np.zeros(0, F32)
        ps = packet_samples if packet_samples > 0 else max(n, 1)
        pre, audio = [], []
        for s in range(0, max(n, 1), ps):
            buf, rate = self.packet(re[s:s + ps], im[s:s + ps])
            pre.append(buf)
            self.packet_rate = rate
            audio.append(self.sink.play(buf, rate) if self.sink_enabled else buf)
        self.pre_sink = np.concatenate(pre).astype(F32)
        return np.concatenate(audio).astype(F32)
