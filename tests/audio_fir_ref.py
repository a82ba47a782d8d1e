"""The audio FIR bank restated in numpy float32 (what rfanalyzer_amd/csrc/audio_fir.hip computes), and an
independent float64 design of the voice high-pass.

Slot with taps t[0 ... T-1], n inputs x and a history of the last H = 4095 inputs:
    y[i] = (((+0.0f + t[0] * x[i]) + t[1] * x[i-1]) + ... + t[T-1] * x[i-T+1])
every product rounded to float32, every sum rounded to float32, in this order; x[j], j < 0, from the
history.  ``fir`` is a loop over the taps with vector operations over the outputs (numpy rounds each
float32 operation once and fuses nothing); ``fir_literal`` is the same statement sample by sample.
No taps: the input, bit for bit."""
import numpy as np

F32 = np.float32
MAX_TAPS = 4096
H = MAX_TAPS - 1


def fir(taps, x, hist=None):
    """(y, history after): the definition over one call."""
    taps = np.asarray(taps, F32).reshape(-1)
    x = np.asarray(x, F32).reshape(-1)
    hist = np.zeros(H, F32) if hist is None else np.asarray(hist, F32)
    assert hist.size == H and taps.size <= MAX_TAPS
    row = np.concatenate([hist, x])                         # row[H + i] = x[i]
    after = row[row.size - H:].copy()
    if taps.size == 0:
        return x.copy(), after
    n = x.size
    acc = np.zeros(n, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(taps.size):
            p = taps[k] * row[H - k:H - k + n]              # float32 * float32, rounded once
            acc = acc + p                                   # rounded once
    return acc, after


def fir_literal(taps, x, hist=None):
    """The same, one output and one tap at a time in numpy float32 scalars."""
    taps = [F32(t) for t in np.asarray(taps, F32).reshape(-1)]
    x = np.asarray(x, F32).reshape(-1)
    hist = np.zeros(H, F32) if hist is None else np.asarray(hist, F32)
    row = np.concatenate([hist, x])
    if not taps:
        return x.copy()
    y = np.empty(x.size, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(x.size):
            acc = F32(0.0)
            for k, t in enumerate(taps):
                p = F32(t * row[H + i - k])
                acc = F32(acc + p)
            y[i] = acc
    return y


class Slot:
    """One slot across calls: taps, and the last H inputs whatever the taps are."""

    def __init__(self, taps=()):
        self.taps = np.asarray(taps, F32).reshape(-1)
        self.hist = np.zeros(H, F32)

    def process(self, x):
        y, self.hist = fir(self.taps, x, self.hist)
        return y

    def reset(self):
        self.hist = np.zeros(H, F32)


def same(got, want, what=""):
    """Finite values and infinities bit for bit; NaN in the same positions."""
    got, want = np.asarray(got, F32), np.asarray(want, F32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), f"{what}: NaN positions differ"
    g, w = got.view(np.int32)[~gn], want.view(np.int32)[~wn]
    if not np.array_equal(g, w):
        at = int(np.flatnonzero(g != w)[0])
        raise AssertionError(f"{what}: {int((g != w).sum())} of {g.size} values differ, first at {at}: "
                             f"{got[~gn][at]!r} against {want[~wn][at]!r}")


def bits_equal(got, want) -> bool:
    return np.array_equal(np.asarray(got, F32).view(np.int32), np.asarray(want, F32).view(np.int32))


def rows(k: int, n: int, seed: int = 5) -> np.ndarray:
    """[k, n] float32 audio-like rows in about +-1."""
    rng = np.random.Generator(np.random.PCG64(seed))
    return (0.3 * rng.standard_normal((k, n))).astype(F32)


def taps_of(t: int, seed: int = 11) -> np.ndarray:
    """t non-zero float32 taps of about 1 / sqrt(t) each."""
    rng = np.random.Generator(np.random.PCG64(seed + t))
    v = rng.standard_normal(t) / np.sqrt(max(t, 1))
    v[np.abs(v) < 1e-3] = 1e-3
    return v.astype(F32)


# ------------------------------------------------------------------ the voice high-pass, independently

def highpass_f64(num_taps: int, rate: float, cutoff_hz: float) -> np.ndarray:
    """A float64 Blackman windowed-sinc low-pass of unit DC gain, spectrally inverted."""
    assert num_taps % 2 == 1
    m = (num_taps - 1) // 2
    n = np.arange(-m, m + 1, dtype=np.float64)
    lp = 2.0 * cutoff_hz / rate * np.sinc(2.0 * cutoff_hz / rate * n) * np.blackman(num_taps)
    lp /= lp.sum()
    hp = -lp
    hp[m] += 1.0
    return hp


def response_db(taps, hz: float, rate: float) -> float:
    """20 log10 |H(hz)| of the taps in float64."""
    t = np.asarray(taps, np.float64)
    w = np.exp(-2j * np.pi * hz / rate * np.arange(t.size))
    return float(20.0 * np.log10(max(abs(np.sum(t * w)), 1e-300)))
