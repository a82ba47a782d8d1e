"""The audio resampler bank restated in numpy float32 (what rfanalyzer_amd/csrc/audio_rs.hip computes), a
float64 version of it, and an independent float64 design of the resampling low-pass.

Handle constants L / D (reduced, L <= D) and taps h[0 ... T-1], J = ceil(T / L).  A slot keeps its last
H = 4095 inputs and an offset r, 0 <= r < D.  A call of n inputs x writes outputs m = 0, 1, ... while
r + m D < n L; output m has u = r + m D, i = u // L, p = u % L and
    y = (((+0.0f + h[p] * x[i]) + h[p+L] * x[i-1]) + ... + h[p+(J-1)L] * x[i-J+1])
taps at or beyond T counting as +0.0f and still multiplied and added, every product and every sum rounded
to float32 in this order; x[j], j < 0, from the history.  Then r <- r + n_out D - n L.  T = 0 (L = D = 1):
y = x bitwise.  PCM: v = y * 32768; NaN -> 0; v >= 32767 -> 32767; v <= -32768 -> -32768; else rint(v).

``resample`` is a loop over the J taps with vector operations over the outputs (numpy rounds each float32
operation once and fuses nothing); ``resample_literal`` is the same statement output by output."""
import numpy as np

F32 = np.float32
H = 4095
MAX_PHASE_TAPS = 4096


def counts(L: int, D: int, r: int, n: int):
    """(n_out, r_next) by the rule's own words: outputs while r + m D < n L."""
    n_out = -((r - n * L) // D) if n * L > r else 0         # ceil((n L - r) / D)
    return n_out, r + n_out * D - n * L


def phase_rows(L: int, taps) -> np.ndarray:
    """g[p][j] = h[p + j L], +0.0f at or beyond T: float32 [L, J]."""
    taps = np.asarray(taps, F32).reshape(-1)
    J = -(-taps.size // L)
    g = np.zeros(J * L, F32)
    g[:taps.size] = taps
    return g.reshape(J, L).T.copy()


def resample(L, D, taps, x, r=0, hist=None, dtype=F32):
    """(y, r after, history after): the definition over one call, in ``dtype`` arithmetic."""
    x = np.asarray(x, F32).reshape(-1)
    hist = np.zeros(H, F32) if hist is None else np.asarray(hist, F32)
    assert hist.size == H and 0 <= r < D
    row = np.concatenate([hist, x])                         # row[H + i] = x[i]
    after = row[row.size - H:].copy()
    n_out, r_next = counts(L, D, r, x.size)
    taps = np.asarray(taps, F32).reshape(-1)
    if taps.size == 0:
        assert L == 1 and D == 1
        return x.astype(dtype), r_next, after
    g = phase_rows(L, taps).astype(dtype)
    J = g.shape[1]
    assert J <= MAX_PHASE_TAPS
    u = r + np.arange(n_out, dtype=np.int64) * D
    i, p = u // L, u % L
    acc = np.zeros(n_out, dtype)
    rowd = row.astype(dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(J):
            prod = g[p, j] * rowd[H + i - j]                # rounded once in dtype
            acc = acc + prod                                # rounded once
    return acc, r_next, after


def resample_literal(L, D, taps, x, r=0, hist=None):
    """The same, one output and one tap at a time in numpy float32 scalars, from h itself."""
    h = [F32(t) for t in np.asarray(taps, F32).reshape(-1)]
    x = np.asarray(x, F32).reshape(-1)
    hist = np.zeros(H, F32) if hist is None else np.asarray(hist, F32)
    row = np.concatenate([hist, x])
    if not h:
        return x.copy()
    J = -(-len(h) // L)
    y = []
    with np.errstate(invalid="ignore", over="ignore"):
        m = 0
        while r + m * D < x.size * L:
            u = r + m * D
            i, p = u // L, u % L
            acc = F32(0.0)
            for j in range(J):
                t = h[p + j * L] if p + j * L < len(h) else F32(0.0)
                acc = F32(acc + F32(t * row[H + i - j]))
            y.append(acc)
            m += 1
    return np.array(y, F32)


def abs_sum(L, D, taps, x, r=0, hist=None):
    """sum_j |g[p][j] x[i-j]| per output in float64: the scale of the float32 rounding bound."""
    x = np.asarray(x, F32).reshape(-1)
    hist = np.zeros(H, F32) if hist is None else np.asarray(hist, F32)
    row = np.abs(np.concatenate([hist, x]).astype(np.float64))
    g = np.abs(phase_rows(L, taps).astype(np.float64))
    n_out, _ = counts(L, D, r, x.size)
    u = r + np.arange(n_out, dtype=np.int64) * D
    i, p = u // L, u % L
    acc = np.zeros(n_out)
    for j in range(g.shape[1]):
        acc += g[p, j] * row[H + i - j]
    return acc


def pcm(y) -> np.ndarray:
    """The conversion, from its text."""
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.asarray(y, F32) * F32(32768.0)
        out = np.zeros(v.shape, np.int16)
        hi, lo, nan = v >= F32(32767.0), v <= F32(-32768.0), np.isnan(v)
        mid = ~(hi | lo | nan)
        out[hi], out[lo] = 32767, -32768
        out[mid] = np.rint(v[mid]).astype(np.int16)         # ties to even
    return out


class Slot:
    """One slot across calls: the last H inputs and the offset."""

    def __init__(self, L, D, taps):
        self.L, self.D, self.taps = L, D, np.asarray(taps, F32).reshape(-1)
        self.reset()

    def reset(self):
        self.hist, self.r = np.zeros(H, F32), 0

    def process(self, x):
        if len(x) == 0:
            return np.zeros(0, F32)
        y, self.r, self.hist = resample(self.L, self.D, self.taps, x, self.r, self.hist)
        return y


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


def same_pcm(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.int16 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    if not np.array_equal(got, want):
        at = int(np.flatnonzero(got != want)[0])
        raise AssertionError(f"{what}: {int((got != want).sum())} of {got.size} PCM values differ, first at {at}: "
                             f"{got[at]} against {want[at]}")


def bits_equal(got, want) -> bool:
    return np.array_equal(np.asarray(got, F32).view(np.int32), np.asarray(want, F32).view(np.int32))


def rows(k: int, n: int, seed: int = 5) -> np.ndarray:
    """[k, n] float32 audio-like rows in about +-1."""
    rng = np.random.Generator(np.random.PCG64(seed))
    return (0.3 * rng.standard_normal((k, n))).astype(F32)


def taps_of(t: int, L: int = 1, seed: int = 21) -> np.ndarray:
    """t non-zero float32 taps whose phase rows have a sum of squares of about 1."""
    rng = np.random.Generator(np.random.PCG64(seed + t))
    v = rng.standard_normal(t) / np.sqrt(max(t / L, 1))
    v[np.abs(v) < 1e-3] = 1e-3
    return v.astype(F32)


# ------------------------------------------------------------------ the low-pass, independently

def lowpass_f64(num_taps: int, rate: float, cutoff_hz: float, gain: float) -> np.ndarray:
    """A float64 Blackman windowed-sinc low-pass with DC gain ``gain``."""
    assert num_taps % 2 == 1
    m = (num_taps - 1) // 2
    n = np.arange(-m, m + 1, dtype=np.float64)
    lp = 2.0 * cutoff_hz / rate * np.sinc(2.0 * cutoff_hz / rate * n) * np.blackman(num_taps)
    return lp * (gain / lp.sum())


def response_db(taps, hz: float, rate: float) -> float:
    """20 log10 |H(hz)| of the taps in float64, at the sample rate ``rate`` the taps run at."""
    t = np.asarray(taps, np.float64)
    w = np.exp(-2j * np.pi * hz / rate * np.arange(t.size))
    return float(20.0 * np.log10(max(abs(np.sum(t * w)), 1e-300)))
