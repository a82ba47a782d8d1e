"""Float64 restatement of the rational-rate channelizer (include/rfa.h, rfa_pfb_create_rational;
DESIGN.md §5.7g).

With x[j] the converted input (j counts samples since creation or reset, x[j] = 0 for j < 0),
real prototype taps g[0..T-1] at rate L * Fs (g[s] = 0 for s >= T), M channels, integers
1 <= L <= D <= L * M with gcd(L, D) = 1 and Tp = ceil(T / L), output n has phase
p_n = (n * D) mod L and newest sample m_n = floor(n * D / L) (Python integers), and channel k is

    y_k[n] = sum_{t=0..Tp-1} g[p_n + t * L] * x[m_n - t] * exp(-j 2 pi k (m_n - t) / M)

Output n is due once sample m_n has been consumed: after c samples ceil(c * L / D) outputs exist.

``direct`` is that sum as written; ``folded`` is u_n[r] = sum of g[p_n + t L] * x[m_n - t] over
(m_n - t) mod M == r followed by ``np.fft.fft`` over r; ``sequential`` is the literal loop of
RationalResampler.resample (dsp/RationalResampler.kt:101-150) on the unmixed stream, which
channel 0 must equal.  Samples come from ``pfb_ref.convert``, so conversion is not part of any
error measured against these.
"""
import math

import numpy as np

from pfb_ref import EPS, convert  # noqa: F401  (convert: re-exported for the tests)


def count(c: int, L: int, D: int) -> int:
    """Outputs produced once c samples are consumed: ceil(c * L / D)."""
    return -(-c * L // D)


def output_count(c0: int, c1: int, L: int, D: int) -> int:
    """Outputs per channel of a call that takes the consumed count from c0 to c1."""
    return count(c1, L, D) - count(c0, L, D)


def phases(g, L: int) -> np.ndarray:
    """gp[p][t] = g[p + t * L], zero padded to Tp = ceil(T / L) per phase; float64 [L, Tp]."""
    g = np.asarray(g, np.float64)
    Tp = -(-len(g) // L)
    gp = np.zeros(L * Tp)
    gp[:len(g)] = g
    return gp.reshape(Tp, L).T.copy()


def _window(x, gp, n, L, D):
    """(g[p_n + t L] * x[m_n - t], m_n - t) for the t with 0 <= m_n - t, t ascending."""
    p, m = (n * D) % L, (n * D) // L
    t = np.arange(min(gp.shape[1], m + 1))
    j = m - t
    return gp[p, t] * x[j], j


def direct(x, g, M: int, L: int, D: int, n_first: int = 0, n_end=None) -> np.ndarray:
    """The defining sum; [M, n_end - n_first] complex128."""
    x = np.asarray(x, np.complex128)
    gp = phases(g, L)
    n_end = count(len(x), L, D) if n_end is None else n_end
    y = np.zeros((M, max(0, n_end - n_first)), np.complex128)
    k = np.arange(M)[:, None]
    for n in range(n_first, n_end):
        v, j = _window(x, gp, n, L, D)
        # k * (m_n - t) is an integer: reduced mod M before the division
        y[:, n - n_first] = (v[None, :] * np.exp(-2j * np.pi * ((k * j[None, :]) % M) / M)).sum(axis=1)
    return y


def folded(x, g, M: int, L: int, D: int, n_first: int = 0, n_end=None) -> np.ndarray:
    """Fold by (m_n - t) mod M, then a forward DFT; [M, n_end - n_first] complex128."""
    x = np.asarray(x, np.complex128)
    gp = phases(g, L)
    n_end = count(len(x), L, D) if n_end is None else n_end
    y = np.zeros((M, max(0, n_end - n_first)), np.complex128)
    for n in range(n_first, n_end):
        v, j = _window(x, gp, n, L, D)
        r = j % M
        u = np.bincount(r, v.real, M) + 1j * np.bincount(r, v.imag, M)
        y[:, n - n_first] = np.fft.fft(u)
    return y


def sequential(x, g, L: int, D: int) -> np.ndarray:
    """RationalResampler.resample as it is written, one packet holding the whole stream: the
    newest sample sits in a delay line; with the phase counter ``ctr`` (0 at the start) below L
    an output is the phase-``ctr`` sub-filter firTaps[ctr][t] = g[ctr + t * L] applied to the
    delay line newest first, then ctr += D, and while ctr >= L: ctr -= L and the next input
    sample is consumed.  Float64, no mixing."""
    x = np.asarray(x, np.complex128)
    g = np.asarray(g, np.float64)
    Tp = -(-len(g) // L)
    fir_taps = [g[p::L] for p in range(L)]         # rows may be one short of Tp: no padding here
    delay = np.zeros(Tp, np.complex128)
    out, ctr, consumed, di = [], 0, 0, 0
    if len(x) == 0:
        return np.zeros(0, np.complex128)
    delay[di] = x[0]
    while consumed < len(x):
        acc, d = 0.0 + 0.0j, di
        for t in fir_taps[ctr]:
            acc += t * delay[d]
            d = d - 1 if d > 0 else Tp - 1
        out.append(acc)
        ctr += D
        while ctr >= L:
            ctr -= L
            di = di + 1 if di + 1 < Tp else 0
            consumed += 1
            if consumed >= len(x):
                break
            delay[di] = x[consumed]
    return np.array(out, np.complex128)


class Stream:
    """The restatement with the handle's call rule: ``process`` takes the next samples of the
    stream and returns the outputs that fall due in that call."""

    def __init__(self, M: int, L: int, D: int, g, form=folded):
        self.M, self.L, self.D, self.g, self.form = M, L, D, np.asarray(g, np.float64), form
        self.x = np.zeros(0, np.complex128)

    def reset(self) -> None:
        self.x = np.zeros(0, np.complex128)

    def process(self, samples) -> np.ndarray:
        c0 = len(self.x)
        self.x = np.concatenate([self.x, np.asarray(samples, np.complex128)])
        return self.form(self.x, self.g, self.M, self.L, self.D, count(c0, self.L, self.D),
                         count(len(self.x), self.L, self.D))


def bound(g, x, M: int, L: int) -> float:
    """Worst-case |y - y_ref| of a float32 fold + DFT per complex output, derived as pfb_ref.bound
    is: an item of the fold is at most ceil(Tp / M) separately rounded multiply-adds of one phase's
    taps, each radix-2-equivalent DFT stage adds about 4 eps on a magnitude bounded by
    sum_t |g[p + t L]| * max|x| of the phase in use:
    eps * (ceil(Tp / M) + 4 * ceil(log2 M)) * max_p sum_t |g[p + t L]| * max|x|, eps = 2^-24."""
    gp = phases(g, L)
    P = -(-gp.shape[1] // M)
    return EPS * (P + 4 * math.ceil(math.log2(M))) * float(np.abs(gp).sum(axis=1).max()) \
        * float(np.abs(np.asarray(x)).max())
