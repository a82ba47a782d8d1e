"""Float64 restatement of the polyphase channelizer (include/rfa.h, rfa_pfb_*).

With x[j] the converted input (j counts samples since creation or reset, x[j] = 0 for j < 0),
real taps h[0..T-1], M channels and decimation D, output n is due once sample
i_n = n * D + D - 1 has been consumed, and channel k is

    y_k[n] = sum_t h[t] * x[i_n - t] * exp(-j 2 pi k (i_n - t) / M)

Two forms: ``direct`` is that sum as written; ``folded`` is
u_n[r] = sum of h[t] * x[i_n - t] over (i_n - t) mod M == r followed by ``np.fft.fft`` over r,
used for the large cases.  Both start from samples converted with the device's float32
formulas (``convert``), so conversion is not part of any error measured against them.
"""
import math

import numpy as np

F32 = np.float32
EPS = 2.0 ** -24


def convert(raw, fmt: str) -> np.ndarray:
    """Raw bytes / array -> complex128 holding the float32 values the device converts to
    (s8: b/128, u8: (b - 127.4f)/128, s16: s/32768, f32: interleaved I,Q as they are)."""
    b = np.frombuffer(raw, np.uint8) if isinstance(raw, (bytes, bytearray, memoryview)) \
        else np.ascontiguousarray(raw).view(np.uint8).reshape(-1)
    if fmt == "s8":
        v = b.view(np.int8).astype(F32) / F32(128.0)
    elif fmt == "u8":
        v = (b.astype(F32) - F32(127.4)) / F32(128.0)
    elif fmt == "s16":
        v = b.view("<i2").astype(F32) / F32(32768.0)
    elif fmt == "f32":
        v = b.view("<f4")
    else:
        raise ValueError(fmt)
    assert v.dtype == F32
    return v[0::2].astype(np.float64) + 1j * v[1::2].astype(np.float64)


def output_count(c0: int, c1: int, D: int) -> int:
    """Outputs per channel of a call that takes the consumed count from c0 to c1."""
    return c1 // D - c0 // D


def _window(x, h, i):
    """(h[t] * x[i - t], i - t) for the t with 0 <= i - t, t ascending."""
    t = np.arange(min(len(h), i + 1))
    j = i - t
    return h[t] * x[j], j


def direct(x, h, M: int, D: int, n_first: int = 0, n_end=None) -> np.ndarray:
    """The defining sum; [M, n_end - n_first] complex128."""
    x = np.asarray(x, np.complex128)
    h = np.asarray(h, np.float64)
    n_end = len(x) // D if n_end is None else n_end
    y = np.zeros((M, max(0, n_end - n_first)), np.complex128)
    k = np.arange(M)[:, None]
    for n in range(n_first, n_end):
        v, j = _window(x, h, n * D + D - 1)
        # k * (i_n - t) is an integer: reduced mod M before the division, so the phase's rounding
        # error does not grow with the sample index
        y[:, n - n_first] = (v[None, :] * np.exp(-2j * np.pi * ((k * j[None, :]) % M) / M)).sum(axis=1)
    return y


def folded(x, h, M: int, D: int, n_first: int = 0, n_end=None) -> np.ndarray:
    """Fold by (i_n - t) mod M, then a forward DFT; [M, n_end - n_first] complex128."""
    x = np.asarray(x, np.complex128)
    h = np.asarray(h, np.float64)
    n_end = len(x) // D if n_end is None else n_end
    y = np.zeros((M, max(0, n_end - n_first)), np.complex128)
    for n in range(n_first, n_end):
        v, j = _window(x, h, n * D + D - 1)
        r = j % M
        u = np.bincount(r, v.real, M) + 1j * np.bincount(r, v.imag, M)
        y[:, n - n_first] = np.fft.fft(u)
    return y


class Stream:
    """The restatement with the handle's call rule: ``process`` takes the next samples of the
    stream and returns the outputs that fall due in that call."""

    def __init__(self, M: int, D: int, h, form=folded):
        self.M, self.D, self.h, self.form = M, D, np.asarray(h, np.float64), form
        self.x = np.zeros(0, np.complex128)

    def reset(self) -> None:
        self.x = np.zeros(0, np.complex128)

    def process(self, samples) -> np.ndarray:
        c0 = len(self.x)
        self.x = np.concatenate([self.x, np.asarray(samples, np.complex128)])
        return self.form(self.x, self.h, self.M, self.D, c0 // self.D, len(self.x) // self.D)


def bound(h, x, M: int) -> float:
    """Worst-case |y - y_ref| of a float32 fold + DFT per complex output:
    eps * (P + 4 * ceil(log2 M)) * sum|h| * max|x|, P = ceil(T / M), eps = 2^-24."""
    h = np.asarray(h, np.float64)
    P = -(-len(h) // M)
    return EPS * (P + 4 * math.ceil(math.log2(M))) * float(np.abs(h).sum()) * float(np.abs(np.asarray(x)).max())
