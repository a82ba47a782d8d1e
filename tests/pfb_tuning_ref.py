"""The channelizer's fine tuning (include/rfa.h, rfa_pfb_set_tuning) restated on
the host: slot j of a tuned handle writes

    i      = (n * m_j) mod Q
    (c, s) = W[i]
    z_re   = y_re * c + y_im * s
    z_im   = y_im * c - y_re * s

with n the absolute output index.  ``rot`` is that formula in numpy float32, one rounding per
operation, on the table ``rfa_pfb_tuning_table`` returns; ``rot64`` is y * exp(-2 pi j i / Q) in
float64.  The index is taken with Python integers, never from the library."""
import ctypes
import functools

import numpy as np

F32 = np.float32


@functools.lru_cache(maxsize=None)
def table(q: int):
    """(cos, sin) float32 arrays of rfa_pfb_tuning_table(q)."""
    import rfanalyzer_amd
    lib = rfanalyzer_amd.lib()
    c, s = np.empty(q, F32), np.empty(q, F32)
    fp = ctypes.POINTER(ctypes.c_float)
    rc = lib.rfa_pfb_tuning_table(q, c.ctypes.data_as(fp), s.ctypes.data_as(fp), q)
    assert rc == 0, rc
    c.setflags(write=False)
    s.setflags(write=False)
    return c, s


def index(q: int, m: int, n_first: int, count: int) -> np.ndarray:
    """(n * m) mod q for n = n_first ... n_first + count - 1, in Python integers."""
    return np.array([((n_first + k) * m) % q for k in range(count)], np.int64)


def rot(y, q: int, m: int, n_first: int = 0) -> np.ndarray:
    """The device's float32 rotation of the complex64 row y (outputs n_first, n_first + 1, ...);
    m == 0 returns y's own bits."""
    y = np.asarray(y, np.complex64)
    if m == 0:
        return y.copy()
    c, s = table(q)
    i = index(q, m, n_first, y.size)
    re, im = y.real.astype(F32), y.imag.astype(F32)
    with np.errstate(invalid="ignore", over="ignore"):
        z_re = (re * c[i]).astype(F32) + (im * s[i]).astype(F32)
        z_im = (im * c[i]).astype(F32) - (re * s[i]).astype(F32)
    out = np.empty(y.size, np.complex64)
    out.real, out.imag = z_re, z_im
    return out


def rot64(y, q: int, m: int, n_first: int = 0) -> np.ndarray:
    """y * exp(-2 pi j ((n m) mod q) / q) in float64."""
    y = np.asarray(y, np.complex128)
    return y * np.exp(-2j * np.pi * index(q, m, n_first, y.size) / q)


def same(a, b) -> None:
    """Bit for bit, NaN payloads aside: np.array_equal(..., equal_nan=True) on both parts."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.array_equal(a.real, b.real, equal_nan=True) and np.array_equal(a.imag, b.imag, equal_nan=True), \
        int(np.flatnonzero(~((a == b) | (np.isnan(a) & np.isnan(b)))).size)
