"""Float32 model of what the channelizer kernels compute for one output time
(rfanalyzer_amd/csrc/channelizer.hip: pfb_kernel / pfb_rational_kernel, pfb_butterfly; DESIGN.md
§5.7f), statement for statement: every product and every sum is rounded to float32 on its own
(the file compiles with contraction off) and in the kernel's order, so a device output must equal
the model's bit for bit.

Fold.  Item r of an output whose newest sample is i sums acc = acc + h[t] * x[i - t] over
t = t0, t0 + M, ... < T with t0 = (i mod M - r) mod M, acc starting at (0, 0).  On the rational path
h is the tap row gp[p_n] (gp[p][t] = g[p + t L], zero padded to Tp) and i = m_n.  Samples older than
the stream are the zeros of the history buffer and are multiplied like any other.

Stages.  Stockham, radix R after p = product of the earlier radices: butterfly i < Q = M / R reads
src[i + r Q], multiplies inputs r >= 1 by tw[k (R - 1) + (r - 1)] with k = i mod p -- only where
p > 1 -- runs the radix's butterfly as written and writes dst[(i - k) R + k + r p].  The stage tables
are pfb_twiddles': angle -2 pi ((k r) mod (p R)) / (p R) in double through the C library's cos and
sin, rounded once.

Vectorised over the outputs of a call, over r, and over the butterflies of a stage; the loops left
are over the taps of an item and the stages.  Samples come from pfb_ref.convert (complex128 holding
the device's float32 values)."""
import math

import numpy as np

F32 = np.float32


# ---------------------------------------------------------------- plan (host side of the file)

def radices(M: int) -> list:
    """pfb_radices: 4s, one 2 for an odd power of two, 3s, 5s."""
    a = b = c = 0
    m = M
    while m % 2 == 0:
        m //= 2
        a += 1
    while m % 3 == 0:
        m //= 3
        b += 1
    while m % 5 == 0:
        m //= 5
        c += 1
    assert m == 1 and 8 <= M <= 4096, M
    return [4] * (a // 2) + [2] * (a % 2) + [3] * b + [5] * c


def twiddles(radix) -> list:
    """Per stage (re, im) float32 arrays of p * (R - 1) entries, entry k * (R - 1) + (r - 1)."""
    out, p = [], 1
    for R in radix:
        n = p * R
        re, im = np.empty(p * (R - 1), F32), np.empty(p * (R - 1), F32)
        for k in range(p):
            for r in range(1, R):
                ang = -2.0 * math.pi * float((k * r) % n) / float(n)
                re[k * (R - 1) + (r - 1)] = math.cos(ang)
                im[k * (R - 1) + (r - 1)] = math.sin(ang)
        out.append((re, im))
        p = n
    return out


# ---------------------------------------------------------------- complex helpers, one rounding per operation

def _cadd(a, b):
    return a[0] + b[0], a[1] + b[1]


def _csub(a, b):
    return a[0] - b[0], a[1] - b[1]


def _cmul(a, w):
    return a[0] * w[0] - a[1] * w[1], a[0] * w[1] + a[1] * w[0]


def _cscale(s, a):
    return s * a[0], s * a[1]


def _mul_mi(m, n):          # m - j n
    return m[0] + n[1], m[1] - n[0]


def _mul_pi(m, n):          # m + j n
    return m[0] - n[1], m[1] + n[0]


HALF = F32(0.5)
SIN60 = F32(0.86602540378443864676)
C1, C2 = F32(0.30901699437494742410), F32(-0.80901699437494742410)
S1, S2 = F32(0.95105651629515357212), F32(0.58778525229247312917)


def _butterfly(R, u):
    if R == 2:
        return [_cadd(u[0], u[1]), _csub(u[0], u[1])]
    if R == 4:
        a, b, c, d = _cadd(u[0], u[2]), _csub(u[0], u[2]), _cadd(u[1], u[3]), _csub(u[1], u[3])
        return [_cadd(a, c), _mul_mi(b, d), _csub(a, c), _mul_pi(b, d)]
    if R == 3:
        t = _cadd(u[1], u[2])
        m = _csub(u[0], _cscale(HALF, t))
        s = _cscale(SIN60, _csub(u[1], u[2]))
        return [_cadd(u[0], t), _mul_mi(m, s), _mul_pi(m, s)]
    assert R == 5
    a1, a2, b1, b2 = _cadd(u[1], u[4]), _cadd(u[2], u[3]), _csub(u[1], u[4]), _csub(u[2], u[3])
    m1 = _cadd(_cadd(u[0], _cscale(C1, a1)), _cscale(C2, a2))
    m2 = _cadd(_cadd(u[0], _cscale(C2, a1)), _cscale(C1, a2))
    n1 = _cadd(_cscale(S1, b1), _cscale(S2, b2))
    n2 = _csub(_cscale(S2, b1), _cscale(S1, b2))
    return [_cadd(_cadd(u[0], a1), a2), _mul_mi(m1, n1), _mul_mi(m2, n2), _mul_pi(m2, n2), _mul_pi(m1, n1)]


def dft(re, im, radix, tw=None):
    """The stage loop on rows [n, M] of float32: (re, im) of the M channels of every row."""
    M = re.shape[1]
    tw = twiddles(radix) if tw is None else tw
    assert re.dtype == F32 and im.dtype == F32 and int(np.prod(radix)) == M
    p = 1
    with np.errstate(invalid="ignore", over="ignore"):
        for R, (wr, wi) in zip(radix, tw):
            Q = M // R
            i = np.arange(Q)
            k = i % p
            j = (i - k) * R + k
            u = [(re[:, i + r * Q], im[:, i + r * Q]) for r in range(R)]
            if p > 1:
                for r in range(1, R):
                    e = k * (R - 1) + (r - 1)
                    u[r] = _cmul(u[r], (wr[e], wi[e]))
            y = _butterfly(R, u)
            nre, nim = np.empty_like(re), np.empty_like(im)
            for r in range(R):
                nre[:, j + r * p], nim[:, j + r * p] = y[r]
            re, im = nre, nim
            p *= R
    return re, im


def fold(xr, xi, origin, rows, newest, M):
    """u[n, r] of the outputs whose newest samples are ``newest`` (absolute indices): xr / xi hold the
    float32 samples from absolute index ``origin`` on (indices below it are never needed), rows[n] is
    output n's tap row (float32 [n, T], or [T] shared by all)."""
    newest = np.asarray(newest, np.int64)
    rows = np.asarray(rows)
    assert rows.dtype == F32 and xr.dtype == F32 and xi.dtype == F32
    T = rows.shape[-1]
    n = newest.size
    r = np.arange(M)[None, :]
    t = (newest[:, None] % M - r) % M                       # t0 of item (n, r)
    ar, ai = np.zeros((n, M), F32), np.zeros((n, M), F32)
    nn = np.arange(n)[:, None]
    with np.errstate(invalid="ignore", over="ignore"):
        while True:
            live = t < T
            if not live.any():
                break
            tc = np.where(live, t, 0)
            h = rows[tc] if rows.ndim == 1 else rows[nn, tc]
            g = newest[:, None] - tc - origin
            assert g[live].min() >= 0, "window reaches below the samples kept"
            g = np.where(live, g, 0)
            sr, si = ar + h * xr[g], ai + h * xi[g]
            ar, ai = np.where(live, sr, ar), np.where(live, si, ai)
            t = t + M
    return ar, ai


def _complex(re, im):
    out = np.empty(re.shape, np.complex64)
    out.real, out.imag = re, im
    return out


class Stream:
    """The model with the handle's call rule and the handle's state: it keeps the newest T' - 1
    converted samples between calls (T' = T, or Tp on the rational path), zeros at the start, as the
    device's history buffer does.  ``process(samples)`` returns [M, outputs due in this call]
    complex64.  L None: rfa_pfb_create (newest sample n D + D - 1); else rfa_pfb_create_rational
    (tap row (n D) mod L, newest sample floor(n D / L), ceil(c L / D) outputs after c samples)."""

    def __init__(self, M: int, D: int, taps, L=None):
        taps = np.asarray(taps)
        assert taps.dtype == F32
        self.M, self.D, self.L = M, D, L
        if L is None:
            self.rows = taps.copy()
        else:
            Tp = -(-taps.size // L)
            gp = np.zeros(L * Tp, F32)
            gp[:taps.size] = taps
            self.rows = gp.reshape(Tp, L).T.copy()          # gp[p][t] = g[p + t L]
        self.T = self.rows.shape[-1]
        self.radix = radices(M)
        self.tw = twiddles(self.radix)
        self.reset()

    def reset(self) -> None:
        self.hr = np.zeros(self.T - 1, F32)
        self.hi = np.zeros(self.T - 1, F32)
        self.done = 0                                       # samples consumed

    def _count(self, c: int) -> int:
        return c // self.D if self.L is None else -(-c * self.L // self.D)

    def process(self, samples) -> np.ndarray:
        s = np.asarray(samples, np.complex128)
        xr = np.concatenate([self.hr, s.real.astype(F32)])
        xi = np.concatenate([self.hi, s.imag.astype(F32)])
        assert np.array_equal(xr[self.T - 1:].astype(np.float64), s.real), "samples must hold float32 values"
        origin = self.done - (self.T - 1)
        n = np.arange(self._count(self.done), self._count(self.done + s.size), dtype=np.int64)
        if self.L is None:
            newest, rows = n * self.D + self.D - 1, self.rows
        else:
            newest, rows = n * self.D // self.L, self.rows[(n * self.D) % self.L]
        self.done += s.size
        self.hr, self.hi = xr[xr.size - (self.T - 1):].copy(), xi[xi.size - (self.T - 1):].copy()
        if n.size == 0:
            return np.zeros((self.M, 0), np.complex64)
        ur, ui = fold(xr, xi, origin, rows, newest, self.M)
        yr, yi = dft(ur, ui, self.radix, self.tw)
        return _complex(yr.T, yi.T)
