"""Restatement of the frequency meter bank (rfa_freq_*) in plain numpy / Python for
the tests to compare with.  The reference has no counterpart: the checks are this restatement and
bounds derived from it.

R1 = sum of x[i] * conj(x[i-1]): term_re = xr*pr + xi*pi, term_im = xi*pr - xr*pi with the float32
inputs widened to float64.  A product of two float32 values is exact in float64, so each term here is
the exact two-product sum rounded once, as on the device; ``math.fsum`` then adds the terms without
further error.  x[-1] is the carried sample; without one the term for i = 0 is left out."""
import math

import numpy as np

TILE = 16384                            # RFA_FREQ_TILE: n up to this is one launch, above it two
U = 2.0 ** -53


def products(re, im, carry=None):
    """The four product arrays (p1, p2 of the real terms; q1, q2 of the imaginary ones, term_im =
    q1 - q2), float64 and exact.  ``carry``: None or the (re, im) pair that precedes the row."""
    xr = np.asarray(re, np.float32).astype(np.float64)
    xi = np.asarray(im, np.float32).astype(np.float64)
    if carry is None:
        pr, pi, xr, xi = xr[:-1], xi[:-1], xr[1:], xi[1:]
    else:
        pr = np.concatenate([[np.float64(np.float32(carry[0]))], xr[:-1]])
        pi = np.concatenate([[np.float64(np.float32(carry[1]))], xi[:-1]])
    with np.errstate(all="ignore"):
        return xr * pr, xi * pi, xi * pr, xr * pi


def _total(t) -> float:
    if not np.isfinite(t).all():
        with np.errstate(all="ignore"):
            return float(t.sum())
    return math.fsum(t)


def r1(re, im, carry=None):
    """(R1_re, R1_im, terms, bound_re, bound_im): the exactly summed once-rounded terms, their
    number, and the distance the device's double accumulation may lie from each sum:
    (terms + 2) * 2^-53 * sum(|p1| + |p2|) -- one rounding per term and one per addition, each at
    most 2^-53 of a partial result that never exceeds the sum of the products' magnitudes (second-
    order terms are covered by the + 2)."""
    p1, p2, q1, q2 = products(re, im, carry)
    n = len(p1)
    with np.errstate(all="ignore"):
        tr, ti = p1 + p2, q1 - q2
        mag_r = float((np.abs(p1) + np.abs(p2)).sum()) if n else 0.0
        mag_i = float((np.abs(q1) + np.abs(q2)).sum()) if n else 0.0
    return _total(tr), _total(ti), n, (n + 2) * U * mag_r, (n + 2) * U * mag_i


def error_hz(r1_re: float, r1_im: float, rate: float) -> float:
    """atan2(im, re) * rate / (2 pi); 0 for R1 = 0, NaN for a sum that is not finite."""
    if not (math.isfinite(r1_re) and math.isfinite(r1_im)):
        return math.nan
    if r1_re == 0.0 and r1_im == 0.0:
        return 0.0
    return math.atan2(r1_im, r1_re) * rate / (2.0 * math.pi)


def estimator_bound_hz(rate: float) -> float:
    """|error_hz - f0| for a row a[i] * exp(j (theta i + phi)) with real a > 0 stored as float32.
    Every exact lag product has phase theta.  Rounding to float32 moves a sample's phase by at most
    asin(sqrt(2) * 2^-25), so each product of stored samples lies within 2^-23.5 rad of theta, and a
    sum of vectors inside a cone stays inside it; 2^-40 covers the double arithmetic and atan2.
    (Both components sitting at the very top of their rounding intervals would allow 2^-23; the
    figure asserted is the stricter one.)"""
    return rate / (2.0 * math.pi) * (2.0 ** -23.5 + 2.0 ** -40)


def step_round(c: float, step: float) -> float:
    """AfcRule's applied correction: the multiple of ``step`` nearest to c, a tie going up."""
    return step * math.floor(c / step + 0.5)
