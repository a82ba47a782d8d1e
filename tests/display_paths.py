"""The case table of the display draw path (rfanalyzer_amd/csrc/display.hip: draw_rows_kernel and
draw_finish_kernel; the viewport arithmetic of rfa_draw_preprocess in engine.hip), shared by
tests/test_display_paths_host.py (CPU: every case's claimed property and the table's coverage, from
``geometry`` alone) and tests/test_gpu_display_paths.py (GPU: every case bit for bit against the
restated draw thread, oracle/display.py Surface, on the engine's own ring and peaks).

A case exists for one property -- how many bins a pixel takes, which pixels are drawn, how the
ring row is stored, where the colour index clamps.  ``geometry`` restates the viewport lines of
AnalyzerSurface.kt:647-671 and the pixel range of :694 in Kotlin's types, Int wraparound included,
and is written apart from oracle/display.py so that the host test holds the one against the other.

Centre frequency 100 MHz and rate 2 MHz throughout, as in tests/test_gpu_display.py."""
import functools
import math
from typing import NamedTuple

import numpy as np

import signals
from oracle import display as od

F32 = np.float32
F0, SR = 100_000_000, 2_000_000
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


# ---------------------------------------------------------------- Kotlin arithmetic

def _int(x: int) -> int:
    """Kotlin Int: wraps to 32 bits."""
    return (x + 2 ** 31) % 2 ** 32 - 2 ** 31


def _to_int(x) -> int:
    """Double.toInt() / Float.toInt(): truncation, NaN -> 0, saturating."""
    x = float(x)
    if math.isnan(x):
        return 0
    return INT_MAX if x >= INT_MAX else INT_MIN if x <= INT_MIN else int(x)


class Geometry(NamedTuple):
    start: int
    end: int
    samples_per_px: np.float32
    first_pixel: int
    last_pixel: int
    lo: int                 # firstPixel + 1 and lastPixel - 1 as Kotlin computes them: pixel i is
    hi: int                 # drawn when lo <= i < hi
    drawn: range            # the drawn pixels of 0 .. width - 1
    hist: dict              # bins per drawn pixel -> number of such pixels
    below_zero: int         # drawn pixels whose first bin index j + start is negative

    @property
    def span(self) -> int:
        return self.end - self.start


@functools.lru_cache(maxsize=None)
def geometry(n: int, frequency: int, sample_rate: int, width: int, vf: int, vsr: int) -> Geometry:
    """AnalyzerSurface.kt:647-652,668,671 and the range and bin loop of :694,699-700."""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        samples_per_hz = F32(n) / F32(sample_rate)                                               # :647
        frequency_diff, sample_rate_diff = vf - frequency, vsr - sample_rate                     # :648-649 (Long)
        start = _to_int((frequency_diff - sample_rate_diff / 2.0) * float(samples_per_hz))       # :650 (Double)
        end = _int(n + _to_int((frequency_diff + sample_rate_diff / 2.0) * float(samples_per_hz)))  # :651
        spp = F32(_int(end - start)) / F32(width)                                                # :652
        first = 0 if start >= 0 else _to_int(F32(_int(start * -1)) / spp)                        # :668
        last = _to_int(F32(_int(n - start)) / spp) if end >= n else _to_int(F32(_int(end - start)) / spp)  # :671
        lo, hi = _int(first + 1), _int(last - 1)                                                 # :694
        drawn = range(min(max(lo, 0), width), min(max(hi, 0), width))
        if len(drawn) == 0:
            drawn = range(0, 0)
        hist, below = {}, 0
        for i in drawn:
            j = _to_int(F32(i) * spp)                                                            # :699
            top = F32(i + 1) * spp
            below += j + start < 0
            c = 0
            while F32(j) < top and j + start < n:                                                # :700
                c += 1
                j += 1
            hist[c] = hist.get(c, 0) + 1
    return Geometry(start, end, spp, first, last, lo, hi, drawn, hist, below)


def colormap(size: int) -> np.ndarray:
    """``size`` distinct colours, none of them the margin's black (0xff000000): a clamp to either
    end, NaN -> entry 0 and a pixel outside the drawn range all look different."""
    return (0x01000000 + np.arange(size)).astype(np.uint32)


# ---------------------------------------------------------------- comparison

def _bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def assert_draw_same(got, exp, what=""):
    """Bit for bit: colours; path y and peak-hold y as int32 where not NaN, NaN at the same places
    (host and device default NaNs differ in sign and payload); autoscale min and max as float32 bit
    patterns, so -0 is not +0, with NaN matched by isnan."""
    colors, path, pk, mm = got
    c2, p2, k2, mm2 = exp
    assert colors.shape == c2.shape and colors.dtype == c2.dtype == np.uint32, (what, colors.shape, c2.shape)
    np.testing.assert_array_equal(colors, c2, err_msg=f"{what}: colours")
    assert (pk is None) == (k2 is None), what
    for name, a, b in (("path_y", path, p2), ("peaks_y", pk, k2)):
        if a is None:
            continue
        assert a.shape == b.shape, (what, name)
        na, nb = np.isnan(a), np.isnan(b)
        assert np.array_equal(na, nb), f"{what}: {name} NaN at {np.flatnonzero(na != nb)[:8]}"
        bad = np.flatnonzero(_bits(a)[~na] != _bits(b)[~nb])
        assert bad.size == 0, (f"{what}: {name} differs at {bad.size} pixels, first "
                               f"{np.flatnonzero(~na)[bad[0]]}: {a[~na][bad[0]]!r} != {b[~nb][bad[0]]!r}")
    for name, a, b in (("autoscale min", mm[0], mm2[0]), ("autoscale max", mm[1], mm2[1])):
        a, b = F32(a), F32(b)
        if np.isnan(a) or np.isnan(b):
            assert np.isnan(a) and np.isnan(b), f"{what}: {name} {a!r} != {b!r}"
        else:
            assert _bits(a) == _bits(b), f"{what}: {name} {a!r} != {b!r}"


# ---------------------------------------------------------------- the table

class Case(NamedTuple):
    group: str
    name: str
    why: str
    n: int
    width: int
    vf: int
    vsr: int
    fmt: str = "s8"
    ring_rows: int = 5
    L: int = 2               # average_length: at most L + 6 rows per draw
    min_db: float = -110.0
    max_db: float = -20.0
    fft_height: int = 480
    cmap: object = 256       # colormap(size), or "gqrx"
    peaks: bool = True
    residues: int = 1        # ring_order the engine must report
    natural: bool = True     # ring_positions() is arange(N)

    @property
    def id(self):
        return f"{self.group}-{self.name}"

    def geometry(self) -> Geometry:
        return geometry(self.n, F0, SR, self.width, self.vf, self.vsr)

    def colormap(self) -> np.ndarray:
        return od.gqrx_colormap() if self.cmap == "gqrx" else colormap(self.cmap)

    def draw_args(self) -> dict:
        return dict(width=self.width, fft_height=self.fft_height, viewport_frequency=self.vf,
                    viewport_sample_rate=self.vsr, min_db=self.min_db, max_db=self.max_db, average_length=self.L,
                    colormap=self.colormap())

    @property
    def frames(self) -> int:
        """Enough to wrap the ring and leave the write index mid-ring (one frame fewer above 128 K,
        where making the signal is what takes the time)."""
        return self.ring_rows + (2 if self.n <= 131072 else 1)

    @property
    def draws(self) -> int:
        """Draws until every row is refreshed: L + 6 rows by the first, then the L + 1 averaged
        rows again and 5 more each (AnalyzerSurface.kt:683-686)."""
        return 1 + -(-max(0, self.ring_rows - (self.L + 6)) // 5)


GROUPS = ("zoom-in", "widths", "margins", "sub-bin", "ring order", "vertical scale")


def _table():
    z = lambda name, why, n, w, vf, vsr, **kw: Case("zoom-in", name, why, n, w, vf, vsr, **kw)
    cases = [
        # R = 12 > L + 6 = 9: these converge over two draws
        z("2048-w1080-sr8", "the application's case: spp 0.24, one bin for most pixels, two for the rest",
          2048, 1080, F0 + 150_000, SR // 8, ring_rows=12, L=3),
        z("2048-w1080-sr64", "spp 0.03: a bin repeated over 33 pixels, an odd negative offset",
          2048, 1080, F0 - 300_001, SR // 64, ring_rows=12, L=3),
        z("256-w1000-full", "the smallest rows, full span, spp 0.256", 256, 1000, F0, SR),
        z("2048-w2049-full", "spp just below 1: no bin repeats, every pixel takes two and shares one with its "
          "neighbour", 2048, 2049, F0, SR),
        z("512-w2049-full", "spp 0.25 over three passes of the finish loop", 512, 2049, F0, SR),
    ]
    cases += [Case("widths", f"w{w}", why, 2048, w, F0, SR) for w, why in (
        (1, "nothing drawn: the one pixel is the margin"), (2, "nothing drawn"), (3, "one pixel drawn"),
        (4, "two pixels drawn"), (257, "one thread in the second 256-thread block"),
        (1025, "one pixel in the second pass of the 1024-thread finish loop"),
        (2049, "a third pass of the finish loop, a ninth block"))]
    m = lambda name, why, vf, vsr: Case("margins", name, why, 2048, 500, vf, vsr)
    cases += [
        m("right-half", "centre at +SR/2: the right half is black", F0 + SR // 2, SR),
        m("left-half", "centre at -SR/2: the left half is black", F0 - SR // 2, SR),
        m("right-of-span", "centre at +2 SR: all black, autoscale (10, -100)", F0 + 2 * SR, SR),
        m("left-of-span", "centre at -2 SR: all black, autoscale (10, -100)", F0 - 2 * SR, SR),
        m("both", "viewport 4 SR wide: black on both sides", F0, 4 * SR),
    ]
    s = lambda name, why, w, vf, vsr: Case("sub-bin", name, why, 256, w, vf, vsr)
    cases += [
        s("right-wrap", "start == end > N: lastPixel is Int.MIN_VALUE, lastPixel - 1 wraps to Int.MAX_VALUE and every "
          "pixel from 1 is drawn from no bins", 1021, 102_323_281, 5509),
        s("left-wrap", "start == end < 0: firstPixel is Int.MAX_VALUE, firstPixel + 1 wraps to Int.MIN_VALUE; "
          "lastPixel - 1 is -1, so nothing is drawn", 39, 98_706_951, 7600),
        s("two-bins", "a 1 Hz viewport: end - start == 2", 500, F0, 1),
    ]
    r = lambda name, why, n, w, vf, vsr, **kw: Case("ring order", name, why, n, w, vf, vsr, ring_rows=3, L=1, **kw)
    cases += [
        r("32K-full", "store tiles with one residue: ring_order 1 and still permuted", 32768, 1111, F0, SR,
          residues=1, natural=False),
        r("64K-full", "store tiles with two residues", 65536, 1111, F0, SR, residues=2, natural=False),
        r("64K-full-f32", "the same order written from f32 input", 65536, 1111, F0, SR, fmt="f32", residues=2,
          natural=False),
        r("256K-zoom", "column blocks, lr = 3", 262144, 1000, F0 + 777_777, SR // 128, residues=8, natural=False),
        r("256K-edge", "column blocks, start < 0: the left margin", 262144, 1000, F0 - SR // 2, SR // 128, residues=8,
          natural=False),
        r("1M-zoom", "column blocks, lr = 5", 1 << 20, 1000, F0 + 777_777, SR // 512, residues=32, natural=False),
        r("1M-edge", "column blocks, start < 0: the left margin", 1 << 20, 1000, F0 - SR // 2, SR // 512, residues=32,
          natural=False),
    ]
    v = lambda name, why, **kw: Case("vertical scale", name, why, 2048, 333, F0, SR, **kw)
    cases += [
        v("flat", "min_db == max_db between the noise and the tone: scale and dbWidth are +inf", min_db=-25.0,
          max_db=-25.0),
        v("height-0", "fft_height == 0: dbWidth 0, y is -0 or +0", fft_height=0),
        v("flat-height-0", "min_db == max_db and fft_height == 0: dbWidth is 0 / 0", min_db=-25.0, max_db=-25.0,
          fft_height=0),
        v("all-bottom", "min_db above every value: every drawn pixel is entry 0", min_db=50.0, max_db=60.0),
        v("all-top", "max_db below every value: every drawn pixel is the last entry", min_db=-400.0, max_db=-300.0),
        v("cmap-1", "a colour map of one entry", cmap=1),
        v("cmap-2", "a colour map of two entries", cmap=2),
        v("cmap-1000", "a colour map larger than 256", cmap=1000, min_db=-120.0, max_db=0.0),
        v("gqrx", "the application's map", cmap="gqrx"),
        v("no-peaks", "peaks_y == nullptr on the C ABI", peaks=False),
    ]
    return cases


ALL = _table()
BY_ID = {c.id: c for c in ALL}
assert len(BY_ID) == len(ALL)


def coverage(cases) -> dict:
    """What the table runs, from ``geometry``'s answers alone."""
    cov = {"groups": set(), "bins": set(), "blocks": set(), "finish_passes": set(), "margins": set(), "wraps": set(),
           "spans": set(), "sizes": set()}
    for c in cases:
        g = c.geometry()
        cov["groups"].add(c.group)
        cov["bins"] |= set(g.hist)
        cov["blocks"].add(-(-c.width // 256))
        cov["finish_passes"].add(-(-c.width // 1024))
        if len(g.drawn) == 0:
            cov["margins"].add("empty")
        else:
            if g.drawn[0] > 1:
                cov["margins"].add("left")
            if g.drawn[-1] < c.width - 2:
                cov["margins"].add("right")
        if g.first_pixel == INT_MAX:
            cov["wraps"].add("first_pixel + 1")
        if g.last_pixel == INT_MIN:
            cov["wraps"].add("last_pixel - 1")
        cov["spans"].add(min(g.span, 3))
        cov["sizes"].add(c.n)
    return cov


# ---------------------------------------------------------------- data

TONES = ((0.13, 0.4), (0.31, 0.02))


@functools.lru_cache(maxsize=None)
def frames(n: int, count: int, fmt: str, seed: int = 21) -> bytes:
    """``count`` frames of two tones in noise: a finite spectrum spread over some 70 dB."""
    return signals.frames_bytes(n, count, fmt, seed=seed, tones=TONES, noise=0.03)
