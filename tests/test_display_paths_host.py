"""CPU: the host side of tests/test_gpu_display_paths.py, so that the GPU module cannot pass for a
reason of its own -- every case of the table (tests/display_paths.py) has the property it is there
for, and the table covers its six groups, both from ``geometry`` alone (a restatement of
AnalyzerSurface.kt:647-671,694 in Kotlin's Int arithmetic); ``geometry`` and the restated draw
(oracle/display.py) agree on which pixels are drawn; the draw follows Kotlin where a bound of the
pixel range wraps; the comparison helper tells -0 from +0 and accepts an expected NaN."""
import numpy as np
import pytest

import display_paths as dp
from oracle import display as od

F32 = np.float32
F0, SR = dp.F0, dp.SR


def _cases(group):
    return [pytest.param(c, id=c.id) for c in dp.ALL if c.group == group]


def _share(g, bins):
    return g.hist.get(bins, 0) / len(g.drawn)


# ---------------------------------------------------------------- geometry by hand

def test_geometry_of_the_issue_example():
    """N = 2048, width 1080, an eighth of the span at +150 kHz: samplesPerHz is float32(2048 / 2e6),
    just below 0.001024, start = int((150 000 + 875 000) * that) = 1049, end = 2048 + int(-725 000 *
    that) = 2048 - 742 = 1306, so 257 bins over 1080 pixels: spp 0.238, pixels 1 .. 1078 drawn, 822
    with one bin and 256 with two."""
    g = dp.geometry(2048, F0, SR, 1080, F0 + 150_000, SR // 8)
    assert (g.start, g.end, g.first_pixel, g.last_pixel) == (1049, 1306, 0, 1080)
    assert g.samples_per_px == F32(257) / F32(1080)
    assert g.drawn == range(1, 1079) and g.hist == {1: 822, 2: 256} and g.below_zero == 0


def test_geometry_of_a_zoomed_out_viewport():
    """The viewport of tests/test_display_oracle.py: N = 1024, width 200, twice the span.  start is
    -511, not -512 (the float32 quotient is just below 0.000512), end 1024 + 511.  10.23 bins per
    pixel counted from the truncated j = (i * spp).toInt() up to (i + 1) * spp: 11 or 12 of them."""
    g = dp.geometry(1024, F0, SR, 200, F0, 2 * SR)
    assert (g.start, g.end) == (-511, 1535) and g.samples_per_px == F32(2046) / F32(200)
    assert g.first_pixel == int(F32(511) / g.samples_per_px) == 49
    assert g.last_pixel == int(F32(1535) / g.samples_per_px) == 150
    assert g.drawn == range(50, 149) and set(g.hist) == {11, 12}


# ---------------------------------------------------------------- every case's property

@pytest.mark.parametrize("c", _cases("zoom-in"))
def test_zoom_in_cases(c):
    """Most pixels repeat a bin, and (float)j < hi gives some of them a second one."""
    g = c.geometry()
    assert g.samples_per_px < 1 and g.span > 2, (c.id, g)
    assert len(g.drawn) >= c.width - 3 and g.below_zero == 0  # (lastPixel may truncate one short)
    if c.name == "2048-w2049-full":
        # spp just below 1 does not repeat bins: j = (i * spp).toInt() = i - 1 and (i + 1) * spp is
        # above i, so every pixel takes bins i - 1 and i and shares one with its neighbour
        assert g.samples_per_px == F32(2048) / F32(2049) and g.hist == {2: 2047}, (c.id, g.hist)
    else:
        assert _share(g, 1) >= 0.70 and g.hist.get(2, 0) >= 1 and set(g.hist) == {1, 2}, (c.id, g.hist)


def test_zoom_in_spans():
    """The cases by hand: 257 and 33 bins (an eighth and a 64th of 2048, the ends truncated apart),
    256 over 1000, 512 over 2049 (a quarter of the pixels start a new bin before the last one ends),
    and 2048 over 2049, where every pixel takes two."""
    spans = {c.name: (c.geometry().span, c.geometry().hist) for c in dp.ALL if c.group == "zoom-in"}
    assert spans["2048-w1080-sr8"] == (257, {1: 822, 2: 256})
    assert spans["2048-w1080-sr64"][0] == 33 and spans["2048-w1080-sr64"][1][1] > 1000
    assert spans["256-w1000-full"][0] == 256
    assert spans["512-w2049-full"][0] == 512 and spans["512-w2049-full"][1][1] > 0.7 * 2047
    assert spans["2048-w2049-full"] == (2048, {2: 2047})


@pytest.mark.parametrize("c", _cases("widths"))
def test_width_cases(c):
    """Full span: pixels 1 .. width - 2 are drawn, so widths 1 and 2 draw nothing and 3 draws one;
    257, 1025 and 2049 put one pixel into a further 256-thread block or finish pass."""
    g = c.geometry()
    assert (g.start, g.end, g.first_pixel, g.last_pixel) == (0, c.n, 0, c.width), (c.id, g)
    assert g.drawn == (range(1, c.width - 1) if c.width > 2 else range(0)), (c.id, g.drawn)


def test_width_edges():
    w = sorted(c.width for c in dp.ALL if c.group == "widths")
    assert w == [1, 2, 3, 4, 257, 1025, 2049]
    assert [-(-x // 256) for x in (257, 2049)] == [2, 9] and [-(-x // 1024) for x in (1025, 2049)] == [2, 3]


@pytest.mark.parametrize("c", _cases("margins"))
def test_margin_cases(c):
    g = c.geometry()
    empty = len(g.drawn) == 0
    assert g.first_pixel > 0 or g.last_pixel < c.width or empty, (c.id, g)
    # black pixels on each side, beyond the one or two that truncation takes from a full span
    left, right = (g.drawn.start, c.width - g.drawn.stop) if not empty else (0, 0)
    if c.name in ("right-of-span", "left-of-span"):
        assert empty and g.samples_per_px > 1, (c.id, g)  # (a positive span, not a sub-bin viewport)
        assert (g.start > c.n) == (c.name == "right-of-span") and (g.end < 0) == (c.name == "left-of-span")
    elif c.name == "right-half":
        assert left == 1 and 0.45 * c.width < right < 0.55 * c.width and g.end > c.n, (c.id, g)
    elif c.name == "left-half":
        assert right <= 2 and 0.45 * c.width < left < 0.55 * c.width and g.start < 0, (c.id, g)
    else:
        assert c.name == "both" and g.start < 0 and g.end > c.n, (c.id, g)
        assert 0.3 * c.width < left < 0.45 * c.width and 0.3 * c.width < right < 0.45 * c.width, (c.id, g)
    assert g.below_zero == 0


@pytest.mark.parametrize("c", _cases("sub-bin"))
def test_sub_bin_cases(c):
    g = c.geometry()
    assert g.samples_per_px == 0 or g.span <= 2, (c.id, g)
    if c.name == "right-wrap":      # (N - start) / 0 = -inf -> Int.MIN_VALUE; - 1 wraps
        assert g.start == g.end > c.n and g.samples_per_px == 0
        assert (g.first_pixel, g.last_pixel, g.lo, g.hi) == (0, dp.INT_MIN, 1, dp.INT_MAX)
        assert g.drawn == range(1, c.width) and g.hist == {0: c.width - 1}
    elif c.name == "left-wrap":     # -start / 0 = +inf -> Int.MAX_VALUE; + 1 wraps; 0 / 0 -> 0
        assert g.start == g.end < 0 and g.samples_per_px == 0
        assert (g.first_pixel, g.last_pixel, g.lo, g.hi) == (dp.INT_MAX, 0, dp.INT_MIN, -1)
        assert len(g.drawn) == 0
    else:
        assert g.span == 2 and 0 <= g.start and g.end <= c.n and len(g.drawn) >= c.width - 3
        assert set(g.hist) == {1} and g.samples_per_px == F32(2) / F32(c.width)


@pytest.mark.parametrize("c", _cases("ring order"))
def test_ring_order_cases(c):
    """The sizes of every stored order above natural; nothing above 128 K draws a full span (the
    restatement is pure Python); each column-block size has a viewport inside the span and one
    whose left part is off it."""
    g = c.geometry()
    assert c.n >= 32768 and not c.natural and (c.ring_rows, c.L) == (3, 1)
    if c.n > 131072:
        assert g.span <= 2100 and len(g.drawn) > 0.4 * c.width, (c.id, g)
        assert (g.start < 0) == c.name.endswith("edge") and (g.first_pixel > 0) == c.name.endswith("edge")
        assert g.below_zero == 0
    else:
        assert (g.start, g.end) == (0, c.n) and c.width == 1111


def test_ring_order_sizes():
    by_n = {}
    for c in dp.ALL:
        if c.group == "ring order":
            by_n.setdefault(c.n, []).append((c.fmt, c.residues))
    assert by_n == {32768: [("s8", 1)], 65536: [("s8", 2), ("f32", 2)], 262144: [("s8", 8)] * 2,
                    1 << 20: [("s8", 32)] * 2}


@pytest.mark.parametrize("c", _cases("vertical scale"))
def test_vertical_scale_cases(c):
    g = c.geometry()
    assert (c.n, c.width) == (2048, 333) and g.drawn == range(1, 332)
    plain = dp.Case("vertical scale", "", "", 2048, 333, F0, SR)
    changed = {f for f in dp.Case._fields if getattr(c, f) != getattr(plain, f)} - {"name", "why"}
    assert changed and changed <= {"min_db", "max_db", "fft_height", "cmap", "peaks"}, (c.id, changed)


def test_vertical_scale_set():
    v = {c.name: c for c in dp.ALL if c.group == "vertical scale"}
    assert v["flat"].min_db == v["flat"].max_db and v["height-0"].fft_height == 0
    assert v["all-bottom"].min_db > 10 and v["all-top"].max_db < -200  # beyond any dB of 8-bit input
    assert {c.cmap for c in v.values()} == {256, 1, 2, 1000, "gqrx"}
    assert [c.name for c in v.values() if not c.peaks] == ["no-peaks"]
    assert [c.id for c in dp.ALL if c.cmap == "gqrx"] == ["vertical scale-gqrx"]


def test_the_table_covers_its_groups():
    cov = dp.coverage(dp.ALL)
    assert cov["groups"] == set(dp.GROUPS)
    assert {0, 1, 2} <= cov["bins"] and max(cov["bins"]) > 32       # no bin, one, two, many
    assert {1, 2, 9} <= cov["blocks"] and cov["finish_passes"] == {1, 2, 3}
    assert cov["margins"] == {"left", "right", "empty"}
    assert cov["wraps"] == {"first_pixel + 1", "last_pixel - 1"}
    assert {0, 2, 3} <= cov["spans"]
    assert cov["sizes"] == {256, 512, 2048, 32768, 65536, 262144, 1 << 20}
    assert {c.draws for c in dp.ALL} == {1, 2}                      # some converge over two draws
    for c in dp.ALL:
        assert c.frames > c.ring_rows and c.L < c.ring_rows, c.id


def test_colormap_is_distinct_and_never_black():
    for size in (1, 2, 256, 1000):
        m = dp.colormap(size)
        assert m.dtype == np.uint32 and m.size == size == np.unique(m).size and od.BLACK not in m
        assert m[0] == 0x01000000


# ---------------------------------------------------------------- geometry against the restated draw

def _draw(c, ring, peaks=None, **kw):
    args = c.draw_args()
    args.update(kw)
    with np.errstate(all="ignore"):
        return od.draw_preprocess(ring, 0, peaks, F0, SR, **args)


@pytest.mark.parametrize("c", [pytest.param(c, id=c.id) for c in dp.ALL if c.n <= 2048])
def test_restated_draw_has_the_geometry_s_pixels(c):
    """One constant row at -61 dB: the restated draw paints exactly ``geometry``'s drawn pixels, the
    rest black with no path point -- two restatements of :647-671,694 written apart."""
    g = c.geometry()
    ring = np.full((1, c.n), -61.0, np.float32)
    colors, path, _, mm = _draw(c, ring, average_length=0)
    drawn = np.zeros(c.width, bool)
    drawn[g.drawn.start:g.drawn.stop] = len(g.drawn) > 0
    np.testing.assert_array_equal(colors[0] != od.BLACK, drawn)  # (-61 dB is past the gqrx map's black entries)
    if 0 in g.hist:                  # no bins: 0 / 0
        assert np.isnan(path).all() and np.isnan(mm).all()
        return
    if not (c.min_db == c.max_db and c.fft_height == 0):  # (dbWidth 0 / 0: every y is NaN)
        np.testing.assert_array_equal(~np.isnan(path), drawn)
    assert mm == ((-61.0, -61.0) if len(g.drawn) else (10.0, -100.0))


def test_kotlin_wraps_last_pixel_minus_one():
    """N = 256, width 1021, viewport 102 323 281 / 5509 on 100 MHz / 2 MHz, by hand from
    AnalyzerSurface.kt.  :647 samplesPerHz = 256f / 2e6f = 1.28e-4.  :650 start = ((2 323 281 -
    (-1 994 491) / 2.0) * samplesPerHz).toInt() = (3 320 526.5 * 1.28e-4).toInt() = 425; :651 end =
    256 + ((2 323 281 - 997 245.5) * samplesPerHz).toInt() = 256 + 169 = 425.  :652 samplesPerPx =
    0f / 1021f = 0.  :668 start >= 0: firstPixel = 0.  :671 end >= fftSize: lastPixel = ((256 -
    425) / 0f).toInt() = (-inf).toInt() = Int.MIN_VALUE.  :694 ``i in (firstPixel + 1)..<lastPixel-1``:
    Int.MIN_VALUE - 1 wraps to Int.MAX_VALUE, so the range is 1 ..< Int.MAX_VALUE and every pixel but
    0 takes the first branch.  :699-700 j = (i * 0f).toInt() = 0 and ``0 < (i + 1) * 0f`` is false:
    no bin is read, counter stays 0.  :706 avg = 0f / 0 = NaN.  :707 the peak y is NaN.  :713-717
    timeAverage is NaN: the path y is NaN, Math.min / max return NaN.  :722-723 NaN.toInt() = 0:
    colormap[0].  :725 pixel 0 is black, its peak y -1."""
    c = dp.BY_ID["sub-bin-right-wrap"]
    assert (c.n, c.width, c.vf, c.vsr) == (256, 1021, 102_323_281, 5509)
    ring = np.random.default_rng(3).uniform(-90, -10, (4, c.n)).astype(np.float32)
    colors, path, peaks_y, (mn, mx) = _draw(c, ring, peaks=ring.max(0))
    cmap = c.colormap()
    assert (colors[:, 0] == od.BLACK).all() and (colors[:, 1:] == cmap[0]).all() and cmap[0] != od.BLACK
    assert np.isnan(path).all() and peaks_y[0] == -1 and np.isnan(peaks_y[1:]).all()
    assert np.isnan(mn) and np.isnan(mx)


def test_kotlin_wraps_first_pixel_plus_one():
    """N = 256, width 39, viewport 98 706 951 / 7600: :650 start = ((-1 293 049 + 996 200) * 1.28e-4)
    .toInt() = (-37.997).toInt() = -37, :651 end = 256 + (-2 289 249 * 1.28e-4).toInt() = 256 - 293 =
    -37, samplesPerPx = 0, :668 firstPixel = (37 / 0f).toInt() = Int.MAX_VALUE and firstPixel + 1
    wraps to Int.MIN_VALUE; :671 end < fftSize: lastPixel = (0 / 0f).toInt() = NaN.toInt() = 0, so
    the range Int.MIN_VALUE ..< -1 holds no pixel: all black, autoscale untouched."""
    c = dp.BY_ID["sub-bin-left-wrap"]
    g = c.geometry()
    assert (g.start, g.end) == (-37, -37)
    ring = np.full((2, c.n), -50.0, np.float32)
    colors, path, peaks_y, mm = _draw(c, ring, peaks=ring[0])
    assert (colors == od.BLACK).all() and np.isnan(path).all() and (peaks_y == -1).all() and mm == (10.0, -100.0)


# ---------------------------------------------------------------- the clamp is defensive

def test_no_positive_span_reaches_a_negative_bin_or_an_empty_pixel():
    """The kernel's ``if (j + a.start < 0) j = -a.start`` (the reference would throw there) and a
    drawn pixel with no bin: a seeded search of 4000 small geometries with a positive bin span finds
    neither, which is why the table has no case for them."""
    rng = np.random.default_rng(2024)
    seen = 0
    for _ in range(4000):
        n = 1 << int(rng.integers(4, 10))
        width = int(rng.integers(1, 300))
        vsr = int(SR * 2.0 ** rng.uniform(-9, 3))
        vf = F0 + int(rng.uniform(-1.5, 1.5) * (SR + vsr) / 2)
        g = dp.geometry.__wrapped__(n, F0, SR, width, vf, vsr)
        if g.span <= 0:
            continue
        seen += 1
        assert g.below_zero == 0 and 0 not in g.hist, (n, width, vf, vsr, g)
    assert seen > 3000


# ---------------------------------------------------------------- the comparison helper

def _result(mn=-50.0, mx=-40.0, y=1.0, pk=2.0, color=5):
    return (np.full((2, 4), color, np.uint32), np.array([np.nan, y, y, np.nan], np.float32),
            None if pk is None else np.array([-1, pk, pk, -1], np.float32), (float(mn), float(mx)))


def test_assert_draw_same_accepts_nan_and_tells_zeros_apart():
    nan = float("nan")
    dp.assert_draw_same(_result(), _result())
    dp.assert_draw_same(_result(mn=nan, mx=nan, y=nan, pk=nan), _result(mn=-nan, mx=nan, y=-nan, pk=nan))
    dp.assert_draw_same(_result(pk=None), _result(pk=None))
    dp.assert_draw_same(_result(mn=-0.0, y=-0.0), _result(mn=-0.0, y=-0.0))
    for bad in (dict(mn=0.0), dict(mn=nan), dict(mx=nan), dict(y=0.0), dict(y=nan), dict(pk=-0.0), dict(pk=None),
                dict(color=6), dict(mx=float(np.nextafter(F32(-40.0), F32(0))))):
        with pytest.raises(AssertionError):
            dp.assert_draw_same(_result(mn=-0.0, y=-0.0, pk=0.0), _result(**{**dict(mn=-0.0, y=-0.0, pk=0.0), **bad}))
