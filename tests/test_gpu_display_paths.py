"""GPU: every path of the display draw kernels (rfanalyzer_amd/csrc/display.hip draw_rows_kernel,
draw_finish_kernel; rfa_draw_preprocess) bit for bit against the restated draw thread
(oracle/display.py Surface) on the engine's own ring() and peaks() -- the case table of
tests/display_paths.py (zoomed-in viewports, width edges, margins, viewports narrower than a bin,
every ring order, the ends of the vertical scale), rows holding NaN and +-inf, and draws across
set_ring_rows / set_fft_size.  tests/test_display_paths_host.py proves on the CPU that each case
has the property it is named for; what depends on the rows themselves is asserted here from the
restatement's answers."""
import numpy as np
import pytest

import display_paths as dp
from oracle import display as od

pytestmark = pytest.mark.gpu

F32 = np.float32
F0, SR = dp.F0, dp.SR


def _engine(rfa, n, fmt, ring_rows, window="blackman"):
    e = rfa.SpectrumEngine(n, window, fmt, avg="none", peak_hold=True, ring_rows=ring_rows)
    e.set_tuning(F0, SR)
    return e


def _both(e, surf, args, peaks=True, what=""):
    """One draw on the device and on the restated draw thread, compared; returns the restatement's."""
    ring, ri, _ = e.ring()
    got = e.draw_preprocess(peaks=peaks, **args)
    with np.errstate(all="ignore"):
        exp = surf.draw(ring, ri, e.peaks() if peaks else None, F0, SR, **args)
    dp.assert_draw_same(got, exp, what)
    return exp


# ---------------------------------------------------------------- 1. the table

@pytest.mark.parametrize("c", [pytest.param(c, id=c.id) for c in dp.ALL])
def test_table_case(rfa, c):
    g, cmap = c.geometry(), c.colormap()
    with _engine(rfa, c.n, c.fmt, c.ring_rows) as e:
        e.process(dp.frames(c.n, c.frames, c.fmt), c.frames, rows=False)
        pos = e.ring_positions()
        assert e.ring_order == c.residues, (c.id, e.ring_order)
        assert np.array_equal(np.sort(pos), np.arange(c.n))
        assert np.array_equal(pos, np.arange(c.n)) == c.natural, c.id
        ring = e.ring()[0]
        assert np.isfinite(ring).all() and not (ring == F32(-9999.0)).any()  # the ring has wrapped
        surf = od.Surface(c.ring_rows)
        for k in range(c.draws):
            colors, path, pk, (mn, mx) = _both(e, surf, c.draw_args(), c.peaks, f"{c.id} draw {k}")
            assert (colors != 0).all(axis=1).sum() == min(c.ring_rows, c.L + 6 + 5 * k), (c.id, k)
        assert not surf.dirty.any()
    # what the case is there for, on the restatement's last answer
    drawn = np.zeros(c.width, bool)
    drawn[g.drawn.start:g.drawn.stop] = len(g.drawn) > 0
    assert (colors[:, ~drawn] == od.BLACK).all() and np.isnan(path[~drawn]).all()
    assert (pk is None) == (not c.peaks) and (pk is None or (pk[~drawn] == -1).all())
    if c.cmap != "gqrx":
        assert (colors[:, drawn] != od.BLACK).all() and np.isin(colors[:, drawn], cmap).all()
    if len(g.drawn) == 0:
        assert (mn, mx) == (10.0, -100.0)
    elif c.name == "right-wrap":
        assert (colors[:, drawn] == cmap[0]).all() and np.isnan(mn) and np.isnan(mx) and np.isnan(pk[drawn]).all()
    else:
        assert mn <= mx and np.isfinite([mn, mx]).all()
    if c.group == "vertical scale":
        idx = colors[:, drawn].astype(np.int64) - 0x01000000
        if c.name == "all-bottom":
            assert (idx == 0).all()
        elif c.name == "all-top":
            assert (idx == c.cmap - 1).all()
        elif c.name == "cmap-1000":
            assert idx.max() > 255 and len(np.unique(idx)) > 50  # the map is used, beyond 256 entries too
        elif c.name == "flat":          # scale = +inf: below min_db entry 0, above it the last one
            assert set(np.unique(idx)) == {0, c.cmap - 1} and np.isinf(path[drawn]).all()
        elif c.name == "height-0":      # y = 0 - (ta - min) * 0: a zero of either sign
            assert (path[drawn] == 0).all()
        elif c.name == "flat-height-0":
            assert np.isnan(path).all()


# ---------------------------------------------------------------- 2. non-finite rows

def _non_finite_frames(n):
    """The frames of tests/test_gpu_window_stats.py test_non_finite_rows, plain ones between them,
    in the order that puts each mix into the three averaged rows: a silent frame (a row of -inf)
    before the one scaled by 2^70 (+inf bins), so that the draw after it adds +inf to -inf; the
    frame with one NaN sample (a row of NaN); a constant one (window none: -inf in every bin but
    one).  The scaled frame overflows in most bins, so one frame is added to the recipe: a tone of
    amplitude 2^67 on a bin centre, +inf in its own few bins and rounding noise elsewhere.  It comes
    after a second silent frame and before the last plain one, so that the last state is NaN in a
    few pixels and -inf in all the others."""
    rng = np.random.default_rng(12)
    plain = (rng.standard_normal((7, 2 * n)) * 0.1).astype(np.float32)
    silent = np.zeros(2 * n, np.float32)
    with_nan = plain[5].copy()
    with_nan[2 * (n // 3)] = np.nan
    scaled = plain[6] * F32(2.0 ** 70)
    constant = np.full(2 * n, 0.5, np.float32)
    tone = 2.0 ** 67 * np.exp(2j * np.pi * (n // 8 + 3) * np.arange(n) / n)
    spike = np.empty(2 * n, np.float32)
    spike[0::2], spike[1::2] = tone.real, tone.imag
    return [("plain", plain[0]), ("silent", silent), ("scaled", scaled), ("plain", plain[1]), ("nan", with_nan),
            ("plain", plain[2]), ("constant", constant), ("plain", plain[3]), ("silent", silent), ("spike", spike),
            ("plain", plain[4])]


@pytest.mark.parametrize("window", ["none", "blackman"])
def test_non_finite_rows(rfa, window):
    """f32 input, one frame at a time, a draw after each (width 300, L = 2, peaks): rows of -inf,
    NaN and +inf bins through the pixel mean, the time average summed newest first, Math.min / max
    (NaN wins) and the colour index (NaN -> entry 0).  Then the last state again at width 2049:
    three passes of the finish loop, the few NaN pixels in other waves than the -inf ones."""
    n, R, L = 4096, 8, 2
    args = dict(width=300, fft_height=480, viewport_frequency=F0, viewport_sample_rate=SR, min_db=-110.0,
                max_db=-20.0, average_length=L, colormap=dp.colormap(256))
    seen = set()
    with _engine(rfa, n, "f32", R, window) as e:
        surf = od.Surface(R)
        kinds = []
        for k, (kind, x) in enumerate(_non_finite_frames(n)):
            e.process(x.tobytes(), 1, rows=False)
            ring, ri, _ = e.ring()
            surf.mark_row(ri)
            kinds.insert(0, kind)
            colors, path, pk, (mn, mx) = _both(e, surf, args, True, f"window {window} frame {k} ({kind})")
            if np.isnan(mn) and np.isnan(mx):
                seen.add("NaN autoscale")
            if np.isneginf(mn) and np.isfinite(mx):
                seen.add("-inf min, finite max")
            if np.isposinf(path).any():
                seen.add("+inf path y")
            # per row and pixel, the pixel mean the average adds: the restated draw of that row alone
            if kinds[:3] == ["scaled", "silent", "plain"]:
                alone = dict(args, average_length=0)
                with np.errstate(all="ignore"):
                    one = [od.draw_preprocess(ring[(ri + r) % R][None], 0, None, F0, SR, **alone)[1] for r in range(2)]
                mean = [(F32(480) - y) for y in one]  # y = 480 - (mean + 110) * dbWidth: same infinities, sign flipped
                mixed = np.isposinf(mean[0]) & np.isneginf(mean[1])
                assert np.isneginf(ring[(ri + 1) % R]).all() and np.isposinf(ring[ri]).any()
                assert mixed.any() and np.isnan(path[mixed]).all() and np.isposinf(path[~mixed][1:-1]).all()
                seen.add("inf - inf")
        assert seen == {"NaN autoscale", "-inf min, finite max", "+inf path y", "inf - inf"}, seen
        wide = dict(args, width=2049)
        colors, path, pk, (mn, mx) = _both(e, surf, wide, True, f"window {window} width 2049")
        assert kinds[:3] == ["plain", "spike", "silent"]
        nan_at = np.flatnonzero(np.isnan(path[1:-1])) + 1
        waves = {(int(p) % 1024) // 64 for p in nan_at}   # pixel p is thread p % 1024 of the finish kernel
        assert 0 < nan_at.size < 2047 and len(waves) < 16, (nan_at.size, waves)
        assert np.isposinf(np.delete(path, nan_at)[1:-1]).all()  # time average -inf: y = +inf
        assert np.isnan(mn) and np.isnan(mx)


# ---------------------------------------------------------------- 3. size changes

def test_draws_across_ring_and_fft_size_changes(rfa):
    """set_ring_rows reallocates the ring and the colour buffer and marks every row
    (FftProcessor.kt:185-195); set_fft_size starts a new ring in another storage order (natural at
    2048, store tiles at 32 K) while the draw thread's colour buffer, of the same width and row
    count, lives on (AnalyzerSurface.kt:620-627): rows the first draws after it do not reach keep
    the colours of the old size."""
    args = dict(width=333, fft_height=480, viewport_frequency=F0 + 150_000, viewport_sample_rate=SR // 3,
                min_db=-110.0, max_db=-20.0, average_length=3, colormap=dp.colormap(256))
    seed = [50]
    with _engine(rfa, 2048, "s8", 12) as e:
        surf = od.Surface(12)

        def feed(k):
            seed[0] += 1
            e.process(dp.frames(e.n, k, "s8", seed[0]), k, rows=False)
            R, ri = e.ring()[0].shape[0], e.ring()[1]
            if surf.dirty.size != R:
                surf.mark_all(R)
            for j in range(min(k, R)):
                surf.mark_row((ri + j) % R)
            return R

        def draw(what):
            return _both(e, surf, args, True, what)[0]

        feed(14)
        draw("R = 12, first draw")          # 9 of 12 rows
        e.set_ring_rows(5)
        assert feed(2) == 5
        c = draw("R = 5")
        assert c.shape == (5, 333) and (c != 0).all()
        e.set_ring_rows(16)
        assert feed(3) == 16                # 3 new rows, 5 kept, 8 of the fill
        c = draw("R = 16, first draw")      # L + 6 = 9 rows
        assert ((c != 0).all(axis=1).sum(), (c == 0).all(axis=1).sum()) == (9, 7)
        c16 = draw("R = 16, second draw")   # the 4 averaged rows and 5 more
        assert ((c16 != 0).all(axis=1).sum(), (c16 == 0).all(axis=1).sum()) == (14, 2)
        assert e.ring_order == 1 and np.array_equal(e.ring_positions(), np.arange(2048))
        e.set_fft_size(32768)
        e.set_tuning(F0, SR)
        surf.mark_all(16)
        assert feed(2) == 16 and e.n == 32768
        assert not np.array_equal(e.ring_positions(), np.arange(32768))
        c = draw("N = 32 K, first draw")
        stale = (c == c16).all(axis=1)
        assert stale.sum() == 7             # the rows not refreshed yet still show the 2048-point colours
        assert (c[stale] != 0).any()
        draws = 1
        while surf.dirty.any():
            c = draw(f"N = 32 K, draw {draws + 1}")
            draws += 1
            assert draws <= 3               # 9 rows, then 5 and 2 beside the averaged ones
        assert draws == 3 and (c != 0).all() and not (c == c16).all(axis=1).any()
        feed(1)
        draw("N = 32 K, a new row")
