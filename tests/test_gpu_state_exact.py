"""GPU: the state kernels checked exactly, on the device's own rows, NaN and inf included.

tests/test_gpu_state.py compares the state with one rebuilt from float64-oracle rows, to
0.01 dB and above the Parseval floor only.  Here the truth is always the rows the device
itself produced (returned by ``process``, read back from the ring, or -- staging path -- the
rows of a second engine fed the same bytes, which the ring must reproduce bit for bit), so
the state arithmetic is checked on its own inputs, on every bin, with no floor:

* ring: the rows bit-identical at ``(-g) mod R`` (write index counting down,
  FftProcessor.kt:226-227), -9999 elsewhere;
* peaks: bit-identical to the NaN-propagating maximum (Math.max, FftProcessor.kt:241-242)
  since the last reset, starting from -999999.  A maximum is exact in any order: no tolerance;
* boxcar: bit-identical to the fp32 sum newest-first divided by L + 1
  (AnalyzerSurface.kt:710-714).  The sum has no product that could contract to an FMA and the
  division is IEEE-rounded, so there is nothing to tolerate; NaN positions compare by mask;
* EMA: against the float64 evaluation of the defined recurrence (oracle/processor.py
  ``ema_reseed``: avg += alpha (x - avg); a non-finite frame makes the average non-finite, a
  non-finite average is re-seeded by the next frame) over the device rows.  NaN, +inf and
  -inf positions must be identical; finite bins must lie within

      ulp32(M) * (1 + 1/alpha),        M = the largest finite |row value| fed.

  Derivation: a step rounds x - em to at most ulp(M) (|x - em| < 2 M), which alpha then scales,
  and rounds the result to at most ulp(M)/2; these errors decay by 1 - alpha per frame, so they
  sum to at most ulp(M) (alpha + 1/2) / alpha = ulp(M) (1 + 1/(2 alpha)).  The chunked scan also
  multiplies the carried average by (1 - alpha)^L formed in fp32, relative error about
  L 2^-24, i.e. at most about ulp(M) / (e alpha) at L = 1/alpha.  Together below the bar.  A CPU
  re-enactment of the kernels' fp32 algebra measured <= 2 ulps at alpha = 0.1 and <= 7 ulps at
  alpha = 0.01 (bars: 11 and 101 ulps), so the bar has >= 5x headroom and is not fitted (the
  device itself: <= 2.3 ulps at 0.1, <= 13 ulps at 0.01; every comparison prints its figure);
* channel means: against the reference's sequential fp32 loop (FftProcessor.kt:150-152) on
  the device rows, ``CHAN_SUM_TOL`` on finite means, non-finite ones by position and kind.

Every update form ``launch_state`` has (fft_kernels.hip) is reached at its smallest shape,
from each row source, with at least two calls so the state carried in is not fresh.  The
non-finite sequences (f32 input, window none: a silent frame is all -inf, a constant frame
-inf in every bin but one, one NaN sample makes the row NaN, noise scaled by 2^70 makes it
+inf) put such frames at the chunk seams of every form and carry a NaN, +inf and -inf
average into the next call; the display and scanner kernels are then run on a ring that
holds such rows, bit-exact against oracle/display.py and oracle/scanner.py.
"""
import numpy as np
import pytest

from oracle import display as od
from oracle import processor
from oracle import scanner as osc
from test_gpu_state import CHAN_SUM_TOL

pytestmark = pytest.mark.gpu

F32 = np.float32
ALPHA = 0.1
BOXCAR_L = 5


# ---------------------------------------------------------------- helpers
def _same_bits(got, exp, what=""):
    """Bit-identical float32 arrays (NaN positions by mask: a NaN has no value to compare)."""
    got, exp = np.asarray(got, F32), np.asarray(exp, F32)
    assert got.shape == exp.shape, what
    nan = np.isnan(exp)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaN positions differ " \
        f"({int(np.isnan(got).sum())} on the device, {int(nan.sum())} expected)"
    bad = got.view(np.int32)[~nan] != exp.view(np.int32)[~nan]
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} values differ"


def _same_kind(got, exp, what=""):
    for kind in (np.isnan, np.isposinf, np.isneginf):
        assert np.array_equal(kind(got), kind(exp)), \
            f"{what}: {kind.__name__} positions differ ({int(kind(got).sum())} on the device, " \
            f"{int(kind(exp).sum())} expected)"


def _ema_bar(m, alpha):
    return float(np.spacing(F32(m))) * (1.0 + 1.0 / alpha)


def _assert_ema(got, exp64, m, alpha, what="", factor=1.0):
    _same_kind(got, exp64, f"{what} EMA")
    fin = np.isfinite(exp64)
    if fin.any():
        worst = float(np.abs(got[fin].astype(np.float64) - exp64[fin]).max())
        bar = factor * _ema_bar(m, alpha)
        print(f"{what}: EMA max |d| {worst:.3e} dB = {worst / float(np.spacing(F32(m))):.2f} ulp(M), "
              f"bar {bar:.3e} (M = {m:.1f})")
        assert worst <= bar, f"{what}: EMA off by {worst:.3e} dB, bar {bar:.3e}"


class Truth:
    """Peaks (fp32, exact) and EMA (float64, the defined recurrence) of the rows fed so far."""

    def __init__(self, n, alpha):
        self.alpha = float(F32(alpha))  # the device holds alpha as a float
        self.peaks = np.full(n, processor.PEAK_FILL, F32)
        self.ema = np.full(n, -np.inf, np.float64)
        self.m = 0.0

    def feed(self, rows):
        with np.errstate(invalid="ignore", over="ignore"):
            for r in rows:
                self.peaks = np.maximum(self.peaks, r)  # NaN wins, like Math.max
                x = r.astype(np.float64)
                self.ema = np.where(np.isfinite(self.ema), self.ema + self.alpha * (x - self.ema), x)
        fin = np.isfinite(rows)
        if fin.any():
            self.m = max(self.m, float(np.abs(rows[fin]).max()))


def _chunk_len(n, frames, tiled=False):
    """Frames per chunk of the form launch_state picks (fft_kernels.hip; engine.hip
    state_chunks = min(32, 2^20 / N)); the whole call for the sequential forms."""
    mc = min(32, max(1, (1 << 20) // n))
    c = min(mc, (frames + 7) // 8)
    if tiled or mc == 1 or c <= 1:
        return frames
    if c >= 8:
        c = 32 if c >= 32 else 16 if c >= 16 else 8
    return -(-frames // c)


def _tuning(n):
    return 433_000_000, 1000 * n  # 1000 Hz per bin


def _channel(n):
    f0 = _tuning(n)[0]
    return f0 - 100_500, f0 + 200_500  # 301 bins right of the centre


def _run(rfa, n, fmt, window, calls, source, ring_rows=None, alpha=ALPHA, precheck=None, label=""):
    """Feed ``calls`` (list of (bytes, n_frames)) and check ring, boxcar, peaks, EMA and the
    channel means after every call against the device's own rows.  Returns (peaks, ema,
    Truth, all device rows of the last call)."""
    frames = [f for _, f in calls]
    total = sum(frames)
    if ring_rows is None:
        ring_rows = {"ring": total, "rows": 5, "staging": min(min(frames) - 1, 40)}[source]
    assert source != "ring" or ring_rows >= total
    assert source != "staging" or ring_rows < min(frames)
    freq, sr = _tuning(n)
    kw = dict(avg="ema", ema_alpha=alpha, peak_hold=True)
    twin = rfa.SpectrumEngine(n, window, fmt, ring_rows=0, **kw) if source == "staging" else None
    truth = Truth(n, alpha)
    tail = np.empty((0, n), F32)  # the newest ring_rows device rows, oldest first
    with rfa.SpectrumEngine(n, window, fmt, ring_rows=ring_rows, **kw) as e:
        e.set_tuning(freq, sr)
        e.set_channel(*_channel(n))
        f = 0
        for k, (data, nf) in enumerate(calls):
            what = f"{label} call {k} ({nf} frames, {source})"
            if source == "rows":
                rows = e.process(data, nf)
            elif source == "ring":
                e.process(data, nf, rows=False)
                ring, _, _ = e.ring()
                rows = ring[[(-g) % ring_rows for g in range(f, f + nf)]]
            else:
                e.process(data, nf, rows=False)
                rows = twin.process(data, nf)
            f += nf
            if precheck:
                precheck(k, rows)
            if ring_rows > 0:
                tail = np.concatenate([tail, rows])[-ring_rows:]
                ring, ri, wi = e.ring()
                assert (ri, wi) == ((-(f - 1)) % ring_rows, (-f) % ring_rows), what
                live = range(max(0, f - ring_rows), f)
                _same_bits(ring[[(-g) % ring_rows for g in live]], tail, f"{what} ring rows")
                if f < ring_rows:
                    assert np.all(ring[[(-g) % ring_rows for g in range(f, ring_rows)]] == processor.RING_FILL)
                length = min(BOXCAR_L, ring_rows - 1)
                acc = np.zeros(n, F32)
                with np.errstate(invalid="ignore", over="ignore"):
                    for r in range(length + 1):
                        acc = acc + ring[(ri + r) % ring_rows]
                    acc = acc / F32(length + 1)
                _same_bits(e.boxcar(length), acc, f"{what} boxcar")
            truth.feed(rows)
            peaks, ema = e.peaks(), e.ema()
            _same_bits(peaks, truth.peaks, f"{what} peaks")
            _assert_ema(ema, truth.ema, truth.m, alpha, what)
            means = e.channel_means()
            assert means.size == nf, what
            with np.errstate(invalid="ignore", over="ignore"):
                exp = np.array([processor.channel_mean(r, n, freq, sr, *_channel(n)) for r in rows], F32)
            _same_kind(means, exp, f"{what} channel means")
            fin = np.isfinite(exp)
            np.testing.assert_allclose(means[fin], exp[fin], rtol=0, atol=CHAN_SUM_TOL, err_msg=what)
    if twin:
        twin.close()
    return peaks, ema, truth, rows


def _s8_calls(n, frames, seed):
    """Noise plus a tone, with a level that differs frame to frame (so the peaks and the
    EMA depend on which frames were taken, in which order)."""
    rng = np.random.default_rng(seed)
    calls = []
    t = np.arange(n)
    tone = np.exp(2j * np.pi * 0.17 * t)
    for nf in frames:
        gain = rng.uniform(0.2, 1.0, (nf, 1))
        x = gain * (0.3 * tone + 0.08 * (rng.standard_normal((nf, n)) + 1j * rng.standard_normal((nf, n))))
        iq = np.empty((nf, 2 * n))
        iq[:, 0::2], iq[:, 1::2] = x.real, x.imag
        calls.append((np.clip(np.rint(iq * 128), -128, 127).astype(np.int8).tobytes(), nf))
    return calls


def _f32_noise(n, frames, seed):
    return (0.1 * np.random.default_rng(seed).standard_normal((frames, 2 * n), dtype=F32)).astype(F32)


# ---------------------------------------------------------------- every form, finite rows
# N = 1024 (state_chunks = 32): <= 8 frames state_kernel, 9 .. 56 partial + combine,
# 57 .. 120 fused<8>, 121 .. 248 fused<16>, >= 249 fused<32> -- both ends of every range,
# from caller rows, the ring and the staging buffer.
@pytest.mark.parametrize("source", ["rows", "ring", "staging"])
@pytest.mark.parametrize("frames", [(1, 8), (9, 56), (57, 120), (121, 248), (249, 300)])
def test_every_form_at_1k(rfa, frames, source):
    _run(rfa, 1024, "s8", "blackman", _s8_calls(1024, frames, sum(frames)), source, label="1 K")


def test_fused32_small_alpha(rfa):
    """alpha = 0.01: the bar is 101 ulp(M); (1 - alpha)^L is furthest from a power it can hold."""
    _run(rfa, 1024, "s8", "blackman", _s8_calls(1024, (300, 249), 5), "ring", alpha=0.01, label="1 K a=.01")


@pytest.mark.parametrize("n,fmt,frames", [
    (131072, "s8", (57, 57)),    # state_chunks 8: fused<8>, ring order 4
    (65536, "s8", (121, 121)),   # state_chunks 16: fused<16>, ring order 2, the 8-bit main kernel
    (65536, "f32", (121, 121)),  # ... the float main kernel
])
def test_fused_forms_at_their_size(rfa, n, fmt, frames):
    if fmt == "s8":
        calls = _s8_calls(n, frames, n)
    else:
        calls = [((_f32_noise(n, nf, n + k) * F32(1 + k)).tobytes(), nf) for k, nf in enumerate(frames)]
    _run(rfa, n, fmt, "blackman", calls, "ring", label=f"{n} {fmt}")


@pytest.mark.parametrize("n", [262144, 524288, 1048576])
def test_tile_forms(rfa, n):
    """Ring read at N >= 256 K: state_tile_kernel<3 | 4 | 5>, 3 + 9 frames, ring of 16."""
    _run(rfa, n, "s8", "blackman", _s8_calls(n, (3, 9), n), "ring", ring_rows=16, label=f"{n} tile")


@pytest.mark.parametrize("n,frames", [(262144, (9, 33)),   # partial + combine with 2 and 4 chunks
                                      (1048576, (3, 9))])  # state_chunks 1: state_kernel
def test_large_n_caller_rows(rfa, n, frames):
    _run(rfa, n, "s8", "blackman", _s8_calls(n, frames, n + 1), "rows", ring_rows=4, label=f"{n} rows")


# ---------------------------------------------------------------- non-finite rows
KINDS = ("silent", "const", "nan", "big")
LAST = ("nan", "big", "const", None)  # last frame of call k: carries NaN, +inf, -inf into call k + 1


def _plan(n, frames, k, tiled=False):
    """Special frames of call k: at frame 0, at both sides of the first chunk seam, an adjacent
    pair inside a chunk, and the last frame; the kinds rotate with k."""
    cl = _chunk_len(n, frames, tiled)
    kr = [KINDS[(k + j) % 4] for j in range(4)]
    plan = {0: kr[0], cl - 1: kr[1], cl % frames: kr[2]}
    p = min(frames // 2 + 1, frames - 2)
    plan[p], plan[p + 1] = kr[3], kr[0]
    if LAST[k % 4]:
        plan[frames - 1] = LAST[k % 4]
    elif frames > 2:
        plan.pop(frames - 1, None)  # ends on plain noise: a finite average at the end
    return plan


def _apply(x, n, plan):
    for pos, kind in plan.items():
        if kind == "silent":
            x[pos] = 0
        elif kind == "const":
            x[pos] = 0.5
        elif kind == "nan":
            x[pos, 2 * (n // 3)] = np.nan  # one NaN sample
        else:
            x[pos] *= F32(2.0 ** 70)
    return x


def _precheck(plans):
    """The preconditions, on the device's rows: what each kind of frame turns into."""
    def check(k, rows):
        for pos, kind in plans[k].items():
            r = rows[pos]
            if kind == "silent":
                assert np.all(np.isneginf(r)), (k, pos, kind)
            elif kind == "const":
                assert np.isfinite(r).any() and np.isneginf(r).any(), (k, pos, kind)
            elif kind == "nan":
                assert np.all(np.isnan(r)), (k, pos, kind)
            else:
                assert np.isposinf(r).any(), (k, pos, kind)
        plain = [p for p in range(len(rows)) if p not in plans[k]]
        assert np.isfinite(rows[plain]).all()
    return check


def _nonfinite_calls(n, frames, seed, tiled=False):
    base = _f32_noise(n, max(frames), seed)
    calls, plans = [], []
    for k, nf in enumerate(frames):
        plans.append(_plan(n, nf, k, tiled))
        x = _apply(base[:nf] * F32(0.5 + 0.37 * k), n, plans[-1])
        calls.append((x.tobytes(), nf))
    return calls, plans


@pytest.mark.parametrize("source", ["rows", "ring", "staging"])
@pytest.mark.parametrize("frames", [8, 9, 56, 57, 120, 121, 248, 249, 300])
def test_non_finite_rows_every_form_at_1k(rfa, frames, source):
    """Four calls of one form; call k ends on a NaN, a +inf, a constant (-inf but one bin)
    and a plain frame, so calls 1 .. 3 start from a NaN, +inf and -inf average."""
    calls, plans = _nonfinite_calls(1024, (frames,) * 4, frames)
    _run(rfa, 1024, "f32", "none", calls, source, precheck=_precheck(plans), label=f"1 K nf {frames}")


def test_non_finite_rows_at_64k(rfa):
    """fused<16> on caller rows at N = 64 K."""
    calls, plans = _nonfinite_calls(65536, (121,) * 4, 64)
    _run(rfa, 65536, "f32", "none", calls, "rows", ring_rows=4, precheck=_precheck(plans), label="64 K nf")


def test_non_finite_rows_at_1m(rfa):
    """state_tile_kernel<5> on the column-order ring at N = 1 M."""
    calls, plans = _nonfinite_calls(1048576, (6, 3, 3, 3), 1, tiled=True)
    _run(rfa, 1048576, "f32", "none", calls, "ring", ring_rows=16, precheck=_precheck(plans), label="1 M nf")


_BATCHED = {}


def _batched(rfa, total):
    """The same frames as calls of 1, calls of 8 and one call (state_kernel twice, then
    fused<8> / fused<32>): per form (rows, peaks, EMA), and the truth from the rows."""
    if total not in _BATCHED:
        n = 1024
        plan = _plan(n, total, 0)
        plan.pop(total - 1)  # ends on plain frames: finite bins to compare
        plan.update({7: "big", 8: "nan", 16: "const", 23: "silent", 24: "silent", 40: "nan", 41: "big"})
        # the last special frames are a NaN and a +inf one with no -inf frame after them (a -inf
        # frame would restart every form alike): four plain frames follow, inside the last chunk
        plan.update({total - 6: "nan", total - 5: "big"})
        x = _apply(_f32_noise(n, total, total), n, plan)
        out = {}
        for step in (1, 8, total):
            calls = [(x[f:f + step].tobytes(), min(step, total - f)) for f in range(0, total, step)]
            with rfa.SpectrumEngine(n, "none", "f32", avg="ema", ema_alpha=ALPHA, peak_hold=True, ring_rows=0) as e:
                rows = np.concatenate([e.process(d, nf) for d, nf in calls])
                out[step] = (rows, e.peaks(), e.ema())
        _precheck([plan])(0, out[1][0])
        truth = Truth(n, ALPHA)
        truth.feed(out[1][0])
        assert np.isnan(truth.peaks).all() and np.isfinite(truth.ema).all()
        _BATCHED.clear()
        _BATCHED[total] = (out, truth)
    return _BATCHED[total]


@pytest.mark.parametrize("total", [57, 300])
def test_non_finite_rows_peaks_do_not_depend_on_batching(rfa, total):
    """Rows and peaks are bit-identical however the frames are cut into calls."""
    out, truth = _batched(rfa, total)
    for step, (rows, peaks, _) in out.items():
        _same_bits(rows, out[1][0], f"rows, calls of {step}")
        _same_bits(peaks, truth.peaks, f"peaks, calls of {step}")


@pytest.mark.parametrize("total", [57, 300])
def test_non_finite_rows_ema_does_not_depend_on_batching(rfa, total):
    """The EMA's non-finite pattern is identical however the frames are cut into calls (the
    chunked scan agrees with the serial recursion), and its finite bins lie within twice the
    bar of one another (each side is within one bar of the float64 recurrence)."""
    out, truth = _batched(rfa, total)
    for step, (_, _, ema) in out.items():
        _assert_ema(ema, out[1][2].astype(np.float64), truth.m, ALPHA, f"calls of {step} vs calls of 1", factor=2.0)
    for step, (_, _, ema) in out.items():
        _assert_ema(ema, truth.ema, truth.m, ALPHA, f"calls of {step}")


# ---------------------------------------------------------------- display and scanner on such a ring
DN, DR, DF0, DSR = 2048, 12, 100_000_000, 2_000_000
# the eleven older rows hold every kind; the newest row is the parameter
OLDER = ("noise", "noise", "silent", "noise", "nan", "noise", "const", "big", "noise", "silent", "noise")


@pytest.fixture(scope="module")
def display_engines(rfa):
    made = {}

    def get(newest):
        if newest not in made:
            order = OLDER + (newest,)
            x = _apply(_f32_noise(DN, DR, 77), DN, {i: k for i, k in enumerate(order) if k != "noise"})
            e = rfa.SpectrumEngine(DN, "none", "f32", avg="none", peak_hold=True, ring_rows=DR)
            e.set_tuning(DF0, DSR)
            e.process(x.tobytes(), DR, rows=False)
            ring, ri, _ = e.ring()
            _precheck([{i: k for i, k in enumerate(order) if k != "noise"}])(0, ring[[(-g) % DR for g in range(DR)]])
            made[newest] = (e, ring, ri)
        return made[newest]
    yield get
    for e, _, _ in made.values():
        e.close()


def _same_draw(got, exp, what):
    colors, path, pk, mm = got
    c2, p2, k2, mm2 = exp
    np.testing.assert_array_equal(colors, c2, err_msg=what)
    _same_bits(path, p2, f"{what} path y")
    _same_bits(pk, k2, f"{what} peak y")
    _same_bits(np.array(mm, F32), np.array(mm2, F32), f"{what} autoscale")


@pytest.mark.parametrize("newest", ["noise", "silent", "const", "nan", "big"])
def test_draw_preprocess_on_non_finite_rows(display_engines, newest):
    """draw_rows_kernel / draw_finish_kernel (kt_toint of NaN and of +-inf, jmin / jmax with
    NaN) bit-exact against oracle/display.py: average_length 7 spans special rows of every
    kind, then 0 draws the newest row alone."""
    e, ring, ri = display_engines(newest)
    surf = od.Surface(DR)
    peaks = e.peaks()
    assert np.isnan(peaks).all()  # the ring holds an all-NaN row
    for length, vf, vsr in ((7, DF0, DSR), (0, DF0 + 150_000, DSR // 3)):
        args = dict(width=333, fft_height=480, viewport_frequency=vf, viewport_sample_rate=vsr, min_db=-110.0,
                    max_db=-20.0, average_length=length, colormap=od.gqrx_colormap())
        got = e.draw_preprocess(peaks=True, **args)
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            exp = surf.draw(ring, ri, peaks, DF0, DSR, **args)
        _same_draw(got, exp, f"newest {newest}, average_length {length}")


@pytest.mark.parametrize("newest", ["noise", "silent", "const", "nan", "big"])
def test_row_window_stats_on_non_finite_rows(display_engines, newest):
    """row_window_kernel: peaks bit-identical to FloatArray.maxOrNull (NaN wins); averages
    (a double sum) of the same kind where non-finite and within 1 ulp where finite."""
    e, ring, ri = display_engines(newest)
    row = ring[ri]
    rng = np.random.default_rng(9)
    lo = rng.integers(0, DN - 1, 150)
    hi = np.minimum(DN - 1, lo + rng.integers(0, 400, 150))
    fin = np.flatnonzero(np.isfinite(row))[:3]  # single-bin windows on finite bins (the constant row has one)
    lo = np.concatenate([[0], lo, fin]).astype(np.int32)
    hi = np.concatenate([[DN - 1], hi, fin]).astype(np.int32)
    pk, av = e.row_window_stats(lo, hi)
    epk, eav = osc.window_stats(row, lo, hi)
    _same_bits(pk, epk, f"newest {newest} window peaks")
    _same_kind(av, eav, f"newest {newest} window averages")
    f = np.isfinite(eav)
    assert np.all(np.abs(av[f].view(np.int32).astype(np.int64) - eav[f].view(np.int32).astype(np.int64)) <= 1)
