"""GPU: the peak work of a warm 64 K call split at first_frame.

A warm call of the staged two-residue 8-bit kernel raises the peaks' shadow only for the frames
below first_frame = n_frames - T(alpha); the state pass reads the frames from first_frame on for
the EMA and takes their peaks in the same loop.  A frame taken by the wrong side is harmless, a
frame taken by neither side loses its records without any error -- so every case here puts its
records at the boundary, and holds the result as tests/test_gpu_peak_raise.py does: against the
sequential restatement on the device's own ring rows, peaks bit for bit, the EMA's non-finite
positions exactly and its finite bins within ulp(M) (1 + 1/alpha).

N = 65536, a ring of 300 rows and about 300 frames per call (600 work items on 256 workgroups,
so a workgroup's items are raising and plain ones), alpha = 0.5 (T = 51, first_frame = 249)
unless a case says otherwise.  Every frame has a gain of its own (the shared noise block) and a
level of its own (the case).
"""
import numpy as np
import pytest

from test_gpu_peak_raise import LOUD, N, PLAIN, QUIET, R, _engine, _last_rows, _noise, tail_frames
from test_gpu_state_exact import F32, Truth, _assert_ema, _same_bits

gpu = pytest.mark.gpu

ALPHA = 0.5


def _first_frame(nf, alpha=ALPHA):
    return max(0, nf - tail_frames(alpha))


def _data(fmt, nf, base, at=()):
    """nf frames at level `base`, frame f at level v for every (f, v) of `at` (0: a silent frame)."""
    lv = np.full((nf, 1), base, F32)
    for f, v in at:
        lv[f] = v
    x = _noise()[:nf] * lv
    if fmt == "u8":
        return np.clip(np.rint(x + F32(127.4)), 0, 255).astype(np.uint8)
    return np.clip(np.rint(x), -128, 127).astype(np.int8)


def _call(e, truth, data, nf, what, alpha=ALPHA):
    assert e.process(data, nf, rows=False) is None
    rows = _last_rows(e, nf)
    truth.feed(rows)
    peaks = e.peaks()
    _same_bits(peaks, truth.peaks, f"{what} peaks")
    if alpha is not None:
        _assert_ema(e.ema(), truth.ema, truth.m, alpha, what)
    return rows, peaks


def _records_of(rows, before, f):
    """Bins whose record after the call is frame f's alone: above the peaks before it and above
    every other frame of the call."""
    others = np.delete(rows, f, 0).max(0)
    return int(((rows[f] > before) & (rows[f] > others)).sum())


def _boundary_case(rfa, fmt, loud, nf=R, alpha=ALPHA):
    """Cold call, a warm call that is quiet but for the frames of `loud`, and a quiet warm call
    after it (the shadow the second call left is the one the third compares against)."""
    with _engine(rfa, fmt, alpha=alpha) as e:
        t = Truth(N, alpha)
        _, p0 = _call(e, t, _data(fmt, nf, PLAIN), nf, f"{fmt} cold", alpha)
        rows, p1 = _call(e, t, _data(fmt, nf, QUIET, loud), nf, f"{fmt} warm, loud {loud}", alpha)
        for f, _ in loud:
            n = _records_of(rows, p0, f)
            print(f"frame {f}: {n} bins hold its record")
            assert n > 0, f"frame {f} sets no record: the case does not test what it says"
        _, p2 = _call(e, t, _data(fmt, nf, QUIET), nf, f"{fmt} warm, quiet after", alpha)
        _same_bits(p2, p1, "peaks after the quiet call")


FF = _first_frame(R)


@gpu
@pytest.mark.parametrize("fmt", ["s8", "u8"])
def test_record_before_the_tail(rfa, fmt):
    """The last raising frame (and frame 0) alone set records."""
    assert FF == 249
    _boundary_case(rfa, fmt, ((FF - 1, LOUD), (0, LOUD * 0.8)))


@gpu
@pytest.mark.parametrize("fmt", ["s8", "u8"])
def test_record_inside_the_tail(rfa, fmt):
    """The first frame the state pass reads (and the last frame) alone set records."""
    _boundary_case(rfa, fmt, ((FF, LOUD), (R - 1, LOUD * 0.8)))


@gpu
@pytest.mark.parametrize("fmt", ["s8", "u8"])
def test_both_boundary_frames_loud(rfa, fmt):
    _boundary_case(rfa, fmt, ((FF - 1, LOUD), (FF, LOUD * 0.9)))


@gpu
def test_silent_boundary_frames(rfa):
    """-inf rows at first_frame - 1 (raised: sets nothing) and at first_frame (read: the average
    restarts there), in a call that is louder everywhere else."""
    with _engine(rfa) as e:
        t = Truth(N, ALPHA)
        _, p0 = _call(e, t, _data("s8", R, PLAIN), R, "cold")
        rows, p1 = _call(e, t, _data("s8", R, LOUD, ((FF - 1, 0), (FF, 0))), R, "warm, silent boundary")
        assert np.all(np.isneginf(rows[[FF - 1, FF]])) and np.isfinite(np.delete(rows, [FF - 1, FF], 0)).all()
        assert np.all(p1 > p0)
        _call(e, t, _data("s8", R, QUIET, ((FF - 1, 0),)), R, "warm, quiet, silent before the tail")


@gpu
def test_frame_count_not_a_multiple_of_eight(rfa):
    """297 frames: 608 items of which the last group of eight holds one frame, so some workgroups
    have no plain item and some an inactive last one; first_frame = 246."""
    nf = 297
    ff = _first_frame(nf)
    _boundary_case(rfa, "s8", ((ff - 1, LOUD), (ff, LOUD * 0.9), (nf - 1, LOUD * 0.95)), nf=nf)


@gpu
def test_split_straddles_ring_row_zero(rfa):
    """Two calls of 176 frames move the ring's write index to 248, so the third call's last
    raised frame lands in ring row 0 and the first frame read in row 299."""
    with _engine(rfa) as e:
        t = Truth(N, ALPHA)
        ff = _first_frame(176)
        _call(e, t, _data("s8", 176, PLAIN), 176, "short call, cold")
        _call(e, t, _data("s8", 176, QUIET, ((ff - 1, LOUD * 0.7),)), 176, "short call, warm")
        _, _, wi = e.ring()
        assert (wi - (FF - 1)) % R == 0 and (wi - FF) % R == R - 1, f"write index {wi}"
        before = e.peaks()
        rows, _ = _call(e, t, _data("s8", R, QUIET, ((FF - 1, LOUD), (FF, LOUD * 0.9))), R, "wrapped call")
        assert _records_of(rows, before, FF - 1) > 0 and _records_of(rows, before, FF) > 0
        _call(e, t, _data("s8", R, QUIET), R, "after the wrapped call")


@gpu
def test_tail_in_sixteen_chunks(rfa):
    """alpha = 0.2: T = 159, sixteen chunks of ten over the tail, first_frame = 141."""
    assert tail_frames(0.2) == 159
    ff = _first_frame(R, 0.2)
    _boundary_case(rfa, "s8", ((ff - 1, LOUD), (ff, LOUD * 0.9)), alpha=0.2)


@gpu
def test_tail_in_eight_chunks_with_one_empty(rfa):
    """alpha = 0.515: T = 49 frames, under the smallest plan's 57, so eight chunks of seven: the
    eighth holds no frame (the fold that tests each chunk), now with the peaks in that fold.  A
    record in the last frame sits in the last chunk that has one."""
    a = 0.515
    assert tail_frames(a) == 49 and 7 * -(-49 // 8) >= 49
    ff = _first_frame(R, a)
    _boundary_case(rfa, "s8", ((ff - 1, LOUD), (ff, LOUD * 0.9), (R - 1, LOUD * 0.95)), alpha=a)


@gpu
def test_tail_covers_the_call(rfa):
    """alpha = 0.1 (the bench line's): T = 336 > 300 frames, first_frame = 0: no frame raises, the
    plain main kernel runs and the state pass reads every row -- call after call."""
    a = 0.1
    assert _first_frame(R, a) == 0
    with _engine(rfa, alpha=a) as e:
        t = Truth(N, a)
        _, p0 = _call(e, t, _data("s8", R, PLAIN), R, "a=.1 cold", a)
        _, p1 = _call(e, t, _data("s8", R, LOUD), R, "a=.1 warm, louder", a)
        assert np.all(p1 > p0)
        _, p2 = _call(e, t, _data("s8", R, QUIET), R, "a=.1 warm, quieter", a)
        _same_bits(p2, p1, "peaks after quieter data")
        rows, p3 = _call(e, t, _data("s8", R, QUIET, ((0, LOUD * 1.2),)), R, "a=.1 later call", a)
        assert _records_of(rows, p2, 0) > 0


@gpu
def test_peak_hold_without_average(rfa):
    """avg none: every frame raises and the state pass reads no row; records in the first and
    the last frame."""
    with _engine(rfa, avg="none", alpha=None) as e:
        t = Truth(N, ALPHA)
        _, p0 = _call(e, t, _data("s8", R, PLAIN), R, "no avg, cold", None)
        rows, _ = _call(e, t, _data("s8", R, QUIET, ((0, LOUD), (R - 1, LOUD * 0.9))), R, "no avg, warm", None)
        assert _records_of(rows, p0, 0) > 0 and _records_of(rows, p0, R - 1) > 0
        _call(e, t, _data("s8", R, QUIET), R, "no avg, warm quieter", None)
