"""CPU: the host side of tests/test_gpu_fft_small.py -- the slot geometry it restates from
fft_kernels.hip, its case lists against that geometry, the reference side of every case (inputs,
float64 oracle, strided layouts), and the condition on its inputs: the reference's own pffft
stays within half of every asserted bar on each of them, so that the GPU module cannot fail for
a reason of its own."""
import numpy as np
import pytest

import golden_util as gu
import oracle
import signals
import test_gpu_fft_paths as tp
import test_gpu_fft_small as ts


def test_slot_geometry_rules():
    # fft_kernels.hip Geo<LOGM>: TPF = M / 16, SLOTS = TPF >= 256 ? 1 : 256 / TPF
    assert [ts.slots(n) for n in ts.SIZES] == [64, 32, 16, 8, 4, 2, 1]
    assert ts.SIZES == tuple(1 << k for k in range(6, 13))
    for n in ts.SIZES:
        s, counts = ts.slots(n), ts.geometry_counts(n)
        assert (n // 16) * s == 256 or (s == 1 and n // 16 == 256)
        assert set(counts) == {c for c in (1, s - 1, s, s + 1, 5 * s + 3) if c > 0}
        assert counts == sorted(counts) and counts[0] == 1 and counts[-1] == 5 * s + 3
        assert s + 1 in counts and (s - 1 in counts or s == 1)
        assert -(-counts[-1] // s) >= 6  # the longest call needs at least six workgroups
        assert ts.capture_frames(n) >= max(counts[-1], ts.STRIDE_FRAMES)
    assert ts.geometry_counts(4096) == [1, 2, 8] and ts.geometry_counts(2048) == [1, 2, 3, 13]
    assert ts.geometry_counts(64) == [1, 63, 64, 65, 323]


def test_case_lists():
    assert ts.GEOMETRY_CASES == [(n, f) for n in ts.SIZES for f in ("s8", "u8", "s16", "f32", "f32p")]
    assert len(ts.STRIDE_CASES) == 24 and len(ts.POINTER_CASES) == 12
    # the strided sizes: the most slots, the largest wave-synchronous size, the one-slot size
    assert [ts.slots(n) for n in ts.STRIDE_SIZES] == [64, 4, 1]
    for n, fmt, gap in ts.STRIDE_CASES:
        stride = n * tp.BPS[fmt] + (16 if gap == "16" else tp.LOAD_ALIGN[fmt])
        assert stride % tp.LOAD_ALIGN[fmt] == 0                       # process_impl accepts it
        assert tp.LOAD_ALIGN[fmt] < n * tp.BPS[fmt]                   # the one-frame stride is too small
    # many workgroups: 66 of them, the last with 5 of 64 slots
    s = ts.slots(ts.MANY_N)
    assert -(-ts.MANY_FRAMES // s) == 66 and ts.MANY_FRAMES % s == 5
    # windows: a full workgroup and one slot
    assert ts.slots(ts.WINDOW_N) + 1 == 9
    # ring: 16 slots, the first call longer than the ring (ring_first = 8), the second shorter
    assert ts.slots(ts.RING_N) == 16
    assert ts.RING_CALLS[0] > ts.RING_ROWS > ts.RING_CALLS[1] and ts.RING_CALLS[0] > ts.slots(ts.RING_N)


@pytest.mark.parametrize("n,fmt", ts.GEOMETRY_CASES, ids=[f"{n}-{f}" for n, f in ts.GEOMETRY_CASES])
def test_reference_side_of_the_captures(n, fmt):
    data, ref = ts.small_case(n, fmt)
    frames, fb = ts.capture_frames(n), n * tp.BPS[fmt]
    assert len(data) == frames * fb and ref.shape == (frames, n) and not ref.flags.writeable
    assert np.isfinite(ref).all()
    assert len({data[f * fb:(f + 1) * fb] for f in range(frames)}) == frames  # every frame differs
    tp.check_rows(ref.copy(), ref, fmt, "oracle vs itself")
    # a prefix of the capture has the prefix of the rows
    k = ts.geometry_counts(n)[-2] if len(ts.geometry_counts(n)) > 1 else 1
    part = oracle.spectrum_rows(data[:k * fb], signals.FORMATS[fmt], n, k, None, oracle.WIN_BLACKMAN)
    np.testing.assert_array_equal(part, ref[:k])
    # a neighbouring frame's row is far outside the bar (a wrong slot or frame index shows)
    assert np.abs(ref[1:] - ref[:-1]).max() > 10 * gu.DB_TOL


@pytest.mark.parametrize("n,fmt,gap", ts.STRIDE_CASES, ids=[f"{c[0]}-{c[1]}-gap{c[2]}" for c in ts.STRIDE_CASES])
def test_reference_side_of_the_strided_cases(n, fmt, gap):
    data, ref = ts.small_case(n, fmt)
    fb, al, frames = n * tp.BPS[fmt], tp.LOAD_ALIGN[fmt], ts.STRIDE_FRAMES
    stride = fb + (16 if gap == "16" else al)
    laid = tp.strided_copy(data, n, fmt, frames, stride)
    assert laid.size == (frames - 1) * stride + fb
    for f in range(frames):  # the frame whole (f32p: both planes), then the loud gap
        assert laid[f * stride:f * stride + fb].tobytes() == data[f * fb:(f + 1) * fb]
        if f + 1 < frames:
            assert (laid[f * stride + fb:(f + 1) * stride] == 0x7f).all()
    got = oracle.spectrum_rows(laid.tobytes(), signals.FORMATS[fmt], n, frames, stride, oracle.WIN_BLACKMAN)
    np.testing.assert_array_equal(got, ref[:frames])
    # frames taken one sample late are far outside the bar
    late = oracle.spectrum_rows(laid.tobytes()[al:] + bytes(al), signals.FORMATS[fmt], n, frames, stride,
                                oracle.WIN_BLACKMAN)
    assert np.abs(late[1:] - ref[1:frames]).max() > 10 * gu.DB_TOL
    if fmt == "f32p":
        # an imaginary plane taken a gap late (as if the gap sat between the planes), not N floats
        # after the frame's start, is far outside the bar (or not finite: the gap is loud)
        b, g = laid.tobytes(), stride - fb
        wrong = b[stride:stride + n * 4] + b[stride + n * 4 + g:stride + n * 8 + g]
        with np.errstate(all="ignore"):
            bad = oracle.spectrum_rows(wrong, signals.FORMATS[fmt], n, 1, None, oracle.WIN_BLACKMAN)
            assert not (np.abs(bad - ref[1:2]) <= 10 * gu.DB_TOL).all()


def test_reference_side_of_the_window_cases():
    frames = ts.slots(ts.WINDOW_N) + 1
    for window, fmt in ts.WINDOW_CASES:
        part, ref = ts.window_case(ts.WINDOW_N, fmt, window, frames)
        assert len(part) == frames * ts.WINDOW_N * tp.BPS[fmt] and ref.shape == (frames, ts.WINDOW_N)
        black = ts.small_case(ts.WINDOW_N, fmt)[1][:frames]
        assert np.abs(ref - black).max() > 1.0  # another window, not the handle's default


def test_reference_side_of_the_ring_case():
    calls = ts.ring_calls()
    assert [f for _, f in calls] == list(ts.RING_CALLS)
    rows = [oracle.spectrum_rows(d, oracle.IN_S8, ts.RING_N, f, None, oracle.WIN_BLACKMAN) for d, f in calls]
    rows = np.concatenate(rows)
    assert np.isfinite(rows).all()
    # the level differs frame to frame: peaks and EMA depend on which frames were taken
    assert len({float(r.max()) for r in rows}) == rows.shape[0]


def test_seam_reference_at_small_sizes():
    for n in ts.SIZES:
        x, exact, ref_db, xw, ref_wdb = tp.seam_reference(n)
        assert x.size == 2 * n and exact.size == n and np.isfinite(ref_db).all() and np.isfinite(ref_wdb).all()


# ---------------------------------------------------------------- input condition
needs_ref = pytest.mark.skipif(not oracle.ref_available(), reason="reference pffft build absent")


def assert_pffft_within_half_the_bars(data, fmt, n, frames, ref, win, what):
    """The reference's own fp32 FFT on this input stays within half of every bar check_rows
    asserts: two correct fp32 transforms differ in the sign of their rounding, not its size."""
    r = oracle.ref_spectrum_rows(data, signals.FORMATS[fmt], n, frames, None, win)
    d = gu.db_diff(r, ref)
    full = gu.full_row_diff(r, ref, bar=None)
    print(f"{what}: pffft vs float64 above the floor {d:.3e} dB, every bin {full:.3e} dB")
    assert d <= gu.DB_TOL / 2, what
    gu.assert_same_peak_bins(r, np.argmax(ref, 1))
    if fmt in ("s8", "u8"):
        assert full <= gu.DB_TOL / 2, what
    elif fmt == "s16":
        assert full <= gu.DB_TOL_S16_EVERY_BIN / 2, what


@needs_ref
@pytest.mark.parametrize("n,fmt", ts.GEOMETRY_CASES, ids=[f"{n}-{f}" for n, f in ts.GEOMETRY_CASES])
def test_pffft_within_half_the_bars_on_the_captures(n, fmt):
    data, ref = ts.small_case(n, fmt)
    assert_pffft_within_half_the_bars(data, fmt, n, ts.capture_frames(n), ref, oracle.WIN_BLACKMAN, f"{n}/{fmt}")


@needs_ref
def test_pffft_within_half_the_bars_on_the_other_inputs():
    data, ref = ts.many_case()
    assert_pffft_within_half_the_bars(data, ts.MANY_FMT, ts.MANY_N, ts.MANY_FRAMES, ref, oracle.WIN_BLACKMAN,
                                      "many workgroups")
    frames = ts.slots(ts.WINDOW_N) + 1
    for window, fmt in ts.WINDOW_CASES:
        part, ref = ts.window_case(ts.WINDOW_N, fmt, window, frames)
        assert_pffft_within_half_the_bars(part, fmt, ts.WINDOW_N, frames, ref, gu.WINDOW_IDS[window],
                                          f"512/{fmt} window {window}")
    for k, (d, f) in enumerate(ts.ring_calls()):
        ref = oracle.spectrum_rows(d, oracle.IN_S8, ts.RING_N, f, None, oracle.WIN_BLACKMAN)
        assert_pffft_within_half_the_bars(d, "s8", ts.RING_N, f, ref, oracle.WIN_BLACKMAN, f"ring call {k}")


@needs_ref
@pytest.mark.parametrize("n", ts.SIZES)
def test_pffft_within_half_the_bars_on_the_seam_input(n):
    x, exact, ref_db, xw, ref_wdb = tp.seam_reference(n)
    r = oracle.ref_fft_ordered(x)
    rel = np.abs(r[0::2].astype(np.float64) + 1j * r[1::2] - exact).max() / np.abs(exact).max()
    d, dw = gu.db_diff(oracle.ref_fft_logmag(x), ref_db), gu.db_diff(oracle.ref_fft_logmag(xw), ref_wdb)
    print(f"{n}: pffft ordered rel err {rel:.3e}, log-mag {d:.3e} dB, windowed {dw:.3e} dB above the floor")
    assert rel <= 1e-6 and d <= gu.DB_TOL / 2 and dw <= gu.DB_TOL / 2
