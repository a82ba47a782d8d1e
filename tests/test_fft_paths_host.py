"""CPU: the host side of tests/test_gpu_fft_paths.py -- its frame-count helper with a made-up CU
count, its case lists against the dispatch rules they restate, and the reference side of every
case (inputs, float64 oracle), so that the GPU module cannot fail there for a reason of its own."""
import numpy as np
import pytest

import oracle
import test_gpu_fft_paths as tp


def test_lds_request_and_resident_bound():
    # fft_wide.hip WGeo<13 | 14 | 15, 32>::LDS_BYTES; 160 KB of LDS per CU
    assert [tp.wide_lds_bytes(lm) for lm in (13, 14, 15)] == [39552, 81280, 158976]
    assert [tp.resident_bound(10, lm) for lm in (13, 14, 15)] == [40, 20, 10]
    assert [tp.ragged_frames(10, lm) for lm in (13, 14, 15)] == [83, 43, 23]
    assert tp.ragged_frames(256, 15) == 515
    for lm in (13, 14, 15):  # more items than workgroups, and not a whole number of rounds
        assert tp.ragged_frames(7, lm) % tp.resident_bound(7, lm) == 3


def test_case_lists_follow_the_dispatch_rules():
    """A staged form exists where the frame fits the exchange buffer (wide_by_fmt stg8 / stg16:
    M * RS * bytes <= HALFP * 8, one sub-FFT per workgroup)."""
    def staged(n, fmt):
        logm = min(15, n.bit_length() - 1)
        m = 1 << logm
        return n * tp.BPS[fmt] <= (m // 2 + m // 64) * 8
    have = {(n, f) for n, f, counts, _ in tp.DIRECT_CASES if f != "f32" and len(counts) == 3}
    want = {(n, f) for n in (8192, 16384, 32768, 65536, 131072) for f in ("s8", "u8", "s16") if staged(n, f)}
    assert have == want and len(want) == 11
    assert not staged(65536, "s16") and not staged(131072, "s8")
    assert {(n, f) for n, f, _ in tp.RAGGED_CASES} == want - {(65536, "s8")}
    assert len(tp.STRIDE_CASES) == 12


@pytest.mark.parametrize("n,fmt", [(8192, "s8"), (8192, "s16"), (65536, "u8")])
def test_reference_side_of_the_ragged_cases(n, fmt):
    cus = 2
    logm = min(15, n.bit_length() - 1)
    frames = tp.ragged_frames(cus, logm)
    data, ref = tp.ragged_case(n, fmt, frames, tp.ragged_base_samples(cus))
    assert len(data) == frames * n * tp.BPS[fmt] and ref.shape == (frames, n)
    assert np.isfinite(ref).all()
    fb = n * tp.BPS[fmt]
    assert len({data[f * fb:(f + 1) * fb] for f in range(frames)}) == frames  # every frame differs
    assert (np.abs(np.argmax(ref, 1) - np.argmax(ref[0])) <= 1).all()          # ... around the same tone


@pytest.mark.parametrize("n,fmt", [(8192, "s8"), (8192, "s16"), (32768, "f32")])
def test_reference_side_of_the_small_cases(n, fmt):
    data, ref = tp._case(n, fmt, 9)
    assert ref.shape == (9, n) and not ref.flags.writeable
    tp.check_rows(ref.copy(), ref, fmt, "oracle vs itself")
    stride = n * tp.BPS[fmt] + tp.LOAD_ALIGN[fmt]
    laid = tp.strided_copy(data, n, fmt, 9, stride)
    # the oracle reads the strided layout as the packed frames; the gap bytes are loud
    got = oracle.spectrum_rows(laid.tobytes(), tp.signals.FORMATS[fmt], n, 9, stride, oracle.WIN_BLACKMAN)
    np.testing.assert_array_equal(got, ref)
    fb = n * tp.BPS[fmt]
    assert (laid[fb:stride] == 0x7f).all()
    shifted = oracle.spectrum_rows(laid.tobytes()[tp.LOAD_ALIGN[fmt]:] + bytes(tp.LOAD_ALIGN[fmt]),
                                   tp.signals.FORMATS[fmt], n, 9, stride, oracle.WIN_BLACKMAN)
    # frames taken one sample late (the window's edge hides the gap itself) are far off the bar
    assert np.abs(shifted[1:] - ref[1:]).max() > 10 * tp.gu.DB_TOL


def test_seam_reference():
    n = 8192
    x, exact, ref_db, xw, ref_wdb = tp.seam_reference(n)
    assert x.size == 2 * n and xw.size == 2 * n and exact.size == n
    k = int(np.argmax(np.abs(exact)))
    assert ref_db[(k + n // 2) % n] == ref_db.max()  # fft-shifted
    assert ref_wdb.max() < ref_db.max()              # the window takes level away
