"""GPU: every FFT kernel the run-time dispatch can pick at N = 8 K ... 128 K, not only the one
an aligned, packed call gets.

Which kernel runs is decided per call from the caller's pointer, frame stride and window
("Which instantiation a call reaches": the table every case below names a row
of, as ``<N>/<formats>/<column>`` with the columns A = 16-byte aligned and packed, U = only
``load_alignment``-aligned, F = foreign window (the seam entries), C = complex output).  The
other GPU modules feed host bytes through ``SpectrumEngine.process``, i.e. column A only.

* §1 ``test_direct_load_kernels_on_unaligned_input``: column U through a device pointer
  ``load_alignment`` bytes into a buffer, beside column A on the same bytes.
* §2 ``test_strided_frames_at_wide_sizes``, ``test_one_frame_ignores_its_stride``: frames with
  a gap between them (a multiple of 16: column A with ``frame_stride`` > frame; otherwise U).
* §4 ``test_persistent_grid_with_uneven_work``: the staged forms' persistent grid with more
  items than resident workgroups and a ragged tail.
* §5 ``test_seam_entries_reach_their_kernels``: columns F and C.
* §6 ``test_state_behind_the_direct_kernel``: ring, peak-hold and EMA fed by column U.
* §7 ``test_misaligned_arguments_are_refused``: what ``load_alignment`` refuses, with no launch.

Bit identity between columns A and U.  The staged and the direct instantiation of one
(N, format) differ in where a raw sample is read from (LDS after an LDS-DMA copy, or a buffer
load), in the grid, and in how the exchanges address LDS (``XST``, four rounds under ``SPLIT``).
The float operations on each sample are the same source expressions in the same order:
``convert_raw`` -> window product (RS = 1: ``x * w``; 64 K residue 0: ``fma(x1, w1, x0 * w0)`` in
the up-front, the chunked and the direct pre-stage alike; 64 K residue 1, 8-bit: ``cmac2`` /
``cmac2x2``, the same four packed instructions per point; 64 K cf32: the same ``add_w16`` /
``cmul`` / ``w64`` chain) -> ``dftw<32, W8>`` / ``pass1`` / ``pass2`` with ``W8`` a function of
the format only -> ``db_unscaled``; both read the same window tables (``window``,
``window_il``, ``window_cw``) and twiddle blob.  So the rows are asserted bit-identical for
every pair, here and in §2 against the packed call.  (The switches RFA_STAGE=0 and
RFA_KERNEL=narrow are read by A/B builds only -- ``#ifdef RFA_AB_BUILD`` in rfa_create;
tests/test_abi.py holds the product library to importing no getenv -- so they have no case.)

Bars: the project's own (golden_util): 0.01 dB above the Parseval floor and identical peak bins
against the float64 oracle for every format; every bin (no floor) within 0.01 dB for 8-bit input
and within DB_TOL_S16_EVERY_BIN for s16, as test_rows_match_reference_pffft_and_oracle holds them.
"""
import ctypes
import functools

import numpy as np
import pytest

import golden_util as gu
import oracle
import signals

pytestmark = pytest.mark.gpu

BPS = {"s8": 2, "u8": 2, "s16": 4, "f32": 8, "f32p": 8}
LOAD_ALIGN = {"s8": 2, "u8": 2, "s16": 4, "f32": 8, "f32p": 4}  # engine.hip load_alignment()
TONES = ((0.173, 0.5), (-0.29, 0.01))                # as test_all_sizes_and_formats_vs_oracle
NOISE = 0.03
RFA_ERR_INVALID = -1


# ---------------------------------------------------------------- shared inputs and bars
@functools.lru_cache(maxsize=None)
def _case(n, fmt, frames, seed=None):
    """(bytes, float64-oracle rows) of ``frames`` consecutive frames of one noisy capture: every
    frame differs, so a frame or residue taken from the wrong place shows."""
    data = signals.frames_bytes(n, frames, fmt, seed=n + 7 * len(fmt) if seed is None else seed,
                                tones=TONES, noise=NOISE)
    ref = oracle.spectrum_rows(data, signals.FORMATS[fmt], n, frames, None, oracle.WIN_BLACKMAN)
    ref.setflags(write=False)
    return data, ref


def check_rows(rows, ref, fmt, what=""):
    """The oracle bars of the module docstring; every figure is printed before it is asserted."""
    d = gu.db_diff(rows, ref)
    full = gu.full_row_diff(rows, ref, bar=None) if fmt != "f32" else float("nan")
    print(f"{what}: max |dB diff| above the floor {d:.3e}, every bin {full:.3e}")
    assert d <= gu.DB_TOL, what
    gu.assert_same_peak_bins(rows, np.argmax(ref, 1))
    if fmt in ("s8", "u8"):
        assert gu.full_row_diff(rows, ref) <= gu.DB_TOL, what
    elif fmt == "s16":
        assert gu.full_row_diff(rows, ref, bar=gu.DB_TOL_S16_EVERY_BIN) <= gu.DB_TOL_S16_EVERY_BIN, what


def _device_copy(torch, raw, off):
    """``raw`` at byte ``off`` of a larger zeroed uint8 device buffer."""
    buf = torch.zeros(raw.size + 64, dtype=torch.uint8, device="cuda")
    t = buf[off:off + raw.size]
    t.copy_(torch.from_numpy(raw))
    return t


def _run_tensor(torch, e, t, frames, n):
    rows = torch.empty((frames, n), dtype=torch.float32, device="cuda")
    e.process_tensor(t, frames, 0, rows)
    torch.cuda.synchronize()
    return rows.cpu().numpy()


# ---------------------------------------------------------------- §1 direct-load kernels
# (N, format, frame counts, table rows).  Frame counts from the code: the direct grid of an
# RS-residue size rounds up to 8 * RS frames with inactive items, so 1, 7 and 9; the staged
# grid is min(items, resident workgroups).  9 alone at 128 K.  The last two have no staged
# form (the frame does not fit the exchange buffer): both offsets take the direct kernel.
DIRECT_CASES = (
    [(n, f, (1, 7, 9), f"{n}/{f}/A+U") for n in (8192, 16384, 32768) for f in ("s8", "u8", "s16")]
    + [(65536, f, (1, 7, 9), f"65536/{f}/A+U") for f in ("s8", "u8")]
    + [(32768, "f32", (1, 7, 9), "32768/f32/A+U"), (65536, "f32", (1, 7, 9), "65536/f32/A+U")]
    + [(65536, "s16", (9,), "65536/s16/A=U"), (131072, "s8", (9,), "131072/s8/A=U")]
)


@pytest.mark.parametrize("n,fmt,counts,row", DIRECT_CASES, ids=[f"{c[0]}-{c[1]}" for c in DIRECT_CASES])
def test_direct_load_kernels_on_unaligned_input(rfa, n, fmt, counts, row):
    """Table rows ``<N>/<fmt>/A`` and ``/U``: the same bytes at a 16-byte aligned device pointer
    (staged form where one exists) and ``load_alignment(fmt)`` bytes further (direct form: buffer
    loads, a grid of one workgroup per item, items rounded up to 8 * RS frames).  Both meet the
    oracle bars and are bit-identical (module docstring: same float operations per sample)."""
    torch = pytest.importorskip("torch")
    data, ref = _case(n, fmt, max(counts))
    raw = np.frombuffer(data, np.uint8)
    al = LOAD_ALIGN[fmt]
    with rfa.SpectrumEngine(n, "blackman", fmt, ring_rows=0) as e:
        for frames in counts:
            part = raw[:frames * n * BPS[fmt]].copy()
            aligned, shifted = _device_copy(torch, part, 0), _device_copy(torch, part, al)
            assert aligned.data_ptr() % 16 == 0
            assert shifted.data_ptr() % 16 != 0 and shifted.data_ptr() % al == 0
            got = [_run_tensor(torch, e, t, frames, n) for t in (aligned, shifted)]
            for rows, off in zip(got, (0, al)):
                check_rows(rows, ref[:frames], fmt, f"{row} {frames} frames at offset {off}")
            np.testing.assert_array_equal(got[0], got[1], err_msg=f"{row} {frames} frames")


# ---------------------------------------------------------------- §2 strided frames
def strided_copy(data, n, fmt, frames, stride):
    """The packed frames laid ``stride`` bytes apart, the gaps filled with a loud constant
    (0x7f bytes: full scale in s8, 0x7f7f = 32639 in s16)."""
    fb = n * BPS[fmt]
    src = np.frombuffer(data, np.uint8)
    out = np.full((frames - 1) * stride + fb, 0x7f, np.uint8)
    for f in range(frames):
        out[f * stride:f * stride + fb] = src[f * fb:(f + 1) * fb]
    return out


STRIDE_FRAMES = 9
STRIDE_CASES = [(n, f, gap) for n in (8192, 65536, 131072) for f in ("s8", "s16") for gap in ("16", "align")]


@pytest.mark.parametrize("n,fmt,gap", STRIDE_CASES, ids=[f"{c[0]}-{c[1]}-gap{c[2]}" for c in STRIDE_CASES])
def test_strided_frames_at_wide_sizes(rfa, n, fmt, gap):
    """9 frames ``frame + 16`` bytes apart (rows ``<N>/<fmt>/A``: the staged form reads
    ``in + f * frame_stride``; 64 K s16 and 128 K have no staged form) and ``frame +
    load_alignment`` bytes apart (rows ``/U``: the direct form), through the host path, which keeps
    the stride.  The reference is the float64 oracle of the frames cut out and packed; the rows
    also equal the packed call's bit for bit (same kernels or the same operations, docstring)."""
    data, ref = _case(n, fmt, STRIDE_FRAMES)
    stride = n * BPS[fmt] + (16 if gap == "16" else LOAD_ALIGN[fmt])
    laid = strided_copy(data, n, fmt, STRIDE_FRAMES, stride)
    with rfa.SpectrumEngine(n, "blackman", fmt, ring_rows=0) as e:
        rows = e.process(laid, STRIDE_FRAMES, frame_stride=stride)
        packed = e.process(data, STRIDE_FRAMES)
    check_rows(rows, ref, fmt, f"{n}/{fmt} stride frame+{stride - n * BPS[fmt]}")
    np.testing.assert_array_equal(rows, packed)


@pytest.mark.parametrize("stride", [2, 16])
def test_one_frame_ignores_its_stride(rfa, stride):
    """One frame with a stride smaller than the frame is accepted (process_impl validates the
    stride for more than one frame only) and the stride must not be used: row 65536/s8/U
    (stride 2) and /A (stride 16) give the packed call's row."""
    n = 65536
    data, ref = _case(n, "s8", STRIDE_FRAMES)
    one = data[:2 * n]
    with rfa.SpectrumEngine(n, "blackman", "s8", ring_rows=0) as e:
        got = e.process(one, 1, frame_stride=stride)
        packed = e.process(one, 1)
    check_rows(got, ref[:1], "s8", f"one frame, stride {stride}")
    np.testing.assert_array_equal(got, packed)


# ---------------------------------------------------------------- §4 persistent grid, ragged
def wide_lds_bytes(logm):
    """Dynamic LDS of fft_wide_kernel<LOGM, PT = 32> (fft_wide.hip WGeo, restated): the pass-1
    and pass-2 twiddle tables plus the padded M / 2 exchange buffer, in float2."""
    m, tpf = 1 << logm, (1 << logm) // 32
    r1 = 32 if logm >= 14 else 16
    r2 = m // (32 * r1)
    lo = 32 if tpf > 256 else 16
    a_alias = logm == 13
    tw = 32 * (r1 - 1) + (0 if a_alias else (tpf // lo) * (r2 - 1)) + lo * (r2 - 1)
    half = m // 2
    return (tw + half + half // 32) * 8


def resident_bound(cus, logm):
    """Upper bound of the staged kernel's resident workgroups: per CU the smaller of its
    __launch_bounds__ minimum (4 at PT = 32) and 160 KB of LDS over its request."""
    return cus * min(4, (160 * 1024) // wide_lds_bytes(logm))


def ragged_frames(cus, logm):
    """More items than resident workgroups, with a ragged tail: twice the bound plus 3."""
    return 2 * resident_bound(cus, logm) + 3


# staged instantiations (N, format, LOGM of the workgroup) without such a call elsewhere in the
# suite: test_config3_batch_every_bin has 64 K s8, test_cf32_staged_next_item_* the cf32 forms;
# 128 K s8 and 64 K s16 have no staged form.  test_config3_state_at_size feeds
# 300 frames of 32 K s8 but returns no rows, so that form is here too.
RAGGED_CASES = [(n, f, lm) for n, lm in ((8192, 13), (16384, 14), (32768, 15)) for f in ("s8", "u8", "s16")]
RAGGED_CASES.append((65536, "u8", 15))


# BASELINE config 3's capture (test_config3_batch_every_bin): the signal golden_util's bars for a
# long 8-bit batch were worked out on
BATCH_TONES, BATCH_NOISE = ((0.1234, 0.4), (-0.377, 0.01)), 0.05


@functools.lru_cache(maxsize=1)
def _capture(samples):
    x = signals.complex_signal(samples, 4, tones=BATCH_TONES, noise=BATCH_NOISE)
    x.setflags(write=False)
    return x


def ragged_case(n, fmt, frames, base_samples):
    """(bytes, oracle rows): ``frames`` frames cut from one shared noisy capture of
    ``base_samples`` samples (computed once for the module), continued by the same capture
    turned a quarter turn where a case needs more (64 K: the same spectrum, other bytes)."""
    x = _capture(base_samples)
    need = n * frames
    if need > x.size:
        x = np.concatenate([x, 1j * x])
    data = signals.quantize(x[:need], fmt)
    return data, oracle.spectrum_rows(data, signals.FORMATS[fmt], n, frames, None, oracle.WIN_BLACKMAN)


def ragged_base_samples(cus):
    return max(n * ragged_frames(cus, lm) for n, _, lm in RAGGED_CASES if n <= 32768)


@pytest.mark.parametrize("n,fmt,logm", RAGGED_CASES, ids=[f"{c[0]}-{c[1]}" for c in RAGGED_CASES])
def test_persistent_grid_with_uneven_work(rfa, n, fmt, logm):
    """Rows ``<N>/<fmt>/A`` (staged, persistent grid min(items, CUs * occupancy)): 2 * bound + 3
    frames, so every workgroup runs two or three items (64 K: four or five, two residues per
    frame) and stages its next item's frame while it works; every bin of every row against
    float64.  (The count is ragged_frames'; at 4 bytes per sample and at 64 K it makes a 67 MB input.)

    Bars: a call is 16.8 M bins (33.8 M at 64 K), where the worst bin is a tail statistic of a
    handful of Rayleigh-deep bins (golden_util: DB_TOL_BATCH_*, measured on this capture at
    64 K s8, where the reference's own pffft has 4 to 9 of 32.8 M bins beyond 0.01 dB).  So the
    bars are config 3's: at most BATCH_EXCEED_SHARE of the bins beyond 0.01 dB, the worst within
    DB_TOL_BATCH_MAX, every peak bin identical.  They hold for every format and size here: the
    capture's own noise (sigma 0.05, 30 dB above s8 quantisation noise) sets the level of every
    bin whatever the sample format, and a shorter transform has less rounding and a higher
    per-bin noise level.  A row from the wrong frame or residue is dB off in all its bins:
    one such row of 8192 bins is a share of 5e-4 and breaks the worst-bin bar too."""
    torch = pytest.importorskip("torch")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    frames = ragged_frames(cus, logm)
    data, ref = ragged_case(n, fmt, frames, ragged_base_samples(cus))
    with rfa.SpectrumEngine(n, "blackman", fmt, ring_rows=0) as e:
        rows = e.process(data, frames)
    worst = gu.full_row_diff(rows, ref, bar=gu.DB_TOL_BATCH_MAX)
    share = gu.exceed_fraction(rows, ref)
    print(f"{n}/{fmt}: {frames} frames over at most {resident_bound(cus, logm)} workgroups: worst bin {worst:.4f} dB, "
          f"share beyond {gu.DB_TOL} dB {share:.2e}, above the floor {gu.db_diff(rows, ref):.3e} dB")
    assert share <= gu.BATCH_EXCEED_SHARE
    assert worst <= gu.DB_TOL_BATCH_MAX
    gu.assert_same_peak_bins(rows, np.argmax(ref, 1))


# ---------------------------------------------------------------- §5 seam entries
def seam_input(n):
    return np.random.default_rng(n).standard_normal(2 * n).astype(np.float32)


def seam_reference(n):
    """float64 truth of the three seam entries on seam_input(n): ordered spectrum, log-mag row,
    Blackman-windowed log-mag row (window product in fp32, NativeDsp.kt:55-58)."""
    x = seam_input(n)
    exact = np.fft.fft(x[0::2].astype(np.float64) + 1j * x[1::2])
    w = oracle.window(n, oracle.WIN_BLACKMAN)
    xw = oracle.windowed_interleaved(x[0::2].copy(), x[1::2].copy(), w)
    exact_w = np.fft.fft(xw[0::2].astype(np.float64) + 1j * xw[1::2])

    def db(s):
        return np.fft.fftshift(10 * np.log10(np.abs(s) / n)).astype(np.float32)
    return x, exact, db(exact), xw, db(exact_w)


@pytest.mark.parametrize("n", [8192, 16384, 32768, 65536, 131072])
def test_seam_entries_reach_their_kernels(rfa, n):
    """Columns F and C.  The seam entries pass a window that is not the handle's own
    (d_window_none / d_window_black are separate tables), so at N = 32 K / 64 K / 128 K
    launch_main sets variant 1 and launch_fft takes the narrow kernel:
    ``fft_logmag`` -> fft_rows_kernel<14, RS, f32> (RS = 2 / 4 / 8), ``windowed_fft_mag`` ->
    fft_rows_kernel<14, RS, f32p>, ``fft_ordered`` -> RFA_CO(14, RS) (rows <N>/f32/F, /f32p/F,
    /f32/C).  At 8 K / 16 K the same entries stay on the wide kernel's direct f32 / f32p forms
    and its complex-output form fft_wide_kernel<13 | 14, 32, 1, f32, CO>.  Against float64
    (0.01 dB; ordered spectrum 2e-6 relative, test_gpu_seam.py's bar) and the reference pffft."""
    check_seam_entries(rfa, n)


def check_seam_entries(rfa, n):
    """The three seam entries of one handle of size ``n`` on seam_input(n), against float64 and,
    where it is built, the reference's pffft (shared with tests/test_gpu_fft_small.py)."""
    x, exact, ref_db, xw, ref_wdb = seam_reference(n)
    with rfa.SpectrumEngine(n, "blackman", "s8", ring_rows=0) as e:
        cx = e.fft_ordered(x)
        mag = e.fft_logmag(x)
        wmag = np.empty(n, np.float32)
        assert e.windowed_fft_mag(x[0::2].copy(), x[1::2].copy(), wmag)
    g = cx[0::2].astype(np.float64) + 1j * cx[1::2]
    rel = np.abs(g - exact).max() / np.abs(exact).max()
    d_mag, d_wmag = gu.db_diff(mag, ref_db), gu.db_diff(wmag, ref_wdb)
    print(f"{n}: ordered rel err {rel:.3e}, fft_logmag {d_mag:.3e} dB, windowed_fft_mag {d_wmag:.3e} dB above the floor")
    assert rel < 2e-6
    assert d_mag <= gu.DB_TOL
    assert d_wmag <= gu.DB_TOL
    if oracle.ref_available():
        r = oracle.ref_fft_ordered(x)
        rr = r[0::2].astype(np.float64) + 1j * r[1::2]
        assert np.abs(g - rr).max() / np.abs(rr).max() < 2e-6
        assert gu.pffft_diff(mag, oracle.ref_fft_logmag(x)) <= gu.DB_TOL
        assert gu.pffft_diff(wmag, oracle.ref_fft_logmag(xw)) <= gu.DB_TOL


# ---------------------------------------------------------------- §6 state behind the direct kernel
def test_state_behind_the_direct_kernel(rfa):
    """Row 65536/s8/U with a ring of 12 rows, peak-hold and EMA: 20 frames at an aligned device
    pointer on one handle and 2 bytes further on a second.  On each handle the device ring --
    read raw and gathered through ``ring_positions``: the direct kernel writes the residue-major
    store-tile order itself -- holds the rows the same call returned, bit for bit, at (-g) mod R;
    peaks and EMA meet the state rules of tests/test_gpu_state_exact.py on those rows.  The two
    handles agree bit for bit (docstring: the two forms round alike)."""
    torch = pytest.importorskip("torch")
    from test_gpu_state_exact import ALPHA, Truth, _assert_ema, _s8_calls, _same_bits
    n, frames, ring_rows = 65536, 20, 12
    raw = np.frombuffer(_s8_calls(n, (frames,), 65)[0][0], np.uint8)
    hip = ctypes.CDLL("libamdhip64.so")
    out = []
    for off in (0, 2):
        t = _device_copy(torch, raw, off)
        assert (t.data_ptr() % 16 == 0) == (off == 0)
        with rfa.SpectrumEngine(n, "blackman", "s8", avg="ema", ema_alpha=ALPHA, peak_hold=True,
                                ring_rows=ring_rows) as e:
            e.set_tuning(433_000_000, 1000 * n)
            rows = _run_tensor(torch, e, t, frames, n)
            e.synchronize()
            ring, ri, wi = e.ring()
            assert (ri, wi) == ((-(frames - 1)) % ring_rows, (-frames) % ring_rows)
            live = list(range(frames - ring_rows, frames))
            at = [(-g) % ring_rows for g in live]
            _same_bits(ring[at], rows[live], f"offset {off}: ring rows (rfa_get_ring)")
            pos = e.ring_positions()
            assert e.ring_order == 2 and np.array_equal(np.sort(pos), np.arange(n))
            r, p, m = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
            assert rfa.lib().rfa_get_device_state(e.handle, ctypes.byref(r), ctypes.byref(p), ctypes.byref(m)) == 0
            dev = np.empty((ring_rows, n), np.float32)
            assert hip.hipMemcpy(ctypes.c_void_p(dev.ctypes.data), r, ctypes.c_size_t(dev.nbytes), 2) == 0
            _same_bits(dev[at][:, pos], rows[live], f"offset {off}: device ring through ring_positions")
            truth = Truth(n, ALPHA)
            truth.feed(rows)
            peaks, ema = e.peaks(), e.ema()
            _same_bits(peaks, truth.peaks, f"offset {off}: peaks")
            _assert_ema(ema, truth.ema, truth.m, ALPHA, f"offset {off}")
        out.append((rows, ring, peaks, ema))
    for a, b, what in zip(out[0], out[1], ("rows", "ring", "peaks", "EMA")):
        _same_bits(b, a, f"aligned vs 2 bytes in: {what}")


# ---------------------------------------------------------------- §7 argument checks
@pytest.mark.parametrize("fmt,bad", [("s8", 1), ("u8", 1), ("s16", 2), ("f32", 4)])
def test_misaligned_arguments_are_refused(rfa, fmt, bad):
    """A pointer or a stride that breaks load_alignment(fmt) -- an odd byte for 8-bit, 2 mod 4
    for s16, 4 mod 8 for f32 -- is refused on the host with RFA_ERR_INVALID before anything is
    launched, and the handle then serves the next valid call (row 8192/<fmt>/U: load_alignment
    bytes in)."""
    torch = pytest.importorskip("torch")
    from rfanalyzer_amd import RfaError
    n, frames = 8192, 2
    data, ref = _case(n, fmt, 9)
    fb = n * BPS[fmt]
    part = np.frombuffer(data, np.uint8)[:frames * fb].copy()
    al = LOAD_ALIGN[fmt]
    t = _device_copy(torch, part, al)
    rows = torch.empty((frames, n), dtype=torch.float32, device="cuda")
    with rfa.SpectrumEngine(n, "blackman", fmt, ring_rows=0) as e:
        e.process_tensor(t, frames, 0, rows)  # (binds the engine to torch's stream)
        for ptr, stride in ((t.data_ptr() - al + bad, 0), (t.data_ptr(), fb + bad)):
            assert ptr % al or stride % al
            with pytest.raises(RfaError) as err:
                e.process_device(ptr, 1, stride, rows.data_ptr())
            assert err.value.status == RFA_ERR_INVALID
            assert "misaligned" in str(err.value)
        got = _run_tensor(torch, e, t, frames, n)
    check_rows(got, ref[:frames], fmt, f"8192/{fmt} after the refusals")
