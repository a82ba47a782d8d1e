"""GPU: ``fft_rows_kernel<LOGM, 1, FMT>`` (csrc/fft_kernels.hip), the kernel of
every call at N = 64 ... 4096, walked the way tests/test_gpu_fft_paths.py walks N = 8 K ... 128 K.

A workgroup holds ``Geo<LOGM>::SLOTS = 256 / (N / 16)`` frames side by side (64, 32, 16, 8, 4,
2 frames at N = 64 ... 2048, one at 4096); each of the seven sizes has its own pass structure
(radix-16 passes plus a trailing 4, 8, none, 2, 4, 8, none).  Every case names the row of the
table in DESIGN.md §5.2 it runs (``<N>/<format>/<column>``, columns A = 16-byte aligned and
packed, U = only ``load_alignment``-aligned pointer, S = frame stride, C = complex output) and the
line of the kernel it aims at:

* §1 ``test_slot_geometry``: 1, SLOTS - 1, SLOTS, SLOTS + 1 and 5 * SLOTS + 3 frames -- ``decode``
  (``frame = u * SLOTS + slot``), ``buf = data + slot * PADM``, the tail slots' ``if (!active)
  return`` and ``issue``'s ``act ? fr : 0``.
* §2 ``test_many_workgroups``: 66 workgroups of 64 slots with a ragged tail.
* §3 ``test_strided_frames``: ``fb = a.in + frame * a.frame_stride`` for every sample format;
  ``load_raw<4>`` reads the imaginary plane at ``f[n + s]`` of that frame, whatever the stride.
* §4 ``test_unaligned_device_pointer``: ``load_raw`` at a pointer that is only
  ``load_alignment``-aligned.
* §5 ``test_other_windows``: the Hann and the all-ones table through ``a.window[tid + t * TPF]``.
* §6 ``test_seam_entries``: ``launch_fft``'s ``RFA_CO(L, 1)`` (complex output) and the f32 / f32p
  forms under the seam windows.
* §7 ``test_ring_written_by_the_kernel``: ``store(row, ring)`` with ``ring_first`` > 0.

Bit identity.  A frame's arithmetic does not depend on its slot, its workgroup or the batch it
came in.  From the source: ``issue`` loads ``raw[t] = load_raw(fb, tid + t * TPF, n)`` with ``tid``
the thread's index inside its slot; ``body`` forms ``convert_raw(raw[t]) * a.window[tid + t *
TPF]`` (one fp32 product per component), ``run_passes`` indexes its twiddles by ``tid`` alone
(``butterflies``: ``k = i & (P - 1)``, ``i = tid + b * TPF``) from tables every workgroup copies
from the same ``tw_coarse`` / ``tw_fine``, the slot only selects the LDS region (``slot * PADM``),
and the epilogue is ``db_unscaled`` of the thread's own values.  ``u``, ``slot`` and ``n_frames``
enter only ``decode`` (which frame) and the store address.  The pointer and the stride enter only
``fb``.  So every call's rows are asserted bit-identical to the same frames of the longest call,
strided and shifted calls to the packed aligned one.

Bars: tests/test_gpu_fft_paths.py ``check_rows`` (0.01 dB above the Parseval floor, identical peak
bins, every bin 0.01 dB for 8-bit input and DB_TOL_S16_EVERY_BIN for s16) against the float64
oracle; tests/test_fft_small_host.py holds the reference's own pffft to half of each bar on
every input used here.

Measured on MI355X (first green run, maxima over the cases of each test; above the floor /
every bin, dB): slot geometry 2.1e-3 / 3.2e-3 (s8 1.8e-3 / 1.8e-3, s16 1.6e-3 / 1.6e-3); many
workgroups 1.8e-3 / 1.8e-3; strides and shifted pointer 1.3e-3 / 2.6e-3; Hann and no window
6.4e-4 / 2.7e-4; seam entries: ordered spectrum 1.6e-7 relative, rows 6.1e-5; ring case: rows
6.1e-5, EMA 1.52 ulp(M) against a bar of 11.  Every bit-identity held.
"""
import ctypes
import functools

import numpy as np
import pytest

import golden_util as gu
import oracle
import signals
import test_gpu_fft_paths as tp
from test_gpu_fft_paths import BPS, LOAD_ALIGN, _device_copy, check_rows, strided_copy

pytestmark = pytest.mark.gpu

SIZES = (64, 128, 256, 512, 1024, 2048, 4096)
FORMATS = ("s8", "u8", "s16", "f32", "f32p")
STRIDE_FRAMES = tp.STRIDE_FRAMES
# seeds of the captures: the middle-size module's rule (n + 7 * len(fmt)) except where the
# reference's own pffft is beyond half a bar on that capture (tests/test_fft_small_host.py)
SEEDS = {(512, "s8"): 512 + 1000}
MANY_N, MANY_FMT, MANY_FRAMES, MANY_SEED = 64, "s8", 64 * 65 + 5, 64 + 14


def slots(n):
    """fft_kernels.hip Geo<LOGM>::SLOTS, restated: 16 points per thread, 256 threads."""
    tpf = n // 16
    return 1 if tpf >= 256 else 256 // tpf


def geometry_counts(n):
    """Frame counts of §1: one, a workgroup short of one slot, a full one, one frame into the
    second, and five workgroups plus three slots; duplicates and zero dropped."""
    s = slots(n)
    return sorted({c for c in (1, s - 1, s, s + 1, 5 * s + 3) if c > 0})


def capture_frames(n):
    """Frames of the one capture per (N, format): the longest call of §1, and the 9 of §3 / §4."""
    return max(5 * slots(n) + 3, STRIDE_FRAMES)


def seed(n, fmt):
    return SEEDS.get((n, fmt), n + 7 * len(fmt))


def small_case(n, fmt):
    """(bytes, float64-oracle Blackman rows) of the capture of (N, format): every frame differs."""
    return tp._case(n, fmt, capture_frames(n), seed(n, fmt))


@functools.lru_cache(maxsize=None)
def window_case(n, fmt, window, frames):
    """Oracle rows of the first ``frames`` frames of the capture under another window."""
    data, _ = small_case(n, fmt)
    part = data[:frames * n * BPS[fmt]]
    ref = oracle.spectrum_rows(part, signals.FORMATS[fmt], n, frames, None, gu.WINDOW_IDS[window])
    ref.setflags(write=False)
    return part, ref


@functools.lru_cache(maxsize=1)
def many_case():
    return tp._case(MANY_N, MANY_FMT, MANY_FRAMES, MANY_SEED)


# ---------------------------------------------------------------- §1 slot geometry
GEOMETRY_CASES = [(n, f) for n in SIZES for f in FORMATS]


@pytest.mark.parametrize("n,fmt", GEOMETRY_CASES, ids=[f"{n}-{f}" for n, f in GEOMETRY_CASES])
def test_slot_geometry(rfa, n, fmt):
    """Row ``<N>/<fmt>/A``: prefixes of one capture of 1, SLOTS - 1, SLOTS, SLOTS + 1 and
    5 * SLOTS + 3 frames at an aligned device pointer.  A wrong ``slot * PADM`` mixes neighbouring
    frames; ``u * SLOTS + slot`` off by one shows from the second workgroup on.  Every call
    writes into a row tensor of the longest call's size that was filled with a sentinel: a tail
    slot that stores although ``frame >= n_frames`` (it has loaded frame 0) changes a row behind
    the call's own, inside the tensor.  Every call meets the bars and equals the same frames of
    the longest call bit for bit; the host path gives the same rows."""
    torch = pytest.importorskip("torch")
    data, ref = small_case(n, fmt)
    fb = n * BPS[fmt]
    counts = geometry_counts(n)
    top = counts[-1]
    assert top <= capture_frames(n)
    dev = _device_copy(torch, np.frombuffer(data, np.uint8)[:top * fb].copy(), 0)
    assert dev.data_ptr() % 16 == 0
    sentinel = 12345.0
    with rfa.SpectrumEngine(n, "blackman", fmt, ring_rows=0) as e:
        got = {}
        for frames in reversed(counts):
            rows = torch.full((top, n), sentinel, dtype=torch.float32, device="cuda")
            e.process_tensor(dev[:frames * fb], frames, 0, rows)
            torch.cuda.synchronize()
            rows = rows.cpu().numpy()
            assert (rows[frames:] == sentinel).all(), f"{n}/{fmt}: {frames} frames wrote behind their rows"
            got[frames] = rows[:frames]
            check_rows(got[frames], ref[:frames], fmt, f"{n}/{fmt}/A {frames} frames ({slots(n)} slots)")
            np.testing.assert_array_equal(got[frames], got[top][:frames], err_msg=f"{n}/{fmt} {frames} frames")
        host = e.process(data[:top * fb], top)
    np.testing.assert_array_equal(host, got[top])


# ---------------------------------------------------------------- §2 many workgroups
def test_many_workgroups(rfa):
    """Row 64/s8/A with 64 * 65 + 5 frames: 66 workgroups (``items = (n_frames + SLOTS - 1) /
    SLOTS``, one item per workgroup: ``Persist`` is false), the last with 5 of 64 slots active;
    0.5 MB in, 1 MB of rows."""
    data, ref = many_case()
    with rfa.SpectrumEngine(MANY_N, "blackman", MANY_FMT, ring_rows=0) as e:
        rows = e.process(data, MANY_FRAMES)
    check_rows(rows, ref, MANY_FMT, f"64/s8/A {MANY_FRAMES} frames over 66 workgroups")


# ---------------------------------------------------------------- §3 strides
STRIDE_SIZES = (64, 1024, 4096)
STRIDE_FORMATS = ("s8", "s16", "f32", "f32p")
STRIDE_CASES = [(n, f, g) for n in STRIDE_SIZES for f in STRIDE_FORMATS for g in ("align", "16")]


@pytest.mark.parametrize("n,fmt,gap", STRIDE_CASES, ids=[f"{c[0]}-{c[1]}-gap{c[2]}" for c in STRIDE_CASES])
def test_strided_frames(rfa, n, fmt, gap):
    """Row ``<N>/<fmt>/S``: 9 frames ``frame + load_alignment`` and ``frame + 16`` bytes apart
    through the host path, which keeps the stride; the gaps hold 0x7f bytes.  A planar frame is
    ``float re[N]`` then ``float im[N]`` (rfa.h RFA_IN_F32_PLANAR), so its gap follows the
    imaginary plane and ``load_raw<4>`` must find that plane N floats after the frame's start,
    not a stride after it.  The rows meet the bars on the packed frames' oracle and equal the
    packed call's bit for bit.  One frame with a stride smaller than the frame (process_impl
    validates the stride for more than one frame only) must not use the stride."""
    data, ref = small_case(n, fmt)
    fb = n * BPS[fmt]
    stride = fb + (16 if gap == "16" else LOAD_ALIGN[fmt])
    laid = strided_copy(data, n, fmt, STRIDE_FRAMES, stride)
    with rfa.SpectrumEngine(n, "blackman", fmt, ring_rows=0) as e:
        rows = e.process(laid, STRIDE_FRAMES, frame_stride=stride)
        packed = e.process(data[:STRIDE_FRAMES * fb], STRIDE_FRAMES)
        one = e.process(data[:fb], 1, frame_stride=LOAD_ALIGN[fmt])
    check_rows(rows, ref[:STRIDE_FRAMES], fmt, f"{n}/{fmt}/S stride frame+{stride - fb}")
    np.testing.assert_array_equal(rows, packed)
    np.testing.assert_array_equal(one, packed[:1])


# ---------------------------------------------------------------- §4 unaligned device pointer
POINTER_CASES = [(n, f) for n in STRIDE_SIZES for f in STRIDE_FORMATS]


@pytest.mark.parametrize("n,fmt", POINTER_CASES, ids=[f"{n}-{f}" for n, f in POINTER_CASES])
def test_unaligned_device_pointer(rfa, n, fmt):
    """Rows ``<N>/<fmt>/A`` and ``/U``: the same 9 frames at a 16-byte aligned device pointer and
    ``load_alignment(fmt)`` bytes further.  One kernel serves both (``load_raw`` is a 2-, 4- or
    8-byte global load); the rows are bit-identical and meet the bars."""
    torch = pytest.importorskip("torch")
    data, ref = small_case(n, fmt)
    raw = np.frombuffer(data, np.uint8)[:STRIDE_FRAMES * n * BPS[fmt]].copy()
    al = LOAD_ALIGN[fmt]
    aligned, shifted = _device_copy(torch, raw, 0), _device_copy(torch, raw, al)
    assert aligned.data_ptr() % 16 == 0
    assert shifted.data_ptr() % 16 != 0 and shifted.data_ptr() % al == 0
    with rfa.SpectrumEngine(n, "blackman", fmt, ring_rows=0) as e:
        got = [tp._run_tensor(torch, e, t, STRIDE_FRAMES, n) for t in (aligned, shifted)]
    for rows, col in zip(got, "AU"):
        check_rows(rows, ref[:STRIDE_FRAMES], fmt, f"{n}/{fmt}/{col}")
    np.testing.assert_array_equal(got[0], got[1])


# ---------------------------------------------------------------- §5 windows
WINDOW_N = 512
WINDOW_CASES = [(w, f) for w in ("hann", "none") for f in ("s8", "f32")]


@pytest.mark.parametrize("window,fmt", WINDOW_CASES, ids=[f"{w}-{f}" for w, f in WINDOW_CASES])
def test_other_windows(rfa, window, fmt):
    """Row 512/<fmt>/A with the Hann and the all-ones window table, SLOTS + 1 = 9 frames (a full
    workgroup and one slot of the next), against the float64 oracle with the same window."""
    frames = slots(WINDOW_N) + 1
    part, ref = window_case(WINDOW_N, fmt, window, frames)
    with rfa.SpectrumEngine(WINDOW_N, window, fmt, ring_rows=0) as e:
        rows = e.process(part, frames)
    check_rows(rows, ref, fmt, f"512/{fmt}/A window {window}")


# ---------------------------------------------------------------- §6 seam entries
@pytest.mark.parametrize("n", SIZES)
def test_seam_entries(rfa, n):
    """Rows ``<N>/f32/C`` (``fft_ordered`` -> ``RFA_CO(L, 1)``: fft_rows_kernel<L, 1, f32, CO>,
    ``out[r + RS * ks]``), ``<N>/f32/A`` under the all-ones seam table (``fft_logmag``) and
    ``<N>/f32p/A`` under the unscaled Blackman seam table (``windowed_fft_mag``), one frame each
    through ``single_frame``: against float64 (ordered spectrum 2e-6 relative, rows 0.01 dB above
    the floor) and against the reference's pffft where it is built (N >= 32 for pffft)."""
    tp.check_seam_entries(rfa, n)


# ---------------------------------------------------------------- §7 ring written by the kernel
RING_N, RING_ROWS, RING_CALLS, RING_SEED = 256, 12, (20, 7), 66


def ring_calls():
    from test_gpu_state_exact import _s8_calls
    return _s8_calls(RING_N, RING_CALLS, RING_SEED)


def test_ring_written_by_the_kernel(rfa):
    """Row 256/s8/A (16 slots) with a ring of 12 rows, peak-hold and EMA; calls of 20 and of 7
    frames with caller rows, so the kernel stores every value twice (``store(row, ring)``) and
    skips the ring for ``frame < ring_first`` = 8 in the first call.  The ring order at this size
    is 1 (no permutation): ``rfa_get_ring`` holds the returned rows bit for bit at (-g) mod R,
    -9999 nowhere once 12 frames are in; peaks and EMA meet the rules of
    tests/test_gpu_state_exact.py on the device's own rows; the rows meet the oracle bars."""
    from oracle import processor
    from test_gpu_state_exact import ALPHA, Truth, _assert_ema, _same_bits
    n, ring_rows = RING_N, RING_ROWS
    truth = Truth(n, ALPHA)
    done = 0
    with rfa.SpectrumEngine(n, "blackman", "s8", avg="ema", ema_alpha=ALPHA, peak_hold=True,
                            ring_rows=ring_rows) as e:
        e.set_tuning(433_000_000, 1000 * n)
        assert e.ring_order == 1
        every = np.empty((0, n), np.float32)
        for k, (data, frames) in enumerate(ring_calls()):
            what = f"256/s8/A call {k} ({frames} frames)"
            rows = e.process(data, frames)
            ref = oracle.spectrum_rows(data, oracle.IN_S8, n, frames, None, oracle.WIN_BLACKMAN)
            check_rows(rows, ref, "s8", what)
            every = np.concatenate([every, rows])
            done += frames
            ring, ri, wi = e.ring()
            assert (ri, wi) == ((-(done - 1)) % ring_rows, (-done) % ring_rows), what
            live = list(range(done - ring_rows, done))
            _same_bits(ring[[(-g) % ring_rows for g in live]], every[live], f"{what}: ring rows (rfa_get_ring)")
            assert not (ring == processor.RING_FILL).any()
            r, p, m = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
            assert rfa.lib().rfa_get_device_state(e.handle, ctypes.byref(r), ctypes.byref(p), ctypes.byref(m)) == 0
            dev = np.empty((ring_rows, n), np.float32)
            hip = ctypes.CDLL("libamdhip64.so")
            assert hip.hipMemcpy(ctypes.c_void_p(dev.ctypes.data), r, ctypes.c_size_t(dev.nbytes), 2) == 0
            _same_bits(dev, ring, f"{what}: device ring, no permutation")
            truth.feed(rows)
            _same_bits(e.peaks(), truth.peaks, f"{what}: peaks")
            _assert_ema(e.ema(), truth.ema, truth.m, ALPHA, what)
