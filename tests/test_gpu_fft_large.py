"""GPU: the large-N pair at N = 256 K, 512 K and 1 M (csrc/fft_large.hip, ``launch_large`` in
engine.hip) on the calls the rest of the suite does not make: several frames,
a pointer that is only ``load_alignment``-aligned, a frame stride, and misaligned 8-bit frames
behind the scratch split.  Every case names the row of the table in DESIGN.md §5.5 it runs
(``<N>/<formats>/<column>``, columns A = 16-byte aligned and packed, U = only
``load_alignment``-aligned pointer, S = frame stride) and the line it aims at:

* §1 ``test_per_tile_front_kernel``: ``dif_front_kernel<S, FMT>`` for s16, f32 and f32p with
  ``blockIdx.y`` > 0 (``a.in + f * a.frame_stride``, ``a.z + f * n``).  Its 16-bit form fetches
  the tile with 16-byte buffer loads (``raw_buffer_load_b128(in_rs, pc * 16, (j * M + m0) * SB)``)
  from a base that is only 4-byte aligned; its planar form reads the imaginary plane at
  ``soff + n * 4`` inside a resource of ``n * SB * PLANES`` bytes, so a stride must not move it.
* §2 ``test_8bit_strides``: stride frame + 16 (``launch_s``: the pipelined kernel's ``stage``
  reads ``a.in + f * a.frame_stride``) and frame + 2 (``launch_large``: ``hipMemcpy2DAsync``
  with ``sp = A.frame_stride`` since ``cnt > 1``).
* §3 ``test_misaligned_8bit_across_the_scratch_split``: 65 frames at 256 K are two scratch
  batches (64 + 1); the second copies from ``a.in + f0 * a.frame_stride`` with ``f0`` = 64 into
  the start of ``d_dit_in``.
* §4 (512 K, S = 16, ``cols_to_rows_kernel<16>``, 32 frames per scratch batch): parameters
  added to tests/test_gpu_parity.py ``test_large_n_batches_cross_the_scratch_split``,
  ``test_large_n_seams`` and ``test_large_n_front_kernel_alignment_paths``.

Bit identity.  One front kernel serves every layout of one (N, format): the per-tile kernel for
16- and 32-bit input, the pipelined kernel for 8-bit input (a misaligned 8-bit call is copied
16-byte aligned first, "so every 8-bit frame takes the same kernel", ``launch_large``).  Pointer
and stride enter only the buffer resource's base (``make_rsrc(a.in + f * a.frame_stride, ...)``);
the per-sample arithmetic -- ``convert_raw``, ``x * w[j]``, ``dft<S>``, the ``C (1 + D)`` twiddle,
kernel B on the scratch -- reads nothing else of the call.  So all layouts of a case are asserted
bit-identical.

Signal: the one of ``test_large_n_batches_cross_the_scratch_split`` (tone 0.4 at 0.2113, noise
0.05, drift 2e-4).  Bars: 0.01 dB above the Parseval floor and identical peak bins against
float64.  The every-bin maximum is printed, not asserted: a call has 0.8 M to 17 M bins and its
worst bin is a tail statistic of a few Rayleigh-deep bins (the reference's own pffft is 0.003 to
0.017 dB off float64 there on these inputs, up to 0.05 dB on other seeds of the 65-frame capture;
tests/test_fft_large_host.py prints it and holds pffft to half the floor bar on every input
chosen here).

Measured on MI355X (first green run, maxima over the cases of each test; above the floor /
every bin, dB): per-tile front kernel 2.4e-3 (512 K f32p) / 0.0162 (512 K s16; 1 M s16 0.0129,
512 K f32 0.0113, every other case below 0.007); 8-bit strides 2.5e-3 / 4.3e-3; 65 frames across
the scratch split 4.7e-3 / 0.0123.  Every bit-identity held.
"""
import functools

import numpy as np
import pytest

import golden_util as gu
import oracle
import signals
import test_gpu_fft_paths as tp
from test_gpu_fft_paths import BPS, LOAD_ALIGN, _device_copy, strided_copy

pytestmark = pytest.mark.gpu

SIZES = (262144, 524288, 1048576)
TONES, NOISE, DRIFT = ((0.2113, 0.4),), 0.05, 2e-4
SCRATCH_BYTES = 128 << 20


def scratch_batch(n):
    """Frames per scratch batch (engine.hip rfa_create: 128 MiB of complex f32 scratch z)."""
    return SCRATCH_BYTES // (8 * n)


@functools.lru_cache(maxsize=2)
def large_case(n, fmt, frames, seed):
    """(bytes, float64-oracle rows) of ``frames`` consecutive frames of one drifting capture."""
    data = signals.frames_bytes(n, frames, fmt, seed, tones=TONES, noise=NOISE, drift=DRIFT)
    ref = oracle.spectrum_rows(data, signals.FORMATS[fmt], n, frames, None, oracle.WIN_BLACKMAN)
    ref.setflags(write=False)
    return data, ref


def check_large(rows, ref, what):
    """The module's bars; every figure is printed before it is asserted (every bin: printed only)."""
    d = gu.db_diff(rows, ref)
    full = gu.full_row_diff(rows, ref, bar=None)
    print(f"{what}: max |dB diff| above the floor {d:.3e}, every bin (not asserted) {full:.3e}")
    assert d <= gu.DB_TOL, what
    gu.assert_same_peak_bins(rows, np.argmax(ref, 1))
    return d, full


# ---------------------------------------------------------------- §1 per-tile front kernel
TILE_FRAMES = 3
TILE_FORMATS = ("s16", "f32", "f32p")
TILE_CASES = [(n, f) for n in SIZES for f in TILE_FORMATS]


def tile_seed(n):
    return n + 3


@pytest.mark.parametrize("n,fmt", TILE_CASES, ids=[f"{n}-{f}" for n, f in TILE_CASES])
def test_per_tile_front_kernel(rfa, n, fmt):
    """Rows ``<N>/<fmt>/A``, ``/U`` and ``/S``: 3 frames (grid (128, 3)) packed at an aligned device
    pointer, packed ``load_alignment`` bytes further, and through the host path ``frame +
    load_alignment`` and ``frame + 16`` bytes apart with 0x7f bytes in the gaps.  All four meet
    the bars and are bit-identical (module docstring)."""
    torch = pytest.importorskip("torch")
    data, ref = large_case(n, fmt, TILE_FRAMES, tile_seed(n))
    raw = np.frombuffer(data, np.uint8)
    fb, al = n * BPS[fmt], LOAD_ALIGN[fmt]
    got = {}
    with rfa.SpectrumEngine(n, "blackman", fmt, ring_rows=0) as e:
        for col, off in (("A", 0), ("U", al)):
            t = _device_copy(torch, raw, off)
            assert t.data_ptr() % al == 0 and (t.data_ptr() % 16 == 0) == (off == 0)
            got[f"{col} offset {off}"] = tp._run_tensor(torch, e, t, TILE_FRAMES, n)
            del t
        for gap in (al, 16):
            laid = strided_copy(data, n, fmt, TILE_FRAMES, fb + gap)
            got[f"S stride frame+{gap}"] = e.process(laid, TILE_FRAMES, frame_stride=fb + gap)
    first = next(iter(got.values()))
    for what, rows in got.items():
        check_large(rows, ref, f"{n}/{fmt}/{what}")
    for what, rows in got.items():
        np.testing.assert_array_equal(rows, first, err_msg=f"{n}/{fmt}/{what}")


# ---------------------------------------------------------------- §2 8-bit strides
BYTE_N, BYTE_FRAMES = 262144, 9


def byte_seed(n):
    return n + 3


@pytest.mark.parametrize("fmt", ["s8", "u8"])
def test_8bit_strides(rfa, fmt):
    """Rows 262144/<fmt>/A and /S, 9 frames through the host path (a 16-byte aligned buffer that
    keeps the stride): packed; ``frame + 16`` bytes apart -- still aligned, ``launch_s`` hands
    ``frame_stride`` to ``dif_front_pipe_kernel``; ``frame + 2`` bytes apart -- ``launch_large``
    copies with ``hipMemcpy2DAsync(d_dit_in, fb, A.in, sp = frame_stride, fb, cnt = 9)``.  Both
    are bit-identical to the packed call and meet the bars."""
    n, frames = BYTE_N, BYTE_FRAMES
    data, ref = large_case(n, fmt, frames, byte_seed(n))
    fb = n * BPS[fmt]
    with rfa.SpectrumEngine(n, "blackman", fmt, ring_rows=0) as e:
        packed = e.process(data, frames)
        check_large(packed, ref, f"{n}/{fmt}/A packed")
        for gap in (16, 2):
            rows = e.process(strided_copy(data, n, fmt, frames, fb + gap), frames, frame_stride=fb + gap)
            check_large(rows, ref, f"{n}/{fmt}/S stride frame+{gap}")
            np.testing.assert_array_equal(rows, packed, err_msg=f"stride frame+{gap}")


# ---------------------------------------------------------------- §3 misaligned, across the split
SPLIT_N = 262144
SPLIT_FRAMES = scratch_batch(SPLIT_N) + 1
# over 17 M bins the floor figure is a tail statistic too: on the parity module's 65-frame capture
# (seed n + 3) the reference's own pffft is 0.0093 dB from float64 at the floor; on this one 0.0043
SPLIT_SEED = SPLIT_N + 10


def test_misaligned_8bit_across_the_scratch_split(rfa):
    """Row 262144/s8/U with 65 frames (34 MB in): 64 per scratch batch, so ``launch_large`` runs
    two batches and the second copies from ``a.in + 64 * frame_stride``.  At an aligned device
    pointer and 2 bytes further: bit-identical, both within the bars."""
    torch = pytest.importorskip("torch")
    n, frames = SPLIT_N, SPLIT_FRAMES
    data, ref = large_case(n, "s8", frames, SPLIT_SEED)
    raw = np.frombuffer(data, np.uint8)
    got = []
    with rfa.SpectrumEngine(n, "blackman", "s8", ring_rows=0) as e:
        for off in (0, 2):
            t = _device_copy(torch, raw, off)
            assert (t.data_ptr() % 16 == 0) == (off == 0) and t.data_ptr() % 2 == 0
            got.append(tp._run_tensor(torch, e, t, frames, n))
            del t
    for rows, off in zip(got, (0, 2)):
        check_large(rows, ref, f"{n}/s8/{'AU'[off > 0]} {frames} frames at offset {off}")
    np.testing.assert_array_equal(got[0], got[1])
