"""GPU: peak-hold raised by the 64 K main kernel, EMA over its live tail only.

A warm call of the staged two-residue 8-bit kernel raises the peaks' storage-order shadow in
its epilogue and the state pass folds it and reads only the last T(alpha) rows; every other
call takes the full pass.  Here every path is held, as tests/test_gpu_state_exact.py holds the
state kernels, against the sequential restatement on the device's own ring rows: peaks bit
for bit, the EMA's non-finite positions exactly and its finite bins within that file's
ulp(M) (1 + 1/alpha) bar.

N = 65536, ring_rows = frames per call = 300 (600 work items on 256 workgroups: more than
two items each), alpha = 0.5 (T = 51: the tail is a small part of the call) unless a case
says otherwise.  The last test needs no GPU: T(alpha), and the 2^-26 dB bound of the tail on
the fp32 recurrence itself.
"""
import numpy as np
import pytest

from test_gpu_state_exact import F32, Truth, _assert_ema, _same_bits

gpu = pytest.mark.gpu

N, R, ALPHA = 65536, 300, 0.5
QUIET, PLAIN, LOUD = 6.0, 12.0, 24.0  # s8 units per unit of noise: 5 sigma of LOUD stays inside int8

_Z = {}


def _noise():
    """One block of complex noise for every case (each frame with a gain of its own, so peaks
    and EMA depend on which frames were taken); levels are this block scaled."""
    if not _Z:
        rng = np.random.default_rng(65536)
        z = rng.standard_normal((R, 2 * N), dtype=F32)
        z *= rng.uniform(0.5, 1.0, (R, 1)).astype(F32)
        _Z["z"] = z
    return _Z["z"]


def _s8(level, frames=R, zero=()):
    x = np.clip(np.rint(_noise()[:frames] * F32(level)), -128, 127).astype(np.int8)
    for f in zero:
        x[f] = 0
    return x


def _u8(level, frames=R):
    return np.clip(np.rint(_noise()[:frames] * F32(level) + F32(127.4)), 0, 255).astype(np.uint8)


def _last_rows(e, nf):
    """The device's rows of the last call, oldest first (the newest at the ring's read index)."""
    ring, ri, _ = e.ring()
    return ring[[(ri + nf - 1 - k) % ring.shape[0] for k in range(nf)]]


def _call(e, truth, data, nf, what, alpha=ALPHA, rows=False):
    got = e.process(data, nf, rows=rows)
    rows = _last_rows(e, nf)
    if got is not None:
        _same_bits(got, rows, f"{what}: caller rows against the ring")
    truth.feed(rows)
    peaks = e.peaks()
    _same_bits(peaks, truth.peaks, f"{what} peaks")
    if alpha is not None:
        _assert_ema(e.ema(), truth.ema, truth.m, alpha, what)
    return rows, peaks


def _engine(rfa, fmt="s8", alpha=ALPHA, ring_rows=R, avg="ema"):
    return rfa.SpectrumEngine(N, "blackman", fmt, avg=avg, ema_alpha=alpha if alpha is not None else 0.1,
                              peak_hold=True, ring_rows=ring_rows)


@gpu
def test_same_data_again_sets_no_record(rfa):
    """Cold call (full pass), then the same bytes on a warm call: no bin rises."""
    with _engine(rfa) as e:
        t = Truth(N, ALPHA)
        _, p0 = _call(e, t, _s8(PLAIN), R, "cold")
        _, p1 = _call(e, t, _s8(PLAIN), R, "warm, same data")
        _same_bits(p1, p0, "peaks after the same data again")


@gpu
def test_louder_data_sets_a_record_in_every_bin(rfa):
    with _engine(rfa) as e:
        t = Truth(N, ALPHA)
        _, p0 = _call(e, t, _s8(PLAIN), R, "cold")
        _, p1 = _call(e, t, _s8(LOUD), R, "warm, louder")
        assert np.all(p1 > p0), f"{int((p1 <= p0).sum())} bins set no record"
        _, p2 = _call(e, t, _s8(PLAIN), R, "warm, plain again")
        _same_bits(p2, p1, "peaks after the louder call")


@gpu
def test_quieter_data_leaves_the_peaks(rfa):
    with _engine(rfa) as e:
        t = Truth(N, ALPHA)
        _, p0 = _call(e, t, _s8(PLAIN), R, "cold")
        rows, p1 = _call(e, t, _s8(QUIET), R, "warm, quieter")
        assert np.all(rows.max(0) < p0)
        _same_bits(p1, p0, "peaks after quieter data")


@gpu
def test_silent_frames_before_and_inside_the_tail(rfa):
    """An all-zero frame is a -inf row: one before the tail (it has decayed like any other
    frame), one inside it (the average restarts there), and a call that ends on one."""
    with _engine(rfa) as e:
        t = Truth(N, ALPHA)
        _call(e, t, _s8(PLAIN), R, "cold")
        rows, _ = _call(e, t, _s8(LOUD, zero=(100, R - 7)), R, "warm, silent frames")
        assert np.all(np.isneginf(rows[[100, R - 7]])) and np.isfinite(np.delete(rows, [100, R - 7], 0)).all()
        _call(e, t, _s8(LOUD, zero=(R - 1,)), R, "warm, ends silent")
        assert np.all(np.isneginf(e.ema()))
        _call(e, t, _s8(PLAIN), R, "warm, from a -inf average")


@gpu
def test_u8(rfa):
    """The other staged 8-bit instantiation."""
    with _engine(rfa, "u8") as e:
        t = Truth(N, ALPHA)
        _, p0 = _call(e, t, _u8(PLAIN), R, "u8 cold")
        _, p1 = _call(e, t, _u8(LOUD), R, "u8 warm, louder")
        assert np.all(p1 > p0)
        _call(e, t, _u8(QUIET), R, "u8 warm, quieter")


@gpu
def test_misaligned_device_pointer_takes_the_direct_kernel(rfa):
    """Frames 2 bytes into a device buffer: not staged, so the full pass; then an aligned
    warm call, and the misaligned one again."""
    import torch

    with _engine(rfa) as e:
        t = Truth(N, ALPHA)
        buf = torch.zeros(2 * N * R + 16, dtype=torch.int8, device="cuda")

        def device_call(level, off, what):
            buf[off:off + 2 * N * R] = torch.from_numpy(_s8(level).reshape(-1)).cuda()
            torch.cuda.synchronize()
            e.process_device(buf.data_ptr() + off, R)
            e.synchronize()
            rows = _last_rows(e, R)
            t.feed(rows)
            _same_bits(e.peaks(), t.peaks, f"{what} peaks")
            _assert_ema(e.ema(), t.ema, t.m, ALPHA, what)

        device_call(PLAIN, 2, "misaligned, cold")
        device_call(LOUD, 2, "misaligned again")
        device_call(PLAIN, 0, "aligned after misaligned")
        device_call(LOUD * 1.2, 0, "aligned, warm")
        device_call(LOUD * 1.4, 2, "misaligned after warm")
        device_call(QUIET, 0, "aligned after misaligned, quieter")


@gpu
def test_caller_rows_take_the_full_pass(rfa):
    with _engine(rfa) as e:
        t = Truth(N, ALPHA)
        _call(e, t, _s8(PLAIN), R, "cold")
        _call(e, t, _s8(LOUD), R, "rows asked for", rows=True)
        _call(e, t, _s8(LOUD * 1.2), R, "after a rows call", rows=False)
        _call(e, t, _s8(PLAIN), R, "warm", rows=False)


@gpu
def test_ring_wrap(rfa):
    """200 frames per call into the ring of 300: the second and third call wrap."""
    nf = 200
    with _engine(rfa) as e:
        t = Truth(N, ALPHA)
        for k, level in enumerate((PLAIN, LOUD, QUIET, LOUD * 1.2)):
            _call(e, t, _s8(level, nf), nf, f"wrap call {k}", rows=False)


@gpu
def test_reset_between_calls(rfa):
    """A state reset and a retune (both reset the peaks) make the next call cold."""
    with _engine(rfa) as e:
        e.set_tuning(100_000_000, 20_000_000)
        t = Truth(N, ALPHA)
        _call(e, t, _s8(LOUD), R, "cold", rows=False)
        _call(e, t, _s8(PLAIN), R, "warm", rows=False)
        e.reset_state()
        t = Truth(N, ALPHA)
        _call(e, t, _s8(QUIET), R, "after reset_state", rows=False)
        _call(e, t, _s8(PLAIN), R, "warm after reset_state", rows=False)
        e.set_tuning(300_000_000, 20_000_000)  # outside the span: ring cleared, peaks and EMA reset
        t = Truth(N, ALPHA)
        _call(e, t, _s8(QUIET), R, "after a retune", rows=False)
        _call(e, t, _s8(QUIET), R, "warm after a retune", rows=False)


@gpu
def test_small_alpha_reads_every_row(rfa):
    """alpha = 0.01: T = 3518 > 300 frames, the state pass reads the whole call."""
    with _engine(rfa, alpha=0.01) as e:
        t = Truth(N, 0.01)
        _call(e, t, _s8(PLAIN), R, "a=.01 cold", alpha=0.01, rows=False)
        _call(e, t, _s8(LOUD), R, "a=.01 warm", alpha=0.01, rows=False)


@gpu
def test_tail_planned_in_sixteen_chunks(rfa):
    """alpha = 0.2: T = 159 of the 300 frames, 16 chunks planned over the tail (alpha = 0.5 takes
    the eight-chunk plan of a short tail)."""
    with _engine(rfa, alpha=0.2) as e:
        t = Truth(N, 0.2)
        _call(e, t, _s8(PLAIN), R, "a=.2 cold", alpha=0.2, rows=False)
        _call(e, t, _s8(LOUD), R, "a=.2 warm", alpha=0.2, rows=False)
        _call(e, t, _s8(QUIET), R, "a=.2 warm, quieter", alpha=0.2, rows=False)


@gpu
def test_bench_alpha_reads_every_row(rfa):
    """alpha = 0.1, the bench line's: T = 336 > 300 frames."""
    with _engine(rfa, alpha=0.1) as e:
        t = Truth(N, 0.1)
        _call(e, t, _s8(PLAIN), R, "a=.1 cold", alpha=0.1, rows=False)
        _call(e, t, _s8(LOUD), R, "a=.1 warm", alpha=0.1, rows=False)


@gpu
def test_peak_hold_without_average(rfa):
    """avg none: a warm call's state pass reads no row at all; the peaks alone tell."""
    with _engine(rfa, avg="none", alpha=None) as e:
        t = Truth(N, ALPHA)
        _, p0 = _call(e, t, _s8(PLAIN), R, "no avg, cold", alpha=None, rows=False)
        _, p1 = _call(e, t, _s8(LOUD), R, "no avg, warm louder", alpha=None, rows=False)
        assert np.all(p1 > p0)
        _call(e, t, _s8(QUIET), R, "no avg, warm quieter", alpha=None, rows=False)


@gpu
def test_f32_call_is_unchanged(rfa):
    """The float kernel has no peak raise: full pass, call after call."""
    z = _noise()
    with _engine(rfa, "f32") as e:
        t = Truth(N, ALPHA)
        _call(e, t, (z * F32(0.05)).tobytes(), R, "f32 first", rows=False)
        _call(e, t, (z * F32(0.1)).tobytes(), R, "f32 second", rows=False)


# ---------------------------------------------------------------- no GPU: the tail rule
def tail_frames(alpha):
    """T(alpha) as the engine computes it (fft_kernels.hip ema_tail_frames): the smallest T with
    (1 - alpha)^T <= 2^-51, in double."""
    keep, t = 1.0 - float(F32(alpha)), 1
    while keep ** t > 2.0 ** -51:
        t += 1
    return t


def _ema32(rows, em, alpha):
    al = F32(alpha)
    for x in rows:
        em = (em + al * (x - em)).astype(F32)  # one rounding more than the kernel's fma: inside the bound's slack
    return em


@pytest.mark.parametrize("alpha,t", [(0.5, 51), (0.1, 336), (0.05, 690)])
def test_tail_rule_on_the_cpu(alpha, t):
    """T(alpha), and the bound it stands for: the sequential fp32 recurrence over 500 random dB
    rows in [-200, 50] from a random carried average, and over the last T rows only from the
    same carried average, agree within 2^-26 dB.

    Why 2^-51 and not the 2^-36 that already gives 2^-26 dB in exact arithmetic: in fp32 the
    two runs' gap lives on the average's grid, shrinks by 1 - alpha a frame only on average, and
    is still one ulp (3.815e-06 dB here, above the bound) in a bin with probability about
    (first gap / ulp) x weight.  At 2^-36 that is 58 / 19 / 13 of 131072 bins at alpha 0.5 / 0.1 /
    0.05 for rows like these; at 2^-44 1 / 0 / 0; at 2^-52 none.  (0.05: T = 690 frames, so a call
    of 500 is read whole.)"""
    assert tail_frames(alpha) == t
    keep = 1.0 - float(F32(alpha))
    assert keep ** t <= 2.0 ** -51 < keep ** (t - 1)
    rng = np.random.default_rng(t)
    rows = rng.uniform(-200.0, 50.0, (500, 4096)).astype(F32)
    em_in = rng.uniform(-200.0, 50.0, 4096).astype(F32)
    full = _ema32(rows, em_in, alpha)
    tail = _ema32(rows[max(0, 500 - t):], em_in, alpha)
    worst = float(np.abs(full.astype(np.float64) - tail.astype(np.float64)).max())
    print(f"alpha {alpha}: T = {t}, full against tail max |d| = {worst:.3e} dB (bound {2.0 ** -26:.3e})")
    assert worst <= 2.0 ** -26
