"""GPU: the rational-rate channelizer (rfa_pfb_create_rational, demod.Channelizer.rational /
for_raster_resampled, RasterReceiverBank(resample=True)) against its float64
restatement tests/pfb_rational_ref.py, and against itself bit for bit where the definition
promises that: however the stream is cut into calls, whichever channels are selected, whatever
the raw format or pointer offset.

Every output sample of every selected channel is compared; nothing is floored or excluded.  The
tolerance is the derived worst case eps * (ceil(Tp / M) + 4 * ceil(log2 M)) * max_p sum_t
|g[p + t L]| * max|x| per complex output (pfb_rational_ref.bound); taps are random in [-1, 1]
unless they are a for_raster_resampled prototype, so a dropped or misplaced tap or a wrong phase
is an O(1) error.  The observed max(err / bound) of every case goes to the session summary.

20 Msps to 96 kHz is L / D = 3 / 625 in lowest terms, so the 20 Msps prototype runs as (M, L, D) =
(800, 3, 625): gcd(L, D) = 1 is part of the definition and the unreduced 6 / 1250 is refused.
The two cases whose windows are longer than the call that yields the counted outputs (M = 800 and
M = 4096) get a first call that fills the history; all outputs of both calls are compared."""
import functools

import numpy as np
import pytest

import golden_util as gu
import pfb_rational_ref as ref
from rfanalyzer_amd import _lib
from rfanalyzer_amd import demod

pytestmark = pytest.mark.gpu

SB = {"s8": 2, "u8": 2, "s16": 4, "f32": 8}


def _raw(fmt, n, seed):
    """n random samples as bytes (uint8 array)."""
    rng = np.random.default_rng(seed)
    if fmt == "f32":
        return rng.uniform(-1, 1, 2 * n).astype("<f4").view(np.uint8)
    if fmt == "s16":
        return rng.integers(-32768, 32768, 2 * n, dtype=np.int16).view(np.uint8)
    return rng.integers(0, 256, 2 * n, dtype=np.uint8)


def _taps(T, seed):
    return np.random.default_rng(seed).uniform(-1, 1, T).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _prototype(fs, spacing, L):
    return demod.create_low_pass_taps(L, L * fs, 0.375 * spacing, 0.25 * spacing, 60)


def _run(fmt, M, L, D, g, raw, sizes=None, channels=None, ch=None):
    """The stream through a rational Channelizer in calls of ``sizes`` samples (one call by
    default): [selected, n] complex64.  Every call's count is checked against the count rule."""
    own = ch is None
    ch = ch or demod.Channelizer.rational(fmt, M, L, D, g)
    try:
        if channels is not None:
            ch.set_channels(channels)
        n = raw.size // SB[fmt]
        parts, pos = [], 0
        for s in (sizes or [n]):
            want = ch.max_outputs(s)
            out = ch.process(raw[pos * SB[fmt]:(pos + s) * SB[fmt]])
            assert all(o.size == want for o in out), (s, want)
            parts.append(np.stack(out))
            pos += s
        assert pos == n
        return np.concatenate(parts, axis=1)
    finally:
        if own:
            ch.close()


def _same(a, b):
    assert a.shape == b.shape, (a.shape, b.shape)
    np.testing.assert_array_equal(np.ascontiguousarray(a).view(np.int32), np.ascontiguousarray(b).view(np.int32))


# ------------------------------------------------------------------ accuracy

# The tile plan (channelizer.hip, pfb_plan_rational; kPfbStageBytes = 64 KiB = 8192 points of
# 8 B): NT times per workgroup as the integer path (16 up to M = 256, 8 at 512, 4 up to 1024, 1 at
# 4096); run = ceil((NT-1) D / L) + Tp samples; rows = min(NT, L) tap rows of Tp floats, indexed by
# phase where L <= NT and by time where L > NT.  Plan A stages run and rows where
# run + ceil(rows Tp / 2) <= 8192 points, plan B only the run where run <= 8192, plan C nothing.
#        id  M     L   D     T       fmt    samples (per call)
CASES = {1: (16, 3, 7, 61, "s8", [500]),                     # 215 outputs; A, rows by phase
         2: (48, 4, 9, 190, "s16", [600]),                   # radix 3; T not a multiple of L (Tp = 48, 2 pad taps)
         3: (80, 12, 125, "proto:1000000:12500", "u8", [2083]),   # the 1 Msps prototype, D > M, 200 outputs; A
         4: (800, 3, 625, "proto:20000000:25000", "s8", [9000, 6250]),  # the 20 Msps prototype; 44 + 30 outputs;
                                                             # NT = 4, run = 625 + 8725 > 8192: C
         5: (4096, 2, 8191, 131072, "u8", [65536, 8192]),    # 17 + 2 outputs; NT = 1, Tp = 65536: C, D = L M - 1
         6: (64, 5, 48, 1280, "f32", [9597]),                # 1000 outputs: 63 workgroups, the last holds 8 of 16
         7: (60, 1, 7, 200, "u8", [700]),                    # L = 1: m_n = n D, 100 outputs
         # plan A, rows by time (L = 9 > NT = 8): 27 outputs
         8: (512, 9, 1024, 900, "s16", [3000]),
         # (cases 9 to 12: 18 outputs of a first call that fills the history, then 9)
         # either side of A | B at M = 512 (NT = 8), L = 3, D = 1024: run = ceil(7 * 1024 / 3) + Tp = 2390 + Tp,
         # rows = 3, so A needs 2390 + Tp + ceil(3 Tp / 2) <= 8192: Tp = 2320 (T = 6960) gives 8190 points
         # and is the last with staged taps, Tp = 2321 (T = 6961) gives 8193 and reads taps from global memory
         9: (512, 3, 1024, 6960, "s8", [6000, 3000]),
         10: (512, 3, 1024, 6961, "s16", [6000, 3000]),
         # either side of B | C, same M, L, D: the run alone needs 2390 + Tp <= 8192: Tp = 5802 (T = 17406) is
         # the last staged run, Tp = 5803 (T = 17407) folds from the history and the raw buffer
         11: (512, 3, 1024, 17406, "u8", [6000, 3000]),
         12: (512, 3, 1024, 17407, "s8", [6000, 3000])}
OUTPUTS = {1: 215, 2: 267, 3: 200, 4: 74, 5: 19, 6: 1000, 7: 100, 8: 27, 9: 27, 10: 27, 11: 27, 12: 27}


@functools.lru_cache(maxsize=None)
def _case(cid):
    M, L, D, T, fmt, sizes = CASES[cid]
    if isinstance(T, str):
        _, fs, sp = T.split(":")
        g = _prototype(int(fs), int(sp), L)
    else:
        g = _taps(T, 100 + cid)
    raw = _raw(fmt, sum(sizes), 200 + cid)
    raw.setflags(write=False)
    return M, L, D, fmt, g, raw, sizes


@functools.lru_cache(maxsize=None)
def _device_run(cid):
    M, L, D, fmt, g, raw, sizes = _case(cid)
    y = _run(fmt, M, L, D, g, raw, sizes=sizes)
    y.setflags(write=False)
    return y


def _check_bound(label, y, want, g, x, M, L):
    b = ref.bound(g, x, M, L)
    err = np.abs(y.astype(np.complex128) - want)
    ratio = float(err.max() / b)
    gu.NOTES.append(f"rational channelizer {label}: max err / bound = {ratio:.4f} over {err.size} outputs")
    print(f"rational channelizer {label}: max err {err.max():.3e}, bound {b:.3e}, ratio {ratio:.4f}")
    assert np.all(np.isfinite(y.view(np.float32)))
    assert ratio <= 1.0, (label, ratio)


@pytest.mark.parametrize("cid", sorted(CASES))
def test_accuracy_against_restatement(rfa, cid):
    M, L, D, fmt, g, raw, sizes = _case(cid)
    y = _device_run(cid)
    assert y.shape == (M, OUTPUTS[cid]) == (M, ref.count(sum(sizes), L, D))
    if cid == 4:
        assert (M, L, D) == demod.Channelizer.raster_ratio(20_000_000, 25_000, 96_000)
        assert ref.output_count(sizes[0], sum(sizes), L, D) == 30
    if cid == 3:
        assert (M, L, D) == demod.Channelizer.raster_ratio(1_000_000, 12_500, 96_000)
    x = ref.convert(raw, fmt)
    want = ref.folded(x, g, M, L, D)
    if cid in (1, 2):                                   # small enough for the defining sum itself
        assert np.abs(want - ref.direct(x, g, M, L, D)).max() <= 1e-12
    if cid == 7:                                        # L = 1: output n ends at sample n * D, not n * D + D - 1
        assert np.abs(want[0] - ref.sequential(x, g, L, D)).max() <= 1e-12
    _check_bound(f"case {cid} (M={M} L={L} D={D} T={len(g)} {fmt})", y, want, g, x, M, L)


# ------------------------------------------------------------------ bit-exact properties

SPLITS = {1: [1, 4, 5, 6, 0, 160, 3, 2, 19, 300],     # calls shorter than D / L and one of 0 samples
          6: [47, 1, 0, 5000, 33, 4516],
          8: [700, 1, 0, 341, 1958],                   # rows by time: a call's first tile starts at any phase
          10: [2731, 269, 6000]}                       # taps from global memory; 2731 samples are exactly 9 outputs


@pytest.mark.parametrize("cid", sorted(SPLITS))
def test_split_invariance(rfa, cid):
    M, L, D, fmt, g, raw, sizes = _case(cid)
    assert sum(SPLITS[cid]) == sum(sizes)
    _same(_run(fmt, M, L, D, g, raw, sizes=SPLITS[cid]), _device_run(cid))


def _device_call(ch, raw, n_sel, stride, sentinel=12345.0, offset_samples=0, fmt="s8"):
    """One rfa_pfb_process call on torch tensors: (re, im, n_out) with rows of ``stride`` floats
    prefilled with the sentinel; the raw stream sits ``offset_samples`` into its buffer."""
    import torch
    dev = torch.device("cuda", 0)
    buf = torch.zeros(raw.size + 8 * SB[fmt], dtype=torch.uint8, device=dev)
    o = offset_samples * SB[fmt]
    buf[o:o + raw.size].copy_(torch.from_numpy(np.array(raw)))
    re = torch.full((n_sel, stride), sentinel, dtype=torch.float32, device=dev)
    im = torch.full((n_sel, stride), sentinel, dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)
    n = ch.process_tensor(buf[o:o + raw.size], re, im)
    torch.cuda.synchronize(dev)
    return re.cpu().numpy(), im.cpu().numpy(), n


def test_selection_rows_equal_all_channels_run_and_padding_is_untouched(rfa):
    M, L, D, fmt, g, raw, _ = _case(1)
    sel = [5, 15, 5, 0, 8]
    full = _device_run(1)
    with demod.Channelizer.rational(fmt, M, L, D, g) as ch:
        assert ch.channels == list(range(M)) and ch.interpolation == L and ch.decimation == D
        ch.set_channels(sel)
        with pytest.raises(_lib.RfaError):
            ch.set_channels([5, 16])                     # invalid: the old selection stays
        assert ch.channels == sel
        re, im, n = _device_call(ch, raw, len(sel), 221, fmt=fmt)
        assert n == 215
        for j, k in enumerate(sel):
            _same(re[j, :n], full[k].real.copy())
            _same(im[j, :n], full[k].imag.copy())
        assert np.all(re[:, n:] == 12345.0) and np.all(im[:, n:] == 12345.0)
        ch.set_channels(None)
        ch.reset()
        _same(_run(fmt, M, L, D, g, raw, ch=ch), full)
        p = ch.plan()
        assert (p["n_channels"], p["decimation"], p["num_taps"]) == (M, D, 61)
        assert ch.ratio == (3, 7, 21)
        _same(ch.taps, g)


@pytest.mark.parametrize("fmt", ["s8", "u8", "s16"])
def test_integer_formats_equal_the_f32_run_of_their_converted_samples(rfa, fmt):
    M, L, D, T = 48, 4, 9, 190
    g, raw = _taps(T, 41), _raw(fmt, 600, 42 + len(fmt))
    x = ref.convert(raw, fmt)
    f = np.empty(2 * x.size, "<f4")
    f[0::2], f[1::2] = x.real, x.imag                    # exact: convert() holds float32 values
    _same(_run(fmt, M, L, D, g, raw), _run("f32", M, L, D, g, f.view(np.uint8)))


@pytest.mark.parametrize("fmt", ["u8", "s16", "f32"])
def test_raw_pointer_off_the_four_sample_grid(rfa, fmt):
    M, L, D, T = 16, 3, 7, 61
    g, raw = _taps(T, 51), _raw(fmt, 203, 52)
    with demod.Channelizer.rational(fmt, M, L, D, g) as ch:
        outs = []
        for off in (0, 1, 2, 3):
            ch.reset()
            re, im, n = _device_call(ch, raw, M, 88, offset_samples=off, fmt=fmt)
            assert n == 87                               # ceil(203 * 3 / 7)
            outs.append((re, im))
        for re, im in outs[1:]:
            _same(re, outs[0][0])
            _same(im, outs[0][1])
    _same(outs[0][0][:, :87], _run(fmt, M, L, D, g, raw).real.copy())


def test_two_runs_and_a_reset_repeat_the_first(rfa):
    M, L, D, fmt, g, raw, _ = _case(6)
    with demod.Channelizer.rational(fmt, M, L, D, g) as ch:
        a = _run(fmt, M, L, D, g, raw, sizes=[2000, 7597], ch=ch)
        ch.reset()
        assert ch.max_outputs(0) == 0 and ch.max_outputs(1) == 1 and ch.max_outputs(10) == 2   # the count starts again
        b = _run(fmt, M, L, D, g, raw, sizes=[2000, 7597], ch=ch)
    _same(a, _device_run(6))
    _same(b, a)


def test_nan_and_inf_stay_inside_their_windows(rfa):
    """The window of output n is the Tp samples m_n - (Tp - 1) ... m_n (padding taps included)."""
    M, L, D, T, fmt = 16, 3, 7, 61, "f32"
    Tp = 21
    g = _taps(T, 61)
    clean = _raw(fmt, 400, 62).view("<f4").copy()
    dirty = clean.copy()
    dirty[2 * 100] = np.nan                              # sample 100, I
    dirty[2 * 103 + 1] = np.inf                          # sample 103, Q
    sizes = [120, 180, 100]                              # the first call's history holds both
    a = _run(fmt, M, L, D, g, clean.view(np.uint8), sizes=sizes)
    b = _run(fmt, M, L, D, g, dirty.view(np.uint8), sizes=sizes)
    assert a.shape == (M, 172)
    m_n = np.arange(a.shape[1]) * D // L
    hit = (m_n >= 100) & (m_n - (Tp - 1) <= 103)         # windows that hold one of them
    assert hit.sum() >= 9 and (~hit).sum() >= 150
    finite = lambda y: np.isfinite(y.real) & np.isfinite(y.imag)       # noqa: E731
    assert np.all(finite(b[:, ~hit]))
    _same(b[:, ~hit], a[:, ~hit])
    assert not np.any(finite(b[:, hit]))                # every channel of a window that holds one
    assert np.all(m_n[-40:] >= 300) and not hit[-40:].any()             # the whole last call is clean


def test_short_stride_is_err_size_and_consumes_nothing(rfa):
    M, L, D, fmt, g, raw, _ = _case(1)
    with demod.Channelizer.rational(fmt, M, L, D, g) as ch:
        with pytest.raises(_lib.RfaError) as e:
            _device_call(ch, raw, M, 214, fmt=fmt)
        assert e.value.status == _lib.RFA_ERR_SIZE
        assert ch.max_outputs(500) == 215 and ch.max_outputs(1) == 1    # nothing was consumed
        re, im, n = _device_call(ch, raw, M, 215, fmt=fmt)
        assert n == 215
        _same(re, _device_run(1).real.copy())
        _same(im, _device_run(1).imag.copy())
        assert all(o.size == 0 for o in ch.process(b""))                # 0 samples: a no-op


def test_get_ratio_on_an_integer_handle(rfa):
    g = _taps(61, 5)
    with demod.Channelizer("s8", 16, 5, g) as ch:
        assert ch.ratio == (1, 5, 61) and ch.interpolation == 1
        assert ch.max_outputs(4) == 0 and ch.max_outputs(5) == 1        # the integer count rule, unchanged
    with demod.Channelizer.rational("s8", 16, 1, 5, g) as ch:
        assert ch.ratio == (1, 5, 61) and ch.max_outputs(1) == 1 and ch.max_outputs(6) == 2


# ------------------------------------------------------------------ RasterReceiverBank(resample=True)

def test_resampled_raster_receiver_bank_equals_channelizer_into_demodulator_bank(rfa):
    FS, SPACING, QRATE = 2_048_000, 8_000, 96_000
    modes, chans = ["nfm", "am", "usb"], [3, 255, 100]
    rng = np.random.default_rng(71)
    sizes = [16384, 16385, 16383, 16384]
    t = np.arange(sum(sizes))
    sig = sum(0.25 * np.exp(2j * np.pi * (((k if k < 128 else k - 256) * SPACING + 500.0) / FS) * t
                            + 1j * 2.0 * np.sin(2 * np.pi * 700.0 / FS * t)) for k in chans)
    sig = sig + 0.02 * (rng.standard_normal(t.size) + 1j * rng.standard_normal(t.size))
    iq = np.empty(2 * t.size)
    iq[0::2], iq[1::2] = sig.real, sig.imag
    raw = np.clip(np.rint(iq * 127 + 127.4), 0, 255).astype(np.uint8)
    with pytest.raises(ValueError):
        demod.RasterReceiverBank("u8", FS, SPACING, modes, chans)       # 21.33: not without resample
    with demod.RasterReceiverBank("u8", FS, SPACING, modes, chans, resample=True) as bank, \
            demod.Channelizer.for_raster_resampled("u8", FS, SPACING, QRATE) as ch, \
            demod.DemodulatorBank(modes) as dm:
        assert (ch.n_channels, ch.interpolation, ch.decimation) == (256, 3, 64)
        assert bank.channels == chans and bank.n_channels == 3 and bank.front.ratio == ch.ratio
        ch.set_channels(chans)
        totals, pos = [0, 0, 0], 0
        for s in sizes:
            pkt = raw[2 * pos:2 * (pos + s)]
            pos += s
            got = bank.process(pkt)
            y = np.stack(ch.process(pkt))
            assert y.shape[1] == ref.output_count(pos - s, pos, 3, 64)
            want = dm.process(y.real.copy(), y.imag.copy())
            assert [a.size for a in got] == [w.size for w in want]
            for k, (a, w) in enumerate(zip(got, want)):
                _same(a, w)
                totals[k] += a.size
        # 96 kHz quadrature to 48 kHz audio is a decimation by 2: one period is one audio sample
        expect = pos * 48_000 / FS
        print(f"resampled raster bank: audio counts {totals}, S * 48000 / Fs = {expect}")
        assert abs(totals[0] - expect) <= 1, (totals, expect)
