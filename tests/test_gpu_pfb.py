"""GPU: the polyphase channelizer (rfa_pfb_*, demod.Channelizer / RasterReceiverBank, DESIGN.md
§5.7f) against its float64 restatement tests/pfb_ref.py, and against itself bit for bit where
the definition promises that: however the stream is cut into calls, whichever channels are
selected, whatever the raw format or pointer offset.

Every output sample of every selected channel is compared; nothing is floored or excluded.
The tolerance is the derived worst case eps * (P + 4 * ceil(log2 M)) * sum|h| * max|x| per
complex output (pfb_ref.bound), P = ceil(T / M); taps are random in [-1, 1], so a dropped or
misplaced tap is an O(1) error, five orders of magnitude above it.  The observed max(err /
bound) of every case goes to the session summary.

Case 7 of the accuracy table: a 4096-sample call after an 8192-sample call at D = 1024 yields
4 outputs by the count rule (12 - 8), not 3; all 4 are compared, and the first call's 8 too."""
import functools

import numpy as np
import pytest

import golden_util as gu
import pfb_ref
from rfanalyzer_amd import _lib
from rfanalyzer_amd import demod

pytestmark = pytest.mark.gpu

SB = {"s8": 2, "u8": 2, "s16": 4, "f32": 8}
FS, SPACING, QRATE = 2_400_000, 25_000, 96_000


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
def _raster_taps():
    return demod.create_low_pass_taps(1, FS, 0.375 * SPACING, 0.25 * SPACING, 60)


def _run(fmt, M, D, h, raw, sizes=None, channels=None, ch=None):
    """The stream through a Channelizer in calls of ``sizes`` samples (one call by default):
    [selected, n] complex64."""
    own = ch is None
    ch = ch or demod.Channelizer(fmt, M, D, h)
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


# ------------------------------------------------------------------ accuracy, one call each

#        id  M     T      D     fmt    samples           taps
CASES = {1: (16, 16, 16, "s8", 7 * 16 + 3),           # critically sampled, P = 1; 3 spare samples
         2: (16, 61, 5, "u8", 40 * 5),                # T not a multiple of M, D does not divide M
         3: (48, 144, 20, "s16", 30 * 20),            # radix 3
         4: (80, 320, 25, "f32", 30 * 25),            # radix 5
         5: (60, 120, 60, "s8", 30 * 60),             # 2^2 * 3 * 5
         6: (96, None, 25, "u8", 200 * 25),           # the app case, for_raster prototype
         8: (4096, 65536, 4096, "u8", 2 * 4096),      # T = 16 M: cannot sit in LDS
         9: (64, 256, 48, "s8", 1000 * 48),           # many workgroups and a ragged tail
         # either side of the staging threshold (channelizer.hip, kPfbStageBytes = 64 KiB): at
         # M = D = 512 a workgroup owns 8 times, 7 * 512 + T samples and T taps are 8 * (3584 + T)
         # + 4 * T bytes of LDS -- T = 3072 is the last staged length, 3073 folds from global memory
         10: (512, 3072, 512, "s8", 9 * 512),
         11: (512, 3073, 512, "s16", 9 * 512)}
OUTPUTS = {1: 7, 2: 40, 3: 30, 4: 30, 5: 30, 6: 200, 8: 2, 9: 1000, 10: 9, 11: 9}


@functools.lru_cache(maxsize=None)
def _case(cid):
    M, T, D, fmt, n = CASES[cid]
    h = _raster_taps() if T is None else _taps(T, 100 + cid)
    raw = _raw(fmt, n, 200 + cid)
    raw.setflags(write=False)
    return M, D, fmt, h, raw


@functools.lru_cache(maxsize=None)
def _one_call(cid):
    M, D, fmt, h, raw = _case(cid)
    y = _run(fmt, M, D, h, raw)
    y.setflags(write=False)
    return y


def _check_bound(label, y, ref, h, x, M):
    b = pfb_ref.bound(h, x, M)
    err = np.abs(y.astype(np.complex128) - ref)
    ratio = float(err.max() / b)
    gu.NOTES.append(f"channelizer {label}: max err / bound = {ratio:.4f} over {err.size} outputs")
    print(f"channelizer {label}: max err {err.max():.3e}, bound {b:.3e}, ratio {ratio:.4f}")
    assert np.all(np.isfinite(y.view(np.float32)))
    assert ratio <= 1.0, (label, ratio)


@pytest.mark.parametrize("cid", sorted(CASES))
def test_accuracy_against_restatement(rfa, cid):
    M, D, fmt, h, raw = _case(cid)
    y = _one_call(cid)
    assert y.shape == (M, OUTPUTS[cid])
    x = pfb_ref.convert(raw, fmt)
    ref = pfb_ref.folded(x, h, M, D)
    if cid in (1, 2):                                   # small enough for the defining sum itself
        assert np.abs(ref - pfb_ref.direct(x, h, M, D)).max() <= 1e-12
    _check_bound(f"case {cid} (M={M} T={len(h)} D={D} {fmt})", y, ref, h, x, M)


def test_accuracy_largest_m_after_history(rfa):
    """Case 7: M = 4096, T = 8192, D = 1024, s8; a 4096-sample call whose windows reach 8191
    samples back into the history an 8192-sample call left."""
    M, T, D, fmt = 4096, 8192, 1024, "s8"
    h = _taps(T, 107)
    raw = _raw(fmt, 8192 + 4096, 207)
    y = _run(fmt, M, D, h, raw, sizes=[8192, 4096])
    assert y.shape == (M, 12)
    x = pfb_ref.convert(raw, fmt)
    ref = pfb_ref.folded(x, h, M, D)
    _check_bound("case 7 (M=4096 T=8192 D=1024 s8, second call)", y[:, 8:], ref[:, 8:], h, x, M)
    _check_bound("case 7 (first call)", y[:, :8], ref[:, :8], h, x, M)


# ------------------------------------------------------------------ bit-exact properties

SPLITS = {2: [1, 4, 5, 6, 0, 160, 3, 2, 19],          # calls shorter than D = 5 and one of 0 samples
          4: [7, 24, 0, 1, 300, 26, 392],
          9: [47, 1, 0, 5000, 33, 20000, 22919]}


@pytest.mark.parametrize("cid", sorted(SPLITS))
def test_split_invariance(rfa, cid):
    M, D, fmt, h, raw = _case(cid)
    assert sum(SPLITS[cid]) == CASES[cid][4]
    _same(_run(fmt, M, D, h, raw, sizes=SPLITS[cid]), _one_call(cid))


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
    M, T, D, fmt, sel = 128, 1024, 100, "s8", [5, 127, 5, 0, 64]
    h, raw = _taps(T, 31), _raw(fmt, 3000, 32)
    full = _run(fmt, M, D, h, raw)
    assert full.shape == (M, 30)
    with demod.Channelizer(fmt, M, D, h) as ch:
        assert ch.channels == list(range(M))
        ch.set_channels(sel)
        assert ch.channels == sel
        with pytest.raises(_lib.RfaError):
            ch.set_channels([5, 128])                    # invalid: the old selection stays
        with pytest.raises(_lib.RfaError):
            ch.set_channels([-1])
        assert ch.channels == sel
        re, im, n = _device_call(ch, raw, len(sel), 37, fmt=fmt)
        assert n == 30
        for j, k in enumerate(sel):
            _same(re[j, :n], full[k].real.copy())
            _same(im[j, :n], full[k].imag.copy())
        assert np.all(re[:, n:] == 12345.0) and np.all(im[:, n:] == 12345.0)
        ch.set_channels(None)                            # back to all channels, natural order
        ch.reset()
        _same(_run(fmt, M, D, h, raw, ch=ch), full)
        p = ch.plan()
        assert (p["n_channels"], p["decimation"], p["num_taps"]) == (M, D, T)
        assert int(np.prod(p["radices"])) == M and set(p["radices"]) <= {2, 3, 4, 5}
        _same(ch.taps, h)


@pytest.mark.parametrize("fmt", ["s8", "u8", "s16"])
def test_integer_formats_equal_the_f32_run_of_their_converted_samples(rfa, fmt):
    M, T, D = 48, 144, 20
    h, raw = _taps(T, 41), _raw(fmt, 600, 42 + len(fmt))
    x = pfb_ref.convert(raw, fmt)
    f = np.empty(2 * x.size, "<f4")
    f[0::2], f[1::2] = x.real, x.imag                    # exact: convert() holds float32 values
    _same(_run(fmt, M, D, h, raw), _run("f32", M, D, h, f.view(np.uint8)))


@pytest.mark.parametrize("fmt", ["u8", "s16", "f32"])
def test_raw_pointer_off_the_four_sample_grid(rfa, fmt):
    M, T, D = 16, 61, 5
    h, raw = _taps(T, 51), _raw(fmt, 203, 52)
    with demod.Channelizer(fmt, M, D, h) as ch:
        outs = []
        for off in (0, 1, 2, 3):
            ch.reset()
            re, im, n = _device_call(ch, raw, M, 41, offset_samples=off, fmt=fmt)
            assert n == 40
            outs.append((re, im))
        for re, im in outs[1:]:
            _same(re, outs[0][0])
            _same(im, outs[0][1])
    _same(outs[0][0][:, :40], _run(fmt, M, D, h, raw).real.copy())


def test_two_runs_and_a_reset_repeat_the_first(rfa):
    M, D, fmt, h, raw = _case(9)
    with demod.Channelizer(fmt, M, D, h) as ch:
        a = _run(fmt, M, D, h, raw, sizes=[10000, 38000], ch=ch)
        ch.reset()
        assert ch.max_outputs(47) == 0 and ch.max_outputs(48) == 1      # the count starts again
        b = _run(fmt, M, D, h, raw, sizes=[10000, 38000], ch=ch)
    _same(a, _one_call(9))
    _same(b, a)
    _same(_run(fmt, M, D, h, raw), a)                                    # a second handle


def test_nan_and_inf_stay_inside_their_windows(rfa):
    M, T, D, fmt = 16, 61, 5, "f32"
    h = _taps(T, 61)
    clean = _raw(fmt, 400, 62).view("<f4").copy()
    dirty = clean.copy()
    dirty[2 * 100] = np.nan                              # sample 100, I
    dirty[2 * 103 + 1] = np.inf                          # sample 103, Q
    sizes = [120, 180, 100]                              # the first call's history holds both
    a = _run(fmt, M, D, h, clean.view(np.uint8), sizes=sizes)
    b = _run(fmt, M, D, h, dirty.view(np.uint8), sizes=sizes)
    i_n = np.arange(a.shape[1]) * D + D - 1
    hit = (i_n >= 100) & (i_n - (T - 1) <= 103)          # windows [i_n - 60, i_n] that hold one of them
    assert hit.sum() >= 12 and (~hit).sum() >= 60
    finite = lambda y: np.isfinite(y.real) & np.isfinite(y.imag)       # noqa: E731
    assert np.all(finite(b[:, ~hit]))
    _same(b[:, ~hit], a[:, ~hit])
    assert not np.any(finite(b[:, hit]))                # every channel of a window that holds one
    assert np.all(i_n[-20:] >= 300) and not hit[-20:].any()             # the whole last call is clean


def test_short_stride_is_err_size_and_consumes_nothing(rfa):
    M, D, fmt, h, raw = _case(2)
    with demod.Channelizer(fmt, M, D, h) as ch:
        with pytest.raises(_lib.RfaError) as e:
            _device_call(ch, raw, M, 39, fmt=fmt)
        assert e.value.status == _lib.RFA_ERR_SIZE
        assert ch.max_outputs(200) == 40 and ch.max_outputs(4) == 0     # nothing was consumed
        re, im, n = _device_call(ch, raw, M, 40, fmt=fmt)
        assert n == 40
        _same(re, _one_call(2).real.copy())
        _same(im, _one_call(2).imag.copy())
        assert all(o.size == 0 for o in ch.process(b""))                # 0 samples: a no-op


def test_channel_of(rfa):
    with demod.Channelizer.for_raster("u8", FS, SPACING, QRATE) as ch:
        assert (ch.n_channels, ch.decimation) == (96, 25)
        assert ch.channel_of(100_000_000, 100_000_000, FS) == 0
        assert ch.channel_of(100_000_000, 100_175_000, FS) == 7
        assert ch.channel_of(100_000_000, 99_975_000, FS) == 95
        with pytest.raises(ValueError):
            ch.channel_of(100_000_000, 100_010_000, FS)
        _same(ch.taps, _raster_taps())


# ------------------------------------------------------------------ RasterReceiverBank

def test_raster_receiver_bank_equals_channelizer_into_demodulator_bank(rfa):
    modes, chans = ["nfm", "am", "usb"], [3, 95, 40]
    rng = np.random.default_rng(71)
    t = np.arange(2 * 16384)
    sig = sum(0.25 * np.exp(2j * np.pi * (((k if k < 48 else k - 96) * SPACING + 1000.0) / FS) * t
                            + 1j * 2.0 * np.sin(2 * np.pi * 700.0 / FS * t)) for k in chans)
    sig = sig + 0.02 * (rng.standard_normal(t.size) + 1j * rng.standard_normal(t.size))
    iq = np.empty(2 * t.size)
    iq[0::2], iq[1::2] = sig.real, sig.imag
    raw = np.clip(np.rint(iq * 127 + 127.4), 0, 255).astype(np.uint8)
    with pytest.raises(ValueError):
        demod.RasterReceiverBank("u8", FS, SPACING, ["nfm", "wfm"])
    with demod.RasterReceiverBank("u8", FS, SPACING, modes, chans) as bank, \
            demod.Channelizer.for_raster("u8", FS, SPACING, QRATE) as ch, \
            demod.DemodulatorBank(modes) as dm:
        assert bank.channels == chans and bank.n_channels == 3
        with pytest.raises(ValueError):
            bank.set_mode(0, "wfm")
        ch.set_channels(chans)
        total = 0
        for p in range(2):
            pkt = raw[p * 2 * 16384:(p + 1) * 2 * 16384]
            got = bank.process(pkt)
            y = np.stack(ch.process(pkt))
            want = dm.process(y.real.copy(), y.imag.copy())
            assert [g.size for g in got] == [w.size for w in want]
            for g, w in zip(got, want):
                _same(g, w)
                total += g.size
        assert total > 0
