"""GPU: the channelizer's fine tuning (rfa_pfb_set_tuning, demod.Channelizer.set_tuning /
set_offsets / for_channels, TunedReceiverBank).

A tuned slot is the untuned output times a table entry picked by the absolute output index, so
almost everything here is bit for bit: every slot of a tuned handle against an untuned twin's
row put through ``pfb_tuning_ref.rot`` (the definition in numpy float32 with the library's own
table and Python's integer index), on the integer and the rational kernel, on every tile plan,
past a 32-bit product, over splits, pointer offsets, a reset and a retune.  One test goes back to
the float64 restatement with the bound eps * (P + 4 ceil(log2 M) + 4) * sum|h| * max|x|, one
checks that a tone off the raster comes to rest, one that TunedReceiverBank is the composition
it claims to be."""
import functools
import math

import numpy as np
import pytest

import golden_util as gu
import pfb_rational_ref as rref
import pfb_ref
import pfb_tuning_ref as tref
from rfanalyzer_amd import _lib
from rfanalyzer_amd import demod

pytestmark = pytest.mark.gpu

SB = {"s8": 2, "u8": 2, "s16": 4, "f32": 8}


def _raw(fmt, n, seed):
    rng = np.random.default_rng(seed)
    if fmt == "f32":
        return rng.uniform(-1, 1, 2 * n).astype("<f4").view(np.uint8)
    if fmt == "s16":
        return rng.integers(-32768, 32768, 2 * n, dtype=np.int16).view(np.uint8)
    return rng.integers(0, 256, 2 * n, dtype=np.uint8)


def _taps(T, seed):
    return np.random.default_rng(seed).uniform(-1, 1, T).astype(np.float32)


def _make(fmt, M, L, D, g):
    """L None: rfa_pfb_create; else rfa_pfb_create_rational."""
    return demod.Channelizer(fmt, M, D, g) if L is None else demod.Channelizer.rational(fmt, M, L, D, g)


def _feed(ch, fmt, raw, sizes=None):
    """The stream through ``ch`` in calls of ``sizes`` samples: [selected, n] complex64."""
    n = raw.size // SB[fmt]
    parts, pos = [], 0
    for s in (sizes or [n]):
        parts.append(np.stack(ch.process(raw[pos * SB[fmt]:(pos + s) * SB[fmt]])))
        pos += s
    assert pos == n
    return np.concatenate(parts, axis=1)


def _twin(fmt, M, L, D, g, raw, sizes=None):
    """All channels of an untuned handle."""
    with _make(fmt, M, L, D, g) as ch:
        assert ch.tuning is None
        return _feed(ch, fmt, raw, sizes)


def _tuned(fmt, M, L, D, g, raw, sel, q, steps, sizes=None):
    with _make(fmt, M, L, D, g) as ch:
        ch.set_channels(sel)
        ch.set_tuning(q, steps)
        assert ch.tuning == (q, list(steps)) and ch.channels == list(sel)
        return _feed(ch, fmt, raw, sizes)


def _check_against_twin(label, full, got, sel, q, steps):
    assert got.shape == (len(sel), full.shape[1]), (label, got.shape, full.shape)
    for j, (k, m) in enumerate(zip(sel, steps)):
        want = tref.rot(full[k], q, m)
        tref.same(got[j], want)
        if m == 0:                                       # untouched: the twin's own bits
            np.testing.assert_array_equal(got[j].view(np.int32), full[k].view(np.int32))
        else:                                            # and the rotation is not a no-op
            assert not np.array_equal(got[j], full[k]), (label, j)


# ------------------------------------------------------------------ 1, 2: the integer kernel

@pytest.mark.parametrize("fmt", ["s8", "u8", "s16", "f32"])
def test_bit_exact_against_untuned_twin(rfa, fmt):
    M, D, T = 8, 3, 19
    g, raw = _taps(T, 11), _raw(fmt, 500, 12 + len(fmt))
    sel, q, steps = [3, 3, 0, 7, 3], 7, [0, 1, -3, 3, 6]
    full = _twin(fmt, M, None, D, g, raw)
    assert full.shape == (M, 166)
    _check_against_twin(fmt, full, _tuned(fmt, M, None, D, g, raw, sel, q, steps), sel, q, steps)


def test_bit_exact_more_slots_than_one_store_pass_and_a_ragged_tile(rfa):
    M, D, T, fmt = 60, 7, 120, "u8"                      # K * NT = 960 items for 256 threads; 100 outputs = 6 tiles + 4
    g, raw = _taps(T, 21), _raw(fmt, 700, 22)
    sel, q, steps = list(range(60)), 96, [j - 30 for j in range(60)]
    full = _twin(fmt, M, None, D, g, raw)
    assert full.shape == (M, 100)
    _check_against_twin("M=60", full, _tuned(fmt, M, None, D, g, raw, sel, q, steps), sel, q, steps)


def test_bit_exact_unstaged_fold(rfa):
    M, D, T, fmt = 512, 512, 3073, "s16"                 # run + taps = 8194 points: the fold reads global memory
    g, raw = _taps(T, 31), _raw(fmt, 9 * 512, 32)
    sel, q, steps = [5, 300], 96_000, [47_999, -1]
    full = _twin(fmt, M, None, D, g, raw)
    assert full.shape == (M, 9)
    _check_against_twin("M=512", full, _tuned(fmt, M, None, D, g, raw, sel, q, steps), sel, q, steps)


# ------------------------------------------------------------------ 3: the rational kernel, one case per plan

#               M    L  D     T      fmt    calls           (the shapes of tests/test_gpu_pfb_rational.py cases 1, 10, 12)
RATIONAL = {"run and taps staged": (16, 3, 7, 61, "s8", [500]),
            "run staged": (512, 3, 1024, 6961, "s16", [6000, 3000]),
            "nothing staged": (512, 3, 1024, 17407, "s8", [6000, 3000])}


@pytest.mark.parametrize("plan", sorted(RATIONAL))
def test_rational_bit_exact_against_untuned_twin(rfa, plan):
    M, L, D, T, fmt, sizes = RATIONAL[plan]
    g, raw = _taps(T, 41 + T), _raw(fmt, sum(sizes), 42 + T)
    sel, q = [3, M - 1, 0, 3, 9], 96_000
    steps = [47_999, -47_999, 0, 1, -5000]
    full = _twin(fmt, M, L, D, g, raw, sizes)
    assert full.shape == (M, rref.count(sum(sizes), L, D))
    _check_against_twin(plan, full, _tuned(fmt, M, L, D, g, raw, sel, q, steps, sizes), sel, q, steps)


# ------------------------------------------------------------------ 4: n * m past 2^32

def test_long_index(rfa):
    M, D, T, fmt = 8, 1, 8, "s8"
    g, raw = _taps(T, 51), _raw(fmt, 70_000, 52)
    q = 1 << 20
    sel, steps = [1, 6, 2], [q - 1, -(q - 1), 524_287]
    assert 69_999 * (q - 1) > 1 << 32
    full = _twin(fmt, M, None, D, g, raw)
    assert full.shape == (M, 70_000)
    _check_against_twin("long", full, _tuned(fmt, M, None, D, g, raw, sel, q, steps), sel, q, steps)


# ------------------------------------------------------------------ 5: split, pointer and reset invariance

def _device_call(ch, fmt, raw, n_sel, stride, offset_samples=0):
    """One rfa_pfb_process call on torch tensors, the raw stream ``offset_samples`` into its buffer."""
    import torch
    dev = torch.device("cuda", 0)
    buf = torch.zeros(raw.size + 8 * SB[fmt], dtype=torch.uint8, device=dev)
    o = offset_samples * SB[fmt]
    buf[o:o + raw.size].copy_(torch.from_numpy(np.array(raw)))
    re = torch.full((n_sel, stride), 12345.0, dtype=torch.float32, device=dev)
    im = torch.full((n_sel, stride), 12345.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)
    n = ch.process_tensor(buf[o:o + raw.size], re, im)
    torch.cuda.synchronize(dev)
    out = np.empty((n_sel, n), np.complex64)
    out.real, out.imag = re.cpu().numpy()[:, :n], im.cpu().numpy()[:, :n]
    assert np.all(re.cpu().numpy()[:, n:] == 12345.0) and np.all(im.cpu().numpy()[:, n:] == 12345.0)
    return out


@pytest.mark.parametrize("L", [None, 3], ids=["integer", "rational"])
def test_split_pointer_and_reset_invariance(rfa, L):
    M, D, T, fmt = 16, 7, 61, "s16"
    g, raw = _taps(T, 61), _raw(fmt, 1000, 62)
    sel, q, steps = [2, 15, 2, 8], 3840, [1, -3839, 0, 1919]
    n_out = 1000 // D if L is None else rref.count(1000, L, D)
    with _make(fmt, M, L, D, g) as ch:
        ch.set_channels(sel)
        ch.set_tuning(q, steps)
        whole = _feed(ch, fmt, raw)
        assert whole.shape == (4, n_out)
        ch.reset()
        assert ch.tuning == (q, steps)                   # a reset keeps the tuning and restarts n
        tref.same(_feed(ch, fmt, raw, [1, 2, 7, 0, 33, 957]), whole)
        ch.reset()
        tref.same(_feed(ch, fmt, raw), whole)
        for off in (1, 2, 3):
            ch.reset()
            tref.same(_device_call(ch, fmt, raw, 4, n_out + 3, offset_samples=off), whole)
    full = _twin(fmt, M, L, D, g, raw)
    _check_against_twin("split", full, whole, sel, q, steps)


# ------------------------------------------------------------------ 6: retune between calls, invalid requests

def _set_tuning_rc(ch, q, steps, count=None):
    arr = None if steps is None else (np.ascontiguousarray(steps, np.int32))
    ptr = None if arr is None else arr.ctypes.data_as(_lib.ctypes.POINTER(_lib.ctypes.c_int32))
    return _lib.lib().rfa_pfb_set_tuning(ch._h, q, ptr, (0 if arr is None else arr.size) if count is None else count)


@pytest.mark.parametrize("L", [None, 3], ids=["integer", "rational"])
def test_retune_between_calls_and_invalid_requests(rfa, L):
    M, D, T, fmt = 16, 5, 61, "u8"
    g, raw = _taps(T, 71), _raw(fmt, 900, 72)
    sel = [4, 11, 4]
    old, new = (96, [5, -7, 0]), (7, [-6, 0, 3])
    cut = 300 * SB[fmt]
    with _make(fmt, M, L, D, g) as ch, _make(fmt, M, L, D, g) as fresh:
        ch.set_channels(sel)
        ch.set_tuning(*old)
        first = _feed(ch, fmt, raw[:cut])
        ch.set_tuning(*new)
        assert ch.tuning == new
        rest = _feed(ch, fmt, raw[cut:])
        fresh.set_channels(sel)
        fresh.set_tuning(*new)
        want = _feed(fresh, fmt, raw)                    # the new tuning from the start, the same n
        assert first.shape[1] + rest.shape[1] == want.shape[1]
        tref.same(rest, want[:, first.shape[1]:])
        assert not np.array_equal(first, want[:, :first.shape[1]])
        # every invalid request is refused and the next call shows `new` still in force
        q = new[0]
        for bad in [(q, [q, 0, 0], None), (q, [0, -q, 0], None),              # a step of +- q
                    (0, [1, 2], 2),                                           # q = 0 with steps given and a wrong count
                    ((1 << 20) + 1, [0, 0, 0], None),                         # q above the limit
                    (q, [1, 2], None), (q, [1, 2, 3, 4], None), (q, [1, 2, 3], 2)]:   # a count that is not the selection's
            assert _set_tuning_rc(ch, *bad) == _lib.RFA_ERR_INVALID, bad
            assert ch.tuning == new, bad
        with pytest.raises(_lib.RfaError):
            ch.set_tuning(q, [q, 0, 0])
        more = _raw(fmt, 200, 73)
        tref.same(_feed(ch, fmt, more), _feed(fresh, fmt, more))
        # set_channels clears the tuning; so does set_tuning(0)
        ch.set_channels(sel)
        assert ch.tuning is None and ch.channels == sel
        fresh.set_tuning(0)
        assert fresh.tuning is None
        more = _raw(fmt, 200, 74)
        a, b = _feed(ch, fmt, more), _feed(fresh, fmt, more)
        np.testing.assert_array_equal(a.view(np.int32), b.view(np.int32))
        ch.set_tuning(*old)                              # a tuning after a removal, the table of an earlier q
        fresh.set_tuning(*old)
        assert ch.tuning == old
        more = _raw(fmt, 200, 75)
        tref.same(_feed(ch, fmt, more), _feed(fresh, fmt, more))
    full = _twin(fmt, M, L, D, g, raw)
    n1 = first.shape[1]
    for j, k in enumerate(sel):
        tref.same(first[j], tref.rot(full[k, :n1], old[0], old[1][j]))
        tref.same(rest[j], tref.rot(full[k, n1:], new[0], new[1][j], n_first=n1))


# ------------------------------------------------------------------ 7: against the float64 restatement

#                  M   L     D  T    fmt   samples  selection        q       steps
RESTATEMENT = {1: (8, None, 3, 19, "u8", 500, [3, 3, 0, 7, 3], 7, [0, 1, -3, 3, 6]),
               2: (60, None, 7, 120, "s16", 700, [0, 59, 17, 30], 96, [-30, 29, 5, 47]),
               3: (16, 3, 7, 61, "s8", 500, [5, 15, 0, 8], 96_000, [47_999, -47_999, 5000, 1])}


@pytest.mark.parametrize("cid", sorted(RESTATEMENT))
def test_accuracy_against_float64_restatement(rfa, cid):
    """|z - z_ref| <= eps * (P + 4 ceil(log2 M) + 4) * sum|h| * max|x|: pfb_ref.bound (the rational
    case: pfb_rational_ref.bound, sum|h| of the phase in use) plus 4 eps for two rounded table
    values, two products and one sum on |y| <= sum|h| * max|x|."""
    M, L, D, T, fmt, n, sel, q, steps = RESTATEMENT[cid]
    g, raw = _taps(T, 80 + cid), _raw(fmt, n, 90 + cid)
    x = pfb_ref.convert(raw, fmt)
    if L is None:
        y = pfb_ref.folded(x, g, M, D)
        P, scale = -(-T // M), float(np.abs(g.astype(np.float64)).sum())
        assert math.isclose(pfb_ref.bound(g, x, M), pfb_ref.EPS * (P + 4 * math.ceil(math.log2(M))) * scale
                            * float(np.abs(x).max()))
    else:
        y = rref.folded(x, g, M, L, D)
        gp = rref.phases(g, L)
        P, scale = -(-gp.shape[1] // M), float(np.abs(gp).sum(axis=1).max())
    bound = pfb_ref.EPS * (P + 4 * math.ceil(math.log2(M)) + 4) * scale * float(np.abs(x).max())
    got = _tuned(fmt, M, L, D, g, raw, sel, q, steps)
    want = np.stack([tref.rot64(y[k], q, m) for k, m in zip(sel, steps)])
    assert got.shape == want.shape
    err = float(np.abs(got.astype(np.complex128) - want).max())
    line = f"tuned channelizer case {cid} (M={M} L={L} D={D} T={T} {fmt} q={q}): max err / bound = {err / bound:.4f}"
    gu.NOTES.append(line)
    print(line, f"(err {err:.3e}, bound {bound:.3e})")
    assert err <= bound, (err, bound)


# ------------------------------------------------------------------ 8: a tone comes to rest

def _tone(fs, f_hz, n, amplitude=0.5):
    ph = 2 * np.pi * ((f_hz * np.arange(n)) % fs) / fs              # exact integer phase, float64
    iq = np.empty(2 * n, "<f4")
    iq[0::2], iq[1::2] = amplitude * np.cos(ph), amplitude * np.sin(ph)
    return iq.view(np.uint8)


@pytest.mark.parametrize("fs,spacing,f_tone,resample,want_k,want_qm",
                         [(2_400_000, 25_000, 7 * 25_000 + 5_000, False, 7, (96, 5)),
                          (2_400_000, 25_000, 7 * 25_000 - 12_500, False, 7, (192, -25)),     # the edge: 8 for + 12 500
                          (2_048_000, 8_000, 7 * 8_000 + 3_000, True, 7, (32, 1))],
                         ids=["+5000", "-12500", "resampled"])
def test_a_tone_off_the_raster_comes_to_rest(rfa, fs, spacing, f_tone, resample, want_k, want_qm):
    """After the filter has filled, |arg(z[n+1] conj(z[n]))| < 1e-3 rad on the tuned slot: fp32
    rounding of a unit-scale tone through the fold, the DFT and the rotation is of order 1e-6
    relative, the bar is three decades above that and 300 times below the untuned slot's step."""
    rate = 96_000
    with demod.Channelizer.for_channels("f32", fs, spacing, rate, passband_hz=22_500, resample=resample) as ch, \
            demod.Channelizer.for_channels("f32", fs, spacing, rate, passband_hz=22_500, resample=resample) as twin:
        k, delta = ch.nearest_channel(0, f_tone, fs)
        assert k == want_k and delta == f_tone - k * spacing
        assert demod.Channelizer.offsets_tuning([delta], rate) == (want_qm[0], [want_qm[1]])
        L, D, Tp = ch.ratio
        fill = -(-Tp * L // D) + (1 if resample else 0)
        n_out = fill + 100
        raw = _tone(fs, f_tone, -(-n_out * D // L))
        ch.set_channels([k])
        ch.set_offsets([delta], rate)
        twin.set_channels([k])
        z = _feed(ch, "f32", raw)[0].astype(np.complex128)[fill:]
        y = _feed(twin, "f32", raw)[0].astype(np.complex128)[fill:]
    assert z.size >= 100 and np.abs(z).min() > 0.4                  # in the pass band: the tone's amplitude is 0.5
    step = np.angle(z[1:] * np.conj(z[:-1]))
    plain = np.angle(y[1:] * np.conj(y[:-1]))
    print(f"tone {f_tone} Hz at {fs}: tuned max |step| {np.abs(step).max():.3e} rad, untuned {np.abs(plain).mean():.4f}")
    assert np.abs(step).max() < 1e-3
    assert np.allclose(plain, 2 * np.pi * delta / rate, atol=1e-3)  # + 5000 Hz: 2 pi 5 / 96 = 0.327


# ------------------------------------------------------------------ 9: the chain

FS, SPACING, CENTER = 2_400_000, 25_000, 433_000_000
MODES = ["nfm", "am", "usb", "nfm"]
FREQS = [CENTER + 7 * SPACING + 5_000, CENTER - 3 * SPACING - 12_500, CENTER + 1, CENTER - 1_190_000 - 3_000]
PACKET = 16_384


@functools.lru_cache(maxsize=None)
def _chain_packets():
    """Three u8 packets: an FM carrier on slot 0's frequency, a weak tone on slot 2's, noise."""
    rng = np.random.default_rng(99)
    t = np.arange(3 * PACKET)
    x = 0.3 * np.exp(2j * np.pi * ((FREQS[0] - CENTER) / FS * t) + 2.0j * np.sin(2 * np.pi * 700.0 / FS * t))
    x = x + 0.1 * np.exp(2j * np.pi * ((FREQS[2] - CENTER + 900.0) / FS * t))
    x = x + 0.02 * (rng.standard_normal(t.size) + 1j * rng.standard_normal(t.size))
    iq = np.empty(2 * t.size)
    iq[0::2], iq[1::2] = x.real, x.imag
    raw = np.clip(np.rint(iq * 128 + 127.4), 0, 255).astype(np.uint8)
    return [raw[2 * p * PACKET:2 * (p + 1) * PACKET] for p in range(3)]


@functools.lru_cache(maxsize=None)
def _composition():
    """Per packet: the rows of a for_channels handle with the bank's selection and offsets, and the
    audio of a DemodulatorBank fed all of them (the unsquelched composition)."""
    with demod.TunedReceiverBank("u8", FS, SPACING, MODES) as bank:
        passband, rate = bank.passband_hz, bank.quadrature_rate
    rows, audio = [], []
    with demod.Channelizer.for_channels("u8", FS, SPACING, rate, passband) as ch, demod.DemodulatorBank(MODES) as dm:
        near = [ch.nearest_channel(CENTER, f, FS) for f in FREQS]
        ch.set_channels([k for k, _ in near])
        ch.set_offsets([d for _, d in near], rate)
        for pkt in _chain_packets():
            y = np.stack(ch.process(pkt))
            rows.append(y)
            audio.append(dm.process(y.real.copy(), y.imag.copy()))
    return near, rows, audio


def _bits(a, b, what):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert np.array_equal(a.view(np.int32), b.view(np.int32)), what


def test_tuned_receiver_bank_equals_channelizer_into_demodulator_bank(rfa):
    near, _, want = _composition()
    assert [k for k, _ in near] == [7, 93, 0, 48] and [d for _, d in near] == [5_000, -12_500, 1, 7_000]
    with demod.TunedReceiverBank("u8", FS, SPACING, MODES) as bank:
        assert bank.passband_hz == SPACING / 2 + max(demod.mode_info(m)[2] for m in MODES)
        assert bank.n_channels == 4 and bank.channels == [0, 1, 2, 3] and bank.front.tuning is None
        bank.set_frequencies(CENTER, FREQS)
        assert bank.channels == [k for k, _ in near] and bank.offsets == [d for _, d in near]
        assert bank.front.tuning == demod.Channelizer.offsets_tuning([d for _, d in near], bank.quadrature_rate)
        with pytest.raises(ValueError):
            bank.set_frequencies(CENTER, FREQS[:3])
        with pytest.raises(ValueError):
            bank.set_frequencies(CENTER, FREQS[:3] + [CENTER + FS])          # beyond Fs / 2
        assert bank.channels == [k for k, _ in near]                         # nothing changed
        for p, pkt in enumerate(_chain_packets()):
            got = bank.process(pkt)
            assert [a.size for a in got] == [w.size for w in want[p]] and all(a.size > 0 for a in got)
            for k in range(4):
                _bits(got[k], want[p][k], (p, k))
    with pytest.raises(ValueError):
        demod.TunedReceiverBank("u8", FS, SPACING, ["nfm", "wfm"])           # two quadrature rates


def test_tuned_receiver_bank_with_squelch(rfa):
    """Slot k's audio is that of a demodulator fed the always-running tuned channelizer's rows on
    the slot's open packets only; a closed slot returns nothing.  Slot 0 hears its carrier, slot 1
    only noise; slots 2 and 3 have no squelch."""
    _, rows, plain = _composition()
    thresholds = [-8.5, -8.5, None, None]
    singles = [demod.DemodulatorBank([m]) for m in MODES]
    try:
        with demod.TunedReceiverBank("u8", FS, SPACING, MODES, squelch=thresholds) as bank:
            bank.squelch_debounce = 1
            bank.set_frequencies(CENTER, FREQS)
            for p, pkt in enumerate(_chain_packets()):
                got = bank.process(pkt)
                gates, levels = bank.open, bank.levels
                assert list(gates) == [True, False, True, True], (p, list(gates), list(levels))
                for k in range(4):                                           # the level is measured on the tuned rows
                    power = float(np.mean(np.abs(rows[p][k].astype(np.complex128)) ** 2))
                    assert abs(float(levels[k]) - 5 * np.log10(power)) < 1e-3, (p, k)
                    if not gates[k]:
                        assert got[k].size == 0
                        continue
                    w = singles[k].process(rows[p][k:k + 1].real.copy(), rows[p][k:k + 1].imag.copy())[0]
                    _bits(got[k], w, (p, k))
                    _bits(got[k], plain[p][k], (p, k, "open on every packet: the unsquelched composition"))
    finally:
        for s in singles:
            s.close()
