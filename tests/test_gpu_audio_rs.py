"""GPU: the audio resampler bank (rfa_audio_rs_*, demod.AudioResamplerBank) and the bank chains built with
``pcm=``.

The reference resamples no audio behind its demodulator; the check is tests/audio_rs_ref.py, the
definition in numpy float32.  Float outputs are compared bit for bit (NaNs by position), PCM value for
value.  The shapes are tests/audio_rs_paths.py, which reach every path rfa_audio_rs_plan reports (asserted
on the CPU in tests/test_audio_rs_host.py and again here)."""
import functools

import numpy as np
import pytest

import audio_rs_paths as paths
import audio_rs_ref as ref
import tone_ref
from rfanalyzer_amd import _lib
from rfanalyzer_amd import demod

pytestmark = pytest.mark.gpu

F32 = np.float32
H = ref.H


@functools.lru_cache(maxsize=None)
def row(n, seed=5):
    return ref.rows(1, n, seed)[0]


@functools.lru_cache(maxsize=None)
def taps_of(t, L):
    return ref.taps_of(t, L)


@pytest.fixture
def bank(rfa):
    made = []

    def _bank(k, L, D, T):
        b = demod.AudioResamplerBank(k, L, D, taps_of(T, L))
        made.append(b)
        return b

    yield _bank
    for b in made:
        b.close()


def dev(x, dtype=F32):
    import torch
    return torch.from_numpy(np.array(x, dtype=dtype, order="C")).cuda()


def check_call(b, slot, x, what):
    """One call of a one-slot bank writing both outputs, against the restatement; offset and count against
    the host rule."""
    L, D = b.ratio
    r0 = b.offset(0)
    assert r0 == slot.r, what
    pcm, f32 = b.process_both(x[None, :])
    want = slot.process(x)
    assert (f32[0].size, b.offset(0)) == demod.audio_rs_counts(L, D, r0, x.size) == ref.counts(L, D, r0, x.size), what
    assert b.offset(0) == slot.r, what
    ref.same(f32[0], want, what)
    ref.same_pcm(pcm[0], ref.pcm(want), what)


# ------------------------------------------------------------------ shapes

@pytest.mark.parametrize("L,D,T", paths.CASES)
def test_one_slot_equals_the_restatement(bank, L, D, T):
    b = bank(1, L, D, T)
    assert b.ratio == (L, D) and ref.bits_equal(b.taps, taps_of(T, L)) and b.taps.size == T
    s = ref.Slot(L, D, taps_of(T, L))
    counts = paths.counts_for(L, D, T)
    x = row(max(counts) + 1)
    for n in counts:
        b.reset()
        s.reset()
        assert b.plan(n)["path"] == ("none" if n == 0 else paths.path_of(L, T))
        check_call(b, s, x[:n], f"{L}/{D} T {T} n {n} from offset 0")
        # the call after it meets the history and the offset this one left
        check_call(b, s, x[1:n + 1], f"{L}/{D} T {T} n {n} from offset {s.r}")
    if D > 1:
        b.reset()
        s.reset()
        check_call(b, s, x[:1], "priming")
        assert b.offset(0) == D - L != 0


def test_the_table_reaches_every_path():
    assert {demod.audio_rs_plan(L, D, T, n)["path"] for L, D, T, n in paths.shapes()} == set(paths.PATHS)


@pytest.mark.parametrize("case,counts", paths.MULTI)
def test_five_slots_with_their_own_counts(bank, case, counts):
    L, D, T = case
    b = bank(5, L, D, T)
    x = ref.rows(5, max(counts), seed=8)
    slots = [ref.Slot(L, D, taps_of(T, L)) for _ in range(5)]
    for call in range(2):                                    # the second call meets five histories and offsets
        pcm = b.process(x, counts)
        want = [slots[k].process(x[k, :counts[k]]) for k in range(5)]
        for k in range(5):
            ref.same_pcm(pcm[k], ref.pcm(want[k]), f"call {call} slot {k}: n {counts[k]}")
            assert b.offset(k) == slots[k].r
    # float rows of the same handle, and the slot without samples kept its state: now it gets some
    zero = counts.index(0)
    again = [50 if k == zero else 0 for k in range(5)]
    got = b.process(x, again, pcm=False)
    ref.same(got[zero], slots[zero].process(x[zero, :50]), "the slot that had no samples")
    assert all(got[k].size == 0 for k in range(5) if k != zero)


# ------------------------------------------------------------------ split invariance

@pytest.mark.parametrize("L,D,T", paths.RAGGED_CASES)
def test_a_ragged_sequence_gives_the_stream_given_whole(bank, L, D, T):
    n = sum(paths.RAGGED)
    x = row(n, seed=7)
    whole_pcm, whole = bank(1, L, D, T).process_both(x[None, :])
    ref.same(whole[0], ref.resample(L, D, taps_of(T, L), x)[0], "whole")
    b = bank(1, L, D, T)
    at, f32, pcm = 0, [], []
    for c in paths.RAGGED:
        r0 = b.offset(0)
        p, f = b.process_both(x[None, at:at + c])
        want_n, r = ref.counts(L, D, r0, c)
        assert demod.audio_rs_counts(L, D, r0, c) == (want_n, r)
        assert f[0].size == want_n and p[0].size == want_n and b.offset(0) == r, f"call of {c}"
        f32.append(f[0])
        pcm.append(p[0])
        at += c
    assert ref.bits_equal(np.concatenate(f32), whole[0]), "the pieces are the whole"
    assert np.array_equal(np.concatenate(pcm), whole_pcm[0])
    assert sum(a.size for a in f32) == ref.counts(L, D, 0, n)[0]


# ------------------------------------------------------------------ int16 rows anywhere

@pytest.mark.parametrize("L,D,T", [(1, 6, 219), (147, 640, 1176), (1, 1, 0)])
def test_int16_rows_with_an_odd_stride_and_a_base_off_a_word(bank, L, D, T):
    import torch
    counts = [2 * paths.tile_inputs(L, D, T) + 31, 700, 0]
    x = ref.rows(3, max(counts), seed=9)
    want = [ref.pcm(ref.resample(L, D, taps_of(T, L), x[k, :c])[0]) for k, c in enumerate(counts)]
    width = max(w.size for w in want)
    xd = dev(x)
    for base_off, stride in ((1, width + 3 + (width & 1)), (2, width + 3 + (width & 1)), (1, width + 4 - (width & 1))):
        flat = torch.full((base_off + 3 * stride + 8,), 0x5a5a, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        b = bank(3, L, D, T)
        ptr = flat.data_ptr() + 2 * base_off
        assert flat.data_ptr() % 4 == 0 and (base_off != 1 or ptr % 4 == 2)
        got_counts = b.process_device(xd.data_ptr(), xd.stride(0), counts, None, 0, ptr, stride)
        b.synchronize()
        got = flat.cpu().numpy()
        assert got_counts == [w.size for w in want]
        for k in range(3):
            lo = base_off + k * stride
            ref.same_pcm(got[lo:lo + want[k].size], want[k], f"base +{base_off} stride {stride} slot {k}")
            assert (got[lo + want[k].size:lo + stride] == 0x5a5a).all(), "behind a row, up to the next one"
        assert (got[:base_off] == 0x5a5a).all() and (got[base_off + 3 * stride:] == 0x5a5a).all()


def test_process_tensor_writes_slices_of_wider_tensors(bank):
    import torch
    L, D, T = 1, 6, 219
    counts = [700, 333]
    x = ref.rows(2, 700, seed=10)
    b = bank(2, L, D, T)
    need = b.max_outputs(700)
    wide_s16 = torch.full((2, need + 9), 77, dtype=torch.int16, device="cuda")
    wide_f32 = torch.full((2, need + 6), 7.0, dtype=torch.float32, device="cuda")
    got = b.process_tensor(dev(x), counts, out_s16=wide_s16[:, 3:3 + need], out_f32=wide_f32[:, 1:1 + need])
    b.synchronize()
    s16, f32 = wide_s16.cpu().numpy(), wide_f32.cpu().numpy()
    for k, c in enumerate(counts):
        want = ref.resample(L, D, taps_of(T, L), x[k, :c])[0]
        assert got[k] == want.size
        ref.same(f32[k, 1:1 + want.size], want)
        ref.same_pcm(s16[k, 3:3 + want.size], ref.pcm(want))
        assert (s16[k, 3 + want.size:] == 77).all() and (s16[k, :3] == 77).all()
        assert (f32[k, 1 + want.size:] == 7.0).all() and f32[k, 0] == 7.0
    with pytest.raises(ValueError):
        b.process_tensor(dev(x), counts)
    with pytest.raises(ValueError):
        b.process_tensor(dev(x), counts, out_s16=wide_s16[:, :need - 1])


# ------------------------------------------------------------------ non-finite inputs, the rails, reset

def test_a_nan_reaches_the_outputs_it_is_a_term_of_in_its_slot_only(bank):
    L, D, T = 1, 6, 219
    tile_in = paths.tile_inputs(L, D, T)
    n = 2 * tile_in + 600
    x = np.array(ref.rows(3, n, seed=14))
    clean_pcm = bank(3, L, D, T).process(x)
    at = tile_in - 100                                       # its outputs cross a tile boundary
    x[1, at] = np.nan
    b = bank(3, L, D, T)
    pcm = b.process(x)
    b2 = bank(3, L, D, T)
    f32 = b2.process(x, pcm=False)
    for k in (0, 2):
        assert np.array_equal(pcm[k], clean_pcm[k]), f"slot {k} changed"
    # output m reads inputs i - J + 1 ... i, i = m D: the NaN is a term of those with i - J < at <= i
    J = T
    m = np.arange(pcm[1].size)
    hit = (m * D >= at) & (m * D - J < at)
    assert hit.sum() in (J // D, J // D + 1)
    assert np.array_equal(np.isnan(f32[1]), hit)
    assert (pcm[1][hit] == 0).all() and np.array_equal(pcm[1][~hit], clean_pcm[1][~hit])
    ref.same(f32[1], ref.resample(L, D, taps_of(T, L), x[1])[0])


def test_amplitude_one_and_a_half_saturates_to_both_rails(bank):
    L, D, taps = demod.resampler_taps(48000, 8000)
    t = np.arange(6000)
    x = (1.5 * np.sin(2 * np.pi * 400.0 / 48000 * t)).astype(F32)
    with demod.AudioResamplerBank(1, L, D, taps) as b:
        pcm = b.process(x[None, :])[0]
    want = ref.pcm(ref.resample(L, D, taps, x)[0])
    ref.same_pcm(pcm, want)
    assert pcm.max() == 32767 and pcm.min() == -32768 and (pcm == 32767).sum() > 50 and (pcm == -32768).sum() > 50


def test_reset_touches_only_its_slot(bank):
    L, D, T = 2, 3, 7
    b = bank(3, L, D, T)
    x = ref.rows(3, 1000, seed=17)
    slots = [ref.Slot(L, D, taps_of(T, L)) for _ in range(3)]
    counts = [500, 502, 503]
    got = b.process(x, counts, pcm=False)
    for k in range(3):
        ref.same(got[k], slots[k].process(x[k, :counts[k]]))
    assert [b.offset(k) for k in range(3)] == [s.r for s in slots] and b.offset(1) != 0
    b.reset(1)
    slots[1].reset()
    assert b.offset(1) == 0 and b.offset(0) == slots[0].r and b.offset(2) == slots[2].r
    got = b.process(x[:, 500:], [400, 400, 400], pcm=False)
    for k in range(3):
        ref.same(got[k], slots[k].process(x[k, 500:900]), f"slot {k} after reset(1)")
    b.reset()
    assert [b.offset(k) for k in range(3)] == [0, 0, 0]
    got = b.process(x, [300] * 3, pcm=False)
    for k in range(3):
        ref.same(got[k], ref.resample(L, D, taps_of(T, L), x[k, :300])[0], "after reset(): zeros again")
    for k in (-2, 3):
        with pytest.raises(_lib.RfaError):
            b.reset(k)


# ------------------------------------------------------------------ errors consume nothing

def test_a_refused_call_consumes_nothing(bank):
    import torch
    L, D, T = 1, 3, 65
    n = 600
    x = ref.rows(2, 2 * n, seed=16)
    xd = dev(x)
    stride = xd.stride(0)
    width = 2 * n

    def run(bad):
        b = bank(2, L, D, T)
        f = torch.zeros(2, width, dtype=torch.float32, device="cuda")
        p = torch.zeros(2, width, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        c1 = b.process_device(xd.data_ptr(), stride, [n, n], f.data_ptr(), width, p.data_ptr(), width)
        if bad is not None:
            offsets = [b.offset(0), b.offset(1)]
            with pytest.raises(_lib.RfaError) as e:
                bad(b, f, p)
            assert e.value.status == _lib.RFA_ERR_INVALID
            assert offsets == [b.offset(0), b.offset(1)]
        c2 = b.process_device(xd.data_ptr() + 4 * n, stride, [n, n - 1], f.data_ptr() + 4 * c1[0], width,
                              p.data_ptr() + 2 * c1[0], width)
        b.synchronize()
        return f.cpu().numpy(), p.cpu().numpy(), c1, c2

    want = run(None)
    xp, sp = xd.data_ptr(), stride
    refused = {
        "float output on the input": lambda b, f, p: b.process_device(xp, sp, [n, n], xp, sp, p.data_ptr(), width),
        "float output overlapping the input": lambda b, f, p: b.process_device(xp, sp, [n, n], xp + 4 * (n - 1), sp,
                                                                                 None, 0),
        "int16 output on the input": lambda b, f, p: b.process_device(xp, sp, [n, n], None, 0, xp + 4 * (n - 1), 2 * sp),
        "the outputs on each other": lambda b, f, p: b.process_device(xp, sp, [n, n], f.data_ptr(), width,
                                                                        f.data_ptr() + 2, 2 * width),
        "a count above in_stride": lambda b, f, p: b.process_device(xp, n - 1, [n, 1], f.data_ptr(), width, None, 0),
        "an output count above f32_stride": lambda b, f, p: b.process_device(xp, sp, [1, n], f.data_ptr(), n // D - 1,
                                                                               None, 0),
        "an output count above s16_stride": lambda b, f, p: b.process_device(xp, sp, [1, n], None, 0, p.data_ptr(),
                                                                               n // D - 1),
        "a null input": lambda b, f, p: b.process_device(0, sp, [0, 1], f.data_ptr(), width, None, 0),
        "both outputs null": lambda b, f, p: b.process_device(xp, sp, [1, 0], None, 0, None, 0),
        "an int16 pointer off a 2-byte boundary": lambda b, f, p: b.process_device(xp, sp, [n, n], None, 0,
                                                                                     p.data_ptr() + 1, width),
        "a float pointer off a 4-byte boundary": lambda b, f, p: b.process_device(xp, sp, [n, n], f.data_ptr() + 2, width,
                                                                                    None, 0),
    }
    for what, bad in refused.items():
        got = run(bad)
        assert ref.bits_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2:] == want[2:], what
    for k, c in enumerate((n, n - 1)):
        s = ref.Slot(L, D, taps_of(T, L))
        first = s.process(x[k, :n])
        second = s.process(x[k, n:n + c])
        assert want[2][k] == first.size and want[3][k] == second.size
        ref.same(want[0][k, :first.size], first)
        if k == 0:
            ref.same(want[0][0, first.size:first.size + second.size], second)
            ref.same_pcm(want[1][0, :first.size + second.size], ref.pcm(np.concatenate([first, second])))
    # counts that are all 0 launch nothing and need no rows
    b = bank(2, L, D, T)
    assert b.process_device(0, 0, [0, 0], None, 0, None, 0) == [0, 0]
    assert all(g.size == 0 for g in b.process(x[:, :0]))


# ------------------------------------------------------------------ what the taps say

def _dft(x, hz, rate):
    """The component at hz over a whole number of its periods, float64: |sum x e^(-j w t)| / N."""
    t = np.arange(x.size)
    return abs(np.sum(np.asarray(x, np.float64) * np.exp(-2j * np.pi * hz / rate * t))) / x.size


def test_a_5_khz_tone_aliases_to_3_khz_by_what_the_taps_say_and_1_khz_keeps_its_level(rfa):
    """At 1 / 6, 48 kHz -> 8 kHz, a 5 kHz row lands on 3 kHz.  Over whole periods of both (8 outputs) behind
    the first J outputs the alias is down by the taps' own float64 |H(5 kHz)| within 1 dB -- or, where |H|
    is below -55 dB, by at least 55 dB.  A 1 kHz row read back from PCM has the amplitude |H(1 kHz)| a
    within: half an LSB of quantisation per sample (a DFT bin of errors bounded by e is bounded by e), the
    float32 bound of the sums (J + 1) 2^-24 sum|h| a, and 2^-24 a for the input's own rounding."""
    L, D, taps = demod.resampler_taps(48000, 8000)
    assert (L, D) == (1, 6)
    J, a = taps.size, 0.5
    lo = -(-J // 8) * 8
    n_out = lo + 8 * 200
    t = np.arange(n_out * D)
    x = np.stack([a * np.sin(2 * np.pi * 5000.0 / 48000 * t + 0.3), a * np.sin(2 * np.pi * 1000.0 / 48000 * t + 1.1)])
    x = x.astype(F32)
    with demod.AudioResamplerBank(2, L, D, taps) as b:
        pcm, f32 = b.process_both(x)
    assert f32[0].size == n_out
    level_in = _dft(x[0, 48 * 10:48 * 110], 5000.0, 48000)
    alias = _dft(f32[0][lo:], 3000.0, 8000)
    h5 = ref.response_db(taps, 5000.0, 48000)
    d5 = 20 * np.log10(alias / level_in)
    print(f"5 kHz in at {20 * np.log10(level_in):.2f} dB -> 3 kHz alias at {20 * np.log10(alias):.2f} dB "
          f"(change {d5:.2f} dB, |H(5 kHz)| {h5:.2f} dB)")
    if h5 < -55.0:
        assert d5 <= -55.0
    else:
        assert abs(d5 - h5) <= 1.0
    h1 = 10 ** (ref.response_db(taps, 1000.0, 48000) / 20)
    in1 = _dft(x[1, 48 * 10:48 * 110], 1000.0, 48000)
    out1 = _dft(pcm[1][lo:].astype(np.float64) / 32768.0, 1000.0, 8000)
    margin = 0.5 / 32768 + (J + 1) * 2.0 ** -24 * float(np.abs(taps.astype(np.float64)).sum()) * a + 2.0 ** -24 * a
    print(f"1 kHz: in {in1:.7f}, out {out1:.7f}, |H(1 kHz)| {h1:.6f}, margin {margin:.2e}")
    assert abs(out1 - h1 * in1) <= margin


# ------------------------------------------------------------------ the chains

FS_RAW = 2_400_000
CALL = 16384
CENTRE = 100_000_000
OFFSETS = [-600_000, -200_000, 200_000, 600_000]
N_CALLS = 40                                                 # 0.27 s, 13107 audio samples per slot
OPEN_AT = 20                                                 # the call before which slot 3's squelch stays closed
TONE = [100.0, None, 100.0, None]
FILTER = ["voice", "voice", None, None]


@functools.lru_cache(maxsize=None)
def raw_calls():
    """u8 raw IQ at 2.4 Msps cut into calls of 16384 samples, four FM signals at OFFSETS: a 100.0 Hz tone under
    a 1 kHz tone, voice alone, a 100.0 Hz tone under voice, a 700 Hz tone."""
    n = N_CALLS * CALL
    rng = np.random.Generator(np.random.PCG64(83))
    t = np.arange(n) / FS_RAW
    sig = [tone_ref.fm(600.0 * np.sin(2 * np.pi * 100.0 * t + 0.7) + 1500.0 * np.sin(2 * np.pi * 1000.0 * t + 0.2), FS_RAW),
           tone_ref.fm(tone_ref.voice(rng, n, FS_RAW, 1500.0), FS_RAW),
           tone_ref.fm(600.0 * np.sin(2 * np.pi * 100.0 * t + 0.3) + tone_ref.voice(rng, n, FS_RAW, 1500.0), FS_RAW),
           tone_ref.fm(2000.0 * np.sin(2 * np.pi * 700.0 * t), FS_RAW)]
    x = sum(0.4 * s * np.exp(2j * np.pi * f * t) for s, f in zip(sig, OFFSETS))
    iq = np.empty(2 * n)
    iq[0::2], iq[1::2] = x.real, x.imag
    u8 = np.clip(np.rint(iq * 128 + 127.4), 0, 255).astype(np.uint8)
    return [u8[2 * CALL * j:2 * CALL * (j + 1)] for j in range(N_CALLS)]


MAKERS = {
    "ReceiverBank": lambda **kw: demod.ReceiverBank("u8", FS_RAW, ["nfm"] * 4, **kw),
    "TunedReceiverBank": lambda **kw: demod.TunedReceiverBank("u8", FS_RAW, 25_000, ["nfm"] * 4, **kw),
}


def _run(make, **kw):
    """Every call's (audio arrays, audio_counts, rows up to audio_counts, squelch gates, tone gates, tone
    qualities, pcm() arrays, pcm_counts, pcm rows up to pcm_counts)."""
    out = []
    with make(squelch=[None, None, None, 200.0], tone=TONE, audio_filter=FILTER, **kw) as chain:
        chain.set_frequencies(CENTRE, [CENTRE + f for f in OFFSETS])
        chain.squelch_debounce = 1                           # closed from the first call whose level is below
        has = hasattr(chain, "audio_rs")
        assert has == (kw.get("pcm") is not None) and (chain.pcm_tensor is None) and chain.pcm_counts is None
        if has:
            assert all(p.size == 0 and p.dtype == np.int16 for p in chain.pcm())
        for j, raw in enumerate(raw_calls()):
            if j == OPEN_AT:
                chain.set_squelch(3, None)
            got = chain.process(raw)
            counts = chain.audio_counts
            audio = chain.audio_tensor.cpu().numpy()
            call = [got, counts, [audio[k, :c].copy() for k, c in enumerate(counts)], chain.open.copy(),
                    chain.tone_open.copy(), chain.tone_quality.copy()]
            if has:
                pcm, pcm_counts = chain.pcm(), chain.pcm_counts
                rows = chain.pcm_tensor.cpu().numpy()
                assert rows.dtype == np.int16 and rows.shape[0] == 4
                call += [pcm, pcm_counts, [rows[k, :c].copy() for k, c in enumerate(pcm_counts)]]
            out.append(call)
        if has:
            assert chain.audio_rs.stream == chain.demods.stream
            ratio, taps = chain.audio_rs.ratio, chain.audio_rs.taps
        else:
            ratio = taps = None
            with pytest.raises(ValueError):
                chain.pcm()
    assert not hasattr(chain, "audio_rs") and chain.pcm_tensor is None
    return out, ratio, taps


@functools.lru_cache(maxsize=None)
def plain_run(name):
    return _run(MAKERS[name])[0]


@pytest.mark.parametrize("name", sorted(MAKERS))
def test_chain_pcm_is_the_restatement_of_the_chains_own_rows(rfa, name):
    plain = plain_run(name)
    got, (L, D), taps = _run(MAKERS[name], pcm=8000)
    want_L, want_D, want_taps = demod.resampler_taps(48000, 8000)
    assert (L, D) == (want_L, want_D) == (1, 6) and ref.bits_equal(taps, want_taps)
    reported = np.array([[len(g) for g in call[0]] for call in got])
    for j, (p, g) in enumerate(zip(plain, got)):
        # audio, counts, gates and qualities are those of the chain without pcm=, call for call
        assert [len(a) for a in p[0]] == [len(a) for a in g[0]] and p[1] == g[1], f"call {j}: counts"
        for k in range(4):
            assert ref.bits_equal(p[0][k], g[0][k]) and ref.bits_equal(p[2][k], g[2][k]), f"call {j} slot {k}"
        assert np.array_equal(p[3], g[3]) and np.array_equal(p[4], g[4]), f"call {j}: gates"
        np.testing.assert_array_equal(p[5], g[5], f"call {j}: qualities")
        # pcm() is cut to pcm_counts, and empty exactly where the chain reports no audio
        for k in range(4):
            if reported[j, k] == 0:
                assert g[6][k].size == 0, f"call {j} slot {k}"
            else:
                assert g[7][k] > 0 and np.array_equal(g[6][k], g[8][k]), f"call {j} slot {k}"
    # slot 0 and 2 are tone-closed throughout, slot 3 squelch-held before OPEN_AT, slot 1 always open
    assert (reported[:, 0] == 0).all() and (reported[:, 2] == 0).all() and (reported[:, 1] > 0).all()
    assert (reported[:OPEN_AT, 3] == 0).all() and (reported[OPEN_AT:, 3] > 0).all()
    assert all(call[7][3] == 0 for call in got[:OPEN_AT]), "a held slot gets no samples: its resampler rests"
    for k in range(4):
        x = np.concatenate([call[2][k] for call in got])
        y = np.concatenate([call[8][k] for call in got])
        ref.same_pcm(y, ref.pcm(ref.resample(L, D, taps, x)[0]), f"slot {k}")
        assert y.size == ref.counts(L, D, 0, x.size)[0]
    assert sum(call[1][1] for call in got) > 2 * H           # the history went round more than twice


def test_pcm_dicts_and_the_raster_chain(rfa):
    L, D, taps = demod.resampler_taps(48000, 16000, transition_hz=2000.0)
    with demod.RasterReceiverBank("u8", FS_RAW, 25_000, ["nfm"] * 2, channels=[5, 17],
                                  pcm={"out_rate": 16000, "transition_hz": 2000.0}) as chain:
        assert chain.audio_rs.ratio == (1, 3) == (L, D) and ref.bits_equal(chain.audio_rs.taps, taps)
        got = chain.process(raw_calls()[0])
        pcm = chain.pcm()
        assert [len(g) for g in got] == chain.audio_counts
        for k in range(2):
            ref.same_pcm(pcm[k], ref.pcm(ref.resample(L, D, taps, got[k])[0]), f"slot {k}")
    with demod.RasterReceiverBank("u8", FS_RAW, 25_000, ["nfm"] * 2, channels=[5, 17],
                                  pcm={"L": 2, "D": 3, "taps": ref.taps_of(7, 2)}) as chain:
        assert chain.audio_rs.ratio == (2, 3)
        got = chain.process(raw_calls()[0])
        for k, p in enumerate(chain.pcm()):
            ref.same_pcm(p, ref.pcm(ref.resample(2, 3, ref.taps_of(7, 2), got[k])[0]), f"slot {k}")
