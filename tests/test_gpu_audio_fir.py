"""GPU: the audio FIR bank (rfa_audio_fir_*, demod.AudioFilterBank) and the bank chains built with
``audio_filter=``.

The reference filters no audio behind its demodulator; the check is tests/audio_fir_ref.py, the
definition in numpy float32.  Finite values and infinities are compared bit for bit and NaNs by
position.  The shapes are tests/audio_fir_paths.py: every tap count against the counts around the
filter's length and around the tile, which reaches every path rfa_audio_fir_plan reports (asserted on
the CPU in tests/test_audio_fir_host.py and again here)."""
import functools

import numpy as np
import pytest

import audio_fir_paths as paths
import audio_fir_ref as ref
import tone_ref
from rfanalyzer_amd import _lib
from rfanalyzer_amd import demod

pytestmark = pytest.mark.gpu

F32 = np.float32
TILE = paths.TILE
H = ref.H
VOICE_T = 1309


@functools.lru_cache(maxsize=None)
def row(n, seed=5):
    return ref.rows(1, n, seed)[0]


@functools.lru_cache(maxsize=None)
def taps_of(t):
    return ref.taps_of(t)


@pytest.fixture
def bank(rfa):
    made = []

    def _bank(k=1, taps=()):
        b = demod.AudioFilterBank(k)
        made.append(b)
        for slot, t in enumerate(taps):
            b.set_taps(slot, t)
        return b

    yield _bank
    for b in made:
        b.close()


def dev(x):
    import torch
    return torch.from_numpy(np.array(x, dtype=F32, order="C")).cuda()


# ------------------------------------------------------------------ shapes

@pytest.mark.parametrize("t,n", paths.SINGLE)
def test_one_slot_equals_the_restatement(bank, t, n):
    taps = taps_of(t)
    b = bank(1, [taps])
    assert ref.bits_equal(b.taps(0), taps)
    x = row(max(n, 1))[:n]
    s = ref.Slot(taps)
    got = b.process(x[None, :])[0]
    assert got.dtype == F32 and got.size == n
    ref.same(got, s.process(x), f"T {t} n {n} path {b.plan(t, n)['path']}")
    # the call after it meets the history this one left
    x2 = row(700, seed=6)
    ref.same(b.process(x2[None, :])[0], s.process(x2), f"T {t} n {n}, the call after")


def test_the_table_reaches_every_path():
    assert {demod.audio_fir_plan(t, n)["path"] for t, n in paths.shapes()} == set(paths.PATHS)
    assert _lib.RFA_AUDIO_FIR_TILE == TILE == demod.audio_fir_plan(1, 1)["tile"]


def test_five_slots_with_their_own_taps_and_counts(bank):
    tap_counts = [t for t, _ in paths.MULTI]
    counts = [n for _, n in paths.MULTI]
    b = bank(5, [taps_of(t) for t in tap_counts])
    assert [b.taps(k).size for k in range(5)] == tap_counts
    x = ref.rows(5, max(counts), seed=8)
    slots = [ref.Slot(taps_of(t)) for t in tap_counts]
    for call in range(2):                                    # the second call meets five different histories
        got = b.process(x, counts)
        for k in range(5):
            assert got[k].size == counts[k]
            ref.same(got[k], slots[k].process(x[k, :counts[k]]), f"call {call} slot {k}: T {tap_counts[k]} n {counts[k]}")
    # the slot without samples kept its history: now it gets some
    got = b.process(x, [0, 50, 0, 0, 0])
    ref.same(got[1], slots[1].process(x[1, :50]), "the slot that had no samples")


def test_one_slot_may_have_a_stride_below_its_count(bank):
    n = TILE + 1
    b = bank(1, [taps_of(65)])
    x, out = dev(row(n)), dev(np.zeros(n))
    b.process_device(x.data_ptr(), 1, [n], out.data_ptr(), 1)
    b.synchronize()
    ref.same(out.cpu().numpy(), ref.fir(taps_of(65), row(n))[0])
    two = bank(2, [taps_of(65)] * 2)                         # with two slots the same strides are refused
    with pytest.raises(_lib.RfaError) as e:
        two.process_device(x.data_ptr(), 1, [2, 2], out.data_ptr(), 1)
    assert e.value.status == _lib.RFA_ERR_INVALID


def test_rows_of_wider_tensors_at_odd_offsets(bank):
    import torch
    counts = [TILE + 1, 300, 77]
    tap_counts = [1309, 3, 64]
    x = ref.rows(3, max(counts), seed=9)
    want = [ref.fir(taps_of(t), x[k, :c])[0] for k, (t, c) in enumerate(zip(tap_counts, counts))]
    wide_in = torch.zeros(3, max(counts) + 29, dtype=torch.float32, device="cuda")
    wide_out = torch.zeros(3, max(counts) + 50, dtype=torch.float32, device="cuda")
    for off in (0, 1, 13):
        b = bank(3, [taps_of(t) for t in tap_counts])
        vin, vout = wide_in[:, off:off + max(counts)], wide_out[:, off + 3:off + 3 + max(counts)]
        vin.copy_(dev(x))
        wide_out.fill_(7.0)
        torch.cuda.synchronize()                             # torch's stream is not the handle's
        b.process_tensor(vin, counts, vout)
        b.synchronize()
        got = vout.cpu().numpy()
        for k in range(3):
            ref.same(got[k, :counts[k]], want[k], f"offset {off} slot {k}")
            assert (got[k, counts[k]:] == 7.0).all()         # nothing behind a slot's count is written
        assert (wide_out[:, :off + 3] == 7.0).all().item()


# ------------------------------------------------------------------ split invariance

def test_a_row_cut_into_calls_gives_the_row_given_whole(bank):
    n = 3 * TILE + 5
    taps = taps_of(VOICE_T)
    x = row(n)
    whole = bank(1, [taps]).process(x[None, :])[0]
    ref.same(whole, ref.fir(taps, x)[0], "whole")
    for cut in (1, VOICE_T - 2, VOICE_T - 1, TILE, TILE + 1):
        b = bank(1, [taps])
        got = np.concatenate([b.process(x[None, :cut])[0], b.process(x[None, cut:])[0]])
        assert ref.bits_equal(got, whole), f"cut at {cut}"
    b = bank(1, [taps])
    pieces = [b.process(x[None, i:i + 1])[0] for i in range(40)] + [b.process(x[None, 40:])[0]]
    assert ref.bits_equal(np.concatenate(pieces), whole), "40 calls of one sample"


# ------------------------------------------------------------------ history

def test_history_reset_and_new_taps_between_calls(bank):
    """Three slots; the taps of slot 0 go 3 -> 4096 -> 3 between calls and the restatement keeps the last
    4095 inputs whatever they are; reset(1) zeroes slot 1 alone.  The calls add up to more than 2 * 4095
    inputs per slot."""
    calls = [700, H + 3, 1, 2 * TILE + 17, 300]
    assert sum(calls) > 2 * H
    x = ref.rows(3, sum(calls), seed=12)
    b = bank(3, [taps_of(3), taps_of(65), taps_of(1309)])
    slots = [ref.Slot(taps_of(3)), ref.Slot(taps_of(65)), ref.Slot(taps_of(1309))]
    at = 0
    for j, n in enumerate(calls):
        if j == 1:                                           # shorter -> longer: the long filter meets inputs from
            b.set_taps(0, taps_of(4096))                     # before it existed
            slots[0].taps = taps_of(4096)
        if j == 3:                                           # longer -> shorter
            b.set_taps(0, taps_of(3))
            slots[0].taps = taps_of(3)
            b.reset(1)
            slots[1].reset()
        got = b.process(x[:, at:at + n])
        for k in range(3):
            ref.same(got[k], slots[k].process(x[k, at:at + n]), f"call {j} slot {k}")
        at += n
    assert b.taps(0).size == 3 and b.taps(2).size == 1309    # reset left the taps
    b.reset()
    fresh = b.process(x[:, :500])
    for k, t in enumerate((3, 65, 1309)):
        ref.same(fresh[k], ref.fir(taps_of(t), x[k, :500])[0], f"after reset() slot {k}: zeros again")


def test_tap_round_trips_and_setter_errors(bank):
    b = bank(2)
    assert b.taps(0).size == 0 and b.taps(1).size == 0
    for t in (0, 1, 4096, 1, 0):
        b.set_taps(1, taps_of(t) if t else None)
        assert ref.bits_equal(b.taps(1), taps_of(t)) and b.taps(1).size == t and b.taps(0).size == 0
    b.set_taps(0, taps_of(3))
    for bad in ([1.0, np.nan], [np.inf], [-np.inf, 1.0], np.ones(4097, F32)):
        with pytest.raises(_lib.RfaError) as e:
            b.set_taps(0, bad)
        assert e.value.status == _lib.RFA_ERR_INVALID
    assert ref.bits_equal(b.taps(0), taps_of(3))
    for k in (-1, 2):
        with pytest.raises(_lib.RfaError):
            b.set_taps(k, taps_of(3))
        with pytest.raises(_lib.RfaError):
            b.reset(k if k > 0 else -2)


# ------------------------------------------------------------------ pass-through and isolation

def test_pass_through_hands_on_the_bits(bank):
    odd = np.array([0x7fc00001, 0xffc12345, 0x7f800001, 0xff800001, 0x7f800000, 0xff800000, 0x80000000, 0x00000000,
                    0x00000001, 0x807fffff, 0x3f800000], np.uint32).view(F32)
    x = np.array(ref.rows(2, TILE + 40, seed=3))
    x[0, :odd.size] = odd
    x[0, TILE + 7:TILE + 7 + odd.size] = odd
    b = bank(2, [(), taps_of(3)])
    got = b.process(x, [TILE + 40, 300])
    assert ref.bits_equal(got[0], x[0]), "no taps: output = input, without delay"
    ref.same(got[1], ref.fir(taps_of(3), x[1, :300])[0])
    # the pass-through slot keeps a history too: with taps it continues from those inputs
    b.set_taps(0, taps_of(65))
    x2 = row(100, seed=4)
    got = b.process(np.stack([x2, x2]), [100, 0])
    ref.same(got[0], ref.fir(taps_of(65), x2, np.concatenate([np.zeros(H, F32), x[0]])[-H:])[0])


def test_a_non_finite_sample_stays_in_its_slot_and_its_t_outputs(bank):
    n, t = 2 * TILE + 100, 65
    tap_counts = [1309, 0, t, 3]
    x = np.array(ref.rows(4, n, seed=14))
    make = lambda: bank(4, [taps_of(c) for c in tap_counts])
    clean = make().process(x)
    p_nan, p_inf = 500, TILE - 10                            # the second one's outputs cross a tile boundary
    x[2, p_nan], x[2, p_inf] = np.nan, np.inf
    got = make().process(x)
    for k in (0, 1, 3):
        assert ref.bits_equal(got[k], clean[k]), f"slot {k} changed"
    changed = np.flatnonzero(got[2].view(np.int32) != clean[2].view(np.int32))
    assert list(changed) == list(range(p_nan, p_nan + t)) + list(range(p_inf, p_inf + t))
    assert not np.isfinite(got[2][changed]).any()
    ref.same(got[2], ref.fir(taps_of(t), x[2])[0])


# ------------------------------------------------------------------ queueing and errors

def test_twelve_queued_calls_with_new_taps_after_the_sixth(bank):
    """More calls in flight than the record ring has entries, and a tap upload between them."""
    import torch
    n = 600
    x = ref.rows(2, 12 * n, seed=15)
    xd = dev(x)

    def run(sync):
        b = bank(2, [taps_of(1309), taps_of(64)])
        out = torch.zeros(2, 12 * n, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        for j in range(12):
            if j == 6:
                b.set_taps(0, taps_of(65))
                b.set_taps(1, taps_of(4096))
            b.process_device(xd.data_ptr() + 4 * j * n, 12 * n, [n, n - j], out.data_ptr() + 4 * j * n, 12 * n)
            if sync:
                b.synchronize()
        b.synchronize()
        return out.cpu().numpy()

    queued, stepped = run(False), run(True)
    assert ref.bits_equal(queued, stepped)
    slots = [ref.Slot(taps_of(1309)), ref.Slot(taps_of(64))]
    for j in range(12):
        if j == 6:
            slots[0].taps, slots[1].taps = taps_of(65), taps_of(4096)
        for k, c in enumerate((n, n - j)):
            ref.same(queued[k, j * n:j * n + c], slots[k].process(x[k, j * n:j * n + c]), f"call {j} slot {k}")


def test_a_refused_call_consumes_nothing(bank):
    import torch
    n = 400
    x = ref.rows(2, 2 * n, seed=16)
    xd = dev(x)
    taps = [taps_of(1309), taps_of(3)]

    def run(bad):
        b = bank(2, taps)
        out = torch.zeros(2, 2 * n, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        b.process_device(xd.data_ptr(), stride, [n, n], out.data_ptr(), stride)
        if bad is not None:
            with pytest.raises(_lib.RfaError) as e:
                bad(b, out)
            assert e.value.status == _lib.RFA_ERR_INVALID
        b.process_device(xd.data_ptr() + 4 * n, stride, [n, n - 1], out.data_ptr() + 4 * n, stride)
        b.synchronize()
        return out.cpu().numpy()

    stride = xd.stride(0)
    assert stride == 2 * n
    want = run(None)
    refused = {
        "in place": lambda b, out: b.process_device(xd.data_ptr(), stride, [n, n], xd.data_ptr(), stride),
        "overlapping rows": lambda b, out: b.process_device(xd.data_ptr(), stride, [n, n], xd.data_ptr() + 4 * (n - 1),
                                                            stride),
        "a count above in_stride": lambda b, out: b.process_device(xd.data_ptr(), n - 1, [n, 1], out.data_ptr(), stride),
        "a count above out_stride": lambda b, out: b.process_device(xd.data_ptr(), stride, [1, n], out.data_ptr(), n - 1),
        "a null input": lambda b, out: b.process_device(0, stride, [0, 1], out.data_ptr(), stride),
        "a null output": lambda b, out: b.process_device(xd.data_ptr(), stride, [1, 0], 0, stride),
    }
    for what, bad in refused.items():
        assert ref.bits_equal(run(bad), want), what
    for k, c in enumerate((n, n - 1)):
        s = ref.Slot(taps[k])
        s.process(x[k, :n])
        ref.same(want[k, n:n + c], s.process(x[k, n:n + c]))
    # counts that are all 0 launch nothing and need no rows
    b = bank(2, taps)
    b.process_device(0, 0, [0, 0], 0, 0)
    assert all(g.size == 0 for g in b.process(x[:, :0]))


# ------------------------------------------------------------------ the chains

FS_RAW = 2_400_000
CALL = 16384
CENTRE = 100_000_000
OFFSETS = [-600_000, -200_000, 200_000, 600_000]
N_CALLS = 40                                                 # 0.27 s, 13107 audio samples per slot
N_TONE_CALLS = 80                                            # 0.55 s: the tone rule's first 0.5 s window closes inside


@functools.lru_cache(maxsize=None)
def raw_calls():
    """u8 raw IQ at 2.4 Msps cut into calls of 16384 samples, four FM signals at OFFSETS: a 100.0 Hz tone
    (600 Hz deviation) under a 1 kHz tone (1500 Hz deviation), a 103.5 Hz tone under voice, a 100.0 Hz
    tone under voice, noise alone."""
    n = N_TONE_CALLS * CALL
    rng = np.random.Generator(np.random.PCG64(79))
    t = np.arange(n) / FS_RAW
    sig = [tone_ref.fm(600.0 * np.sin(2 * np.pi * 100.0 * t + 0.7) + 1500.0 * np.sin(2 * np.pi * 1000.0 * t + 0.2), FS_RAW),
           tone_ref.fm(600.0 * np.sin(2 * np.pi * 103.5 * t + 1.9) + tone_ref.voice(rng, n, FS_RAW, 1500.0), FS_RAW),
           tone_ref.fm(600.0 * np.sin(2 * np.pi * 100.0 * t + 0.3) + tone_ref.voice(rng, n, FS_RAW, 1500.0), FS_RAW),
           0.2 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))]
    x = sum(0.4 * s * np.exp(2j * np.pi * f * t) for s, f in zip(sig, OFFSETS))
    iq = np.empty(2 * n)
    iq[0::2], iq[1::2] = x.real, x.imag
    u8 = np.clip(np.rint(iq * 128 + 127.4), 0, 255).astype(np.uint8)
    return [u8[2 * CALL * j:2 * CALL * (j + 1)] for j in range(N_TONE_CALLS)]


def _receiver_bank(**kw):
    return demod.ReceiverBank("u8", FS_RAW, ["nfm"] * 4, **kw)


def _tuned_bank(**kw):
    return demod.TunedReceiverBank("u8", FS_RAW, 25_000, ["nfm"] * 4, **kw)


MAKERS = {"ReceiverBank": _receiver_bank, "TunedReceiverBank": _tuned_bank}


def _run(make, n_calls, **kw):
    """Every call's (reported counts, audio_counts, the rows up to audio_counts, tone_open, tone_quality)."""
    out = []
    with make(**kw) as chain:
        chain.set_frequencies(CENTRE, [CENTRE + f for f in OFFSETS])
        for raw in raw_calls()[:n_calls]:
            got = chain.process(raw)
            counts = chain.audio_counts
            audio = chain.audio_tensor.cpu().numpy()
            gate, q = chain.tone_open, chain.tone_quality
            out.append(([len(g) for g in got], counts, [audio[k, :c].copy() for k, c in enumerate(counts)],
                        None if gate is None else gate.copy(), None if q is None else q.copy()))
            for k, g in enumerate(got):                      # what process returns is the head of audio_tensor's row
                assert ref.bits_equal(g, audio[k, :len(g)])
        has_fir = hasattr(chain, "audio_fir")
        if has_fir:
            assert chain.audio_fir.stream == chain.demods.stream
    return out, has_fir


@functools.lru_cache(maxsize=None)
def plain_run(name):
    return _run(MAKERS[name], N_CALLS)[0]


def _stream(run, k):
    return np.concatenate([call[2][k] for call in run])


@pytest.mark.parametrize("name", sorted(MAKERS))
def test_chain_with_every_entry_none_equals_a_chain_without_the_keyword(rfa, name):
    plain = plain_run(name)
    got, has_fir = _run(MAKERS[name], N_CALLS, audio_filter=[None] * 4)
    assert has_fir
    for j, (p, g) in enumerate(zip(plain, got)):
        assert p[0] == g[0] == p[1] == g[1], f"call {j}: counts"
        for k in range(4):
            assert ref.bits_equal(p[2][k], g[2][k]), f"call {j} slot {k}"
    with MAKERS[name]() as chain:
        assert not hasattr(chain, "audio_fir") and chain.audio_counts is None and chain._filtered is None
        with pytest.raises(ValueError):
            chain.set_audio_filter(0, "voice")
        chain.set_frequencies(CENTRE, [CENTRE + f for f in OFFSETS])
        chain.process(raw_calls()[0])
        assert chain._filtered is None and chain.audio_tensor is chain._audio


@pytest.mark.parametrize("name", sorted(MAKERS))
def test_chain_with_voice_filters_equals_the_restatement_on_the_plain_rows(rfa, name):
    plain = plain_run(name)
    got, _ = _run(MAKERS[name], N_CALLS, audio_filter=["voice", None, "voice", None])
    voice = demod.voice_taps()
    assert voice.size == VOICE_T
    for j, (p, g) in enumerate(zip(plain, got)):
        assert p[0] == g[0] == g[1], f"call {j}: the reported counts stay, audio_counts are the demodulators'"
    for k in range(4):
        x = _stream(plain, k)
        want = ref.fir(voice, x)[0] if k in (0, 2) else x
        ref.same(_stream(got, k), want, f"slot {k}")
    assert sum(c[1][0] for c in got) > 2 * H + VOICE_T       # the history went round more than twice


def _dft_db(x, hz):
    """The component at hz of a whole number of its periods, float64, in dB."""
    t = np.arange(x.size)
    return 20.0 * np.log10(abs(np.sum(x.astype(np.float64) * np.exp(-2j * np.pi * hz / demod.AUDIO_RATE * t))) / x.size)


@pytest.mark.parametrize("name", sorted(MAKERS))
def test_the_tone_is_suppressed_by_what_the_taps_say(rfa, name):
    """Slot 0 carries 100.0 Hz under 1 kHz.  Over whole periods of both (480 samples) behind the first T
    samples, the 100 Hz component falls by the taps' own float64 |H(100 Hz)| within 1 dB -- or, where
    |H| is below -55 dB, by at least 55 dB -- and the 1 kHz component moves by less than 0.1 dB."""
    plain = plain_run(name)
    got, _ = _run(MAKERS[name], N_CALLS, audio_filter=["voice", None, None, None])
    voice = demod.voice_taps()
    x, y = _stream(plain, 0), _stream(got, 0)
    periods = (x.size - VOICE_T) // 480
    assert periods >= 20
    lo, hi = VOICE_T, VOICE_T + 480 * periods
    h100 = ref.response_db(voice, 100.0, demod.AUDIO_RATE)
    d100 = _dft_db(y[lo:hi], 100.0) - _dft_db(x[lo:hi], 100.0)
    d1k = _dft_db(y[lo:hi], 1000.0) - _dft_db(x[lo:hi], 1000.0)
    print(f"{name}: {periods} periods; 100 Hz {_dft_db(x[lo:hi], 100.0):.2f} dB -> {_dft_db(y[lo:hi], 100.0):.2f} dB "
          f"(change {d100:.2f} dB, |H(100 Hz)| {h100:.2f} dB); 1 kHz change {d1k:.4f} dB")
    if h100 < -55.0:
        assert d100 <= -55.0
    else:
        assert abs(d100 - h100) <= 1.0
    assert abs(d1k) < 0.1


@pytest.mark.parametrize("name", sorted(MAKERS))
def test_the_tone_meter_reads_the_unfiltered_rows(rfa, name):
    """tone= with and without the filter: the same reported counts, gates and qualities call for call,
    and the filtered stream is continuous across the calls that are reported with 0."""
    tone = [100.0, 100.0, 100.0, None]
    toned, _ = _run(MAKERS[name], N_TONE_CALLS, tone=tone)
    both, _ = _run(MAKERS[name], N_TONE_CALLS, tone=tone, audio_filter=["voice", None, "voice", None])
    for j, (a, b) in enumerate(zip(toned, both)):
        assert a[0] == b[0] and a[1] == b[1], f"call {j}: counts"
        assert np.array_equal(a[3], b[3]), f"call {j}: gates"
        np.testing.assert_array_equal(a[4], b[4], f"call {j}: qualities")
    gates = np.array([c[3] for c in both])
    reported = np.array([c[0] for c in both])
    print(f"{name}: slot 0 opens at call {int(np.argmax(gates[:, 0]))}; qualities at the end {both[-1][4]}")
    assert gates[-1, 0] and gates[-1, 2] and not gates[:, 1].any() and gates[:, 3].all()
    assert not gates[:40, 0].any() and (reported[~gates[:, 0], 0] == 0).all() and (reported[gates[:, 0], 0] > 0).all()
    voice = demod.voice_taps()
    for k in (0, 2):                                         # closed for most calls, continuous all the same
        ref.same(_stream(both, k), ref.fir(voice, _stream(toned, k))[0], f"slot {k}")
    for k in (1, 3):
        assert ref.bits_equal(_stream(both, k), _stream(toned, k))


def test_set_audio_filter_and_the_raster_chain(rfa):
    voice = demod.voice_taps()
    with demod.RasterReceiverBank("u8", FS_RAW, 25_000, ["nfm"] * 2, channels=[5, 17],
                                  audio_filter=[None, [0.5, 0.25]]) as chain:
        assert chain.audio_fir.taps(0).size == 0 and list(chain.audio_fir.taps(1)) == [0.5, 0.25]
        chain.set_audio_filter(0, "voice")
        assert ref.bits_equal(chain.audio_fir.taps(0), voice)
        chain.set_audio_filter(1, None)
        assert chain.audio_fir.taps(1).size == 0
        for bad in (-1, 2):
            with pytest.raises(ValueError):
                chain.set_audio_filter(bad, None)
        with pytest.raises(ValueError):
            chain.set_audio_filter(0, "bass")
        got = chain.process(raw_calls()[0])
        assert [len(g) for g in got] == chain.audio_counts and chain.audio_fir.stream == chain.demods.stream
        plain_rows = chain._audio.cpu().numpy()
        ref.same(got[0], ref.fir(voice, plain_rows[0, :len(got[0])])[0])
        assert ref.bits_equal(got[1], plain_rows[1, :len(got[1])])
    assert not hasattr(chain, "audio_fir") and chain._filtered is None
