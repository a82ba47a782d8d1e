"""GPU: the tone meter bank (rfa_tone_*, demod.ToneMeterBank), the tone squelch on a demodulator bank's
audio and the bank chains built with ``tone=``.

The reference has nothing to compare with; the checks are tests/tone_ref.py.  Meter: the eight sums
per slot equal the restatement bit for bit -- the plan of tests/slot_sum_plan.py on terms formed with
the library's own phasors (rfa_tone_phasor fills the device's table) -- for per-slot counts on either
side of every path: one launch, two launches, a slot without samples, the fold's second fetch.  Chain:
decisions with wide margins (quality about 0.07 against 0.01, guard power ratio about 50 against 4,
confirmed on the CPU with the restated demodulator), and the restated rule on the device's own sums
call for call.  Equivalence: ``tone=`` leaves the audio bit for bit and only zeroes counts."""
import functools

import numpy as np
import pytest

import slot_sum_plan as plan
import tone_ref
from rfanalyzer_amd import _lib
from rfanalyzer_amd import demod

pytestmark = pytest.mark.gpu

F32 = np.float32
TILE = plan.TILE
RATE = 48000
M = 10 * RATE
PROBES = [(670, 693, 2541), (693, 2541, 670), (2541, 670, 693)]      # 67.0 / 69.3 / 254.1 Hz, turned per slot
COUNTS = [(0, 1, 257), (63, 64, 65), (4097, TILE, TILE + 1), (2 * TILE + 1, 40000, 5), (0, 64 * TILE + 1, 0)]


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.int64)


def same_bits(got, want, what=""):
    np.testing.assert_array_equal(bits(got), bits(want), what)


@functools.lru_cache(maxsize=None)
def rows(width):
    """[3, width] audio rows: the real rows of slot_sum_plan.pin_rows."""
    return plan.pin_rows(width)[0]


def want_sums(audio, counts, bases, probes=PROBES, rate=RATE):
    """[8, 3] of the restatement on the library's phasors."""
    table = tone_ref.library_table(rate)
    return np.stack([tone_ref.sums(audio[k, :counts[k]], probes[k], bases[k], rate, table)
                     for k in range(len(counts))], axis=1)


@pytest.fixture
def meter(rfa):
    made = []

    def _meter(k=3, rate=RATE, probes=PROBES):
        m = demod.ToneMeterBank(k, rate)
        made.append(m)
        for slot, f10 in enumerate(probes or []):
            m.set_probes(slot, f10)
        return m

    yield _meter
    for m in made:
        m.close()


def dev(x):
    import torch
    return torch.from_numpy(np.array(x, order="C")).cuda()           # a copy: the cached inputs are read-only


# ------------------------------------------------------------------ sums

@pytest.mark.parametrize("counts", COUNTS)
def test_sums_equal_the_restatement(meter, counts):
    m = meter()
    assert [m.probes(k) for k in range(3)] == [list(p) for p in PROBES]
    audio = rows(max(counts))
    sums, n = m.process(audio, counts)
    assert sums.dtype == np.float64 and sums.shape == (8, 3) and n.dtype == np.int64
    assert list(n) == list(counts)
    same_bits(sums, want_sums(audio, counts, [0, 0, 0]), f"counts {counts}")
    for k, c in enumerate(counts):
        if c == 0:                                           # zero sums, +0.0
            assert not sums[:, k].any() and not np.signbit(sums[:, k]).any()
    # the same rows again: the index went on by each slot's own count
    sums, n = m.process(audio, counts)
    same_bits(sums, want_sums(audio, counts, [c % M for c in counts]), f"counts {counts}, second call")


def test_no_samples_at_all_launch_nothing_and_read_zero(meter):
    m = meter()
    audio = rows(257)
    m.process(audio, (5, 6, 7))
    for call in range(2):
        sums, n = m.process(audio, (0, 0, 0))
        assert not sums.any() and not n.any()
    sums, _ = m.process(audio, (5, 6, 7))
    same_bits(sums, want_sums(audio, (5, 6, 7), [5, 6, 7]), "the counters stayed")


def test_a_row_cut_into_calls_meets_the_absolute_index(meter):
    m = meter()
    audio = rows(40000)
    cuts = [0, 1, 4097, 16385, 40000]
    for lo, hi in zip(cuts, cuts[1:]):
        sums, n = m.process(audio[:, lo:hi])
        assert list(n) == [hi - lo] * 3
        same_bits(sums, want_sums(audio[:, lo:hi], [hi - lo] * 3, [lo] * 3), f"piece {lo}:{hi}")
    # after break the index starts at 0: slot 1 alone, then every slot
    m.break_(1)
    sums, _ = m.process(audio[:, :300])
    same_bits(sums, want_sums(audio, [300] * 3, [40000, 0, 40000]), "break(1)")
    m.break_()
    sums, _ = m.process(audio[:, :300])
    same_bits(sums, want_sums(audio, [300] * 3, [0, 0, 0]), "break()")
    m.reset()
    sums, n = m.collect()
    assert not sums.any() and not n.any()
    sums, _ = m.process(audio[:, :300])
    same_bits(sums, want_sums(audio, [300] * 3, [0, 0, 0]), "reset")
    assert [m.probes(k) for k in range(3)] == [list(p) for p in PROBES]


def test_the_counter_crossing_m_meets_the_same_phasors(meter):
    """At 8000 Hz M is 80000: a call that ends 10 samples short of M, then one that crosses it."""
    rate, big = 8000, 80000 - 10
    m = meter(rate=rate)
    audio = rows(big)
    sums, _ = m.process(audio)
    same_bits(sums, want_sums(audio, [big] * 3, [0, 0, 0], rate=rate), "up to M - 10")
    sums, _ = m.process(audio[:, :40])
    want = want_sums(audio, [40] * 3, [big] * 3, rate=rate)
    same_bits(sums, want, "across M")
    # ... which are the phasors of the absolute sample: samples 10 ... 39 of the call are 0 ... 29 after a break
    table = tone_ref.library_table(rate)
    for f10 in PROBES[0]:
        assert np.array_equal(tone_ref.indices(f10, big, 40, rate)[10:], tone_ref.indices(f10, 0, 30, rate))
    sums, _ = m.process(audio[:, :7])
    same_bits(sums, want_sums(audio, [7] * 3, [30] * 3, rate=rate), "the counter is kept modulo M")
    assert table.shape == (80000, 2)


def test_sums_do_not_depend_on_offset_stride_or_slot_order(meter):
    import torch
    counts = (2 * TILE + 1, 40000, 5)
    audio = rows(max(counts))
    m = meter()
    want = want_sums(audio, counts, [0, 0, 0])
    wide = torch.zeros(3, max(counts) + 77, dtype=torch.float32, device="cuda")
    for off in (0, 1, 13):
        view = wide[:, off:off + max(counts)]
        view.copy_(dev(audio))
        m.break_()
        sums, n = m.process_tensor(view, counts)
        same_bits(sums, want, f"offset {off}, stride {wide.stride(0)}")
        assert list(n) == list(counts)
    # the slots turned round, with their probes
    order = [2, 0, 1]
    t = meter(probes=[PROBES[k] for k in order])
    sums, n = t.process(np.stack([audio[k] for k in order]), [counts[k] for k in order])
    same_bits(sums, want[:, order], "slot order")
    # more slots in the handle: K is not in the sum
    six = meter(6, probes=list(PROBES) + list(PROBES))
    sums, _ = six.process(np.concatenate([audio, audio]), list(counts) + list(counts))
    same_bits(sums, np.concatenate([want, want], axis=1), "K = 6")


def test_a_nan_stays_in_its_slot(meter):
    counts = (4097, TILE + 1, 300)
    audio = np.array(rows(max(counts)))
    clean, _ = meter().process(audio, counts)
    for bad in (np.nan, np.inf, -np.inf):
        audio[1, 9000] = bad
        sums, _ = meter().process(audio, counts)
        same_bits(sums[:, [0, 2]], clean[:, [0, 2]], f"{bad} in slot 1")
        assert not np.isfinite(sums[:6, 1]).any() and not np.isfinite(sums[6, 1])
        assert not np.isfinite(sums[7, 1])
    audio[1, 9000] = 0.25
    same_bits(meter().process(audio, counts)[0][:, [0, 2]], clean[:, [0, 2]])


def test_an_unused_probe_reads_plus_zero(meter):
    probes = [(670, 0, 2541), (0, 0, 0), (0, 693, 0)]
    m = meter(probes=probes)
    counts = (TILE + 1, 257, 4097)
    audio = rows(max(counts))
    sums, _ = m.process(audio, counts)
    same_bits(sums, want_sums(audio, counts, [0, 0, 0], probes=probes))
    for k, f10s in enumerate(probes):
        for j, f10 in enumerate(f10s):
            pair = sums[2 * j:2 * j + 2, k]
            assert (pair != 0.0).all() if f10 else (not pair.any() and not np.signbit(pair).any()), (k, j)
    assert (sums[6] > 0).all() and (sums[7] != 0).all()


def test_a_count_above_the_stride_is_invalid_and_consumes_nothing(meter):
    import torch
    m = meter()
    audio = rows(300)
    a = dev(audio)
    first, _ = m.process_tensor(a, (300, 200, 100))
    for bad in ((301, 1, 1), (1, 1, 2 ** 40)):
        with pytest.raises(_lib.RfaError) as e:
            m.process_device(a.data_ptr(), 300, bad)
        assert e.value.status == _lib.RFA_ERR_INVALID
    with pytest.raises(_lib.RfaError) as e:
        m.process_device(0, 300, (1, 1, 1))                  # a NULL row with a count above 0
    assert e.value.status == _lib.RFA_ERR_INVALID
    sums, n = m.collect()                                    # nothing new: the values repeat
    same_bits(sums, first)
    assert list(n) == [300, 200, 100]
    sums, _ = m.process_tensor(a, (10, 10, 10))
    same_bits(sums, want_sums(audio, (10, 10, 10), [300, 200, 100]), "the counters stayed where the good call left them")
    for k, f10 in ((3, (1, 2, 3)), (0, (RATE * 5, 0, 0)), (0, (-1, 0, 0))):
        with pytest.raises(_lib.RfaError):
            m.set_probes(k, f10)
    torch.cuda.synchronize()


def test_two_calls_before_one_collect_give_the_second_calls_values(meter):
    m = meter()
    audio = rows(TILE + 1)
    a = dev(audio)
    m.process_device(a.data_ptr(), a.stride(0), (TILE + 1, 300, 7))         # two launches
    m.process_device(a.data_ptr(), a.stride(0), (100, 0, 9))                # one
    sums, n = m.collect()
    assert list(n) == [100, 0, 9]
    same_bits(sums, want_sums(audio, (100, 0, 9), [TILE + 1, 300, 7]))
    again, n2 = m.collect()
    same_bits(again, sums)
    assert list(n2) == list(n)
    # more calls in flight than the record ring has entries
    for call in range(20):
        m.process_device(a.data_ptr(), a.stride(0), (call + 1, 2, 3))
    sums, n = m.collect()
    base = [TILE + 1 + 100 + sum(range(1, 20)), 300 + 2 * 19, 7 + 9 + 3 * 19]
    assert list(n) == [20, 2, 3]
    same_bits(sums, want_sums(audio, (20, 2, 3), base), "the twentieth call")


# ------------------------------------------------------------------ the squelch on a demodulator bank

FS_Q = 96000


@functools.lru_cache(maxsize=None)
def quadrature():
    return tuple(tone_ref.four_signals(int(1.5 * FS_Q), FS_Q))


def test_tone_squelch_on_a_demodulator_bank(rfa):
    """Four NFM slots in calls of 4096, every slot asked for 100.0 Hz (guards 97.4 and 103.5): the slot
    with the 100.0 Hz tone under voice opens behind its first window and stays open; the slots with a
    103.5 Hz tone, with voice alone and with noise alone never open."""
    import torch
    sig = quadrature()
    n = sig[0].size
    re = dev(np.stack([s.real for s in sig]).astype(F32))
    im = dev(np.stack([s.imag for s in sig]).astype(F32))
    audio = torch.zeros(4, 4096, dtype=torch.float32, device="cuda")
    f10 = demod._tone_probes(100.0)
    assert f10 == [1000, 974, 1035]
    rule, ref = demod.ToneRule(4, RATE), tone_ref.Rule(4, RATE)
    gates, seen = [], np.zeros(4, np.int64)
    first_open = None
    with demod.DemodulatorBank(["nfm"] * 4) as bank, demod.ToneMeterBank(4, RATE) as meter:
        for k in range(4):
            meter.set_probes(k, f10)
        for j, lo in enumerate(range(0, n, 4096)):
            hi = min(lo + 4096, n)
            counts = bank.process_tensor(re[:, lo:hi], im[:, lo:hi], audio)
            if meter.stream != bank.stream:
                meter.set_stream(bank.stream)                # one stream, as in a chain
            # what a chain does behind its demodulators: collect call j-1, step the rule, enqueue call j
            sums, cnt = meter.collect()
            gate = rule.update(sums, cnt)
            assert list(gate) == ref.update(sums, cnt), f"call {j}"
            np.testing.assert_array_equal(rule.quality, ref.q)
            seen += cnt
            if first_open is None and seen[0] >= 0.5 * RATE:
                first_open = j                               # call j-1 completed slot 0's first window
            meter.process_device(audio.data_ptr(), audio.stride(0), counts)
            gates.append(list(gate))
        bank.synchronize()
        q = rule.quality
    gates = np.array(gates)
    print(f"first window complete before call {first_open}; quality at the end {q}")
    assert first_open == 12                                  # 12 calls of 2048 audio samples pass 24000
    assert not gates[:first_open, 0].any() and gates[first_open:, 0].all()
    assert not gates[:, 1:].any()
    assert q[0] > 0.03 and (q[1:] < 0.005).all()             # decisions with margins, not tolerances


# ------------------------------------------------------------------ the chains

FS_RAW = 2_400_000
CALL = 131072
CENTRE = 100_000_000
OFFSETS = [-600_000, -200_000, 200_000, 600_000]
N_CALLS = 13                                                 # 0.71 s: one window and the call after it


@functools.lru_cache(maxsize=None)
def raw_calls():
    """u8 raw IQ at 2.4 Msps carrying the four signals at OFFSETS, cut into calls; then one call of silence."""
    n = N_CALLS * CALL
    sig = tone_ref.four_signals(n, FS_RAW, seed=78)
    t = np.arange(n) / FS_RAW
    x = sum(0.4 * s * np.exp(2j * np.pi * f * t) for s, f in zip(sig, OFFSETS))
    iq = np.empty(2 * n)
    iq[0::2], iq[1::2] = x.real, x.imag
    u8 = np.clip(np.rint(iq * 128 + 127.4), 0, 255).astype(np.uint8)
    return [u8[2 * CALL * j:2 * CALL * (j + 1)] for j in range(N_CALLS)]


def _bank(**kw):
    b = demod.ReceiverBank("u8", FS_RAW, ["nfm"] * 4, **kw)
    b.set_frequencies(CENTRE, [CENTRE + f for f in OFFSETS])
    return b


def test_receiver_bank_with_tones_leaves_the_audio_and_zeroes_counts(rfa):
    calls = raw_calls()
    with _bank() as plain, _bank(tone=[100.0, 100.0, 100.0, None]) as toned:
        assert plain.tone_open is None and plain.tone_quality is None and not hasattr(plain, "tone_meter")
        with pytest.raises(ValueError):
            plain.set_tone(0, 100.0)
        assert list(toned.tone_open) == [False, False, False, True]
        opened = []
        for j, raw in enumerate(calls):
            want = plain.process(raw)
            got_counts = toned.process_device(*_stage(toned, raw))
            toned.synchronize()
            gate = toned.tone_open
            audio = toned.audio_tensor.cpu().numpy()
            for k in range(4):
                assert got_counts[k] == (len(want[k]) if gate[k] else 0), (j, k)
                assert np.array_equal(audio[k, :len(want[k])].view(np.int32), want[k].view(np.int32)), (j, k)
            opened.append(list(gate))
        opened = np.array(opened)
        q = toned.tone_quality
        print(f"gates per call {opened.astype(int).tolist()}; quality {q}")
        assert opened[:, 3].all() and not opened[:, 1:3].any()       # no tone asked: open; wrong tone, no tone: closed
        first = int(np.argmax(opened[:, 0]))
        assert opened[first:, 0].all() and not opened[:first, 0].any() and 0 < first < N_CALLS
        # the first window is 24000 audio samples, 131072 raw samples are 2621.44: calls 0 ... 9 pass it, and
        # call 10 collects call 9's sums
        assert first == 10
        assert q[0] > 0.03 and q[1] < 0.005 and q[2] < 0.005 and np.isnan(q[3])
        # set_tone: slot 3 gets a tone and starts closed, slot 0 loses its and reads open
        toned.set_tone(3, 100.0)
        toned.set_tone(0, None)
        assert list(toned.tone_open) == [True, False, False, False]
        assert toned.tone_meter.probes(3) == [1000, 974, 1035] and toned.tone_meter.probes(0) == [0, 0, 0]
        for bad in (-1, 4):
            with pytest.raises(ValueError):
                toned.set_tone(bad, 100.0)
    assert not hasattr(toned, "tone_meter") and toned.tone_open is None


def _stage(chain, raw):
    """One host packet into the chain's raw staging buffer: (device address, samples)."""
    import torch
    buf = np.ascontiguousarray(raw)
    chain._buffers(buf.size, buf.size // 2)
    chain.synchronize()
    chain._raw[:buf.size].copy_(torch.from_numpy(buf.copy()))
    torch.cuda.synchronize()
    return chain._raw.data_ptr(), buf.size // 2


def test_a_slot_the_carrier_squelch_closes_resets_its_tone_gate(rfa):
    calls = raw_calls()
    silence = np.full(2 * CALL, 127, np.uint8)
    with _bank(squelch=[-15.0, None, None, None], tone=[100.0, None, None, None]) as chain:
        chain.squelch_debounce = 1
        for raw in calls[:12]:
            counts = chain.process(raw)
        assert chain.open[0] and chain.tone_open[0] and len(counts[0]) > 0
        print(f"levels {chain.levels}; quality {chain.tone_quality}")
        counts = chain.process(silence)                      # the carrier gate closes: no audio from slot 0
        assert not chain.open[0] and len(counts[0]) == 0
        assert chain.tone_open[0]                            # the tone gate lags by one call
        counts = chain.process(calls[12])                    # the carrier is back; the call before had no samples
        assert chain.open[0] and not chain.tone_open[0] and len(counts[0]) == 0
        assert np.isnan(chain.tone_quality[0])
        assert all(len(c) > 0 for c in counts[1:]) and chain.tone_open[1:].all()


def test_the_other_chains_take_the_keyword(rfa):
    for make in (lambda: demod.RasterReceiverBank("u8", FS_RAW, 25_000, ["nfm"] * 2, channels=[5, 17],
                                                  tone=[100.0, None]),
                 lambda: demod.TunedReceiverBank("u8", FS_RAW, 25_000, ["nfm"] * 2, tone=[100.0, None])):
        with make() as chain:
            counts = chain.process(raw_calls()[0])
            assert list(chain.tone_open) == [False, True]
            assert len(counts[0]) == 0 and len(counts[1]) > 0
            assert chain.tone_meter.stream == chain.demods.stream
