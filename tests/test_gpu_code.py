"""GPU: the code meter bank (rfa_code_*, demod.CodeMeterBank), the DCS code squelch on a demodulator
bank's audio and the bank chains built with ``code=``.

The reference has nothing to compare with; the checks are tests/code_ref.py.  Meter: first index, sub-cell
sums, bad count and sample count per slot equal the restatement -- int64, compared with np.array_equal:
no tolerance exists here -- for counts and counters on either side of every path: a slot without samples,
one sample, a sub-cell less one, a sub-cell plus one, several blocks, counters on a sub-cell's first
sample, one before it and inside it.  Chain: decisions with wide margins (score 0.997 against 0.8 for
the right code, at most 0.58 otherwise, confirmed on the CPU with the restated demodulator), and the
restated rule on the device's own sub-cells call for call.  Equivalence: ``code=`` leaves the audio bit
for bit and only zeroes counts."""
import functools

import numpy as np
import pytest

import code_ref
from rfanalyzer_amd import _lib
from rfanalyzer_amd import demod

pytestmark = pytest.mark.gpu

F32 = np.float32
RATE = 48000
SPECIAL = [np.nan, np.inf, -np.inf, 32768.0, -32768.0, 32768.0 - 2.0 ** -9, -(32768.0 - 2.0 ** -9), 1e-40, -1e-40,
           1.4e-45, -0.0, 2.0 ** -25, 3 * 2.0 ** -25, -(2.0 ** -25), -3 * 2.0 ** -25, 5 * 2.0 ** -25, 2.0 ** -26,
           2.0 ** -24, 0.25, -0.25]
N_BAD = 5


@functools.lru_cache(maxsize=None)
def rows(k, width, seed=11):
    """[k, width] audio rows of about the size the demodulators write; read-only."""
    a = (np.random.default_rng(seed).standard_normal((k, width)) * 0.1).astype(F32)
    a.setflags(write=False)
    return a


@pytest.fixture
def meter(rfa):
    made = []

    def _meter(k=5, rate=RATE):
        m = demod.CodeMeterBank(k, rate)
        made.append(m)
        return m

    yield _meter
    for m in made:
        m.close()


def dev(x):
    import torch
    return torch.from_numpy(np.array(x, order="C")).cuda()           # a copy: the cached inputs are read-only


def check(got, audio, counts, refs, what=""):
    """One call's results against the restated slots (code_ref.Carry), which this advances."""
    first, cells, bad, n = got
    assert first.dtype == bad.dtype == n.dtype == np.int64
    for k, (c, ref) in enumerate(zip(counts, refs)):
        wfirst, wcells, wbad = ref.call(audio[k, :c])
        assert cells[k].dtype == np.int64
        assert np.array_equal(cells[k], wcells), f"{what} slot {k}: sums"
        assert (first[k], bad[k], n[k]) == (wfirst, wbad, c), f"{what} slot {k}"


# ------------------------------------------------------------------ sums

# at 48 kHz sub-cell 1 starts at sample 45, sub-cell 201 at sample 8974
@pytest.mark.parametrize("bases,counts", [((0, 45, 44, 20, 8974), (0, 1, 44, 46, 327)),
                                          ((45, 0, 8973, 44, 20), (16385, 327, 46, 44, 1)),
                                          ((44, 44, 0, 45, 8974), (46, 16385, 0, 23500, 12000))])
def test_one_call_equals_the_restatement(meter, bases, counts):
    m = meter()
    refs = [code_ref.Carry(RATE) for _ in range(5)]
    lead = rows(5, max(bases), seed=3)
    check(m.process(lead, bases), lead, bases, refs, "lead")           # the counters to where the call starts
    assert [r.g for r in refs] == list(bases)
    audio = np.array(rows(5, max(counts)))
    for k, c in enumerate(counts):                                     # every slot that has room holds the specials
        if c >= 40:
            audio[k, 7 + k:7 + k + len(SPECIAL)] = np.array(SPECIAL, F32)
    got = m.process(audio, counts)
    check(got, audio, counts, refs, f"bases {bases} counts {counts}")
    assert [int(b) for b in got[2]] == [N_BAD if c >= 40 else 0 for c in counts]
    # the same rows again: the counters went on by each slot's own count, the carries with them
    check(m.process(audio, counts), audio, counts, refs, "again")


def test_quantised_samples_on_their_own(meter):
    """One sample per call and slot: the sub-cell sum is q(a), or 0 and a bad count."""
    m = meter(len(SPECIAL))
    a = np.array(SPECIAL, F32).reshape(-1, 1)
    first, cells, bad, n = m.process(a)
    assert not first.any() and list(n) == [1] * len(SPECIAL)
    assert all(c.size == 0 for c in cells)                             # sample 1 still falls into sub-cell 0: held back
    m2 = meter(len(SPECIAL))
    wide = np.zeros((len(SPECIAL), 45), F32)
    wide[:, :1] = a
    first, cells, bad2, n = m2.process(wide)                           # 45 samples complete sub-cell 0
    q, isbad = code_ref.quantise(a[:, 0])
    assert np.array_equal(np.array([c[0] for c in cells]), np.where(isbad, 0, q)) and all(c.size == 1 for c in cells)
    assert list(bad) == list(bad2) == [int(b) for b in isbad] and int(isbad.sum()) == N_BAD
    want = {2.0 ** -25: 0, 3 * 2.0 ** -25: 2, -3 * 2.0 ** -25: -2, 5 * 2.0 ** -25: 2, 2.0 ** -24: 1,
            32768.0 - 2.0 ** -9: 2 ** 39 - 2 ** 15, 0.25: 2 ** 22}
    for v, w in want.items():
        assert cells[SPECIAL.index(v)][0] == w, v


def test_a_bad_sample_stays_in_its_slot(meter):
    counts = (4097, 12000, 300, 46, 0)
    audio = np.array(rows(5, max(counts)))
    clean = meter().process(audio, counts)
    assert not clean[2].any()
    for bad in (np.nan, np.inf, -np.inf, 32768.0):
        audio[1, 9000] = bad
        got = meter().process(audio, counts)
        assert list(got[2]) == [0, 1, 0, 0, 0]
        for k in (0, 2, 3, 4):
            assert np.array_equal(got[1][k], clean[1][k])
        j = code_ref.subcell(9000, RATE)
        diff = np.flatnonzero(got[1][1] != clean[1][1])
        assert list(diff) == [j] and got[1][1][j] == clean[1][1][j] - code_ref.quantise(rows(5, 12000)[1, 9000:9001])[0][0]


@pytest.mark.parametrize("rate", [48000, 8000])
def test_a_stream_cut_into_calls_gives_the_sub_cells_of_the_stream_given_whole(meter, rate):
    n, K = 6000, 3
    stream = np.array(rows(K, n, seed=rate))
    stream[2, 100:100 + len(SPECIAL)] = np.array(SPECIAL, F32)
    whole_meter = meter(K, rate)
    wfirst, wcells, wbad, wn = whole_meter.process(stream)
    for k in range(K):
        assert np.array_equal(wcells[k], code_ref.completed(stream[k], rate)) and wfirst[k] == 0
    assert list(wbad) == [0, 0, N_BAD]
    rng = np.random.default_rng(rate + 1)
    for trial in range(3):
        m = meter(K, rate)
        refs = [code_ref.Carry(rate) for _ in range(K)]
        pos = [0] * K
        got = [[] for _ in range(K)]
        bad = np.zeros(K, np.int64)
        calls = 0
        while min(pos) < n:
            counts = [0 if rng.integers(4) == 0 else int(min(n - p, rng.integers(1, 1500))) for p in pos]
            width = max(max(counts), 1)
            audio = np.zeros((K, width), F32)
            for k, (p, c) in enumerate(zip(pos, counts)):
                audio[k, :c] = stream[k, p:p + c]
            res = m.process(audio, counts)
            check(res, audio, counts, refs, f"trial {trial} call {calls}")
            for k in range(K):
                if res[1][k].size:
                    assert res[0][k] == len(got[k])                    # the index goes on without a gap
                    got[k] += list(res[1][k])
                pos[k] += counts[k]
            bad += res[2]
            calls += 1
        assert calls > 6
        for k in range(K):
            assert np.array_equal(np.array(got[k], np.int64), wcells[k]), (trial, k)
        assert np.array_equal(bad, wbad)


def test_sums_do_not_depend_on_k_stride_offset_entry_or_run(meter):
    import torch
    counts33 = [(37 * k * k + 1) % 30000 for k in range(33)]
    counts33[5], counts33[20] = 0, 30000
    audio = rows(33, 30000)
    m = meter(33)
    host = m.process(audio, counts33)
    check(host, audio, counts33, [code_ref.Carry(RATE) for _ in range(33)], "K = 33")
    # the device entry on a wider tensor at an offset: audio_stride above every n
    wide = torch.zeros(33, 30000 + 77, dtype=torch.float32, device="cuda")
    for off in (0, 1, 13):
        view = wide[:, off:off + 30000]
        view.copy_(dev(audio))
        m.break_()
        got = m.process_tensor(view, counts33)
        for a, b in zip(got, host):
            assert all(np.array_equal(x, y) for x, y in zip(a, b)), f"offset {off}"
    # two runs, and K = 1 on each row alone
    again = meter(33).process(audio, counts33)
    for a, b in zip(again, host):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    for k in (0, 7, 20):
        one = meter(1)
        got = one.process(audio[k:k + 1], [counts33[k]])
        assert np.array_equal(got[1][0], host[1][k]) and got[2][0] == host[2][k] and got[0][0] == host[0][k]
        t = dev(audio[k:k + 1, :counts33[k] + 5])
        one.break_()
        got = one.process_tensor(t, [counts33[k]])                      # K = 1: the stride is not looked at
        assert np.array_equal(got[1][0], host[1][k])


def test_no_samples_at_all_launch_nothing(meter):
    m = meter(3)
    audio = rows(3, 300)
    refs = [code_ref.Carry(RATE) for _ in range(3)]
    check(m.process(audio, (50, 60, 70)), audio, (50, 60, 70), refs)
    for call in range(2):
        first, cells, bad, n = m.process(audio, (0, 0, 0))
        assert not n.any() and not bad.any() and all(c.size == 0 for c in cells)
        assert list(first) == [code_ref.subcell(g, RATE) for g in (50, 60, 70)]
    check(m.process(audio, (50, 60, 70)), audio, (50, 60, 70), refs, "the counters and the carries stayed")
    m.break_(1)
    refs[1] = code_ref.Carry(RATE)
    check(m.process(audio, (50, 60, 70)), audio, (50, 60, 70), refs, "break(1)")
    m.reset()
    refs = [code_ref.Carry(RATE) for _ in range(3)]
    check(m.process(audio, (300, 200, 100)), audio, (300, 200, 100), refs, "reset")


def test_state_and_argument_errors_consume_nothing(meter):
    import torch
    m = meter(3)
    audio = rows(3, 300)
    a = dev(audio)
    refs = [code_ref.Carry(RATE) for _ in range(3)]
    m.process_device(a.data_ptr(), a.stride(0), (300, 200, 100))
    with pytest.raises(_lib.RfaError) as e:
        m.process_device(a.data_ptr(), a.stride(0), (10, 10, 10))        # the call before is uncollected
    assert e.value.status == _lib.RFA_ERR_STATE
    with pytest.raises(_lib.RfaError) as e:
        m.process(audio, (10, 10, 10))
    assert e.value.status == _lib.RFA_ERR_STATE
    check(m.collect(), audio, (300, 200, 100), refs, "the first call")
    again = m.collect()                                                  # nothing new: the values repeat
    assert list(again[3]) == [300, 200, 100] and [c.size for c in again[1]] == [6, 4, 2]
    for bad in ((301, 1, 1), (1, 1, 2 ** 40)):
        with pytest.raises(_lib.RfaError) as e:
            m.process_device(a.data_ptr(), 300, bad)
        assert e.value.status == _lib.RFA_ERR_INVALID
    with pytest.raises(_lib.RfaError) as e:
        m.process_device(0, 300, (1, 1, 1))                              # a NULL row with a count above 0
    assert e.value.status == _lib.RFA_ERR_INVALID
    with pytest.raises(_lib.RfaError) as e:
        m._call("process", a.data_ptr(), 300, None)
    assert e.value.status == _lib.RFA_ERR_INVALID
    for k in (3, -2):
        with pytest.raises(_lib.RfaError):
            m.break_(k)
    # the counters and the carries are where the good call left them
    check(m.process_tensor(a, (10, 10, 10)), audio, (10, 10, 10), refs, "after the errors")
    # a break while a call is uncollected drops what that call holds of the slot
    m.process_device(a.data_ptr(), a.stride(0), (300, 300, 300))
    m.break_(1)
    first, cells, bad, n = m.collect()
    assert cells[1].size == 0 and first[1] == 0 and n[1] == 0 and cells[0].size > 0 and n[0] == 300
    for k in (0, 2):
        refs[k].call(audio[k, :300])
    refs[1] = code_ref.Carry(RATE)
    check(m.process_tensor(a, (100, 100, 100)), audio, (100, 100, 100), refs, "after the break")
    torch.cuda.synchronize()


# ------------------------------------------------------------------ the squelch on a demodulator bank

FS_Q = 96000
WANTED = ["023"] * 4


@functools.lru_cache(maxsize=None)
def quadrature():
    return tuple(code_ref.four_signals(int(1.5 * FS_Q), FS_Q))


def test_code_squelch_on_a_demodulator_bank(rfa):
    """Four NFM slots in calls of 4096, every slot asked for 023: the slot with 023 under voice opens behind
    its first window and stays open; the slots with 047 (023 inverted), with 025 under voice and with voice
    alone never open."""
    import torch
    sig = quadrature()
    n = sig[0].size
    re = dev(np.stack([s.real for s in sig]).astype(F32))
    im = dev(np.stack([s.imag for s in sig]).astype(F32))
    audio = torch.zeros(4, 4096, dtype=torch.float32, device="cuda")
    rule = demod.CodeRule(4)
    for k, entry in enumerate(WANTED):
        rule.set_code(k, *demod.dcs_parse(entry))
    ref = code_ref.Rule(4, 0.8, 2, [code_ref.word(0o023)] * 4)
    assert (rule.words, rule.threshold, rule.hang, rule.need) == (4, 0.8, 2, ref.need)
    gates, done = [], np.zeros(4, np.int64)
    first_open = None
    with demod.DemodulatorBank(["nfm"] * 4) as bank, demod.CodeMeterBank(4, RATE) as meter:
        for j, lo in enumerate(range(0, n, 4096)):
            hi = min(lo + 4096, n)
            counts = bank.process_tensor(re[:, lo:hi], im[:, lo:hi], audio)
            if meter.stream != bank.stream:
                meter.set_stream(bank.stream)                # one stream, as in a chain
            # what a chain does behind its demodulators: collect call j-1, step the rule, enqueue call j
            first, cells, bad, cnt = meter.collect()
            gate = rule.update(first, [c.size for c in cells], cells, bad, cnt)
            assert list(gate) == ref.update(first, cells, bad, cnt), f"call {j}"
            np.testing.assert_allclose(rule.score, ref.score, rtol=0, atol=1e-12)
            assert not bad.any()
            done += [c.size for c in cells]
            if first_open is None and done[0] >= rule.need:
                first_open = j                               # call j-1 completed slot 0's first window
            meter.process_device(audio.data_ptr(), audio.stride(0), counts)
            gates.append(list(gate))
        meter.collect()
        bank.synchronize()
        score = rule.score
    gates = np.array(gates)
    print(f"first window complete before call {first_open}; scores at the end {score}")
    assert first_open == 17                                  # 744 sub-cells are 33215 audio samples, 2048 to the call
    assert not gates[:first_open, 0].any() and gates[first_open:, 0].all()
    assert not gates[:, 1:].any()
    assert score[0] > 0.95 and (score[1:] < 0.7).all()       # decisions with margins, not tolerances


# ------------------------------------------------------------------ the chains

FS_RAW = 2_400_000
CALL = 131072
CENTRE = 100_000_000
OFFSETS = [-600_000, -200_000, 200_000, 600_000]
N_CALLS = 15                                                 # 0.82 s: one window and the calls after it


@functools.lru_cache(maxsize=None)
def raw_calls():
    """u8 raw IQ at 2.4 Msps carrying the four signals at OFFSETS, cut into calls."""
    n = N_CALLS * CALL
    sig = code_ref.four_signals(n, FS_RAW, seed=92)
    t = np.arange(n) / FS_RAW
    x = sum(0.4 * s * np.exp(2j * np.pi * f * t) for s, f in zip(sig, OFFSETS))
    iq = np.empty(2 * n)
    iq[0::2], iq[1::2] = x.real, x.imag
    u8 = np.clip(np.rint(iq * 128 + 127.4), 0, 255).astype(np.uint8)
    return [u8[2 * CALL * j:2 * CALL * (j + 1)] for j in range(N_CALLS)]


def _receiver(**kw):
    return demod.ReceiverBank("u8", FS_RAW, ["nfm"] * 4, **kw)


def _tuned(**kw):
    return demod.TunedReceiverBank("u8", FS_RAW, 25_000, ["nfm"] * 4, **kw)


def _tune(chain):
    chain.set_frequencies(CENTRE, [CENTRE + f for f in OFFSETS])
    return chain


def _stage(chain, raw):
    """One host packet into the chain's raw staging buffer: (device address, samples)."""
    import torch
    buf = np.ascontiguousarray(raw)
    chain._buffers(buf.size, buf.size // 2)
    chain.synchronize()
    chain._raw[:buf.size].copy_(torch.from_numpy(buf.copy()))
    torch.cuda.synchronize()
    return chain._raw.data_ptr(), buf.size // 2


@pytest.mark.parametrize("make", [_receiver, _tuned], ids=["ReceiverBank", "TunedReceiverBank"])
def test_a_chain_with_codes_leaves_the_audio_and_zeroes_counts(rfa, make):
    calls = raw_calls()
    with _tune(make()) as plain, _tune(make(code=WANTED)) as coded:
        assert plain.code_open is None and plain.code_score is None and not hasattr(plain, "code_meter")
        with pytest.raises(ValueError):
            plain.set_code(0, "023")
        assert list(coded.code_open) == [False] * 4
        assert coded.code_meter.stream == coded.demods.stream
        opened, total, due = [], 0, None
        for j, raw in enumerate(calls):
            want = plain.process(raw)
            got_counts = coded.process_device(*_stage(coded, raw))
            coded.synchronize()
            gate = coded.code_open
            audio = coded.audio_tensor.cpu().numpy()
            for k in range(4):
                assert got_counts[k] == (len(want[k]) if gate[k] else 0), (j, k)
                assert np.array_equal(audio[k, :len(want[k])].view(np.int32), want[k].view(np.int32)), (j, k)
            opened.append(list(gate))
            # the rule sees call j's sub-cells in call j + 1
            total += len(want[0])
            if due is None and code_ref.subcell(total, RATE) >= coded._code.need:
                due = j + 1
        opened = np.array(opened)
        score = coded.code_score
        print(f"gates per call {opened.astype(int).tolist()}; scores {score}; first window seen in call {due}")
        assert due is not None and 0 < due < N_CALLS - 1
        assert not opened[:due, 0].any() and opened[due:, 0].all()
        assert not opened[:, 1:].any()                               # the inverse code, another code, no code
        assert score[0] > 0.95 and (score[1:] < 0.7).all()
        # set_code: slot 0 loses its code and reads open, slot 1 is asked for what it carries and starts closed
        coded.set_code(0, None)
        coded.set_code(1, "023I")
        assert list(coded.code_open) == [True, False, False, False] and np.isnan(coded.code_score[1])
        for bad in (-1, 4):
            with pytest.raises(ValueError):
                coded.set_code(bad, "023")
        with pytest.raises(ValueError):
            coded.set_code(2, "0234")
    assert not hasattr(coded, "code_meter") and coded.code_open is None


def test_a_chain_with_code_none_is_the_chain_without_the_keyword(rfa):
    calls = raw_calls()[:3]
    with _tune(_receiver()) as plain, _tune(_receiver(code=None)) as none:
        assert not hasattr(none, "code_meter") and none._code is None and none.code_open is None
        for raw in calls:
            want, got = plain.process(raw), none.process(raw)
            assert [len(w) for w in want] == [len(g) for g in got] and all(len(w) > 0 for w in want)
            assert all(np.array_equal(w.view(np.int32), g.view(np.int32)) for w, g in zip(want, got))


def test_codes_with_the_other_keywords(rfa):
    """With a tone on another slot, the filter and the resampler: a code-closed slot is treated as a
    tone-closed one -- 0 counts, no PCM -- and its streams stay continuous."""
    calls = raw_calls()[:2]
    with _tune(_receiver(code=["023", None, None, None], tone=[None, 100.0, None, None], audio_filter=["voice"] * 4,
                         pcm=8000)) as chain:
        for raw in calls:
            got = chain.process(raw)
            assert [len(g) > 0 for g in got] == [False, False, True, True]
            pcm = chain.pcm()
            assert [len(p) > 0 for p in pcm] == [False, False, True, True]
            assert all(c > 0 for c in chain.pcm_counts) and all(c > 0 for c in chain.audio_counts)
        assert list(chain.code_open) == [False, True, True, True] and list(chain.tone_open) == [True, False, True, True]
        with pytest.raises(ValueError):
            chain.set_code(1, "023")                                 # the slot has a tone
    with pytest.raises(ValueError):
        _receiver(code=["023", None, None, None], tone=[100.0, None, None, None])
    with demod.RasterReceiverBank("u8", FS_RAW, 25_000, ["nfm"] * 2, channels=[5, 17], code=["023", None]) as raster:
        got = raster.process(calls[0])
        assert list(raster.code_open) == [False, True] and len(got[0]) == 0 and len(got[1]) > 0
