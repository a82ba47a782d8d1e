"""GPU: the audio IIR bank (rfa_audio_iir_*, demod.AudioIirBank) and the bank chains built with
``audio_iir=``.

The reference has no recursive filter; the check is tests/audio_iir_ref.py, the definition of the blocked
recurrence in numpy float32.  Finite values and infinities are compared bit for bit and NaNs by position.
C is the plan's chunk in samples (blocks per chunk x 128): the counts sit around a block and around a
chunk, fresh and behind a first call that leaves the head block under way."""
import functools

import numpy as np
import pytest

import audio_iir_ref as ref
from rfanalyzer_amd import _lib
from rfanalyzer_amd import demod

pytestmark = pytest.mark.gpu

F32 = np.float32
B = ref.B
C = _lib.RFA_AUDIO_IIR_CHUNK_BLOCKS * B
LONG = 2 * C + 5


@functools.lru_cache(maxsize=None)
def sections(name):
    if name is None:
        return None
    if name == "notch8":                                     # eight sections: four notches twice
        return np.concatenate([ref.notch_sections(hz, r) for hz, r in
                               ((1000.0, 0.999), (50.0, 0.99), (2000.0, 0.995), (400.0, 0.98))] * 2)
    return demod._audio_iir_sections(name)


@functools.lru_cache(maxsize=None)
def row(n, seed=5):
    x = ref.rows(1, n, seed)[0]
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def long_whole(name):
    """The restatement's row of row(LONG) given whole, computed once."""
    y = ref.blocked(sections(name), row(LONG))
    y.setflags(write=False)
    return y


@pytest.fixture
def bank(rfa):
    made = []

    def _bank(k=1, secs=()):
        b = demod.AudioIirBank(k)
        made.append(b)
        for slot, s in enumerate(secs):
            b.set_sections(slot, s)
        return b

    yield _bank
    for b in made:
        b.close()


def dev(x):
    import torch
    return torch.from_numpy(np.array(x, dtype=F32, order="C")).cuda()


# ------------------------------------------------------------------ counts around a block and a chunk

def test_plan_reports_the_chunk():
    p = demod.audio_iir_plan(5, LONG)
    assert p["block"] == B and p["block"] * p["chunk_blocks"] == C and p["chunks"] == 3 and p["path"] == "blocked"
    assert demod.audio_iir_plan(5, C)["chunks"] == 1 and demod.audio_iir_plan(5, C, 1)["chunks"] == 2


@pytest.mark.parametrize("n", [1, 127, 128, 129, C - 1, C, C + 1, LONG])
def test_counts_fresh_and_behind_a_partial_head_block(bank, n):
    """Slot 0 fresh, slot 1 behind a call of 1 sample, slot 2 behind a call of 127: the head block of the
    last two is under way with a carried z."""
    sec = sections("voice+deemphasis")
    b = bank(3, [sec] * 3)
    slots = [ref.Slot(sec) for _ in range(3)]
    firsts = [0, 1, 127]
    head = ref.rows(3, 127, seed=7)
    got = b.process(head, firsts)
    for k in range(3):
        ref.same(got[k], slots[k].process(head[k, :firsts[k]]), f"first call, slot {k}")
    x = np.stack([row(n, seed=10 + k) for k in range(3)])
    got = b.process(x)
    for k in range(3):
        assert got[k].dtype == F32 and got[k].size == n
        ref.same(got[k], slots[k].process(x[k]), f"n {n} behind {firsts[k]}")
    x2 = ref.rows(3, 300, seed=6)                            # the call after it meets the carry this one left
    got = b.process(x2)
    for k in range(3):
        ref.same(got[k], slots[k].process(x2[k]), f"n {n} behind {firsts[k]}, the call after")


# ------------------------------------------------------------------ split invariance

@pytest.mark.parametrize("name", ["voice+deemphasis", "notch8"])
def test_a_row_cut_into_calls_gives_the_row_given_whole(bank, name):
    sec = sections(name)
    x = row(LONG)
    whole = bank(1, [sec]).process(x[None, :])[0]
    ref.same(whole, long_whole(name), "whole")
    rng = np.random.Generator(np.random.PCG64(31))
    cuts = set(int(c) for c in rng.integers(1, LONG, 10))
    cuts |= set(range(5 * B - 3, 5 * B + 4)) | set(range(C - 3, C + 4))      # single samples across a block and a chunk edge
    b = bank(1, [sec])
    pieces, at = [], 0
    for c in sorted(cuts) + [LONG]:
        pieces.append(b.process(x[None, at:c])[0])
        at = c
    assert ref.bits_equal(np.concatenate(pieces), whole), f"{len(pieces)} calls"


# ------------------------------------------------------------------ slots of their own

def test_five_slots_with_their_own_sections_and_counts(bank):
    """S = 0, 1, 4, 5, 8 in one launch; slot 1 has no samples on alternate calls and keeps its carry; slot 3's
    row is shorter than a block."""
    names = [None, "deemphasis", "voice", "voice+deemphasis", "notch8"]
    b = bank(5, [sections(n) for n in names])
    assert [b.sections(k).shape[0] for k in range(5)] == [0, 1, 4, 5, 8]
    for k, n in enumerate(names):
        assert n is None or ref.bits_equal(b.sections(k), sections(n))
    slots = [ref.Slot(sections(n)) for n in names]
    x = ref.rows(5, C + 300, seed=8)
    at = 0
    for call, counts in enumerate(([700, 333, C + 300, 50, 129], [128, 0, 5, 77, 1000], [1, 200, 0, 100, 127],
                                   [C + 1, 0, 300, 1, 0], [300, 300, 300, 127, 300])):
        got = b.process(x, counts)
        for k in range(5):
            assert got[k].size == counts[k]
            ref.same(got[k], slots[k].process(x[k, :counts[k]]), f"call {call} slot {k}: S {len(slots[k].sec)} n {counts[k]}")


def test_pass_through_hands_on_the_bits(bank):
    odd = np.array([0x7fc00001, 0xffc12345, 0x7f800001, 0xff800001, 0x7f800000, 0xff800000, 0x80000000, 0x00000000,
                    0x00000001, 0x807fffff, 0x3f800000], np.uint32).view(F32)
    x = np.array(ref.rows(2, C + 40, seed=3))
    x[0, :odd.size] = odd
    x[0, C + 7:C + 7 + odd.size] = odd
    b = bank(2, [None, sections("deemphasis")])
    got = b.process(x, [C + 40, 300])
    assert ref.bits_equal(got[0], x[0]), "no sections: output = input"
    ref.same(got[1], ref.blocked(sections("deemphasis"), x[1, :300]))


def test_a_non_finite_sample_stays_in_its_slot_from_its_block_on(bank):
    n = 6 * B + 50
    names = ["voice", None, "voice+deemphasis", "deemphasis"]
    x = np.array(ref.rows(4, n, seed=14))
    make = lambda: bank(4, [sections(s) for s in names])
    clean = make().process(x)
    p_nan = 2 * B + 40
    x[2, p_nan], x[2, 4 * B + 3] = np.nan, np.inf
    b = make()
    got = b.process(x)
    for k in (0, 1, 3):
        assert ref.bits_equal(got[k], clean[k]), f"slot {k} changed"
    assert ref.bits_equal(got[2][:p_nan], clean[2][:p_nan]) and not np.isfinite(got[2][p_nan:]).any()
    s = ref.Slot(sections(names[2]))
    ref.same(got[2], s.process(x[2]))
    x2 = ref.rows(4, 300, seed=15)
    got = b.process(x2)                                      # the state stays non-finite ...
    assert not np.isfinite(got[2]).any()
    ref.same(got[2], s.process(x2[2]))
    b.reset(2)                                               # ... until the slot is reset; the others go on
    s.reset()
    after = b.process(x2)
    ref.same(after[2], s.process(x2[2]), "after reset(2)")
    assert ref.bits_equal(after[2], ref.blocked(sections(names[2]), x2[2]))
    cont = make()
    cont.process(x[:, :n])
    cont.process(x2)
    want = cont.process(x2)
    for k in (0, 1, 3):
        assert ref.bits_equal(after[k], want[k]), f"slot {k} after reset(2)"


def test_a_burst_decays_through_subnormals_to_zero(bank):
    sec = sections("deemphasis")
    x = np.concatenate([row(1000, seed=17), np.zeros(40000, F32)])
    want = ref.blocked(sec, x)
    tiny = np.finfo(F32).tiny
    subnormal = (want != 0) & (np.abs(want) < tiny)
    zero_from = int(np.flatnonzero(want != 0)[-1]) + 1
    print(f"{int(subnormal.sum())} subnormal outputs, exact zeros from sample {zero_from} on")
    assert subnormal.sum() > 100 and 1000 < zero_from < 10000 and (want[zero_from:] == 0).all()
    got = bank(1, [sec]).process(x[None, :])[0]
    assert ref.bits_equal(got, want)


# ------------------------------------------------------------------ queueing, determinism, errors

def test_new_sections_and_reset_between_queued_calls(bank):
    """Ten calls in flight, more than the record ring holds; set_sections(0) and reset(1) sit between the
    fifth and the sixth: the calls before see the old sections, the calls after a zeroed slot, slot 2
    nothing."""
    import torch
    n = 600
    x = ref.rows(3, 10 * n, seed=15)
    xd = dev(x)
    names = ["voice", "voice+deemphasis", "notch8"]

    def run(sync):
        b = bank(3, [sections(s) for s in names])
        out = torch.zeros(3, 10 * n, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        for j in range(10):
            if j == 5:
                b.set_sections(0, sections("deemphasis"))
                b.reset(1)
            b.process_device(xd.data_ptr() + 4 * j * n, 10 * n, [n, n - j, n], out.data_ptr() + 4 * j * n, 10 * n)
            if sync:
                b.synchronize()
        b.synchronize()
        return out.cpu().numpy()

    queued, stepped = run(False), run(True)
    assert ref.bits_equal(queued, stepped)
    assert ref.bits_equal(queued, run(False)), "two runs give the same bits"
    slots = [ref.Slot(sections(s)) for s in names]
    for j in range(10):
        if j == 5:
            slots[0].set_sections(sections("deemphasis"))
            slots[1].reset()
        for k, c in enumerate((n, n - j, n)):
            ref.same(queued[k, j * n:j * n + c], slots[k].process(x[k, j * n:j * n + c]), f"call {j} slot {k}")


def test_process_host_equals_process_and_two_runs_agree(bank):
    import torch
    names = ["voice+deemphasis", "deemphasis"]
    counts = [C + 77, 500]
    x = ref.rows(2, C + 77, seed=19)
    host = bank(2, [sections(s) for s in names]).process(x, counts)
    again = bank(2, [sections(s) for s in names]).process(x, counts)
    b = bank(2, [sections(s) for s in names])
    xd, out = dev(x), torch.full((2, C + 100), 7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    b.process_tensor(xd, counts, out)
    b.synchronize()
    got = out.cpu().numpy()
    for k in range(2):
        assert ref.bits_equal(host[k], again[k]) and ref.bits_equal(host[k], got[k, :counts[k]])
        assert (got[k, counts[k]:] == 7.0).all()             # nothing behind a slot's count is written
        ref.same(host[k], ref.blocked(sections(names[k]), x[k, :counts[k]]))


def test_a_refused_call_consumes_nothing(bank):
    import torch
    n = 400
    x = ref.rows(2, 2 * n, seed=16)
    xd = dev(x)
    secs = [sections("voice"), sections("deemphasis")]

    def run(bad):
        b = bank(2, secs)
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
        s = ref.Slot(secs[k])
        s.process(x[k, :n])
        ref.same(want[k, n:n + c], s.process(x[k, n:n + c]))
    b = bank(2, secs)                                        # counts that are all 0 launch nothing and need no rows
    b.process_device(0, 0, [0, 0], 0, 0)
    assert all(g.size == 0 for g in b.process(x[:, :0]))
    for bad in ([[1.0, 0.0, 0.0, 0.0, 1.0]], [[1.0, 0.0, 0.0, -1.5, 0.5]], [[np.nan, 0.0, 0.0, 0.0, 0.0]],
                np.zeros((9, 5), F32)):
        with pytest.raises(_lib.RfaError) as e:
            b.set_sections(0, bad)
        assert e.value.status == _lib.RFA_ERR_INVALID
    assert ref.bits_equal(b.sections(0), secs[0])
    for k in (-1, 2):
        with pytest.raises(_lib.RfaError):
            b.set_sections(k, secs[0])
        with pytest.raises(_lib.RfaError):
            b.reset(k if k > 0 else -2)


# ------------------------------------------------------------------ the chains

FS_RAW = 2_400_000
PACKET = 16384
BIG = 50 * (C + 700)                                         # more than C audio samples per slot
CALLS = (PACKET, PACKET, BIG, PACKET)
CENTRE = 100_000_000
OFFSETS = [-600_000, -200_000, 200_000, 600_000]
IIR = ["voice+deemphasis", None, "voice", "deemphasis"]


@functools.lru_cache(maxsize=None)
def raw_calls():
    """u8 raw IQ at 2.4 Msps: noise, which every demodulator turns into audio."""
    rng = np.random.Generator(np.random.PCG64(79))
    return [rng.integers(0, 256, 2 * n, dtype=np.uint8) for n in CALLS]


def _receiver_bank(**kw):
    chain = demod.ReceiverBank("u8", FS_RAW, ["nfm"] * 4, **kw)
    chain.set_frequencies(CENTRE, [CENTRE + f for f in OFFSETS])
    return chain


def _tuned_bank(**kw):
    chain = demod.TunedReceiverBank("u8", FS_RAW, 25_000, ["nfm"] * 4, **kw)
    chain.set_frequencies(CENTRE, [CENTRE + f for f in OFFSETS])
    return chain


def _raster_bank(**kw):
    return demod.RasterReceiverBank("u8", FS_RAW, 25_000, ["nfm"] * 4, channels=[5, 17, 40, 70], **kw)


MAKERS = {"ReceiverBank": _receiver_bank, "TunedReceiverBank": _tuned_bank, "RasterReceiverBank": _raster_bank}


def _rows(t, counts):
    rows = t.cpu().numpy()
    return [rows[k, :c].copy() for k, c in enumerate(counts)]


def _run(make, **kw):
    """Per call: reported counts, audio_counts, the demodulators' rows, the IIR bank's, the filter's, what
    process returned, pcm(), and the gates and qualities."""
    out = []
    with make(**kw) as chain:
        for raw in raw_calls():
            got = chain.process(raw)
            counts = chain.audio_counts
            for k, g in enumerate(got):                      # what process returns is the head of audio_tensor's row
                assert ref.bits_equal(g, chain.audio_tensor[k, :len(g)].cpu().numpy())
            out.append({
                "reported": [len(g) for g in got], "counts": counts, "plain": _rows(chain._audio, counts),
                "iir": None if chain._iir_rows is None else _rows(chain._iir_rows, counts),
                "fir": None if chain._filtered is None else _rows(chain._filtered, counts),
                "last": _rows(chain.audio_tensor, counts),
                "pcm": chain.pcm() if hasattr(chain, "audio_rs") else None,
                "gates": (chain.tone_open, chain.code_open), "quality": (chain.tone_quality, chain.code_score)})
        attrs = sorted(vars(chain))                          # before close() takes the handles away
        for name in ("audio_iir", "audio_fir", "audio_rs"):
            if hasattr(chain, name):
                assert getattr(chain, name).stream == chain.demods.stream
    return out, attrs


@functools.lru_cache(maxsize=None)
def plain_run(name):
    return _run(MAKERS[name])


@functools.lru_cache(maxsize=None)
def iir_run(name):
    return _run(MAKERS[name], audio_iir=IIR)


@pytest.mark.parametrize("name", sorted(MAKERS))
def test_chain_rows_equal_the_bank_on_the_plain_rows(bank, name):
    plain, _ = plain_run(name)
    got, _ = iir_run(name)
    assert min(plain[0]["counts"]) > 2 * B and min(plain[2]["counts"]) > C     # a small packet, a call longer than C
    b = bank(4, [sections(s) for s in IIR])
    for j, (p, g) in enumerate(zip(plain, got)):
        assert p["reported"] == g["reported"] == p["counts"] == g["counts"], f"call {j}: counts"
        assert g["fir"] is None and g["pcm"] is None
        width = max(p["counts"])
        rows = np.zeros((4, width), F32)
        for k, r in enumerate(p["plain"]):
            rows[k, :r.size] = r
            assert ref.bits_equal(g["plain"][k], r), f"call {j} slot {k}: the demodulators' rows"
        want = b.process(rows, p["counts"])
        for k in range(4):
            assert ref.bits_equal(g["iir"][k], want[k]) and ref.bits_equal(g["last"][k], want[k]), f"call {j} slot {k}"
    assert ref.bits_equal(np.concatenate([g["iir"][1] for g in got]), np.concatenate([p["plain"][1] for p in plain]))
    k = 0                                                    # and the bank is the restatement on the whole stream
    ref.same(np.concatenate([g["iir"][k] for g in got]),
             ref.blocked(sections(IIR[k]), np.concatenate([p["plain"][k] for p in plain])), "slot 0 against the restatement")


@pytest.mark.parametrize("name", sorted(MAKERS))
def test_filter_and_resampler_read_the_iir_rows(rfa, name):
    fir = ["voice", [0.5, 0.25], None, None]
    got, _ = _run(MAKERS[name], audio_iir=IIR, audio_filter=fir, pcm=8000)
    with_iir, _ = iir_run(name)
    with demod.AudioFilterBank(4) as f, demod.AudioResamplerBank.for_rates(4, 8000) as rs:
        f.set_taps(0, demod.voice_taps())
        f.set_taps(1, [0.5, 0.25])
        for j, (a, g) in enumerate(zip(with_iir, got)):
            assert a["counts"] == g["counts"] == g["reported"]
            width = max(g["counts"])
            rows = np.zeros((4, width), F32)
            for k in range(4):
                assert ref.bits_equal(g["iir"][k], a["iir"][k]), f"call {j} slot {k}: the IIR rows"
                rows[k, :g["counts"][k]] = g["iir"][k]
            filtered = f.process(rows, g["counts"])
            for k in range(4):
                assert ref.bits_equal(g["fir"][k], filtered[k]) and ref.bits_equal(g["last"][k], filtered[k]), (j, k)
                rows[k, :g["counts"][k]] = filtered[k]
            pcm = rs.process(rows, g["counts"])
            for k in range(4):
                assert np.array_equal(g["pcm"][k], pcm[k]) and pcm[k].size > 0, f"call {j} slot {k}: pcm"


@pytest.mark.parametrize("name", sorted(MAKERS))
def test_meters_read_the_demodulators_rows(rfa, name):
    """tone= and code= with and without audio_iir=: the same reported counts, gates and qualities call for call."""
    kw = {"tone": [100.0, None, 103.5, None], "code": [None, "023", None, None]}
    a, _ = _run(MAKERS[name], **kw)
    b, _ = _run(MAKERS[name], audio_iir=IIR, **kw)
    for j, (p, g) in enumerate(zip(a, b)):
        assert p["reported"] == g["reported"] and p["counts"] == g["counts"], f"call {j}: counts"
        for x, y in zip(p["gates"] + p["quality"], g["gates"] + g["quality"]):
            np.testing.assert_array_equal(x, y, f"call {j}")
        for k in range(4):
            assert ref.bits_equal(p["plain"][k], g["plain"][k])
    assert any(np.isfinite(g["quality"][0]).any() for g in b), "no tone window was evaluated"


@pytest.mark.parametrize("name", sorted(MAKERS))
def test_audio_iir_none_adds_nothing(rfa, name):
    plain, attrs = plain_run(name)
    got, got_attrs = _run(MAKERS[name], audio_iir=None)
    assert attrs == got_attrs and "audio_iir" not in attrs and "_iir_rows" not in attrs
    for j, (p, g) in enumerate(zip(plain, got)):
        assert p["reported"] == g["reported"] and p["counts"] == g["counts"] and g["iir"] is None
        for k in range(4):
            assert ref.bits_equal(p["last"][k], g["last"][k]), f"call {j} slot {k}"
    with MAKERS[name]() as chain:
        assert chain._iir_rows is None
        with pytest.raises(ValueError):
            chain.set_audio_iir(0, "voice")
        chain.process(raw_calls()[0])
        assert chain._iir_rows is None and chain.audio_tensor is chain._audio


def test_set_audio_iir(rfa):
    with _raster_bank(audio_iir=[None, [[0.5, 0.25, 0.0, -0.5, 0.0]], None, None]) as chain:
        assert chain.audio_iir.sections(0).shape == (0, 5) and list(chain.audio_iir.sections(1)[0]) == [0.5, 0.25, 0.0, -0.5, 0.0]
        chain.set_audio_iir(0, "voice")
        assert ref.bits_equal(chain.audio_iir.sections(0), demod.tone_strip_sections())
        chain.set_audio_iir(1, None)
        assert chain.audio_iir.sections(1).shape == (0, 5)
        for bad in (-1, 4):
            with pytest.raises(ValueError):
                chain.set_audio_iir(bad, None)
        with pytest.raises(ValueError):
            chain.set_audio_iir(0, "bass")
        got = chain.process(raw_calls()[0])
        plain = chain._audio.cpu().numpy()
        ref.same(got[0], ref.blocked(demod.tone_strip_sections(), plain[0, :len(got[0])]))
        assert ref.bits_equal(got[1], plain[1, :len(got[1])])
    assert not hasattr(chain, "audio_iir") and chain._iir_rows is None
