"""GPU: the front-end channel bank (rfa_ddc_bank_*, demod.FrontEndBank / ReceiverBank,
SURVEY.md §8(f) row 4b).  Slot k of a bank must equal, bit for bit, a single-channel
``demod.FrontEnd`` created with the same arguments and given the same calls; two small cases
are also held directly against oracle/demod.py.

Not covered: a retune in which one slot is rejected.  The only rejection is an empty mixer
table, and no rate/offset pair produces one (tests/test_ddc_bank_host.py shows why), so the
all-or-nothing rule of rfa_ddc_bank_set_frequencies cannot be driven from outside."""
import numpy as np
import pytest

from oracle import demod as od
from rfanalyzer_amd import _lib
from rfanalyzer_amd import demod

pytestmark = pytest.mark.gpu

FMT = {"s8": od.IN_S8, "u8": od.IN_U8, "s16": od.IN_S16LE}
SB = {"s8": 2, "u8": 2, "s16": 4}
CENTER = 100_000_000
RAGGED = [16384, 7, 1, 0, 5000, 12345]
OFFSETS3 = [130_000, -700_000, 0]           # three table lengths; the last is the folded case


def _raw(fmt, n, seed):
    rng = np.random.default_rng(seed)
    if fmt == "s16":
        return rng.integers(-32768, 32768, 2 * n, dtype=np.int16).view(np.uint8)
    return rng.integers(0, 256, 2 * n, dtype=np.uint8)


def _same(a, b):
    assert a.shape == b.shape, (a.shape, b.shape)
    np.testing.assert_array_equal(np.ascontiguousarray(a).view(np.int32), np.ascontiguousarray(b).view(np.int32))


def _chunks(raw, fmt, sizes):
    pos = 0
    for n in sizes:
        yield raw[pos * SB[fmt]:(pos + n) * SB[fmt]]
        pos += n


def _channels(offsets):
    return [CENTER + o for o in offsets]


def _make(fmt, sr, out, offsets, resampler=False):
    bank = demod.FrontEndBank(fmt, sr, out, len(offsets), resampler=resampler)
    fes = [demod.FrontEnd(fmt, sr, out, resampler=resampler) for _ in offsets]
    bank.set_frequencies(CENTER, _channels(offsets))
    for fe, ch in zip(fes, _channels(offsets)):
        fe.set_frequencies(CENTER, ch)
    return bank, fes


def _same_mixers(bank, fes):
    for k, fe in enumerate(fes):
        c, _, mf, ci = fe.mixer()
        assert bank.channel(k) == (mf, len(c), ci), k


def _call_both(bank, fes, chunk):
    """One call on the bank and on every handle; outputs and mixer state must agree."""
    re, im = bank.process(chunk)
    assert re.shape == im.shape and re.shape[0] == len(fes)
    for k, fe in enumerate(fes):
        r_re, r_im = fe.process(chunk)
        _same(re[k], r_re)
        _same(im[k], r_im)
    _same_mixers(bank, fes)
    return re, im


def _close(bank, fes):
    bank.close()
    for fe in fes:
        fe.close()


# ------------------------------------------------------------------ 1, 2: tables, ragged calls, formats

@pytest.mark.parametrize("fmt", ["u8", "s8", "s16"])
def test_different_tables_and_ragged_calls(rfa, fmt):
    bank, fes = _make(fmt, 2_400_000, 96_000, OFFSETS3)
    assert len({bank.channel(k)[1] for k in range(3)}) == 3          # three table lengths
    assert bank.channel(2)[0] == 2_400_000                           # offset 0 folds by +sample rate
    assert bank.ratio() == fes[0].ratio()
    _same(bank.taps, fes[0].taps)
    refs = None
    if fmt == "u8":                                                  # the restatement itself, not only the sibling
        refs = [od.FrontEnd(FMT[fmt], 2_400_000, 96_000) for _ in OFFSETS3]
        for ref, ch in zip(refs, _channels(OFFSETS3)):
            ref.set_frequencies(CENTER, ch)
    raw = _raw(fmt, sum(RAGGED), 21 + len(fmt))
    for chunk in _chunks(raw, fmt, RAGGED):
        re, im = _call_both(bank, fes, chunk)
        for k, ref in enumerate(refs or []):
            r_re, r_im = ref.process(chunk)
            _same(re[k], r_re)
            _same(im[k], r_im)
            assert bank.channel(k) == (ref.cos_freq, len(ref.cos_t), ref.cosine_index)
    _close(bank, fes)


@pytest.mark.parametrize("fmt,sr,out", [("u8", 2_400_000, 96_000),       # ratio 1/25
                                        ("s8", 20_000_000, 384_000)])    # ratio 12/625: per-lane phase rows
def test_polyphase_mode(rfa, fmt, sr, out):
    offsets = [130_000, -700_000]
    bank, fes = _make(fmt, sr, out, offsets, resampler=True)
    assert bank.ratio() == fes[0].ratio()
    refs = None
    if fmt == "u8":
        refs = [od.ResamplerFrontEnd(FMT[fmt], sr, out) for _ in offsets]
        for ref, ch in zip(refs, _channels(offsets)):
            ref.set_frequencies(CENTER, ch)
    raw = _raw(fmt, sum(RAGGED), 33)
    for chunk in _chunks(raw, fmt, RAGGED):
        re, im = _call_both(bank, fes, chunk)
        for k, ref in enumerate(refs or []):
            r_re, r_im = ref.process(chunk)
            _same(re[k], r_re)
            _same(im[k], r_im)
    _close(bank, fes)


# ------------------------------------------------------------------ 3: filter longer than the LDS

def test_long_filter_uses_several_lds_chunks(rfa):
    # 20 MHz -> 10 kHz: D = 2000, 21 819 taps; against two device handles only
    bank, fes = _make("s8", 20_000_000, 10_000, [130_000, -2_700_000])
    assert bank.ratio() == (1, 2000, 21_819)
    sizes = [150_000, 80_001]
    raw = _raw("s8", sum(sizes), 8)
    for chunk in _chunks(raw, "s8", sizes):
        _call_both(bank, fes, chunk)
    _close(bank, fes)


# ------------------------------------------------------------------ 4: splitting into calls

def test_whole_buffer_equals_packets(rfa):
    raw = _raw("s8", 200_000, 11)
    a = demod.FrontEndBank("s8", 2_400_000, 48_000, 3)
    b = demod.FrontEndBank("s8", 2_400_000, 48_000, 3)
    for bank in (a, b):
        bank.set_frequencies(CENTER, _channels(OFFSETS3))
    whole = a.process(raw)
    parts = [b.process(raw[k:k + 2 * 4096]) for k in range(0, raw.size, 2 * 4096)]
    assert len(parts) == 49
    _same(whole[0], np.concatenate([p[0] for p in parts], axis=1))
    _same(whole[1], np.concatenate([p[1] for p in parts], axis=1))
    assert [a.channel(k) for k in range(3)] == [b.channel(k) for k in range(3)]
    a.close(), b.close()


# ------------------------------------------------------------------ 5, 8: device pointers

@pytest.mark.parametrize("fmt", ["u8", "s16"])
def test_misaligned_input_gives_the_same_bits(rfa, fmt):
    import torch

    n = 30_001                                     # not a multiple of 4: the scalar tail runs
    raw = _raw(fmt, n, 5)
    sb = SB[fmt]
    dev = torch.device("cuda", 0)
    aligned = torch.from_numpy(raw.copy()).to(dev)
    shifted = torch.empty(raw.size + sb, dtype=torch.uint8, device=dev)[sb:]   # off by one sample
    shifted.copy_(aligned)
    assert aligned.data_ptr() % (4 * sb) == 0 and shifted.data_ptr() % (4 * sb) == sb
    outs = []
    for t in (aligned, shifted):
        bank = demod.FrontEndBank(fmt, 2_400_000, 96_000, 3)
        bank.set_frequencies(CENTER, _channels(OFFSETS3))
        cap = bank.max_outputs(n)
        shape = (3, cap)
        re = torch.zeros(shape, dtype=torch.float32, device=dev)
        im = torch.zeros(shape, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()                   # the bank's own stream does not wait for torch's
        got = bank.process_tensor(t, re, im)
        torch.cuda.synchronize()
        outs.append((got, re.cpu().numpy()[:, :got], im.cpu().numpy()[:, :got]))
        bank.close()
    assert outs[0][0] == outs[1][0] == n // 25
    _same(outs[0][1], outs[1][1])
    _same(outs[0][2], outs[1][2])
    # and both equal the handles (host path: aligned staging buffer)
    fes = [demod.FrontEnd(fmt, 2_400_000, 96_000) for _ in OFFSETS3]
    for k, (fe, ch) in enumerate(zip(fes, _channels(OFFSETS3))):
        fe.set_frequencies(CENTER, ch)
        r_re, r_im = fe.process(raw)
        _same(outs[1][1][k], r_re)
        _same(outs[1][2][k], r_im)
        fe.close()


def test_output_rows_and_stride(rfa):
    import torch

    n = 16_384
    raw = _raw("u8", 2 * n, 17)
    dev = torch.device("cuda", 0)
    raw_t = torch.from_numpy(raw.copy()).to(dev)
    bank, fes = _make("u8", 2_400_000, 96_000, OFFSETS3)
    want = n // 25                                            # 655 outputs of the first call
    sentinel = np.float32(-12345.5)
    stride = want + 37
    shape = (3, stride)
    re = torch.full(shape, float(sentinel), dtype=torch.float32, device=dev)
    im = torch.full(shape, float(sentinel), dtype=torch.float32, device=dev)
    # a stride that is too small: RFA_ERR_SIZE, nothing enqueued, no state advanced
    before = [bank.channel(k) for k in range(3)]
    torch.cuda.synchronize()
    with pytest.raises(_lib.RfaError) as e:
        bank.process_device(raw_t.data_ptr(), n, re.data_ptr(), im.data_ptr(), want - 1)
    assert e.value.status == _lib.RFA_ERR_SIZE
    assert [bank.channel(k) for k in range(3)] == before
    torch.cuda.synchronize()
    assert (re.cpu().numpy() == sentinel).all() and (im.cpu().numpy() == sentinel).all()
    # rows at k * stride, the floats between the rows untouched
    got = bank.process_tensor(raw_t[:2 * n], re, im)
    torch.cuda.synchronize()
    assert got == want
    g_re, g_im = re.cpu().numpy(), im.cpu().numpy()
    for k, fe in enumerate(fes):
        r_re, r_im = fe.process(raw[:2 * n])
        _same(g_re[k, :got], r_re)
        _same(g_im[k, :got], r_im)
    assert (g_re[:, got:] == sentinel).all() and (g_im[:, got:] == sentinel).all()
    bank.set_stream(None)
    _call_both(bank, fes, raw[2 * n:])                        # the refused call left no trace
    _close(bank, fes)


# ------------------------------------------------------------------ 6: retune

def test_retune_one_slot_of_three(rfa):
    bank, fes = _make("u8", 2_400_000, 96_000, OFFSETS3)
    raw = _raw("u8", 4 * 9_001, 6)
    chunks = list(_chunks(raw, "u8", [9_001] * 4))
    _call_both(bank, fes, chunks[0])
    kept = [bank.channel(k) for k in range(3)]
    assert kept[0][2] != 0 and kept[1][2] != 0             # (slot 2's folded table has one entry)
    # slot 1 moves; slots 0 and 2 keep table and cosine index; no delay line is touched
    offsets = [OFFSETS3[0], 455_000, OFFSETS3[2]]
    bank.set_frequencies(CENTER, _channels(offsets))
    fes[1].set_frequencies(CENTER, CENTER + 455_000)
    assert bank.channel(0) == kept[0] and bank.channel(2) == kept[2]
    assert bank.channel(1)[0] == -455_000 and bank.channel(1)[2] == 0
    _same_mixers(bank, fes)
    _call_both(bank, fes, chunks[1])
    # the same frequencies again: nothing changes
    state = [bank.channel(k) for k in range(3)]
    bank.set_frequencies(CENTER, _channels(offsets))
    assert [bank.channel(k) for k in range(3)] == state
    _call_both(bank, fes, chunks[2])
    # all three move, one of them back to its first channel (a new table: index 0 again)
    offsets = [-130_000, OFFSETS3[1], 12_500]
    bank.set_frequencies(CENTER, _channels(offsets))
    for fe, ch in zip(fes, _channels(offsets)):
        fe.set_frequencies(CENTER, ch)
    assert [bank.channel(k)[2] for k in range(3)] == [0, 0, 0]
    _call_both(bank, fes, chunks[3])
    _close(bank, fes)


# ------------------------------------------------------------------ 7: sample-rate change

def test_sample_rate_change(rfa):
    bank, fes = _make("u8", 2_400_000, 48_000, OFFSETS3)
    raw = _raw("u8", 3 * 15_000, 12)
    chunks = list(_chunks(raw, "u8", [15_000] * 3))
    _call_both(bank, fes, chunks[0])

    def retune_all(rate):
        bank.set_sample_rate(rate)
        with pytest.raises(_lib.RfaError) as e:           # every mixer is invalid after a rate change
            bank.process(chunks[1])
        assert e.value.status == _lib.RFA_ERR_STATE
        with pytest.raises(_lib.RfaError):
            bank.channel(0)
        bank.set_frequencies(CENTER, _channels(OFFSETS3))
        for fe, ch in zip(fes, _channels(OFFSETS3)):
            fe.set_sample_rate(rate)
            fe.set_frequencies(CENTER, ch)
        assert bank.ratio() == fes[0].ratio()
        _same_mixers(bank, fes)

    retune_all(2_410_000)                                  # same decimation: filter and delay lines kept
    assert bank.ratio()[1] == 50
    assert bank.channel(0)[0] == od.mix_frequency(CENTER, CENTER + OFFSETS3[0], 2_410_000)
    _call_both(bank, fes, chunks[1])
    retune_all(1_200_000)                                  # new decimation: rebuilt, delay lines zeroed
    assert bank.ratio()[1] == 25
    _same(bank.taps, od.decimator_taps(1_200_000, 48_000)[1])
    _call_both(bank, fes, chunks[2])
    with pytest.raises(_lib.RfaError):                     # a rejected rate leaves rate and filter as they were
        bank.set_sample_rate(60_000)
    assert bank.ratio()[1] == 25
    _close(bank, fes)


# ------------------------------------------------------------------ 9: channel counts

def test_one_channel_equals_the_single_handle(rfa):
    bank, fes = _make("s8", 2_400_000, 96_000, [-455_000])
    raw = _raw("s8", sum(RAGGED), 9)
    for chunk in _chunks(raw, "s8", RAGGED):
        _call_both(bank, fes, chunk)
    _close(bank, fes)


SPLIT = 256                                   # RFA_DDC_BANK_LAUNCH_CHANNELS
SPLIT_SIZES = [4096, 4096]


def _split_offsets(k):
    return [(i - 128) * 9_000 + 1_234 for i in range(k)]


@pytest.fixture(scope="module")
def split_reference(rfa):
    """SPLIT + 1 single handles run once over the two calls; read-only for the tests below."""
    raw = _raw("u8", sum(SPLIT_SIZES), 99)
    raw.setflags(write=False)
    rows = []
    for off in _split_offsets(SPLIT + 1):
        with demod.FrontEnd("u8", 2_400_000, 96_000) as fe:
            fe.set_frequencies(CENTER, CENTER + off)
            outs = [fe.process(c) for c in _chunks(raw, "u8", SPLIT_SIZES)]
            c, _, mf, ci = fe.mixer()
            rows.append((outs, (mf, len(c), ci)))
    return raw, rows


@pytest.mark.parametrize("k", [SPLIT, SPLIT + 1])
def test_launch_bound_and_the_split(rfa, split_reference, k):
    raw, rows = split_reference
    with demod.FrontEndBank("u8", 2_400_000, 96_000, k) as bank:
        bank.set_frequencies(CENTER, _channels(_split_offsets(k)))
        for j, chunk in enumerate(_chunks(raw, "u8", SPLIT_SIZES)):
            re, im = bank.process(chunk)
            assert re.shape[0] == k
            want_re = np.stack([rows[s][0][j][0] for s in range(k)])
            want_im = np.stack([rows[s][0][j][1] for s in range(k)])
            _same(re, want_re)
            _same(im, want_im)
        assert [bank.channel(s) for s in range(k)] == [rows[s][1] for s in range(k)]


# ------------------------------------------------------------------ errors

def test_process_needs_every_mixer(rfa):
    with demod.FrontEndBank("u8", 2_400_000, 96_000, 2) as bank:
        with pytest.raises(_lib.RfaError) as e:
            bank.process(b"\x00" * 64)
        assert e.value.status == _lib.RFA_ERR_STATE
        with pytest.raises(ValueError):
            bank.set_frequencies(CENTER, [CENTER + 1000])        # one frequency per channel
        assert bank.process(b"")[0].shape == (2, 0)


# ------------------------------------------------------------------ 10: ReceiverBank

def test_receiver_bank_equals_receivers(rfa):
    modes = ["nfm", "nfm", "am"]
    assert len({demod.mode_info(m)[0] for m in modes}) == 1
    offsets = [130_000, -455_000, 12_500]
    raw = _raw("u8", 6 * 16_384, 42)
    packets = list(_chunks(raw, "u8", [16_384] * 6))
    with demod.ReceiverBank("u8", 2_400_000, modes) as rxb:
        rxb.set_frequencies(CENTER, _channels(offsets))
        got = [rxb.process(p) for p in packets]
        assert all(len(g) == 3 for g in got)
        with pytest.raises(ValueError):
            rxb.set_mode(0, "wfm")                               # another quadrature rate
        rxb.set_mode(0, "nfm")
    for k, (mode, ch) in enumerate(zip(modes, _channels(offsets))):
        with demod.Receiver("u8", 2_400_000, mode) as rx:
            rx.set_frequencies(CENTER, ch)
            for j, p in enumerate(packets):
                want = rx.process(p)
                assert want.size > 0
                _same(got[j][k], want)


def test_receiver_bank_rejects_mixed_quadrature_rates(rfa):
    with pytest.raises(ValueError):
        demod.ReceiverBank("u8", 2_400_000, ["nfm", "wfm"])
    with pytest.raises(ValueError):
        demod.ReceiverBank("u8", 2_400_000, [])
