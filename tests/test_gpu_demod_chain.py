"""GPU: the demodulator (rfanalyzer_amd/csrc/demod.hip through rfa_demod_* and
demod.Demodulator / demod.Receiver) against the restated chain of
tests/demod_chain_ref.py.

AM, LSB, USB and CW audio, every filter's taps and the carried state are
compared bit for bit (int32 views, NaN positions by mask).  FM's products are
exact and only the angle may differ: the device's double atan2 and the host's
are each accurate to about an ulp of a double, so their float casts differ with
probability near 2^-27 per sample.  With the audio sink off every FM sample must
be within 2 float32 ulps (1 from the angle, doubled at most by rounding the
product with quadratureGain); with it on within 2^-20 * max|x| * sum|taps| (each
input off by at most 2^-22 relative, times 4 for the re-rounded partial sums);
and at most 1 sample in 1000 may differ at all.
"""
import functools

import numpy as np
import pytest

import demod_chain_ref as ref
from oracle import demod as od

pytestmark = pytest.mark.gpu

F32 = np.float32
PACKETS = [1, 0, 2, 26, 27, 28, 181, 182, 363, 1000, 4097]
TOTAL = sum(PACKETS)
EXACT = [ref.AM, ref.LSB, ref.USB, ref.CW]
FM = [ref.NFM, ref.WFM]
ALL = EXACT + FM
NAME = ref.MODE_NAMES


@functools.lru_cache(maxsize=None)
def noise(n=TOTAL, seed=11):
    rng = np.random.Generator(np.random.PCG64(seed))
    re = (0.3 * rng.standard_normal(n)).astype(F32)
    im = (0.3 * rng.standard_normal(n)).astype(F32)
    re.setflags(write=False)
    im.setflags(write=False)
    return re, im


def tone(mode, n=3000):
    rate = ref.MODE_INFO[mode][0]
    f = {ref.AM: 0.0, ref.NFM: 1500.0, ref.WFM: 20000.0, ref.LSB: -1000.0, ref.USB: 1000.0, ref.CW: 750.0}[mode]
    t = np.arange(n)
    env = 1 + 0.5 * np.cos(2 * np.pi * 1000.0 * t / rate) if mode == ref.AM else 1.0
    x = 0.4 * env * np.exp(2j * np.pi * f * t / rate)
    return x.real.astype(F32), x.imag.astype(F32)


def split(re, im, sizes):
    out, s = [], 0
    for n in sizes:
        out.append((re[s:s + n], im[s:s + n]))
        s += n
    return out


def even(total, ps):
    ps = ps if ps > 0 else max(total, 1)
    return [min(ps, total - s) for s in range(0, max(total, 1), ps)]


def assert_same(got, want, what=""):
    got, want = np.asarray(got, F32), np.asarray(want, F32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), (what, "NaN positions", int(gn.sum()), int(wn.sum()))
    bad = np.nonzero((got.view(np.int32) != want.view(np.int32)) & ~gn)[0]
    assert bad.size == 0, (what, bad.size, bad[:5], got[bad[:5]], want[bad[:5]])


def assert_state(dev, chain, what=""):
    assert_same(np.array(dev.state(), F32), np.array(chain.state(), F32), what + " state")


def ordered(x):
    i = np.asarray(x, F32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


def assert_fm(got, want, chain, sink, what=""):
    """The module docstring's FM bars; prints the number of differing samples."""
    got, want = np.asarray(got, F32), np.asarray(want, F32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    differ = int(np.count_nonzero(got.view(np.int32) != want.view(np.int32)))
    print(f"{what}: {differ} of {got.size} samples differ from the restatement")
    if got.size == 0:
        return
    if sink:
        x = chain.pre_sink
        bound = 2.0 ** -20 * float(np.max(np.abs(x))) if x.size else 0.0
        for t in chain.sink.taps_in_use(chain.packet_rate):
            bound *= float(np.sum(np.abs(t.astype(np.float64))))
        err = float(np.max(np.abs(got.astype(np.float64) - want.astype(np.float64))))
        assert err <= bound, (what, err, bound)
    else:
        ulps = int(np.max(np.abs(ordered(got) - ordered(want))))
        assert ulps <= 2, (what, ulps)
    assert differ * 1000 <= got.size, (what, differ, got.size)


def check(mode, got, want, chain, sink, what):
    if mode in FM:
        assert_fm(got, want, chain, sink, what)
    else:
        assert_same(got, want, what)


@functools.lru_cache(maxsize=None)
def reference(mode, ps, sink=True):
    """The restatement over the noise, one call of packet size ps: (audio, state, the chain
    afterwards).  Shared between tests: nobody may feed the returned chain again."""
    re, im = noise()
    c = ref.DemodChain(mode, audio_sink=sink)
    audio = c.process(re, im, ps)
    audio.setflags(write=False)
    return audio, c.state(), c


@pytest.fixture
def make(rfa):
    from rfanalyzer_amd import demod
    made = []

    def _make(mode, sink=True):
        d = demod.Demodulator(mode, audio_sink=sink)
        made.append(d)
        return d

    yield _make
    for d in made:
        d.close()


# ------------------------------------------------------------------ taps

def test_taps_are_bit_identical(make):
    z = np.zeros(4, F32)
    for mode in ALL:
        d, c = make(mode), ref.DemodChain(mode)
        assert d.taps("user")[0].size == 0                  # no filter before the first packet
        d.process(z, z)
        c.process(z, z)
        re, im, dec = d.taps("user")
        assert_same(re, c.user.taps, NAME[mode] + " user taps")
        assert dec == 1 and re.size == 27 and not im.any()
        assert_same(d.taps("audio1")[0], c.sink.f1.taps, "audio1")
        assert_same(d.taps("audio2")[0], c.sink.f2.taps, "audio2")
        assert d.taps("audio1")[2] == 2 and d.taps("audio2")[2] == 4
        assert d.taps("audio1")[0].size == 9 and d.taps("audio2")[0].size == 13
        if mode in (ref.LSB, ref.USB, ref.CW):
            re, im, dec = d.taps("bandpass")
            assert_same(re, c.band.tr, NAME[mode] + " band-pass re")
            assert_same(im, c.band.ti, NAME[mode] + " band-pass im")
            assert dec == c.band.d and re.size == 181
        else:
            assert d.taps("bandpass")[0].size == 0


def test_width_limits_give_the_restatements_taps(make):
    for mode in (ref.AM, ref.WFM, ref.USB, ref.LSB, ref.CW):
        for w in (ref.MODE_INFO[mode][1], ref.MODE_INFO[mode][2], ref.MODE_INFO[mode][1] + 1):
            d, c = make(mode), ref.DemodChain(mode)
            d.channelWidth = w
            c.set_width(w)
            assert d.channelWidth == c.width
            z = np.zeros(3, F32)
            d.process(z, z)
            c.process(z, z)
            assert_same(d.taps("user")[0], c.user.taps, f"{NAME[mode]} {w} user")
            if c.band is not None:
                assert_same(d.taps("bandpass")[0], c.band.tr, f"{NAME[mode]} {w} band re")
                assert_same(d.taps("bandpass")[1], c.band.ti, f"{NAME[mode]} {w} band im")


# ------------------------------------------------------------------ packets and calls

@pytest.mark.parametrize("mode", ALL, ids=lambda m: NAME[m])
def test_packet_list_as_separate_calls(make, mode):
    re, im = noise()
    d, c = make(mode), ref.DemodChain(mode)
    for k, (r, i) in enumerate(split(re, im, PACKETS)):
        want = c.process(r, i)
        assert d.max_outputs(len(r)) == len(want)
        got = d.process(r, i)
        check(mode, got, want, c, True, f"{NAME[mode]} call {k} ({len(r)} samples)")
        assert_state(d, c, f"{NAME[mode]} call {k}")


@pytest.mark.parametrize("ps", [1, 27, 1000, 0])
@pytest.mark.parametrize("mode", ALL, ids=lambda m: NAME[m])
def test_one_call_split_into_packets(make, mode, ps):
    re, im = noise()
    want, state, c = reference(mode, ps)
    d = make(mode)
    assert d.max_outputs(TOTAL) == len(want)
    got = d.process(re, im, ps)
    check(mode, got, want, c, True, f"{NAME[mode]} one call, packets of {ps}")
    assert_same(np.array(d.state(), F32), np.array(state, F32), "state")
    # one call per packet: the same bits, FM included (device against device)
    e = make(mode)
    parts = [e.process(r, i) for r, i in split(re, im, even(TOTAL, ps))]
    assert_same(np.concatenate(parts), got, f"{NAME[mode]} call per packet of {ps}")
    assert_same(np.array(e.state(), F32), np.array(d.state(), F32), "state, call per packet")


@pytest.mark.parametrize("mode", ALL, ids=lambda m: NAME[m])
def test_audio_sink_off_is_the_demodulators_buffer(make, mode):
    re, im = noise()
    want, state, c = reference(mode, 1000, False)
    d = make(mode, sink=False)
    got = d.process(re, im, 1000)
    check(mode, got, want, c, False, f"{NAME[mode]} sink off")
    assert_same(np.array(d.state(), F32), np.array(state, F32), "state")


@pytest.mark.parametrize("mode", ALL, ids=lambda m: NAME[m])
def test_tone(make, mode):
    re, im = tone(mode)
    for sink in (True, False):
        d, c = make(mode, sink), ref.DemodChain(mode, audio_sink=sink)
        d.audioVolumeLevel = 0.5
        c.volume = F32(0.5)
        for ps in (700, 0):
            want = c.process(re, im, ps)
            got = d.process(re, im, ps)
            check(mode, got, want, c, sink, f"{NAME[mode]} tone sink={sink} ps={ps}")
            assert_state(d, c, NAME[mode] + " tone")
        assert np.isfinite(got).all() and np.abs(got).max() > 1e-3


def test_silent_first_am_packet_is_nan(make):
    z = np.zeros(64, F32)
    re, im = noise()
    for sink in (False, True):
        d, c = make(ref.AM, sink), ref.DemodChain(ref.AM, audio_sink=sink)
        want, got = c.process(z, z), d.process(z, z)
        assert np.isnan(want).all() and want.size > 0
        assert_same(got, want, "silent AM packet")
        assert_state(d, c, "silent AM packet")
        assert_same(d.process(re[:500], im[:500]), c.process(re[:500], im[:500]), "AM after silence")
        assert_state(d, c, "AM after silence")


# ------------------------------------------------------------------ rebuild rules

def test_width_change_rebuilds_the_user_filter(make):
    re, im = noise()
    for mode in (ref.AM, ref.NFM, ref.USB):
        d, c = make(mode, False), ref.DemodChain(mode, audio_sink=False)
        a = slice(0, 600)
        check(mode, d.process(re[a], im[a]), c.process(re[a], im[a]), c, False, "before")
        w = ref.MODE_INFO[mode][1] + 123
        d.channelWidth = w
        c.set_width(w)
        b = slice(600, 1200)
        want, got = c.process(re[b], im[b]), d.process(re[b], im[b])
        if mode != ref.USB:
            assert len(got) == 599                              # a fresh filter drops one sample
        check(mode, got, want, c, False, NAME[mode] + " after the width change")
        assert_same(d.taps("user")[0], c.user.taps, "user taps after the width change")
        assert_state(d, c, "width change")
        # the same width again: no rebuild, nothing dropped
        d.channelWidth = w
        want, got = c.process(re[a], im[a]), d.process(re[a], im[a])
        if mode != ref.USB:
            assert len(got) == 600
        check(mode, got, want, c, False, NAME[mode] + " same width")


def test_band_pass_is_rebuilt_between_usb_lsb_cw(make):
    re, im = noise()
    d, c = make(ref.USB), ref.DemodChain(ref.USB)
    pos = 0
    for mode in (ref.USB, ref.LSB, ref.CW, ref.USB, ref.USB):
        d.demodulationMode = mode
        c.set_mode(mode)
        assert d.channelWidth == c.width == ref.MODE_INFO[mode][3]
        s = slice(pos, pos + 700)
        pos += 700
        assert_same(d.process(re[s], im[s], 300), c.process(re[s], im[s], 300), NAME[mode] + " in the round")
        assert_same(d.taps("bandpass")[0], c.band.tr, NAME[mode] + " band re")
        assert_same(d.taps("bandpass")[1], c.band.ti, NAME[mode] + " band im")
        assert d.taps("bandpass")[2] == c.band.d
        assert_state(d, c, NAME[mode] + " in the round")
    # CW's integer rule: 750 + 301 / 2 == (750 + 150.5f).toInt(), so 300 -> 301 keeps the filter
    for w in (300, 301, 302):
        d.demodulationMode = ref.CW
        c.set_mode(ref.CW)
        d.channelWidth = w
        c.set_width(w)
        s = slice(pos, pos + 400)
        pos += 400
        assert_same(d.process(re[s], im[s]), c.process(re[s], im[s]), f"CW width {w}")
        assert_same(d.taps("bandpass")[0], c.band.tr, f"CW width {w} taps")


def test_am_wfm_am_keeps_the_audio_filters(make):
    re, im = noise()
    d, c = make(ref.AM), ref.DemodChain(ref.AM)
    pos = 0
    for mode in (ref.AM, ref.WFM, ref.AM, ref.NFM, ref.USB, ref.WFM):
        d.demodulationMode = mode
        c.set_mode(mode)
        s = slice(pos, pos + 801)
        pos += 801
        want, got = c.process(re[s], im[s], 400), d.process(re[s], im[s], 400)
        check(mode, got, want, c, True, NAME[mode] + " in the AM/WFM round")
        assert_state(d, c, NAME[mode] + " in the AM/WFM round")


def test_off_returns_nothing_and_moves_nothing(make):
    re, im = noise()
    d, c = make(ref.AM), ref.DemodChain(ref.AM)
    assert_same(d.process(re[:500], im[:500]), c.process(re[:500], im[:500]), "before OFF")
    before = d.state()
    d.demodulationMode = ref.OFF
    assert d.max_outputs(500) == 0
    assert d.process(re[:500], im[:500]).size == 0
    assert_same(np.array(d.state(), F32), np.array(before, F32), "state across OFF")
    d.demodulationMode = ref.AM                                # same width: the filter carries on
    assert_same(d.process(re[500:900], im[500:900]), c.process(re[500:900], im[500:900]), "after OFF")
    assert_state(d, c, "after OFF")
    o = make(ref.OFF)
    assert o.process(re[:10], im[:10]).size == 0 and o.channelWidth == 0


def test_reset_equals_a_new_handle(make):
    re, im = noise()
    for mode in (ref.AM, ref.WFM, ref.LSB):
        d, fresh, c = make(mode), make(mode), ref.DemodChain(mode)
        d.process(re[:1500], im[:1500], 400)
        d.reset()
        assert d.state() == (0.0, 0.0, 0.0)
        got = d.process(re[100:1300], im[100:1300], 500)
        assert_same(got, fresh.process(re[100:1300], im[100:1300], 500), NAME[mode] + " reset")
        check(mode, got, c.process(re[100:1300], im[100:1300], 500), c, True, NAME[mode] + " reset")
        assert_state(d, c, "reset")


# ------------------------------------------------------------------ capacity

@pytest.mark.parametrize("mode", [ref.AM, ref.WFM, ref.USB], ids=lambda m: NAME[m])
def test_capacity_one_short_consumes_nothing(rfa, mode):
    import ctypes

    import torch

    from rfanalyzer_amd import _lib, demod
    re, im = noise()
    c = ref.DemodChain(mode)
    with demod.Demodulator(mode) as d:
        d.process(re[:300], im[:300])
        c.process(re[:300], im[:300])
        before = d.state()
        n = 1000
        want = c.process(re[300:300 + n], im[300:300 + n], 256)
        assert d.max_outputs(n) == len(want)
        t_re = torch.from_numpy(re[300:300 + n].copy()).cuda()
        t_im = torch.from_numpy(im[300:300 + n].copy()).cuda()
        out = torch.full((len(want),), 7.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        got = ctypes.c_size_t(99)
        rc = _lib.lib().rfa_demod_process(d._h, t_re.data_ptr(), t_im.data_ptr(), n, 256, out.data_ptr(),
                                          len(want) - 1, ctypes.byref(got))
        assert rc == _lib.RFA_ERR_SIZE and got.value == 0
        assert_same(np.array(d.state(), F32), np.array(before, F32), "state after RFA_ERR_SIZE")
        assert (out.cpu().numpy() == 7.0).all()
        assert d.process_device(t_re.data_ptr(), t_im.data_ptr(), n, out.data_ptr(), len(want), 256) == len(want)
        d.synchronize()
        check(mode, out.cpu().numpy(), want, c, True, NAME[mode] + " after RFA_ERR_SIZE")
        assert_state(d, c, "after RFA_ERR_SIZE")


# ------------------------------------------------------------------ Receiver and torch streams

def _raw_u8(n, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    t = np.arange(n)
    x = 0.4 * np.exp(2j * np.pi * (0.02 * t + 0.002 * np.sin(2 * np.pi * t / 2400.0)))
    x = x + 0.05 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    iq = np.empty(2 * n)
    iq[0::2], iq[1::2] = x.real, x.imag
    return np.clip(np.rint(iq * 128 + 127.4), 0, 255).astype(np.uint8)


@pytest.mark.parametrize("mode", [ref.NFM, ref.USB], ids=lambda m: NAME[m])
def test_receiver_u8_to_audio(rfa, mode):
    from rfanalyzer_amd import demod
    fe = od.ResamplerFrontEnd(od.IN_U8, 2_400_000, ref.MODE_INFO[mode][0])
    c = ref.DemodChain(mode)
    freqs = [(100_000_000, 100_048_000), (100_000_000, 100_048_000), (100_000_000, 99_930_000)]
    with demod.Receiver("u8", 2_400_000, mode) as rx:
        for k, (f, cf) in enumerate(freqs):
            raw = _raw_u8(16384, 20 + k)
            rx.set_frequencies(f, cf)
            fe.set_frequencies(f, cf)
            got = rx.process(raw.tobytes())
            want = c.process(*fe.process(raw))
            assert got.size > 16384 // 60
            check(mode, got, want, c, True, f"Receiver {NAME[mode]} packet {k}")
        assert_state(rx.demod, c, "Receiver")


def test_receiver_mode_change_retunes_the_front_end(rfa):
    from rfanalyzer_amd import demod
    raw = _raw_u8(16384, 31)
    with demod.Receiver("u8", 2_400_000, "nfm") as rx:
        rx.set_frequencies(100_000_000, 100_048_000)
        a = rx.process(raw.tobytes())
        rx.mode = "cw"
        assert rx.front.output_sample_rate == 48000 and rx.demod.channelWidth == 300
        b = rx.process(raw.tobytes())
        assert abs(a.size - 16384 // 50) <= 2 and abs(b.size - 16384 // 50) <= 2   # 48 kHz either way


def test_process_tensor_is_ordered_on_torch_stream(make):
    """process_tensor runs on torch's current stream: a torch op producing the input just
    before, and one reading the output just after, see the right data."""
    import torch
    re, im = noise()
    want, _, c = reference(ref.USB, 1000)
    d = make(ref.USB)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        src_re = torch.from_numpy(re.copy()).to("cuda")
        src_im = torch.from_numpy(im.copy()).to("cuda")
        big = torch.empty(64 << 20, dtype=torch.uint8, device="cuda")
        big.fill_(1)                                        # keeps the stream busy ahead of the copies
        t_re, t_im = torch.empty_like(src_re), torch.empty_like(src_im)
        t_re.copy_(src_re)                                  # producers on the current (side) stream
        t_im.copy_(src_im)
        out = torch.empty(d.max_outputs(TOTAL), dtype=torch.float32, device="cuda")
        n = d.process_tensor(t_re, t_im, out, 1000)
        res = out[:n].clone()                               # consumer on the same stream
    s.synchronize()
    assert_same(res.cpu().numpy(), want, "process_tensor")
