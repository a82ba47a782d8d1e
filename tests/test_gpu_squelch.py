"""GPU: the squelch bank (rfa_squelch_*, demod.SquelchBank), the demodulator bank's hold and the
bank chains built with ``squelch=``.

Levels are compared with tests/squelch_ref.py (float32 terms, their exactly rounded float64 sum,
5 * log10 in double, cast) within one float32 ulp -- the margin covers a double-rounding boundary
of the cast and nothing else: the device's double sum differs from the exact one by at most some
tens of 2^-53 relative, 1e-14 dB, against a float32 ulp of 6e-8 dB or more at the levels used
(every finite level of the inputs is asserted to lie at least 0.1 dB from 0, where float32 is
finer than that).  Sums are compared bit for bit between runs, strides, alignments and bank sizes.
The rule is compared with the restated Kotlin loop on every call, after asserting that every
restated level lies at least 1 dB from its threshold.  Held demodulator slots and gated chains are
compared bit for bit with single handles that were given only the open calls."""
import functools

import numpy as np
import pytest

import slot_sum_plan as plan
import squelch_ref
from rfanalyzer_amd import _lib
from rfanalyzer_amd import demod

pytestmark = pytest.mark.gpu

F32 = np.float32
ONE_LAUNCH = 16384                       # RFA_SQUELCH_ONE_LAUNCH_MAX = RFA_SQUELCH_TILE of include/rfa.h
RAGGED = 3 * ONE_LAUNCH + 777            # four tiles, the last one ragged
LENGTHS = [1, 63, 64, 65, 255, 256, 257, 4095, 4097, ONE_LAUNCH - 1, ONE_LAUNCH, ONE_LAUNCH + 1, RAGGED]
AMPLITUDES = [1e-4, 3e-3, 1.0, 0.0, 0.1]                       # K = 5; row 3 is all zero
NAN_ROW, INF_ROW = 1, 4


def same(got, want, what=""):
    got, want = np.ascontiguousarray(got, F32), np.ascontiguousarray(want, F32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.nonzero(got.view(np.int32) != want.view(np.int32))[0]
    assert bad.size == 0, (what, bad.size, bad[:5], got[bad[:5]], want[bad[:5]])


@functools.lru_cache(maxsize=None)
def rows(n, special=False):
    """[5, n] uniform noise of the five amplitudes; ``special``: one NaN in row 1, one +inf in row 4."""
    rng = np.random.Generator(np.random.PCG64(7000 + n))
    re = np.stack([(a * rng.uniform(-1, 1, n)).astype(F32) for a in AMPLITUDES])
    im = np.stack([(a * rng.uniform(-1, 1, n)).astype(F32) for a in AMPLITUDES])
    if special:
        im[NAN_ROW, n // 2] = np.nan
        re[INF_ROW, n - 1] = np.inf
    re.setflags(write=False)
    im.setflags(write=False)
    return re, im


@functools.lru_cache(maxsize=None)
def ref_levels(n, special=False):
    re, im = rows(n, special)
    return tuple(squelch_ref.level(re[k], im[k]) for k in range(len(AMPLITUDES)))


@functools.lru_cache(maxsize=None)
def ref_sums(n):
    re, im = rows(n)
    return tuple(squelch_ref.exact_sum(re[k], im[k]) for k in range(len(AMPLITUDES)))


def check_levels(got, want, what):
    for k, (g, w) in enumerate(zip(got, want)):
        if np.isfinite(w):
            assert abs(float(w)) >= 0.1, (what, k, w)             # a condition on the inputs (module docstring)
        assert squelch_ref.within_one_ulp(g, w), (what, k, g, w)
        if not np.isfinite(w):
            assert str(F32(g)) == str(F32(w)), (what, k, g, w)    # -inf, nan, inf exactly


@pytest.fixture
def bank(rfa):
    made = []

    def _bank(k):
        b = demod.SquelchBank(k)
        made.append(b)
        return b

    yield _bank
    for b in made:
        b.close()


def dev(x):
    import torch
    return torch.from_numpy(np.array(x, order="C")).cuda()           # a copy: the cached inputs are read-only


# ------------------------------------------------------------------ levels

@pytest.mark.parametrize("n", LENGTHS)
def test_levels_equal_the_restatement(bank, n):
    sq = bank(5)
    re, im = rows(n)
    levels, opn = sq.process(re, im)
    assert levels.dtype == F32 and opn.dtype == bool and opn.all()      # no threshold: always open
    check_levels(levels, ref_levels(n), f"n {n}")
    assert levels[3] == -np.inf
    st = sq.state()
    for k, want in enumerate(ref_sums(n)):                               # the double sum itself
        assert abs(st["sums"][k] - want) <= 1e-13 * want, (n, k, st["sums"][k], want)
    same(st["levels"], levels)
    # one NaN and one +inf
    levels, _ = sq.process(*rows(n, True))
    check_levels(levels, ref_levels(n, True), f"n {n}, special")
    assert np.isnan(levels[NAN_ROW]) and levels[INF_ROW] == np.inf and levels[3] == -np.inf
    # device rows give the same sums as host rows
    sums = sq.state()["sums"]
    sq.process_tensor(dev(rows(n, True)[0]), dev(rows(n, True)[1]))
    np.testing.assert_array_equal(sq.state()["sums"].view(np.int64), sums.view(np.int64))


@pytest.mark.parametrize("n", [257, 4097, ONE_LAUNCH, ONE_LAUNCH + 1, RAGGED])
def test_sums_do_not_move_with_run_stride_alignment_or_bank_size(bank, n):
    import torch
    re, im = rows(n)
    sq = bank(5)
    sq.process_tensor(dev(re), dev(im))
    base = sq.state()["sums"].copy()
    bits = lambda s: np.asarray(s, np.float64).view(np.int64)            # noqa: E731
    # run to run
    sq.process_tensor(dev(re), dev(im))
    np.testing.assert_array_equal(bits(sq.state()["sums"]), bits(base))
    # channel_stride n + 7
    wide_re = torch.zeros((5, n + 7), dtype=torch.float32, device="cuda")
    wide_im = torch.zeros_like(wide_re)
    wide_re[:, :n] = dev(re)
    wide_im[:, :n] = dev(im)
    sq.process_tensor(wide_re[:, :n], wide_im[:, :n])
    np.testing.assert_array_equal(bits(sq.state()["sums"]), bits(base))
    # rows that start 1, 2 and 3 floats off a 16-byte boundary
    stride = n + 8 - n % 8                                               # a multiple of 8 floats: every row alike
    for off in (1, 2, 3):
        flat_re = torch.zeros(5 * stride + 8, dtype=torch.float32, device="cuda")
        flat_im = torch.zeros_like(flat_re)
        assert flat_re.data_ptr() % 16 == 0 and flat_im.data_ptr() % 16 == 0
        for k in range(5):
            flat_re[off + k * stride:off + k * stride + n] = dev(re[k])
            flat_im[off + k * stride:off + k * stride + n] = dev(im[k])
        torch.cuda.synchronize()
        sq.process_device(flat_re.data_ptr() + 4 * off, flat_im.data_ptr() + 4 * off, stride, n)
        np.testing.assert_array_equal(bits(sq.state()["sums"]), bits(base), f"offset {off}")
    # the same row in banks of 1, 5 and 300 slots
    for k_count, slot in ((1, 0), (300, 299), (300, 150)):
        other = bank(k_count)
        big_re = np.zeros((k_count, n), F32)
        big_im = np.zeros((k_count, n), F32)
        big_re[slot], big_im[slot] = re[2], im[2]
        other.process(big_re, big_im)
        s = other.state()["sums"]
        assert bits(s[slot:slot + 1])[0] == bits(base[2:3])[0], (k_count, slot)
        assert not s[np.arange(k_count) != slot].any()


assert plan.POWER_LENGTHS == LENGTHS + plan.LONG


@pytest.mark.parametrize("n", plan.POWER_LENGTHS)
def test_sums_equal_the_summation_plan_bit_for_bit(bank, n):
    """The order of every addition (tests/slot_sum_plan.py), on finite rows of which two are enveloped;
    the long lengths reach the tile fold's second fetch."""
    sq = bank(plan.K)
    sq.process(*plan.pin_rows(n))
    np.testing.assert_array_equal(sq.state()["sums"].view(np.int64), plan.power_sums(n).view(np.int64))


def test_sums_of_strided_unaligned_rows_equal_the_summation_plan(bank):
    import torch
    n = RAGGED
    re, im = plan.pin_rows(n)
    stride = (n // 4 + 2) * 4                                            # beyond n, and every row starts alike
    wide_re = torch.zeros((plan.K, stride), dtype=torch.float32, device="cuda")
    wide_im = torch.zeros_like(wide_re)
    wide_re[:, 1:n + 1] = dev(re)
    wide_im[:, 1:n + 1] = dev(im)
    for k in range(plan.K):
        assert wide_re[k, 1:].data_ptr() % 16 == 4 and wide_im[k, 1:].data_ptr() % 16 == 4
    sq = bank(plan.K)
    sq.process_tensor(wide_re[:, 1:n + 1], wide_im[:, 1:n + 1])
    np.testing.assert_array_equal(sq.state()["sums"].view(np.int64), plan.power_sums(n).view(np.int64))


def test_1024_slots(bank):
    n = 300
    re, im = rows(n)
    sq = bank(5)
    sq.process(re, im)
    base = sq.state()["sums"]
    big = bank(1024)
    idx = np.arange(1024) % 5
    levels, opn = big.process(re[idx], im[idx])
    np.testing.assert_array_equal(big.state()["sums"].view(np.int64), base[idx].view(np.int64))
    check_levels(levels[:5], ref_levels(n), "1024 slots")
    assert opn.all()
    with pytest.raises(_lib.RfaError) as e:
        demod.SquelchBank(1025)
    assert e.value.status == _lib.RFA_ERR_INVALID


def test_no_samples_keep_the_level_and_step_the_rule(bank):
    sq = bank(5)
    sq.debounce = 2
    for k in range(5):
        sq.set(k, -3.0)
    assert sq.get(0) == -3.0 and sq.debounce == 2
    empty = np.zeros((5, 0), F32)
    levels, opn = sq.process(empty, empty)                    # before any sample: the initial level
    assert (levels == F32(-999.0)).all() and opn.all()
    assert list(sq.state()["counters"]) == [1] * 5
    sq.reset()
    n = 257
    levels, opn = sq.process(*rows(n))
    want_open = [False, False, True, False, False]            # only amplitude 1 is above -3 dB
    assert [lv > -3.0 for lv in ref_levels(n)] == want_open
    assert list(opn) == [True] * 5                            # the first unsatisfied call: 1 < 2
    kept, opn = sq.process(empty, empty)
    same(kept, levels, "levels of an empty call")
    assert list(opn) == want_open
    assert list(sq.state()["counters"]) == [2, 2, 0, 2, 2]
    sq.set(0, None)
    assert sq.get(0) is None
    kept, opn = sq.process_device(0, 0, 0, 0)
    same(kept, levels)
    assert list(opn) == [True] + want_open[1:]
    # errors change nothing
    with pytest.raises(_lib.RfaError):
        sq.process_device(0, 0, 300, 257)                      # null rows with samples
    x = dev(rows(n)[0])
    with pytest.raises(_lib.RfaError):
        sq.process_device(x.data_ptr(), x.data_ptr(), n - 1, n)   # rows that overlap
    assert list(sq.state()["counters"]) == [0, 2, 0, 2, 2]
    same(sq.state()["levels"], levels)
    sq.reset()
    st = sq.state()
    assert (st["levels"] == F32(-999.0)).all() and not st["counters"].any()


# ------------------------------------------------------------------ the rule on the device's levels

THRESHOLDS = [-30.0, -50.0, None, -30.0]
HIGH, LOW = 0.1, 1e-6                     # tones of these amplitudes read -10 dB and -60 dB
CALLS = 70


def _amplitude(call, slot):
    if slot == 0:                         # closes after the debounce, reopens at 60
        return HIGH if call < 5 or call >= 60 else LOW
    if slot == 1:                         # a short gap that a debounce of 3 closes, then a long one
        return HIGH if call < 2 or 10 <= call < 13 else LOW
    if slot == 2:                         # no squelch: open whatever the level
        return LOW
    return HIGH if 55 <= call < 58 else LOW   # unsatisfied from creation


@functools.lru_cache(maxsize=None)
def rule_inputs():
    n = 655
    ph = 2 * np.pi * 0.013 * np.arange(n)
    out = []
    for call in range(CALLS):
        amp = np.array([_amplitude(call, k) for k in range(4)])[:, None]
        out.append(((amp * np.cos(ph + call)).astype(F32), (amp * np.sin(ph + call)).astype(F32)))
    return out


@pytest.mark.parametrize("debounce", [50, 3])
def test_rule_on_the_devices_levels(bank, debounce):
    sq = bank(4)
    sq.debounce = debounce
    gates = [squelch_ref.Gate(t, debounce) for t in THRESHOLDS]
    for k, t in enumerate(THRESHOLDS):
        sq.set(k, t)
    history = []
    for call, (re, im) in enumerate(rule_inputs()):
        want_open = [g.feed(re[k], im[k]) for k, g in enumerate(gates)]
        for k, g in enumerate(gates):                          # a condition on the inputs
            assert g.threshold is None or abs(float(g.level) - g.threshold) >= 1.0, (call, k, g.level)
        levels, opn = sq.process(re, im)
        for k, g in enumerate(gates):
            assert squelch_ref.within_one_ulp(levels[k], g.level), (call, k, levels[k], g.level)
        st = sq.state()
        assert list(opn) == want_open == list(st["open"]), (call, list(opn), want_open)
        assert list(st["counters"]) == [g.counter for g in gates], call
        history.append(want_open)
    h = np.array(history)
    assert h[:, 2].all()                                       # the slot without squelch never closes
    assert not h[:, 0].all() and h[60:, 0].all()               # slot 0 closed and reopened
    assert list(h[:, 3]) == [c < debounce - 1 or 55 <= c < 57 + debounce for c in range(CALLS)]


# ------------------------------------------------------------------ hold

HOLD_MODES = ["am", "nfm", "usb", "cw", "lsb"]
HOLD_SIZES = [4096, 4096, 1, 4096, 4096, 5, 4096, 4096, 0, 4096, 4096, 160, 4096, 4096, 4096, 4096]
SENTINEL = 7.0
USB_WIDTH = 2000


def _held(call, slot):
    if slot == 0:
        return call % 3 == 1
    if slot == 1:
        return True                                   # held throughout
    if slot == 2:
        return 3 <= call < 7                          # its width changes at call 4, while held
    if slot == 3:
        return call < 2 or 9 <= call < 11             # held from creation: no filter before call 2
    return 5 <= call < 8                              # slot 4 is also "off" from call 5 to call 9


@functools.lru_cache(maxsize=None)
def hold_inputs(k_count, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    n = sum(HOLD_SIZES)
    re = (0.3 * rng.standard_normal((k_count, n))).astype(F32)
    im = (0.3 * rng.standard_normal((k_count, n))).astype(F32)
    return re, im


def _compare_slot(b, k, h, what):
    assert b.mode(k) == h.demodulationMode and b.channel_width(k) == h.channelWidth, what
    same(np.array(b.state(k), F32), np.array(h.state(), F32), f"{what} state")
    for which in demod.TAPS:
        b_re, b_im, b_dec = b.taps(k, which)
        h_re, h_im, h_dec = h.taps(which)
        assert b_dec == h_dec, (what, which)
        same(b_re, h_re, f"{what} {which} taps")
        same(b_im, h_im, f"{what} {which} taps (im)")


def _run_hold(modes, held, events, seed):
    """The bank with holds against one Demodulator per slot that gets only its slot's non-held
    calls; ``events(call, set_mode, set_width)`` applies the same setting changes to both."""
    import torch
    K = len(modes)
    re, im = hold_inputs(K, seed)
    b = demod.DemodulatorBank(modes)
    hs = [demod.Demodulator(m) for m in modes]
    try:
        assert not any(b.hold(k) for k in range(K))
        cap = max(HOLD_SIZES) + 16                    # no slot writes more audio than it was given samples, plus a carry
        now = [False] * K
        pos = 0
        for call, n in enumerate(HOLD_SIZES):
            events(call, lambda k, m: (b.set_mode(k, m), setattr(hs[k], "demodulationMode", m)),
                   lambda k, w: (b.set_channel_width(k, w), setattr(hs[k], "channelWidth", w)))
            for k in range(K):
                if held(call, k) != now[k]:
                    now[k] = held(call, k)
                    b.set_hold(k, now[k])
                assert b.hold(k) == now[k]
            counts = b.max_outputs(n)
            out = torch.full((K, cap + 3), SENTINEL, dtype=torch.float32, device="cuda")
            d_re, d_im = dev(re[:, pos:pos + n]), dev(im[:, pos:pos + n])
            got = b.process_tensor(d_re, d_im, out[:, :cap], 1000)
            b.synchronize()
            audio = out.cpu().numpy()
            assert got == counts
            for k in range(K):
                what = f"call {call} ({n}) slot {k}"
                if now[k]:
                    assert got[k] == 0 and (audio[k] == SENTINEL).all(), what
                else:
                    want = hs[k].process(re[k, pos:pos + n], im[k, pos:pos + n], 1000)
                    assert got[k] == want.size, what
                    same(audio[k, :got[k]], want, what)
                    assert (audio[k, got[k]:] == SENTINEL).all(), what
                _compare_slot(b, k, hs[k], what)
            pos += n
    finally:
        b.close()
        for h in hs:
            h.close()


def test_held_slots_equal_demodulators_given_only_their_open_calls(rfa):
    with demod.Demodulator("usb") as h:
        assert h.channelWidth != USB_WIDTH                     # the change at call 4 is a change
        h.channelWidth = USB_WIDTH
        assert h.channelWidth == USB_WIDTH                     # and inside the mode's limits

    def events(call, set_mode, set_width):
        if call == 4:
            set_width(2, USB_WIDTH)         # on a held slot: designed at its first open call (7)
        if call == 5:
            set_mode(4, "off")              # off and held
        if call == 10:
            set_mode(4, "lsb")

    _run_hold(HOLD_MODES, _held, events, 11)


def test_held_wfm_slots(rfa):
    _run_hold(["wfm", "wfm"], lambda call, k: k == 0 and call % 2 == 0, lambda *a: None, 12)


def test_a_bank_of_one_held_slot_and_the_slot_checks(rfa):
    with demod.DemodulatorBank(["nfm"]) as b:
        b.set_hold(0, True)
        assert b.max_outputs(4096) == [0]
        re, im = hold_inputs(1, 13)
        assert [a.size for a in b.process(re[:, :4096], im[:, :4096])] == [0]
        assert b.taps(0, "user")[0].size == 0                  # no call ever built its filter
        b.set_hold(0, False)
        with demod.Demodulator("nfm") as h:
            same(b.process(re[:, :4096], im[:, :4096])[0], h.process(re[0, :4096], im[0, :4096]))
        for k in (-1, 1):
            with pytest.raises(_lib.RfaError) as e:
                b.set_hold(k, True)
            assert e.value.status == _lib.RFA_ERR_INVALID
            with pytest.raises(_lib.RfaError):
                b.hold(k)


# ------------------------------------------------------------------ chains

FS, SPACING, PACKET, PACKETS = 2_400_000, 25_000, 16_384, 70
CENTER = 100_000_000
RASTER = [5, 17, 40, 90]                                  # raster channels of the four slots
OFFSETS = [(c if c < 48 else c - 96) * SPACING for c in RASTER]
CARRIER, NOISE = 0.3, 0.02                                # a carrier reads about -5 dB, the noise about -24 dB
CHAIN_THRESHOLDS = [-8.5, -8.5, -8.5, None]              # slot 2 never has a carrier, slot 3 no squelch


def _carrier_on(packet, slot):
    if slot == 0:
        return packet < 10 or 20 <= packet < 25
    if slot == 1:
        return packet < 5 or packet >= 63
    return False


@functools.lru_cache(maxsize=None)
def chain_packets():
    """70 u8 packets: bursting carriers on the channels of slots 0 and 1 over Gaussian noise."""
    rng = np.random.Generator(np.random.PCG64(4242))
    out = []
    for p in range(PACKETS):
        t = p * PACKET + np.arange(PACKET)
        x = NOISE * (rng.standard_normal(PACKET) + 1j * rng.standard_normal(PACKET))
        for k in (0, 1):
            if _carrier_on(p, k):
                x = x + CARRIER * np.exp(2j * np.pi * OFFSETS[k] / FS * t)
        iq = np.empty(2 * PACKET)
        iq[0::2], iq[1::2] = x.real, x.imag
        out.append(np.clip(np.rint(iq * 128 + 127.4), 0, 255).astype(np.uint8))
    return out


def _receiver_bank(squelch):
    rx = demod.ReceiverBank("u8", FS, ["nfm"] * 4, squelch=squelch)
    rx.set_frequencies(CENTER, [CENTER + o for o in OFFSETS])
    return rx


def _receiver_front(rx):
    fe = demod.FrontEndBank("u8", FS, rx.quadrature_rate, 4, resampler=True)
    fe.set_frequencies(CENTER, [CENTER + o for o in OFFSETS])
    return fe


def _raster_bank(squelch):
    return demod.RasterReceiverBank("u8", FS, SPACING, ["nfm"] * 4, channels=RASTER, squelch=squelch)


def _raster_front(rx):
    fe = demod.Channelizer.for_raster("u8", FS, SPACING, rx.quadrature_rate)
    fe.set_channels(RASTER)
    return fe


def _planar(out):
    """A front end's host output as (re[4, n], im[4, n]): FrontEndBank gives the pair, Channelizer
    one complex64 array per channel."""
    if isinstance(out, tuple):
        return np.ascontiguousarray(out[0], F32), np.ascontiguousarray(out[1], F32)
    z = np.stack(out)
    return np.ascontiguousarray(z.real, F32), np.ascontiguousarray(z.imag, F32)


CHAINS = {"receiver": (_receiver_bank, _receiver_front), "raster": (_raster_bank, _raster_front)}


def _run_chain(make, debounce, switch_stream_at=None):
    """Every packet through a chain built with the thresholds: (gates, levels, audio) per packet."""
    import torch
    gates, levels, audio = [], [], []
    side = torch.cuda.Stream()
    with make(CHAIN_THRESHOLDS) as rx:
        assert isinstance(rx.squelch, demod.SquelchBank)
        if debounce is not None:
            rx.squelch_debounce = debounce
        assert rx.squelch_debounce == (50 if debounce is None else debounce)
        for p, raw in enumerate(chain_packets()):
            if p == switch_stream_at:
                rx.set_stream(side.cuda_stream)
                assert rx.squelch.stream == rx.front.stream == rx.demods.stream == side.cuda_stream
            got = rx.process(raw)
            gates.append(rx.open.copy())
            levels.append(rx.levels.copy())
            audio.append(got)
            assert [g.size > 0 for g in got] == list(rx.open), p        # a closed slot returns nothing
    return gates, levels, audio


def _check_chain(name, debounce):
    make, make_front = CHAINS[name]
    gates, levels, audio = _run_chain(make, debounce)
    d = 50 if debounce is None else debounce
    # the chain's own front-end output, from a second front end without squelch on the same stream
    ref_gates = [squelch_ref.Gate(t, d) for t in CHAIN_THRESHOLDS]
    banks = [demod.DemodulatorBank(["nfm"]) for _ in range(4)]
    single = demod.Demodulator("nfm")
    want_audio = [[] for _ in range(4)]
    single_audio = []
    with make(None) as plain:
        assert plain.squelch is None and plain.levels is None and plain.open is None     # no squelch handle
        with pytest.raises(ValueError):
            plain.set_squelch(0, -10.0)
        fe = make_front(plain)
        try:
            fe.set_stream(plain.demods.stream)
            for p, raw in enumerate(chain_packets()):
                re, im = _planar(fe.process(raw))
                assert re.shape == im.shape and re.shape[0] == 4
                want_open = [g.feed(re[k], im[k]) for k, g in enumerate(ref_gates)]
                for k, g in enumerate(ref_gates):                  # a condition on the inputs
                    assert g.threshold is None or abs(float(g.level) - g.threshold) >= 1.0, (p, k, g.level)
                    assert squelch_ref.within_one_ulp(levels[p][k], g.level), (p, k, levels[p][k], g.level)
                    if k < 2:                                      # the carriers are where the slots listen
                        assert (g.level > g.threshold) == _carrier_on(p, k), (p, k, g.level)
                assert list(gates[p]) == want_open, (p, list(gates[p]), want_open)
                for k in range(4):
                    if want_open[k]:
                        want_audio[k].append(banks[k].process(re[k:k + 1], im[k:k + 1])[0])
                if want_open[1]:
                    single_audio.append(single.process(re[1], im[1]))
        finally:
            fe.close()
            single.close()
            for b in banks:
                b.close()
    g = np.array(gates)
    assert g[:, 3].all() and not g[:, 2].all()                 # no squelch: open; never a carrier: closes
    for k in range(4):
        got = np.concatenate([a[k] for a in audio])
        same(got, np.concatenate(want_audio[k]), f"{name} slot {k}")
    same(np.concatenate([a[1] for a in audio]), np.concatenate(single_audio), f"{name} slot 1 against a Demodulator")
    return g, audio


@pytest.mark.parametrize("name", ["receiver", "raster"])
def test_chain_gates_and_audio_debounce_3(rfa, name):
    g, _ = _check_chain(name, 3)
    assert not g[12:20, 0].any() and g[20:27, 0].all() and not g[27:, 0].any()    # closes two packets after a burst
    assert not g[7:63, 1].any() and g[63:, 1].all()
    assert list(g[:, 2]) == [p < 2 for p in range(PACKETS)]


def test_chain_gates_and_audio_default_debounce(rfa):
    g, _ = _check_chain("receiver", None)
    assert g[:, 0].all()                                       # 49 packets past its last burst: beyond packet 70
    assert g[:54, 1].all() and not g[54:63, 1].any() and g[63:, 1].all()
    assert list(g[:, 2]) == [p < 49 for p in range(PACKETS)]


def test_chain_set_stream_then_a_call_gives_the_same_audio(rfa):
    _, _, first = _run_chain(_receiver_bank, 3)
    _, _, second = _run_chain(_receiver_bank, 3, switch_stream_at=8)
    for p, (a, b) in enumerate(zip(first, second)):
        for k in range(4):
            same(a[k], b[k], f"packet {p} slot {k}")


def test_chain_squelch_true_and_set_squelch(rfa):
    with _receiver_bank(True) as rx:
        assert rx.squelch is not None and [rx.squelch.get(k) for k in range(4)] == [None] * 4
        rx.squelch_debounce = 1
        got = rx.process(chain_packets()[0])
        assert rx.open.all() and all(a.size > 0 for a in got)
        rx.set_squelch(2, -8.5)
        got = rx.process(chain_packets()[1])
        assert list(rx.open) == [True, True, False, True] and got[2].size == 0
        assert rx.demods.hold(2) and not rx.demods.hold(0)
        rx.set_squelch(2, None)
        got = rx.process(chain_packets()[2])
        assert rx.open.all() and got[2].size > 0 and not rx.demods.hold(2)
    with pytest.raises(ValueError):
        _receiver_bank([-8.5] * 3)
