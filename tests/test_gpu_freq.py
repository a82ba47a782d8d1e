"""GPU: the frequency meter bank (rfa_freq_*, demod.FrequencyMeterBank) and the bank chains built
with ``afc=``.

The reference has nothing to compare with; the checks are tests/freq_ref.py and derived bounds.
Sums: each within (terms + 2) * 2^-53 * sum(|p1| + |p2|) of the exactly summed once-rounded terms
(one rounding per term, one per addition).  Invariance, the carry and the non-finite rows are
compared bit for bit.  Chains: the corrections the rule must reach are first confirmed on the CPU
with restated front ends (every estimate within 5 Hz of the carrier's true offset, which is less
than the 7.5 Hz that separate each offset from the next rounding boundary of the 25 Hz step), then
asserted on the device together with bit-identical audio from a chain without AFC that is given
the same ``set_frequencies`` calls between the same packets."""
import functools

import numpy as np
import pytest

import freq_ref
import pfb_ref
import pfb_tuning_ref as tref
import slot_sum_plan as plan
from oracle import demod as odemod
from rfanalyzer_amd import _lib
from rfanalyzer_amd import demod

pytestmark = pytest.mark.gpu

F32 = np.float32
TILE = freq_ref.TILE
LENGTHS = [0, 1, 2, 63, 64, 65, 257, 4097, TILE, TILE + 1, 2 * TILE + 1, 40000]
AMPLITUDES = [1.0, 1e-3, 0.3]                              # K = 3


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.int64)


def same_bits(got, want, what=""):
    for name, g, w in zip(("re", "im"), got[:2], want[:2]):
        np.testing.assert_array_equal(bits(g), bits(w), f"{what} {name}")
    np.testing.assert_array_equal(got[2], want[2], f"{what} terms")


@functools.lru_cache(maxsize=None)
def rows(n, seed=0):
    """[3, n] rows: a drifting tone plus uniform noise, scaled by the three amplitudes."""
    rng = np.random.Generator(np.random.PCG64(9100 + n + 7919 * seed))
    ph = 2 * np.pi * (0.013 * np.arange(n) + 1e-7 * np.arange(n) ** 2)
    re = np.stack([(a * (0.6 * np.cos(ph + k) + 0.4 * rng.uniform(-1, 1, n))).astype(F32)
                   for k, a in enumerate(AMPLITUDES)])
    im = np.stack([(a * (0.6 * np.sin(ph + k) + 0.4 * rng.uniform(-1, 1, n))).astype(F32)
                   for k, a in enumerate(AMPLITUDES)])
    re.setflags(write=False)
    im.setflags(write=False)
    return re, im


@functools.lru_cache(maxsize=None)
def ref(n, carried, seed=0):
    """freq_ref.r1 per slot of rows(n): without a carry, or with the row's own last sample as one."""
    re, im = rows(n, seed)
    return tuple(freq_ref.r1(re[k], im[k], (re[k, -1], im[k, -1]) if carried else None) for k in range(3))


def check_sums(got, want, what):
    g_re, g_im, g_terms = got
    for k, (w_re, w_im, terms, b_re, b_im) in enumerate(want):
        print(f"{what} slot {k}: terms {terms}, |d re| {abs(g_re[k] - w_re):.3e} (bound {b_re:.3e}), "
              f"|d im| {abs(g_im[k] - w_im):.3e} (bound {b_im:.3e})")
        assert g_terms[k] == terms, (what, k, g_terms[k], terms)
        assert abs(g_re[k] - w_re) <= b_re, (what, k, g_re[k], w_re, b_re)
        assert abs(g_im[k] - w_im) <= b_im, (what, k, g_im[k], w_im, b_im)


@pytest.fixture
def bank(rfa):
    made = []

    def _bank(k):
        b = demod.FrequencyMeterBank(k)
        made.append(b)
        return b

    yield _bank
    for b in made:
        b.close()


def dev(x):
    import torch
    return torch.from_numpy(np.array(x, order="C")).cuda()           # a copy: the cached inputs are read-only


# ------------------------------------------------------------------ sums

@pytest.mark.parametrize("n", LENGTHS)
def test_sums_equal_the_restatement(bank, n):
    fm = bank(3)
    re, im = rows(n)
    got = fm.process(re, im)
    assert got[0].dtype == np.float64 and got[2].dtype == np.int64
    if n == 0:
        for call in range(2):
            assert not got[0].any() and not got[1].any() and not got[2].any()
            got = fm.process(re, im)
        return
    check_sums(got, ref(n, False), f"n {n}, no carry")
    assert list(got[2]) == [n - 1] * 3
    # the same rows again: the predecessor of sample 0 is the last sample of the call before
    got = fm.process(re, im)
    check_sums(got, ref(n, True), f"n {n}, carried")
    assert list(got[2]) == [n] * 3
    same_bits(fm.collect(), got, "collect repeats the last call")
    # device rows give the same sums as host rows
    fm.break_()
    same_bits(fm.process_tensor(dev(re), dev(im)), fm_fresh(bank, re, im), f"n {n} device rows")


def fm_fresh(bank, re, im):
    return bank(re.shape[0]).process(re, im)


@pytest.mark.parametrize("n", [257, 4097, TILE + 1, 40000])
def test_sums_do_not_move_with_run_stride_alignment_or_bank_size(bank, n):
    import torch
    re, im = rows(n)
    fm = bank(3)
    base = fm.process_tensor(dev(re), dev(im))
    # run to run
    fm.reset()
    same_bits(fm.process_tensor(dev(re), dev(im)), base, "second run")
    # channel_stride n + 7
    wide_re = torch.zeros((3, n + 7), dtype=torch.float32, device="cuda")
    wide_im = torch.zeros_like(wide_re)
    wide_re[:, :n] = dev(re)
    wide_im[:, :n] = dev(im)
    fm.reset()
    same_bits(fm.process_tensor(wide_re[:, :n], wide_im[:, :n]), base, "stride n + 7")
    # rows that start 1, 2 and 3 floats off a 16-byte boundary
    stride = n + 8 - n % 8                                               # a multiple of 8 floats: every row alike
    for off in (1, 2, 3):
        flat_re = torch.zeros(3 * stride + 8, dtype=torch.float32, device="cuda")
        flat_im = torch.zeros_like(flat_re)
        assert flat_re.data_ptr() % 16 == 0 and flat_im.data_ptr() % 16 == 0
        for k in range(3):
            flat_re[off + k * stride:off + k * stride + n] = dev(re[k])
            flat_im[off + k * stride:off + k * stride + n] = dev(im[k])
        torch.cuda.synchronize()
        fm.reset()
        fm.process_device(flat_re.data_ptr() + 4 * off, flat_im.data_ptr() + 4 * off, stride, n)
        same_bits(fm.collect(), base, f"offset {off}")
    # the same row in banks of 1 and 300 slots
    for k_count, slot in ((1, 0), (300, 299), (300, 150)):
        other = bank(k_count)
        big_re = np.zeros((k_count, n), F32)
        big_im = np.zeros((k_count, n), F32)
        big_re[slot], big_im[slot] = re[2], im[2]
        s_re, s_im, terms = other.process(big_re, big_im)
        assert (bits(s_re[slot]), bits(s_im[slot])) == (bits(base[0][2]), bits(base[1][2])), (k_count, slot)
        others = np.arange(k_count) != slot
        assert not s_re[others].any() and not s_im[others].any() and (terms == n - 1).all()


assert plan.R1_LENGTHS == LENGTHS + plan.LONG


def same_as_plan(got, n, carried, what):
    want_re, want_im = plan.r1_sums(n, carried)
    np.testing.assert_array_equal(bits(got[0]), bits(want_re), f"{what} re")
    np.testing.assert_array_equal(bits(got[1]), bits(want_im), f"{what} im")
    assert list(got[2]) == [n if carried else max(n - 1, 0)] * plan.K, what


@pytest.mark.parametrize("n", plan.R1_LENGTHS)
def test_sums_equal_the_summation_plan_bit_for_bit(bank, n):
    """The order of every addition (tests/slot_sum_plan.py), on finite rows of which two are enveloped,
    without a carry and with the previous call's last sample; the long lengths reach the tile fold's
    second fetch."""
    fm = bank(plan.K)
    re, im = plan.pin_rows(n)
    same_as_plan(fm.process(re, im), n, False, f"n {n}, no carry")
    same_as_plan(fm.process(re, im), n, n > 0, f"n {n}, carried")


def test_sums_of_strided_unaligned_rows_equal_the_summation_plan(bank):
    import torch
    n = 40000
    re, im = plan.pin_rows(n)
    stride = (n // 4 + 2) * 4                                            # beyond n, and every row starts alike
    wide_re = torch.zeros((plan.K, stride), dtype=torch.float32, device="cuda")
    wide_im = torch.zeros_like(wide_re)
    wide_re[:, 1:n + 1] = dev(re)
    wide_im[:, 1:n + 1] = dev(im)
    for k in range(plan.K):
        assert wide_re[k, 1:].data_ptr() % 16 == 4 and wide_im[k, 1:].data_ptr() % 16 == 4
    fm = bank(plan.K)
    same_as_plan(fm.process_tensor(wide_re[:, 1:n + 1], wide_im[:, 1:n + 1]), n, False, "no carry")
    same_as_plan(fm.process_tensor(wide_re[:, 1:n + 1], wide_im[:, 1:n + 1]), n, True, "carried")


def test_1024_slots(bank):
    n = 300
    re, im = rows(n)
    base = bank(3).process(re, im)
    big = bank(1024)
    idx = np.arange(1024) % 3
    got = big.process(re[idx], im[idx])
    same_bits(got, (base[0][idx], base[1][idx], base[2][idx]), "1024 slots")
    with pytest.raises(_lib.RfaError) as e:
        demod.FrequencyMeterBank(1025)
    assert e.value.status == _lib.RFA_ERR_INVALID


def test_argument_errors_of_a_live_handle_change_nothing(bank):
    fm = bank(3)
    re, im = rows(257)
    first = fm.process(re, im)
    x = dev(re)
    for args in ((0, 0, 300, 257), (x.data_ptr(), 0, 300, 257), (x.data_ptr(), x.data_ptr(), 256, 257)):
        with pytest.raises(_lib.RfaError) as e:
            fm.process_device(*args)                          # null rows with samples; rows that overlap
        assert e.value.status == _lib.RFA_ERR_INVALID
    for k in (-2, 3):
        with pytest.raises(_lib.RfaError):
            fm.break_(k)
    same_bits(fm.collect(), first, "after the errors")
    got = fm.process(re, im)
    assert list(got[2]) == [257] * 3                          # the carry is still there
    check_sums(got, ref(257, True), "after the errors")
    with pytest.raises(ValueError):
        fm.process(re[:2], im[:2])


# ------------------------------------------------------------------ the carry

PAIRS = [(300, 300), (TILE + 1, 5), (5, TILE + 1), (20000, 20000)]      # either side of one launch / two launches
REPEATS = 8


@pytest.mark.parametrize("na,nb", PAIRS)
def test_carry_across_calls(bank, na, nb):
    re, im = rows(na + nb, seed=1)
    a = (dev(re[:, :na]), dev(im[:, :na]))
    b = (dev(re[:, na:]), dev(im[:, na:]))
    empty = (dev(re[:, :0]), dev(im[:, :0]))
    want = tuple(freq_ref.r1(re[k, na:], im[k, na:], (re[k, na - 1], im[k, na - 1])) for k in range(3))
    fm = bank(3)
    first = None
    for rep in range(REPEATS):                                # a misplaced carry write would show as a difference
        fm.reset()
        got_a = fm.process_tensor(*a)
        assert list(got_a[2]) == [na - 1] * 3
        got = fm.process_tensor(*b)
        if first is None:
            first = got
            check_sums(got, want, f"{na}+{nb}")
            assert list(got[2]) == [nb] * 3
        same_bits(got, first, f"{na}+{nb} repeat {rep}")
    fresh = bank(3).process_tensor(*b)                        # no predecessor at all
    assert list(fresh[2]) == [nb - 1] * 3
    # break_(1): slot 1 starts again, the others keep their predecessor
    fm.reset()
    fm.process_tensor(*a)
    fm.break_(1)
    got = fm.process_tensor(*b)
    assert list(got[2]) == [nb, nb - 1, nb]
    for k in range(3):
        w = fresh if k == 1 else first
        assert (bits(got[0][k]), bits(got[1][k])) == (bits(w[0][k]), bits(w[1][k])), k
    # reset: every slot starts again
    fm.reset()
    got = fm.collect()
    assert not got[0].any() and not got[1].any() and not got[2].any()
    fm.process_tensor(*a)
    fm.reset()
    same_bits(fm.process_tensor(*b), fresh, "after reset")
    # a call of no samples launches nothing, reads zero and keeps the carry
    fm.reset()
    fm.process_tensor(*a)
    got = fm.process_tensor(*empty)
    assert not got[0].any() and not got[1].any() and not got[2].any()
    same_bits(fm.process_tensor(*b), first, "after an empty call")


# ------------------------------------------------------------------ non-finite rows

@pytest.mark.parametrize("n", [300, 20000])
@pytest.mark.parametrize("value", [np.nan, np.inf])
def test_a_non_finite_sample_stays_in_its_slot(bank, n, value):
    re, im = rows(n)
    clean = bank(3).process(re, im)
    bad_re, bad_im = re.copy(), im.copy()
    bad_im[1, n // 2] = value
    got = bank(3).process(bad_re, bad_im)
    assert not np.isfinite(got[0][1]) and not np.isfinite(got[1][1])
    for k in (0, 2):
        assert (bits(got[0][k]), bits(got[1][k])) == (bits(clean[0][k]), bits(clean[1][k])), k
    assert list(got[2]) == [n - 1] * 3
    assert np.isnan(demod.frequency_error_hz(got[0][1], got[1][1], 96000))


# ------------------------------------------------------------------ chains

FS, SPACING, PACKET, CENTER, RATE = 2_400_000, 25_000, 16_384, 100_000_000, 96_000
# nominal offsets at which the table mixer of the ReceiverBank's front end is exact, and within
# 0.5 Hz of the request at nominal + the correction below (its tables hold a whole number of cycles
# in at most 500 samples, so most frequencies are met to some Hz only; asserted in cpu_estimates)
NOMINAL = [370_000, -505_000, -200_000, 140_000]
DELTA = [1305, -2120, 0, 630]
WANT = [1300.0, -2125.0, 0.0, 625.0]
STEP, INTERVAL, CALLS = 25.0, 2, 8                        # the first interval and six more calls
MARGIN_HZ = 5.0
CARRIER, DEPTH, TONE_HZ = 0.12, 0.8, 1000.0


@functools.lru_cache(maxsize=None)
def chain_packets(present=(True, True, True, True)):
    """CALLS u8 packets: AM carriers, 80 % tone modulation, at nominal + delta of the slots present."""
    t = np.arange(CALLS * PACKET)
    x = np.zeros(t.size, np.complex128)
    for k, on in enumerate(present):
        if on:
            env = 1.0 + DEPTH * np.sin(2 * np.pi * (TONE_HZ + 100 * k) / FS * t)
            x += CARRIER * env * np.exp(2j * np.pi * ((NOMINAL[k] + DELTA[k]) / FS * t))
    iq = np.empty(2 * t.size)
    iq[0::2], iq[1::2] = x.real, x.imag
    raw = np.clip(np.rint(iq * 128 + 127.4), 0, 255).astype(np.uint8)
    assert raw.min() > 0 and raw.max() < 255                   # no clipping
    return [raw[2 * p * PACKET:2 * (p + 1) * PACKET] for p in range(CALLS)]


def _freqs(corr):
    return [CENTER + f + int(c) for f, c in zip(NOMINAL, corr)]


class _RestatedReceiverFront:
    """oracle.demod.ResamplerFrontEnd per slot: the ReceiverBank's front end, float32 as the device."""

    def __init__(self):
        self.slots = [odemod.ResamplerFrontEnd(odemod.IN_U8, FS, RATE) for _ in NOMINAL]

    def tune(self, corr):
        for fe, f in zip(self.slots, _freqs(corr)):
            fe.set_frequencies(CENTER, f)

    def process(self, raw):
        out = [fe.process(raw) for fe in self.slots]
        return [re for re, _ in out], [im for _, im in out]


@functools.lru_cache(maxsize=None)
def _raster_rows(passband):
    """All raster channels of the packets in float64 (tests/pfb_ref.py): [M, outputs] per packet."""
    (M, L, D), taps = demod.Channelizer.channels_design(FS, SPACING, RATE, passband)
    assert L == 1
    stream = pfb_ref.Stream(M, D, taps)
    return M, [stream.process(pfb_ref.convert(raw, "u8")) for raw in chain_packets()]


class _RestatedTunedFront:
    """The TunedReceiverBank's front end in float64: the raster channel nearest to each slot, rotated
    by the offset that is left (tests/pfb_tuning_ref.py rot64)."""

    def __init__(self, passband):
        self.M, self.rows = _raster_rows(passband)
        self.p = self.done = 0

    def tune(self, corr):
        near = [demod.Channelizer.nearest_raster_channel(self.M, CENTER, f, FS) for f in _freqs(corr)]
        self.sel = [k for k, _ in near]
        self.q, self.steps = demod.Channelizer.offsets_tuning([d for _, d in near], RATE)

    def process(self, raw):
        y = self.rows[self.p]
        z = [tref.rot64(y[k], self.q, m, self.done) for k, m in zip(self.sel, self.steps)]
        self.p += 1
        self.done += y.shape[1]
        return [v.real for v in z], [v.imag for v in z]


def cpu_estimates(front):
    """The chain's loop on the CPU with a restated front end: per interval and slot, the estimate
    applied + error_hz of the interval's accumulated R1.  Asserts that every estimate lies within
    MARGIN_HZ of the carrier's true offset and rounds to WANT."""
    applied = [0.0] * 4
    carry = [None] * 4
    acc = np.zeros((4, 2))
    front.tune(applied)
    out = []
    for p, raw in enumerate(chain_packets()):
        re, im = front.process(raw)
        for k in range(4):
            s = freq_ref.r1(F32(re[k]), F32(im[k]), carry[k])
            acc[k] += s[:2]
            carry[k] = (re[k][-1], im[k][-1])
        if (p + 1) % INTERVAL == 0:
            est = [applied[k] + freq_ref.error_hz(acc[k, 0], acc[k, 1], RATE) for k in range(4)]
            print(f"cpu estimates after packet {p}: {est}")
            for k in range(4):
                assert abs(est[k] - DELTA[k]) < MARGIN_HZ, (p, k, est[k])
                assert freq_ref.step_round(est[k], STEP) == WANT[k], (p, k, est[k])
                if freq_ref.step_round(est[k], STEP) != applied[k]:
                    carry[k] = None                            # retuned: the phase jumps
            applied = [freq_ref.step_round(e, STEP) for e in est]
            front.tune(applied)
            acc[:] = 0.0
            out.append(est)
    return out


def _tuned(**kw):
    return demod.TunedReceiverBank("u8", FS, SPACING, ["am"] * 4, **kw)


def _receiver(**kw):
    return demod.ReceiverBank("u8", FS, ["am"] * 4, **kw)


def _same_audio(got, want, what):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.size > 0, (what, k, g.shape, w.shape)
        assert np.array_equal(g.view(np.int32), w.view(np.int32)), (what, k)


@pytest.mark.parametrize("kind", ["tuned", "receiver"])
def test_chain_reaches_the_corrections_and_is_the_meter_plus_setter_calls(rfa, kind):
    make = _tuned if kind == "tuned" else _receiver
    with make(afc={"interval": INTERVAL}) as rx, make(afc=None) as plain:
        assert isinstance(rx.meter, demod.FrequencyMeterBank) and not hasattr(plain, "meter")
        assert plain.corrections is None and plain.frequency_errors is None
        assert list(rx._afc.limit_hz) == [demod.mode_info("am")[3] / 2] * 4 and rx._afc.step_hz == STEP
        cpu_estimates(_RestatedTunedFront(rx.passband_hz) if kind == "tuned" else _RestatedReceiverFront())
        assert rx.meter.stream == rx.front.stream == rx.demods.stream
        rx.set_frequencies(CENTER, _freqs([0] * 4))
        plain.set_frequencies(CENTER, _freqs([0] * 4))
        applied = [0.0] * 4
        for p, raw in enumerate(chain_packets()):
            got, want = rx.process(raw), plain.process(raw)
            _same_audio(got, want, f"{kind} packet {p}")
            corr = list(rx.corrections)
            print(f"{kind} packet {p}: corrections {corr}, errors {list(rx.frequency_errors)}")
            assert corr == ([0.0] * 4 if p + 1 < INTERVAL else WANT), (p, corr)
            if (p + 1) % INTERVAL == 0:                        # the estimate behind it, as on the CPU
                for k in range(4):
                    assert abs(applied[k] + rx.frequency_errors[k] - DELTA[k]) < MARGIN_HZ, (p, k)
            if corr != applied:                                # the chain retuned: the same call for the other
                plain.set_frequencies(CENTER, _freqs(corr))
                applied = corr
        if kind == "tuned":
            assert rx.offsets == plain.offsets and rx.channels == plain.channels
        # a user's set_frequencies starts the rule again
        rx.set_frequencies(CENTER, _freqs([0] * 4))
        assert list(rx.corrections) == [0.0] * 4 and np.isnan(rx.frequency_errors).all()


def test_afc_none_is_the_chain_as_it_was(rfa):
    """No meter handle, and the audio of the composition the chain is defined by: a FrontEndBank into a
    DemodulatorBank on the same packets."""
    with _receiver() as rx:
        assert not hasattr(rx, "meter") and rx._afc is None and rx.corrections is None
        rx.set_frequencies(CENTER, _freqs([0] * 4))
        with demod.FrontEndBank("u8", FS, RATE, 4, resampler=True) as fe, demod.DemodulatorBank(["am"] * 4) as dm:
            fe.set_frequencies(CENTER, _freqs([0] * 4))
            for p, raw in enumerate(chain_packets()[:3]):
                re, im = fe.process(raw)
                _same_audio(rx.process(raw), dm.process(re, im), f"packet {p}")


def test_squelch_and_mode_gate_the_rule(rfa):
    """Slot 2 is in USB; slot 3's carrier is absent and its squelch closed: neither ever moves, and the
    two AM slots with a carrier reach their corrections."""
    packets = chain_packets((True, True, True, False))
    threshold = -15.0
    with demod.TunedReceiverBank("u8", FS, SPACING, ["am", "am", "usb", "am"], squelch=[threshold] * 4,
                                 afc={"interval": INTERVAL}) as rx:
        rx.squelch_debounce = 1
        rx.set_frequencies(CENTER, _freqs([0] * 4))
        for p, raw in enumerate(packets):
            rx.process(raw)
            levels, gates = rx.levels, rx.open
            print(f"packet {p}: levels {list(levels)}, corrections {list(rx.corrections)}")
            assert (levels[:3] > threshold + 1).all() and levels[3] < threshold - 1, (p, list(levels))
            assert list(gates) == [True, True, True, False]
            corr, errs = rx.corrections, rx.frequency_errors
            assert corr[2] == 0 and corr[3] == 0 and np.isnan(errs[2]) and np.isnan(errs[3]), (p, corr, errs)
            if p + 1 >= INTERVAL:
                assert list(corr[:2]) == WANT[:2], (p, list(corr))
    # the same packets without the squelch: the slot without a carrier is active and is given an estimate
    with demod.TunedReceiverBank("u8", FS, SPACING, ["am", "am", "usb", "am"], afc={"interval": INTERVAL}) as rx:
        rx.set_frequencies(CENTER, _freqs([0] * 4))
        for raw in packets[:INTERVAL]:
            rx.process(raw)
        errs = rx.frequency_errors
        assert np.isnan(errs[2]) and np.isfinite(errs[3]) and list(rx.corrections[:2]) == WANT[:2]


def test_set_stream_moves_the_meter_and_nothing_is_metered_before_set_frequencies(rfa):
    import torch
    side = torch.cuda.Stream()
    with _tuned(afc=True) as rx:
        rx.process(chain_packets()[0])                        # no nominal frequencies yet: raster channels 0 .. 3
        assert list(rx.meter.collect()[2]) == [0] * 4 and np.isnan(rx.frequency_errors).all()
        rx.set_stream(side.cuda_stream)
        assert rx.meter.stream == rx.front.stream == rx.demods.stream == side.cuda_stream
        rx.set_frequencies(CENTER, _freqs([0] * 4))
        rx.process(chain_packets()[1])
        terms = rx.meter.collect()[2]
        assert (terms > 0).all() and len(set(terms)) == 1
        rx.set_stream(None)
        assert rx.meter.stream == rx.demods.stream != side.cuda_stream
    with pytest.raises(ValueError):
        demod.RasterReceiverBank("u8", FS, SPACING, ["nfm"] * 4, afc=True)
