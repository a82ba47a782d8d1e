"""CPU: the host-only side of the tone meter and the tone squelch -- the restatement (tests/tone_ref.py)
against exactly summed terms, rfa_tone_phasor against numpy, rfa_tone_quality, demod.ToneRule on made-up
sums against the restated rule, demod.tone_guards, the argument checks of rfa_tone_* that come before
the device is looked for, the chains' ``tone`` keyword without a device, and tools/tone_host_check (the
same host paths under ASan + UBSan)."""
import ctypes
import inspect
import math
import os
import subprocess

import numpy as np
import pytest

import slot_sum_plan as plan
import tone_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, NODEVICE = -1, -4
RATE = 48000
PROBES = (670, 693, 2541)                                   # 67.0 / 69.3 / 254.1 Hz


@pytest.fixture(scope="module")
def lib():
    import rfanalyzer_amd
    rfanalyzer_amd.build()
    return rfanalyzer_amd.lib()


# ------------------------------------------------------------------ the restatement

@pytest.mark.parametrize("n", [1, 257, 4097, plan.TILE + 1, 40000])
def test_restated_sums_are_within_the_bound_of_the_exact_sums(n):
    """Each component within (terms + 2) * 2^-53 * sum|term| of math.fsum of the once-rounded terms."""
    table = tone_ref.numpy_table(RATE)
    rows = plan.pin_rows(n)[0]
    for k in range(plan.K):
        base = (0, 479_999, 123_456)[k]
        terms = tone_ref.terms(rows[k], PROBES, base, RATE, table)
        got = tone_ref.sums(rows[k], PROBES, base, RATE, table)
        for c, t in enumerate(terms):
            exact = math.fsum(t)
            bound = (t.size + 2) * 2.0 ** -53 * math.fsum(np.abs(t))
            print(f"n {n} slot {k} component {c}: |d| {abs(got[c] - exact):.3e} (bound {bound:.3e})")
            assert abs(got[c] - exact) <= bound, (n, k, c)
        # the power's products are exact and the plain sum's terms are the samples
        a = rows[k].astype(np.float64)
        assert np.array_equal(terms[6], a * a) and np.array_equal(terms[7], a)
        assert all(float(np.float32(v)) * float(np.float32(v)) == p for v, p in zip(rows[k][:50], terms[6][:50]))


def test_restated_index_is_the_absolute_sample_times_the_probe_modulo_m():
    M = tone_ref.modulus(RATE)
    assert M == 480000
    for f10, base, n in ((670, 0, 100), (2541, M - 1, 100), (239_999, M - 3, 50), (1, 0, 20)):
        want = [(f10 * (base + i)) % M for i in range(n)]                   # Python integers: no overflow
        assert list(tone_ref.indices(f10, base, n, RATE)) == want
        # base is kept modulo M: a counter that ran past M meets the same phasors
        assert list(tone_ref.indices(f10, base + 7 * M, n, RATE)) == want
    # a row cut anywhere meets the phasors of the row given whole
    whole = tone_ref.indices(1035, 17, 1000, RATE)
    cut = np.concatenate([tone_ref.indices(1035, 17, 333, RATE), tone_ref.indices(1035, (17 + 333) % M, 667, RATE)])
    assert np.array_equal(whole, cut)
    # the largest products stay inside int64: f10 < 5 * rate, base + i < M + 2^36
    assert (5 * 384000) * (10 * 384000 + 2 ** 36) < 2 ** 63


def test_unused_probe_sums_to_plus_zero():
    table = tone_ref.numpy_table(8000)
    a = plan.pin_rows(257)[0][0]
    s = tone_ref.sums(a, (670, 0, 2541), 5, 8000, table)
    assert s[2] == 0.0 and s[3] == 0.0 and not np.signbit(s[2:4]).any()
    assert s[0] != 0.0 and s[4] != 0.0 and s[6] > 0.0


# ------------------------------------------------------------------ host-only entries

@pytest.mark.parametrize("rate", [8000, 48000, 384000])
def test_phasor_against_numpy(lib, rate):
    """Within 2^-52 of numpy's cos and sin of the same double angle ((2 pi) * p) / M."""
    M = tone_ref.modulus(rate)
    ps = sorted({0, 1, M // 4, M // 4 + 1, M // 2, M - 1, *np.random.default_rng(rate).integers(0, M, 3000).tolist()})
    if rate == 8000:
        ps = list(range(M))
    th = (2.0 * np.pi * np.array(ps, np.float64)) / float(M)
    want_c, want_s = np.cos(th), np.sin(th)
    c, s = ctypes.c_double(9), ctypes.c_double(9)
    worst = 0.0
    for i, p in enumerate(ps):
        assert lib.rfa_tone_phasor(rate, p, ctypes.byref(c), ctypes.byref(s)) == 0
        worst = max(worst, abs(c.value - want_c[i]), abs(s.value - want_s[i]))
    print(f"rate {rate}: max |phasor - numpy| = {worst:.3e} (bound {2.0 ** -52:.3e})")
    assert worst <= 2.0 ** -52
    assert lib.rfa_tone_phasor(rate, 0, ctypes.byref(c), ctypes.byref(s)) == 0 and (c.value, s.value) == (1.0, 0.0)
    if rate == 8000:
        assert np.abs(tone_ref.library_table(rate) - tone_ref.numpy_table(rate)).max() <= 2.0 ** -52


def test_phasor_argument_errors(lib):
    c, s = ctypes.c_double(9), ctypes.c_double(9)
    rc, rs = ctypes.byref(c), ctypes.byref(s)
    for rate, p in ((7999, 0), (384001, 0), (0, 0), (-48000, 0), (48000, -1), (48000, 480000), (8000, 80000)):
        assert lib.rfa_tone_phasor(rate, p, rc, rs) == INVALID, (rate, p)
    assert lib.rfa_tone_phasor(48000, 0, None, rs) == INVALID and lib.rfa_tone_phasor(48000, 0, rc, None) == INVALID
    assert (c.value, s.value) == (9.0, 9.0)
    assert lib.rfa_tone_phasor(8000, 79999, rc, rs) == 0 and lib.rfa_tone_phasor(384000, 3839999, rc, rs) == 0


def test_quality_equals_the_restatement(lib):
    from rfanalyzer_amd import demod
    rng = np.random.default_rng(3)
    for sc, ss, p, s1 in rng.standard_normal((200, 4)) * 10.0 ** rng.integers(-6, 6, (200, 1)):
        n = int(rng.integers(1, 100000))
        p = abs(p)
        got = lib.rfa_tone_quality(sc, ss, p, s1, n)
        want = tone_ref.quality(sc, ss, p, s1, n)
        assert got == demod.tone_quality(sc, ss, p, s1, n)
        assert got == want or abs(got - want) <= 4 * 2.0 ** -52 * abs(want), (sc, ss, p, s1, n)
    # a pure tone at the probe over whole periods: n A / 2 against n A^2 / 2
    assert lib.rfa_tone_quality(500.0, 0.0, 500.0, 0.0, 1000) == pytest.approx(1.0, rel=1e-15)
    assert lib.rfa_tone_quality(300.0, 400.0, 500.0, 0.0, 1000) == pytest.approx(1.0, rel=1e-15)
    # no AC power: a constant row (n P = S1^2), an empty one, rounding below zero
    assert lib.rfa_tone_quality(1.0, 1.0, 4.0, 2.0, 1) == 0.0
    assert lib.rfa_tone_quality(0.0, 0.0, 0.0, 0.0, 0) == 0.0
    assert lib.rfa_tone_quality(1.0, 0.0, 1.0, 2.0, 3) == 0.0
    for bad in (math.inf, -math.inf, math.nan):
        for args in ((bad, 0.0, 1.0, 0.0), (0.0, bad, 1.0, 0.0), (0.0, 0.0, bad, 0.0), (0.0, 0.0, 1.0, bad)):
            assert math.isnan(lib.rfa_tone_quality(*args, 10)) and math.isnan(tone_ref.quality(*args, 10))


# ------------------------------------------------------------------ the rule

def _sums(K, q, n, guard=(0.0, 0.0), phase=0.3):
    """Sums [8, K] of n samples whose probe 0 has quality q against unit AC power, guards at the given
    share of probe 0's power."""
    s = np.zeros((8, K))
    amp = math.sqrt(q * n * n / 2.0)                       # 2 |C|^2 / (n * n) = q with P = n, S1 = 0
    s[0], s[1] = amp * math.cos(phase), amp * math.sin(phase)
    for j, g in enumerate(guard, 1):
        s[2 * j] = amp * math.sqrt(g)
    s[6] = n
    return s


def _rules(K=2, **kw):
    from rfanalyzer_amd import demod
    return demod.ToneRule(K, RATE, **kw), tone_ref.Rule(K, RATE, **kw)


def _step(rules, sums, n, active=None):
    got = rules[0].update(sums, n, active)
    want = rules[1].update(sums, n, active)
    assert list(got) == want
    np.testing.assert_array_equal(rules[0].quality, rules[1].q)
    return list(got)


def test_rule_defaults_are_the_documented_ones():
    r, _ = _rules()
    assert (r.window_s, r.threshold, r.guard_ratio, r.hang, r.rate) == (0.5, 0.01, 4.0, 2, 48000.0)
    assert list(r.open) == [False, False] and np.isnan(r.quality).all()


def test_rule_window_boundary_inside_a_call():
    """24000 samples make a window: calls of 5000 reach it inside the fifth, which is evaluated whole."""
    rules = _rules()
    n = np.array([5000, 5000])
    for call in range(4):
        assert _step(rules, _sums(2, 0.05, 5000), n) == [False, False]
        assert np.isnan(rules[0].quality).all()
    assert _step(rules, _sums(2, 0.05, 5000), n) == [True, True]            # 25000 >= 24000
    assert rules[0].quality[0] == pytest.approx(0.05, rel=1e-12)            # the five calls' sums add in phase
    # the accumulators were cleared: four more calls decide nothing, the fifth does
    for call in range(4):
        assert _step(rules, _sums(2, 0.0, 5000), n) == [True, True]
    assert _step(rules, _sums(2, 0.0, 5000), n) == [True, True]             # one miss: hang is 2
    for call in range(4):
        _step(rules, _sums(2, 0.0, 5000), n)
    assert _step(rules, _sums(2, 0.0, 5000), n) == [False, False]           # the second miss in a row
    # slots reach their windows on their own counts
    rules = _rules()
    assert _step(rules, _sums(2, 0.05, 24000), np.array([23999, 24000])) == [False, True]
    assert _step(rules, _sums(2, 0.05, 1), np.array([1, 1])) == [True, True]


def test_rule_call_longer_than_a_window():
    rules = _rules()
    n = np.array([100000, 100000])
    assert _step(rules, _sums(2, 0.05, 100000), n) == [True, True]
    assert _step(rules, _sums(2, 0.005, 100000), n) == [True, True]         # a miss
    assert _step(rules, _sums(2, 0.05, 100000), n) == [True, True]          # a hit clears the count
    assert _step(rules, _sums(2, 0.005, 100000), n) == [True, True]
    assert _step(rules, _sums(2, 0.005, 100000), n) == [False, False]


def test_rule_resets_an_inactive_slot_and_one_without_samples():
    rules = _rules(3)
    n = np.array([30000] * 3)
    assert _step(rules, _sums(3, 0.05, 30000), n) == [True] * 3
    assert _step(rules, _sums(3, 0.05, 30000), n, [True, False, True]) == [True, False, True]
    assert _step(rules, _sums(3, 0.05, 30000), np.array([30000, 30000, 0])) == [True, True, False]
    assert math.isnan(rules[0].quality[2])
    # half a window, an inactive call, half a window: the halves do not add up
    rules = _rules(1)
    half = np.array([12000])
    assert _step(rules, _sums(1, 0.05, 12000), half) == [False]
    assert _step(rules, _sums(1, 0.05, 12000), half, [False]) == [False]
    assert _step(rules, _sums(1, 0.05, 12000), half) == [False]
    assert _step(rules, _sums(1, 0.05, 12000), half) == [True]


def test_rule_hang():
    for hang in (1, 3):
        rules = _rules(1, hang=hang)
        n = np.array([24000])
        assert _step(rules, _sums(1, 0.05, 24000), n) == [True]
        for miss in range(hang - 1):
            assert _step(rules, _sums(1, 0.0, 24000), n) == [True]
        assert _step(rules, _sums(1, 0.0, 24000), n) == [False]
        assert _step(rules, _sums(1, 0.05, 24000), n) == [True]


def test_rule_non_finite_sum_is_a_miss():
    rules = _rules(2, hang=1)
    n = np.array([24000, 24000])
    assert _step(rules, _sums(2, 0.05, 24000), n) == [True, True]
    bad = _sums(2, 0.05, 24000)
    bad[:, 1] = np.nan
    assert _step(rules, bad, n) == [True, False]
    assert math.isnan(rules[0].quality[1]) and rules[0].quality[0] == pytest.approx(0.05)
    bad = _sums(2, 0.05, 24000)
    bad[4, 0] = np.inf                                       # a guard alone: q is finite, the comparison fails
    assert _step(rules, bad, n) == [False, True]
    assert _step(rules, _sums(2, 0.05, 24000), n) == [True, True]           # the next window is clean


def test_rule_guards_decide_where_q_passes():
    n = np.array([24000, 24000])
    rules = _rules()
    assert _step(rules, _sums(2, 0.05, 24000, guard=(0.2, 0.24)), n) == [True, True]      # below 1 / 4
    rules = _rules()
    assert _step(rules, _sums(2, 0.05, 24000, guard=(0.0, 0.26)), n) == [False, False]    # q passes, a guard does not
    assert rules[0].quality[0] == pytest.approx(0.05)
    rules = _rules()
    assert _step(rules, _sums(2, 0.05, 24000, guard=(0.3, 0.0)), n) == [False, False]
    # an unused guard is not asked; a slot without probe 0 reads open and is never evaluated
    rules = _rules()
    for r in rules[:1]:
        r.set_used(0, [True, True, False])
        r.set_used(1, [False, False, False])
    rules[1].used = [[True, True, False], [False, False, False]]
    assert list(rules[0].open) == [False, True]
    assert _step(rules, _sums(2, 0.05, 24000, guard=(0.0, 9.0)), n) == [True, True]
    assert math.isnan(rules[0].quality[1])
    rules = _rules(guard_ratio=1.0)
    assert _step(rules, _sums(2, 0.05, 24000, guard=(0.9, 0.9)), n) == [True, True]
    # the threshold is exclusive
    s = _sums(2, 0.05, 24000)
    q = tone_ref.quality(s[0, 0], s[1, 0], s[6, 0], s[7, 0], 24000)
    rules = _rules(threshold=q)
    assert _step(rules, s, n) == [False, False]


def test_rule_arguments_and_reset():
    from rfanalyzer_amd import demod
    for bad in ({"window_s": 0}, {"window_s": math.nan}, {"threshold": -1}, {"guard_ratio": -1}, {"hang": 0},
                {"hang": 1.5}):
        with pytest.raises(ValueError):
            demod.ToneRule(2, RATE, **bad)
    with pytest.raises(ValueError):
        demod.ToneRule(0, RATE)
    with pytest.raises(ValueError):
        demod.ToneRule(2, 0.0)
    r = demod.ToneRule(2, RATE)
    with pytest.raises(ValueError):
        r.update(np.zeros((8, 3)), np.zeros(3))
    with pytest.raises(ValueError):
        r.update(np.zeros((2, 2)), np.zeros(2))
    for k in (-1, 2):
        with pytest.raises(ValueError):
            r.reset(k)
        with pytest.raises(ValueError):
            r.set_used(k, [True] * 3)
    with pytest.raises(ValueError):
        r.set_used(0, [True])
    n = np.array([24000, 24000])
    assert list(r.update(_sums(2, 0.05, 24000), n)) == [True, True]
    r.reset(1)
    assert list(r.open) == [True, False] and math.isnan(r.quality[1]) and not math.isnan(r.quality[0])
    r.reset()
    assert list(r.open) == [False, False] and np.isnan(r.quality).all()


# ------------------------------------------------------------------ guards and the table

def test_ctcss_table():
    from rfanalyzer_amd import demod
    t = demod.CTCSS_TONES
    assert len(t) == 50 and t[0] == 67.0 and t[-1] == 254.1 and list(t) == sorted(set(t)) == list(tone_ref.CTCSS)
    gaps = np.diff(t)
    assert gaps.min() == pytest.approx(2.3) and all(round(x * 10) == pytest.approx(x * 10) for x in t)


def test_tone_guards():
    from rfanalyzer_amd import demod
    assert demod.tone_guards(100.0) == (97.4, 103.5) == tone_ref.guards(100.0)
    assert demod.tone_guards(69.3) == (67.0, 71.9) and demod.tone_guards(250.3) == (241.8, 254.1)
    assert demod.tone_guards(100.04) == (97.4, 103.5)                       # a table tone to 0.05 Hz
    for hz in (67.0, 254.1, 150.0, 100.2, 1000.0):                          # both ends and off-table tones
        want = (round(hz * 0.965 * 10) / 10, round(hz * 1.035 * 10) / 10)
        assert demod.tone_guards(hz) == want == tone_ref.guards(hz), hz
    assert demod.tone_guards(67.0) == (64.7, 69.3) and demod.tone_guards(150.0) == (144.8, 155.2)
    for hz in demod.CTCSS_TONES:
        assert demod.tone_guards(hz) == tone_ref.guards(hz)
    assert demod._tone_probes(100.0) == [1000, 974, 1035] and demod._tone_probes(None) == [0, 0, 0]


# ------------------------------------------------------------------ the library without a device

def _create(lib, n_channels, rate=RATE):
    h = ctypes.c_void_p(1)
    rc = lib.rfa_tone_create(0, n_channels, rate, ctypes.byref(h))
    if rc == 0:
        lib.rfa_tone_destroy(h)
    return rc, h.value


def test_argument_errors_come_before_the_device(lib):
    assert lib.rfa_tone_create(0, 4, RATE, None) == INVALID
    for k in (0, -1, 1025, -2 ** 31, 2 ** 31 - 1):
        assert _create(lib, k) == (INVALID, None), k
    for rate in (7999, 384001, 0, -1, 2 ** 31 - 1):
        assert _create(lib, 4, rate) == (INVALID, None), rate


def test_valid_request_without_a_device_is_nodevice(lib):
    import torch
    for k, rate in ((1, 8000), (32, 48000), (1024, 48000)):
        rc, h = _create(lib, k, rate)
        if not torch.cuda.is_available():
            assert (rc, h) == (NODEVICE, None)
        else:
            assert rc == 0


def test_null_handle_answers(lib):
    s = ctypes.c_void_p(0)
    assert lib.rfa_tone_destroy(None) == INVALID
    assert lib.rfa_tone_last_error(None) == b"null handle"
    assert lib.rfa_tone_set_stream(None, None) == INVALID
    assert lib.rfa_tone_get_stream(None, ctypes.byref(s)) == INVALID
    assert lib.rfa_tone_synchronize(None) == INVALID
    v = ctypes.c_int32(9)
    f = (ctypes.c_int32 * 3)(9, 9, 9)
    d = (ctypes.c_double * 8)(*[9.0] * 8)
    t = (ctypes.c_int64 * 1)(9)
    n = (ctypes.c_size_t * 1)(0)
    assert lib.rfa_tone_get_channels(None, ctypes.byref(v), ctypes.byref(v)) == INVALID
    assert lib.rfa_tone_set_probes(None, 0, f) == INVALID and lib.rfa_tone_get_probes(None, 0, f) == INVALID
    assert lib.rfa_tone_break(None, 0) == INVALID and lib.rfa_tone_break(None, -1) == INVALID
    assert lib.rfa_tone_reset(None) == INVALID
    assert lib.rfa_tone_process(None, None, 0, n) == INVALID
    assert lib.rfa_tone_collect(None, d, t) == INVALID
    assert lib.rfa_tone_process_host(None, None, 0, n, d, t) == INVALID
    assert (v.value, list(f), list(d), list(t)) == (9, [9, 9, 9], [9.0] * 8, [9])


def test_meter_bank_sits_on_the_handle_base():
    from rfanalyzer_amd import demod
    assert issubclass(demod.ToneMeterBank, demod._Handle) and demod.ToneMeterBank._prefix == "rfa_tone"
    for name in ("close", "set_stream", "synchronize", "stream", "__enter__", "__exit__", "__del__", "_call"):
        assert name not in vars(demod.ToneMeterBank), name
    for name in ("set_probes", "probes", "process_device", "collect", "process", "process_tensor", "break_", "reset"):
        assert name in vars(demod.ToneMeterBank), name


# ------------------------------------------------------------------ the chains' keyword without a device

def test_tone_is_a_keyword_of_every_bank_chain():
    from rfanalyzer_amd import demod
    for cls in (demod.ReceiverBank, demod.TunedReceiverBank, demod.RasterReceiverBank):
        p = inspect.signature(cls.__init__).parameters["tone"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None
    for name in ("tone_open", "tone_quality"):
        assert isinstance(vars(demod._BankChain)[name], property)
    assert "set_tone" in vars(demod._BankChain)
    assert "tone_meter" not in vars(demod._BankChain)        # no meter attribute unless a chain asks for tones


def test_tone_keyword_is_checked_before_any_handle_is_made():
    """These raise on a machine with a device and on one without, before a handle exists."""
    from rfanalyzer_amd import demod
    fs, spacing = 2_400_000, 25_000
    for make in (lambda **kw: demod.ReceiverBank("u8", fs, ["nfm", "am"], **kw),
                 lambda **kw: demod.TunedReceiverBank("u8", fs, spacing, ["nfm", "am"], **kw),
                 lambda **kw: demod.RasterReceiverBank("u8", fs, spacing, ["nfm", "am"], **kw)):
        for bad in (True, 100.0, "100.0", 100):
            with pytest.raises(TypeError):
                make(tone=bad)
        for bad in ([100.0, "67.0"], [True, None], [[100.0], None]):
            with pytest.raises(TypeError):
                make(tone=bad)
        for bad in ([100.0], [100.0, None, None], [0.0, None], [-67.0, None], [math.nan, None], [24000.0, None],
                    [23500.0, None]):                                        # the upper guard leaves the band
            with pytest.raises(ValueError):
                make(tone=bad)


def test_valid_tone_without_a_device_fails_at_the_device():
    import torch
    if torch.cuda.is_available():
        return                                              # with a device tests/test_gpu_tone.py builds these chains
    from rfanalyzer_amd import _lib, demod
    with pytest.raises(_lib.RfaError) as e:
        demod.ReceiverBank("u8", 2_400_000, ["nfm"] * 2, tone=[100.0, None])
    assert e.value.status == NODEVICE


def test_host_check_program_passes_under_sanitizers(lib):
    """tools/tone_host_check: tone.hip's host side built with -fsanitize=address,undefined into a
    stand-alone program that walks the host-only entries and the error paths."""
    exe = os.path.join(ROOT, "tools", "tone_host_check")
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tools"), exe], capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "tone_host_check ok" in r.stdout
