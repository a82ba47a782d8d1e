"""CPU: the host-only side of the frequency meter and AFC -- rfa_freq_error_hz against its restatement
(tests/freq_ref.py), the estimator's derived bound on AM carriers, demod.AfcRule on made-up sums, the
argument checks of rfa_freq_* that come before the device is looked for, the null-handle answers, the
chains' ``afc`` keyword without a device, and tools/freq_host_check (the same host paths under
ASan + UBSan)."""
import ctypes
import inspect
import math
import os
import subprocess

import numpy as np
import pytest

import freq_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, NODEVICE = -1, -4
RATE = 96000.0


@pytest.fixture(scope="module")
def lib():
    import rfanalyzer_amd
    rfanalyzer_amd.build()
    return rfanalyzer_amd.lib()


# ------------------------------------------------------------------ Hz of a pair of sums

def test_error_hz_equals_the_restatement(lib):
    from rfanalyzer_amd import demod
    rng = np.random.default_rng(5)
    for re, im in rng.standard_normal((200, 2)) * 10.0 ** rng.integers(-300, 300, (200, 1)):
        got = lib.rfa_freq_error_hz(re, im, RATE)
        assert got == demod.frequency_error_hz(re, im, RATE)
        assert abs(got - freq_ref.error_hz(re, im, RATE)) <= 1e-11 * RATE
    for re, im in ((0.0, 0.0), (-0.0, 0.0), (0.0, -0.0), (-0.0, -0.0)):
        assert lib.rfa_freq_error_hz(re, im, RATE) == 0.0      # not atan2's pi for (-0, +0)
    for bad in (math.inf, -math.inf, math.nan):
        for re, im in ((bad, 1.0), (1.0, bad), (bad, bad), (bad, 0.0), (0.0, bad)):
            assert math.isnan(lib.rfa_freq_error_hz(re, im, RATE)) and math.isnan(freq_ref.error_hz(re, im, RATE))
    assert lib.rfa_freq_error_hz(0.0, 1.0, RATE) == pytest.approx(RATE / 4, rel=1e-15)
    assert lib.rfa_freq_error_hz(-1.0, 0.0, RATE) == pytest.approx(RATE / 2, rel=1e-15)
    assert lib.rfa_freq_error_hz(0.0, -1e-300, RATE) == pytest.approx(-RATE / 4, rel=1e-15)


def _am_row(n, f0, phi=0.4, amplitude=0.3, depth=0.8, tone_hz=700.0):
    i = np.arange(n)
    a = amplitude * (1.0 + depth * np.sin(2 * np.pi * tone_hz / RATE * i + 0.3))
    assert (a > 0).all()
    ph = 2 * np.pi * f0 / RATE * i + phi
    return (a * np.cos(ph)).astype(np.float32), (a * np.sin(ph)).astype(np.float32)


@pytest.mark.parametrize("f0", [0.0, 1300.0, -2125.0, 12500.0])
def test_estimator_bound_on_an_am_carrier(lib, f0):
    """|error_hz - f0| <= rate / (2 pi) * (2^-23.5 + 2^-40) for a[i] * exp(j (theta i + phi)), a > 0,
    stored as float32 (freq_ref.estimator_bound_hz has the derivation): 1.3e-3 Hz at 96 kHz."""
    bound = freq_ref.estimator_bound_hz(RATE)
    assert bound == RATE / (2 * math.pi) * (2.0 ** -23.5 + 2.0 ** -40) and 1.2e-3 < bound < 1.4e-3
    for n in (2, 3, 65, 655, 16385):
        re, im = _am_row(n, f0)
        s_re, s_im, terms, _, _ = freq_ref.r1(re, im)
        assert terms == n - 1
        err = lib.rfa_freq_error_hz(s_re, s_im, RATE)
        print(f"f0 {f0} n {n}: |error_hz - f0| = {abs(err - f0):.3e} Hz (bound {bound:.3e})")
        assert abs(err - f0) <= bound, (f0, n, err)


def test_restatement_carry_and_terms():
    rng = np.random.default_rng(9)
    re = rng.uniform(-1, 1, 700).astype(np.float32)
    im = rng.uniform(-1, 1, 700).astype(np.float32)
    z = re.astype(np.complex128) + 1j * im.astype(np.complex128)
    whole = freq_ref.r1(re, im)
    direct = (z[1:] * np.conj(z[:-1])).sum()
    assert whole[2] == 699 and abs(whole[0] - direct.real) <= whole[3] and abs(whole[1] - direct.imag) <= whole[4]
    a = freq_ref.r1(re[:300], im[:300])
    b = freq_ref.r1(re[300:], im[300:], (re[299], im[299]))
    assert (a[2], b[2]) == (299, 400)
    assert abs(a[0] + b[0] - whole[0]) <= 2.0 ** -52 * abs(whole[0]) + 1e-300
    assert abs(a[1] + b[1] - whole[1]) <= 2.0 ** -52 * abs(whole[1]) + 1e-300
    assert freq_ref.r1(re[:1], im[:1])[:3] == (0.0, 0.0, 0)          # one sample, no predecessor: no term
    assert freq_ref.r1(re[:0], im[:0])[:3] == (0.0, 0.0, 0)
    one = freq_ref.r1(re[:1], im[:1], (re[5], im[5]))
    assert one[2] == 1 and one[0] == float(re[0]) * float(re[5]) + float(im[0]) * float(im[5])


# ------------------------------------------------------------------ the rule

def _sums(hz, scale=3.0):
    th = 2 * np.pi * np.asarray(hz, np.float64) / RATE
    return scale * np.cos(th), scale * np.sin(th)


def _rule(k=4, **kw):
    from rfanalyzer_amd import demod
    kw.setdefault("limit_hz", 5000.0)
    return demod.AfcRule(k, RATE, **kw)


def test_rule_counts_calls_and_rounds_to_the_step():
    r = _rule(interval=3)
    assert r.step_hz == 25 and r.gain == 1.0 and _rule().interval == 8            # the documented defaults
    assert list(r.corrections) == [0] * 4 and np.isnan(r.errors_hz).all()
    hz = [1305.0, -2120.0, 0.0, 630.0]
    assert r.update(*_sums(hz)) == [] and r.update(*_sums(hz)) == []
    assert list(r.corrections) == [0] * 4 and np.isnan(r.errors_hz).all()          # nothing before the interval
    assert r.update(*_sums(hz)) == [0, 1, 3]                                       # slot 2 is where it was
    assert list(r.corrections) == [1300.0, -2125.0, 0.0, 625.0]
    np.testing.assert_allclose(r.errors_hz, hz, atol=1e-9)
    # what is left after the retune is below half a step: the correction stays, call after call
    left = [5.0, 5.0, 0.0, 5.0]
    for _ in range(4):
        assert r.update(*_sums(left)) == [] and r.update(*_sums(left)) == [] and r.update(*_sums(left)) == []
        assert list(r.corrections) == [1300.0, -2125.0, 0.0, 625.0]
    np.testing.assert_allclose(r.errors_hz, left, atol=1e-9)
    # a residual beyond half a step moves it again
    more = [20.0, 12.6, -12.4, -13.0]
    assert r.update(*_sums(more)) == [] and r.update(*_sums(more)) == []
    assert r.update(*_sums(more)) == [0, 1, 3]
    assert list(r.corrections) == [1325.0, -2100.0, 0.0, 600.0]
    # a tie goes up
    for c, want in ((12.5, 25.0), (-12.5, 0.0), (37.4, 25.0), (-37.6, -50.0)):
        assert freq_ref.step_round(c, 25.0) == want


def test_rule_accumulates_the_sums_not_the_estimates():
    r = _rule(1, interval=2)
    strong, weak = _sums([400.0], 100.0), _sums([-400.0], 1.0)
    r.update(*strong)
    r.update(*weak)
    want = freq_ref.error_hz(strong[0][0] + weak[0][0], strong[1][0] + weak[1][0], RATE)
    assert r.errors_hz[0] == pytest.approx(want, abs=1e-9) and 380 < want < 400
    assert list(r.corrections) == [freq_ref.step_round(want, 25.0)]


def test_rule_passes_over_inactive_zero_and_non_finite_slots():
    r = _rule(5, interval=2)
    re, im = _sums([800.0] * 5)
    re[2] = im[2] = 0.0                                     # R1 = 0
    re[3] = np.nan
    im[4] = np.inf
    active = [True, False, True, True, True]
    assert r.update(re, im, active) == []
    assert r.update(re, im, active) == [0]
    assert list(r.corrections) == [800.0, 0, 0, 0, 0]
    assert np.isnan(r.errors_hz[1:]).all()
    # a slot that was active on one call of the interval counts with that call's sums alone
    ok_re, ok_im = _sums([-300.0] * 5)
    assert r.update(ok_re, ok_im, [False, True, False, False, False]) == []
    assert r.update(ok_re, ok_im, [False] * 5) == [1]
    assert list(r.corrections) == [800.0, -300.0, 0, 0, 0]
    # a NaN on one call spoils that slot's interval and nothing else; the next interval is clean
    last = [False, False, True, True, True]
    assert r.update(re, im, last) == [] and r.update(ok_re, ok_im, last) == [2]
    assert list(r.corrections)[2:] == [-300.0, 0, 0] and np.isnan(r.errors_hz[3:]).all()
    last[2] = False
    assert r.update(ok_re, ok_im, last) == [] and r.update(ok_re, ok_im, last) == [3, 4]
    assert list(r.corrections) == [800.0, -300.0, -300.0, -300.0, -300.0]
    with pytest.raises(ValueError):
        r.update(re[:4], im[:4])


def test_rule_clamps_per_slot():
    r = _rule(3, interval=1, limit_hz=[4000.0, 1000.0, 0.0])
    assert r.update(*_sums([3000.0] * 3)) == [0, 1]
    assert list(r.corrections) == [3000.0, 1000.0, 0.0]
    assert r.update(*_sums([3000.0] * 3)) == [0]            # 6000 asked for, 4000 allowed
    assert list(r.corrections) == [4000.0, 1000.0, 0.0]
    assert r.update(*_sums([-9000.0] * 3)) == [0, 1]
    assert list(r.corrections) == [-4000.0, -1000.0, 0.0]
    np.testing.assert_allclose(r.errors_hz, [-9000.0] * 3, atol=1e-9)      # the estimate itself is not clamped


def test_rule_gain_below_one_approaches_without_overshoot():
    r = _rule(1, interval=1, gain=0.5)
    true, seen = 1000.0, []
    for _ in range(12):
        r.update(*_sums([true - r.corrections[0]]))
        seen.append(float(r.corrections[0]))
    assert seen[:4] == [500.0, 750.0, 875.0, 950.0]         # 500, 750, 875, 937.5 -> the nearest step
    assert seen == sorted(seen) and seen[-1] == 1000.0 and max(seen) == 1000.0


def test_rule_reset():
    r = _rule(3, interval=2)
    r.update(*_sums([500.0] * 3))
    r.update(*_sums([500.0] * 3))
    r.update(*_sums([-200.0] * 3))                          # half an interval in the accumulators
    r.reset(1)
    assert list(r.corrections) == [500.0, 0.0, 500.0] and np.isnan(r.errors_hz[1])
    assert r.update(*_sums([0.0] * 3), [False, True, False]) == [0, 2]    # the count went on; slot 1 starts from its new sums
    assert list(r.corrections) == [300.0, 0.0, 300.0]
    r.reset()
    assert list(r.corrections) == [0.0] * 3 and np.isnan(r.errors_hz).all()
    assert r.update(*_sums([100.0] * 3)) == []              # the count starts again
    assert r.update(*_sums([100.0] * 3)) == [0, 1, 2]
    for k in (-1, 3):
        with pytest.raises(ValueError):
            r.reset(k)


def test_rule_arguments():
    from rfanalyzer_amd import demod
    p = inspect.signature(demod.AfcRule.__init__).parameters
    assert p["limit_hz"].default is inspect.Parameter.empty and p["limit_hz"].kind is inspect.Parameter.KEYWORD_ONLY
    for bad in ({"step_hz": 0}, {"step_hz": math.nan}, {"interval": 0}, {"interval": 2.5}, {"gain": 0}, {"gain": 1.5},
                {"limit_hz": -1.0}, {"limit_hz": [1.0, math.nan, 1.0, 1.0]}, {"limit_hz": [1.0, 2.0]}):
        with pytest.raises(ValueError):
            _rule(**bad)
    with pytest.raises(ValueError):
        demod.AfcRule(0, RATE, limit_hz=1.0)
    with pytest.raises(ValueError):
        demod.AfcRule(2, 0.0, limit_hz=1.0)
    with pytest.raises(TypeError):
        demod.AfcRule(2, RATE)                              # no default limit


# ------------------------------------------------------------------ the library without a device

def _create(lib, n_channels):
    h = ctypes.c_void_p(1)
    rc = lib.rfa_freq_create(0, n_channels, ctypes.byref(h))
    if rc == 0:
        lib.rfa_freq_destroy(h)
    return rc, h.value


def test_argument_errors_come_before_the_device(lib):
    assert lib.rfa_freq_create(0, 4, None) == INVALID
    for k in (0, -1, 1025, -2 ** 31, 2 ** 31 - 1):
        assert _create(lib, k) == (INVALID, None), k


def test_valid_request_without_a_device_is_nodevice(lib):
    import torch
    for k in (1, 32, 1024):
        rc, h = _create(lib, k)
        if not torch.cuda.is_available():
            assert (rc, h) == (NODEVICE, None)
        else:
            assert rc == 0


def test_null_handle_answers(lib):
    s = ctypes.c_void_p(0)
    assert lib.rfa_freq_destroy(None) == INVALID
    assert lib.rfa_freq_last_error(None) == b"null handle"
    assert lib.rfa_freq_set_stream(None, None) == INVALID
    assert lib.rfa_freq_get_stream(None, ctypes.byref(s)) == INVALID
    assert lib.rfa_freq_get_stream(None, None) == INVALID
    assert lib.rfa_freq_synchronize(None) == INVALID
    v = ctypes.c_int32(9)
    d = (ctypes.c_double * 2)(9.0, 9.0)
    t = (ctypes.c_int64 * 2)(9, 9)
    assert lib.rfa_freq_get_channels(None, ctypes.byref(v)) == INVALID
    assert lib.rfa_freq_break(None, 0) == INVALID and lib.rfa_freq_break(None, -1) == INVALID
    assert lib.rfa_freq_reset(None) == INVALID
    assert lib.rfa_freq_process(None, None, None, 0, 0) == INVALID
    assert lib.rfa_freq_collect(None, d, d, t) == INVALID
    assert lib.rfa_freq_process_host(None, None, None, 0, 0, d, d, t) == INVALID
    assert (v.value, list(d), list(t)) == (9, [9.0, 9.0], [9, 9])


def test_meter_bank_sits_on_the_handle_base():
    from rfanalyzer_amd import demod
    assert issubclass(demod.FrequencyMeterBank, demod._Handle) and demod.FrequencyMeterBank._prefix == "rfa_freq"
    for name in ("close", "set_stream", "synchronize", "stream", "__enter__", "__exit__", "__del__", "_call"):
        assert name not in vars(demod.FrequencyMeterBank), name
    for name in ("process_device", "collect", "process", "process_tensor", "break_", "reset"):
        assert name in vars(demod.FrequencyMeterBank), name
    assert callable(demod.frequency_error_hz)


# ------------------------------------------------------------------ the chains' keyword without a device

def test_afc_is_a_keyword_of_the_chains_that_can_tune():
    from rfanalyzer_amd import demod
    for cls in (demod.ReceiverBank, demod.TunedReceiverBank, demod.RasterReceiverBank):
        p = inspect.signature(cls.__init__).parameters["afc"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None
    for name in ("frequency_errors", "corrections"):
        assert isinstance(vars(demod._BankChain)[name], property)
    assert "meter" not in vars(demod._BankChain)            # no meter attribute unless a chain asks for AFC


def test_afc_keyword_is_checked_before_any_handle_is_made():
    """These raise on a machine with a device and on one without, before a handle exists."""
    from rfanalyzer_amd import demod
    fs, spacing = 2_400_000, 25_000
    for afc in (True, {}, {"interval": 2}):
        with pytest.raises(ValueError, match="cannot tune"):
            demod.RasterReceiverBank("u8", fs, spacing, ["nfm"] * 2, afc=afc)
    for make in (lambda **kw: demod.ReceiverBank("u8", fs, ["nfm", "am"], **kw),
                 lambda **kw: demod.TunedReceiverBank("u8", fs, spacing, ["nfm", "am"], **kw)):
        with pytest.raises(TypeError):
            make(afc="yes")
        with pytest.raises(TypeError):
            make(afc=[1, 2])
        with pytest.raises(TypeError):
            make(afc={"no_such_keyword": 1})
        for bad in ({"interval": 0}, {"step_hz": -25}, {"gain": 2.0}, {"limit_hz": [1.0, 2.0, 3.0]}):
            with pytest.raises(ValueError):
                make(afc=bad)


def test_afc_rule_of_a_chain_defaults_to_half_the_modes_default_width():
    from rfanalyzer_amd import demod
    modes = ["am", "nfm", "usb", "lsb"]
    rule, defaulted = demod._afc_rule(True, modes, 96000)
    assert defaulted and list(rule.limit_hz) == [demod.mode_info(m)[3] / 2 for m in modes] == [4000, 5000, 1400, 1400]
    assert (rule.step_hz, rule.interval, rule.gain, rule.rate) == (25.0, 8, 1.0, 96000.0)
    rule, defaulted = demod._afc_rule({"limit_hz": 300, "interval": 2}, modes, 96000)
    assert not defaulted and list(rule.limit_hz) == [300.0] * 4 and rule.interval == 2
    assert demod._afc_rule(None, modes, 96000) == (None, False) == demod._afc_rule(False, modes, 96000)
    assert [m for m in demod.MODES if demod.MODES[m] in demod._AFC_MODE_IDS] == ["am", "nfm", "wfm"]


def test_valid_afc_without_a_device_fails_at_the_device():
    import torch
    if torch.cuda.is_available():
        return                                              # with a device tests/test_gpu_freq.py builds these chains
    from rfanalyzer_amd import _lib, demod
    with pytest.raises(_lib.RfaError) as e:
        demod.ReceiverBank("u8", 2_400_000, ["nfm"] * 2, afc={"interval": 2})
    assert e.value.status == NODEVICE


def test_host_check_program_passes_under_sanitizers(lib):
    """tools/freq_host_check: freq.hip's host side built with -fsanitize=address,undefined into a
    stand-alone program that walks the host-only entry and the error paths."""
    exe = os.path.join(ROOT, "tools", "freq_host_check")
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tools"), exe], capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "freq_host_check ok" in r.stdout
