"""CPU: the host-only side of the audio resampler bank -- the restatement (tests/audio_rs_ref.py) against
the literal nested loops and against float64 within the derived bound, the counts rule against its closed
form, across splits and against rfa_audio_rs_counts, rfa_audio_rs_plan and the case table of the device
tests, the conversion at ties, rails, NaN and infinities and its round trip through the s16 input
conversion, demod.resampler_taps against an independent float64 design, every ValueError and
RFA_ERR_INVALID that comes before the device is looked for, recording.AudioLogWriter, the chains' ``pcm``
keyword without a device, and tools/audio_rs_host_check (the same host paths under ASan + UBSan)."""
import ctypes
import inspect
import os
import re
import subprocess
import wave

import numpy as np
import pytest

import audio_rs_paths as paths
import audio_rs_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, NODEVICE = -1, -4
F32 = np.float32


@pytest.fixture(scope="module")
def lib():
    import rfanalyzer_amd
    rfanalyzer_amd.build()
    return rfanalyzer_amd.lib()


# ------------------------------------------------------------------ the restatement

SMALL = [(1, 1, 5), (1, 2, 9), (1, 6, 20), (2, 3, 1), (2, 3, 7), (2, 3, 8), (5, 7, 3), (147, 160, 100), (147, 640, 300)]


@pytest.mark.parametrize("L,D,T", SMALL)
def test_restatement_equals_the_literal_loops(L, D, T):
    taps = ref.taps_of(T, L)
    x = ref.rows(1, max(300, D), seed=3)[0]
    hist = ref.rows(1, ref.H, seed=4)[0]
    for r in sorted({0, 1 % D, D - 1}):
        for n in (0, 1, D, 97, 300):
            y, r_next, after = ref.resample(L, D, taps, x[:n], r, hist)
            lit = ref.resample_literal(L, D, taps, x[:n], r, hist)
            assert ref.bits_equal(y, lit), (r, n)
            assert (y.size, r_next) == ref.counts(L, D, r, n) and 0 <= r_next < D
            assert ref.bits_equal(after, np.concatenate([hist, x[:n]])[-ref.H:])


@pytest.mark.parametrize("L,D,T", SMALL + [(1, 6, 219), (147, 640, 16384)])
def test_restatement_against_float64_within_the_derived_bound(L, D, T):
    """J products and J sums, each rounded once to float32 (relative 2^-24), and the float32 taps and samples
    themselves exact in both: |y32 - y64| <= (J + 1) 2^-24 sum_j |h_j x_j| per output, to first order."""
    taps = ref.taps_of(T, L)
    x = ref.rows(1, 4000, seed=6)[0]
    y32 = ref.resample(L, D, taps, x)[0]
    y64 = ref.resample(L, D, taps, x, dtype=np.float64)[0]
    J = -(-T // L)
    bound = (J + 1) * 2.0 ** -24 * ref.abs_sum(L, D, taps, x)
    err = np.abs(y32.astype(np.float64) - y64)
    assert y32.size == y64.size == ref.counts(L, D, 0, x.size)[0] and (err <= bound).all(), float((err / bound).max())
    assert err.max() > 0 or J == 1


def test_restatement_order_padding_and_pass_through():
    # the sum starts at +0.0f and runs from the newest sample: (1e8 + 1) - 1e8 in float32 is 0, not 1
    y = ref.resample(1, 1, [1.0, 1.0, -1.0], [1e8, 1.0, 1e8])[0]
    assert y[2] == F32(F32(F32(0.0) + F32(1e8)) + F32(1.0)) - F32(1e8) == 0.0
    # a zero-padded tap is still multiplied and added: 0 * inf is a term
    with np.errstate(invalid="ignore"):
        y = ref.resample(2, 3, [1.0], [1.0, np.inf, 1.0])[0]       # J = 1; phase 1 is padding alone
    assert y.size == 2 and y[0] == 1.0 and np.isnan(y[1])       # u = 3: i = 1, p = 1: +0.0f * inf
    # -0.0 products: +0.0f + -0.0f is +0.0f
    y = ref.resample(1, 1, [1.0], np.array([-0.0], F32))[0]
    assert y.view(np.int32)[0] == 0
    # no taps: the bits, NaN payloads included
    odd = np.array([0x7fc00001, 0xffc12345, 0x7f800000, 0x80000000, 0x00000001], np.uint32).view(F32)
    y, r, _ = ref.resample(1, 1, [], odd)
    assert ref.bits_equal(y, odd) and r == 0


# ------------------------------------------------------------------ the counts rule

RATIOS = sorted({(L, D) for L, D, _ in paths.CASES} | {(1, 1024), (160, 1023), (159, 160), (1, 7)})


@pytest.mark.parametrize("L,D", RATIOS)
def test_counts_rule_closed_form_splits_and_the_library(lib, L, D):
    rng = np.random.Generator(np.random.PCG64(L * 2000 + D))
    n_out, r_next = ctypes.c_size_t(0), ctypes.c_int32(0)
    for n in [0, 1, 2, D - 1, D, D + 1, 12345, 2 ** 31 + 11, 2 ** 36 - 1, 2 ** 36]:
        for r in sorted({0, D // 2, D - 1}):
            got = ref.counts(L, D, r, n)
            # the rule in its own words: outputs while r + m D < n L
            m = got[0]
            assert (m == 0 or r + (m - 1) * D < n * L) and r + m * D >= n * L and 0 <= got[1] < D
            assert got[0] == ((n * L - r + D - 1) // D if n * L > r else 0)
            assert lib.rfa_audio_rs_counts(L, D, r, n, ctypes.byref(n_out), ctypes.byref(r_next)) == 0
            assert (n_out.value, r_next.value) == got, (n, r)
        assert lib.rfa_audio_rs_max_outputs(L, D, n) == -(-n * L // D) == ref.counts(L, D, 0, n)[0]
    for total in (1000, 2 ** 36):
        whole = ref.counts(L, D, 0, total)
        for _ in range(5):
            cuts = np.sort(rng.integers(0, total + 1, 6))
            r, outs = 0, 0
            for n in np.diff(np.concatenate([[0], cuts, [total]])):
                assert lib.rfa_audio_rs_counts(L, D, r, int(n), ctypes.byref(n_out), ctypes.byref(r_next)) == 0
                assert (n_out.value, r_next.value) == ref.counts(L, D, r, int(n))
                r, outs = r_next.value, outs + n_out.value
            assert (outs, r) == whole


def test_counts_and_plan_argument_errors(lib):
    n_out, r_next = ctypes.c_size_t(77), ctypes.c_int32(77)
    plan = (ctypes.c_int32 * 5)(*[-9] * 5)
    bad_ratios = [(0, 1), (-1, 6), (161, 640), (2, 1), (1, 1025), (2, 4), (147, 147), (6, 9), (2 ** 31 - 1, 2 ** 31 - 1)]
    for L, D in bad_ratios:
        assert lib.rfa_audio_rs_counts(L, D, 0, 10, ctypes.byref(n_out), ctypes.byref(r_next)) == INVALID, (L, D)
        assert lib.rfa_audio_rs_max_outputs(L, D, 10) == 0
        assert lib.rfa_audio_rs_plan(L, D, 4, 10, plan) == INVALID
    for r in (-1, 6, 2 ** 31 - 1):
        assert lib.rfa_audio_rs_counts(1, 6, r, 10, ctypes.byref(n_out), ctypes.byref(r_next)) == INVALID
    assert lib.rfa_audio_rs_counts(1, 6, 0, 2 ** 36 + 1, ctypes.byref(n_out), ctypes.byref(r_next)) == INVALID
    assert lib.rfa_audio_rs_counts(1, 6, 0, 10, None, ctypes.byref(r_next)) == INVALID
    assert lib.rfa_audio_rs_counts(1, 6, 0, 10, ctypes.byref(n_out), None) == INVALID
    assert lib.rfa_audio_rs_max_outputs(1, 6, 2 ** 36 + 1) == 0
    for L, D, T in [(1, 6, 0), (2, 3, 0), (1, 1, -1), (1, 6, 4097), (2, 3, 8193), (147, 640, 16385), (1, 1, 2 ** 31 - 1)]:
        assert lib.rfa_audio_rs_plan(L, D, T, 10, plan) == INVALID, (L, D, T)
    assert lib.rfa_audio_rs_plan(1, 6, 4, 2 ** 36 + 1, plan) == INVALID
    assert lib.rfa_audio_rs_plan(1, 6, 4, 10, None) == INVALID
    assert (n_out.value, r_next.value, list(plan)) == (77, 77, [-9] * 5)
    assert lib.rfa_audio_rs_plan(1, 6, 4096, 10, plan) == 0 and lib.rfa_audio_rs_plan(2, 3, 8192, 10, plan) == 0


# ------------------------------------------------------------------ the plan and the case table

def test_plan_fields(lib):
    from rfanalyzer_amd import _lib, demod
    for L, D, T in paths.CASES + ((1, 1024, 4096), (1, 1024, 1), (160, 1023, 16384), (2, 1023, 8192)):
        tile = demod.audio_rs_plan(L, D, T, 1)["tile"]
        assert 1 <= tile <= _lib.RFA_AUDIO_RS_MAX_TILE and tile & (tile - 1) == 0
        for n in (0, 1, D, paths.tile_inputs(L, D, T), paths.tile_inputs(L, D, T) + D, 2 ** 36):
            p = demod.audio_rs_plan(L, D, T, n)
            n_out = -(-n * L // D)
            assert p["tile"] == tile and p["path"] == ("none" if n == 0 else paths.path_of(L, T))
            assert p["workgroups"] == min(-(-n_out // tile), 2 ** 31 - 1)
            assert p["outputs_per_thread"] * 256 >= min(n_out, tile) and (p["outputs_per_thread"] == 0) == (n == 0)
            J = -(-T // L)
            if n == 0 or T == 0:
                assert p["lds_bytes"] == 0
            else:
                # the taps of every phase, and the tile's inputs with J - 1 before them
                span = ((L - 1) + (tile - 1) * D) // L + J
                assert p["lds_bytes"] % 16 == 0 and p["lds_bytes"] >= 4 * (L * J + span)
                assert p["lds_bytes"] <= 160 * 1024                  # a CU's LDS
    # the tile shrinks where its inputs would not fit, and only there
    assert demod.audio_rs_plan(1, 6, 219, 1)["tile"] == 1024 and demod.audio_rs_plan(1, 1024, 4096, 1)["tile"] < 64
    assert demod.audio_rs_plan(147, 640, 16384, 1)["lds_bytes"] > 64 * 1024


def test_case_table_reaches_every_path(lib):
    from rfanalyzer_amd import demod
    seen = {}
    for L, D, T, n in paths.shapes():
        seen.setdefault(demod.audio_rs_plan(L, D, T, n)["path"], []).append((L, D, T, n))
    assert set(seen) == set(paths.PATHS), sorted(seen)
    per_thread = {demod.audio_rs_plan(L, D, T, n)["outputs_per_thread"] for L, D, T, n in paths.shapes()}
    assert per_thread == {0, 1, 2, 4}                        # every dispatch of the tile body
    # what the issue asks of the table
    assert any(T == 0 for _, _, T in paths.CASES) and any(T < L for L, _, T in paths.CASES)
    assert any(T % L and T > L for L, _, T in paths.CASES) and any(T % L == 0 and T and L > 1 for L, _, T in paths.CASES)
    assert (1, 2, 4096) in paths.CASES and (147, 640, 16384) in paths.CASES
    assert {(L, D) for L, D, _ in paths.CASES} == {(1, 1), (1, 2), (1, 3), (1, 6), (2, 3), (147, 160), (147, 640)}
    for L, D, T in paths.CASES:
        t = paths.tile_inputs(L, D, T)
        assert {0, 1, D - 1, D, D + 1, t - 1, t, t + 1} <= set(paths.counts_for(L, D, T))
        assert demod.audio_rs_plan(L, D, T, max(paths.counts_for(L, D, T)))["workgroups"] == 3
    assert all(0 in counts and len(counts) == 5 for _, counts in paths.MULTI)


# ------------------------------------------------------------------ the conversion

def test_conversion_at_ties_rails_nan_and_infinities():
    k = np.arange(-32767, 32767)
    ties = ((k + 0.5) / 32768.0).astype(F32)                 # exact in float32
    assert np.array_equal(ties.astype(np.float64) * 32768.0, k + 0.5)
    want = np.where(k % 2 == 0, k, k + 1)                    # k + 0.5 to the even neighbour
    want = np.clip(want, -32768, 32767)
    assert np.array_equal(ref.pcm(ties), want.astype(np.int16))
    assert list(ref.pcm(np.array([0.5, 1.5, 2.5, -0.5, -1.5, -2.5], F32) / F32(32768.0))) == [0, 2, 2, 0, -2, -2]
    one = F32(1.0)
    cases = [(one, 32767), (-one, -32768), (F32(32767.0 / 32768.0), 32767), (F32(32766.5 / 32768.0), 32766),
             (F32(32766.75 / 32768.0), 32767), (F32(-32767.5 / 32768.0), -32768), (F32(-32767.25 / 32768.0), -32767),
             (F32(1.5), 32767), (F32(-1.5), -32768), (F32(3e38), 32767), (F32(-3e38), -32768),
             (F32(np.inf), 32767), (F32(-np.inf), -32768), (F32(np.nan), 0), (F32(0.0), 0), (F32(-0.0), 0),
             (np.array([0xffc00001], np.uint32).view(F32)[0], 0), (F32(1e-30), 0)]
    got = ref.pcm(np.array([c[0] for c in cases], F32))
    assert list(got) == [c[1] for c in cases]


def test_pcm_read_back_through_the_s16_conversion_is_exactly_q_over_32768():
    from oracle import demod as odemod
    q = np.arange(-32768, 32768).astype(np.int16)
    values, also = odemod.lut(odemod.IN_S16LE, np.repeat(q, 2).astype("<i2").tobytes())
    assert values.dtype == F32 and values.size == q.size and np.array_equal(values, also)
    assert np.array_equal(values.astype(np.float64), q.astype(np.float64) / 32768.0)
    assert np.array_equal(ref.pcm(values)[1:], q[1:]) and ref.pcm(values)[0] == -32768


# ------------------------------------------------------------------ the design

@pytest.mark.parametrize("out_rate", [8000, 16000])
def test_resampler_taps_against_an_independent_design(out_rate):
    """The voice filter's criterion: within 0.5 dB of a float64 Blackman windowed-sinc of the same length
    and edges wherever that design is above -60 dB."""
    from rfanalyzer_amd import demod
    L, D, taps = demod.resampler_taps(48000, out_rate)
    assert (L, D) == (1, 48000 // out_rate) and taps.dtype == F32 and taps.size % 2 == 1
    stop = out_rate / 2.0
    cutoff = stop - 0.15 * stop / 2.0
    mine = ref.lowpass_f64(taps.size, 48000.0 * L, cutoff, float(L))
    rows = []
    for hz in np.concatenate([np.arange(0.0, 24000.0, 50.0), [0.85 * stop, cutoff, stop]]):
        a, b = ref.response_db(taps, hz, 48000.0 * L), ref.response_db(mine, hz, 48000.0 * L)
        rows.append((hz, a, b))
        if b > -60.0:
            assert abs(a - b) <= 0.5, (hz, a, b)
    print(f"{out_rate} Hz: {taps.size} taps; " + "; ".join(
        f"{hz:.0f} Hz {ref.response_db(taps, hz, 48000.0 * L):.2f} dB"
        for hz in (0.0, 1000.0, 0.85 * stop, cutoff, stop, stop + 1000.0, 2 * stop)))
    assert abs(ref.response_db(taps, 0.0, 48000.0)) < 0.01                   # gain L = 1
    # the reference's design puts its -6 dB point at the cutoff, the middle of the transition band: the
    # stopband edge itself is at about -23 dB and the asked-for attenuation is reached one band further on
    assert all(a < -60.0 for hz, a, _ in rows if hz >= stop + 0.15 * stop)


def test_resampler_taps_ratios_and_limits():
    from rfanalyzer_amd import demod
    assert demod.resampler_taps()[:2] == (1, 6) and demod.resampler_taps()[2].size == 219
    assert demod.resampler_taps(48000, 16000)[:2] == (1, 3)
    assert demod.resampler_taps(48000, 32000)[:2] == (2, 3)
    L, D, taps = demod.resampler_taps(48000, 11025, transition_hz=2000.0)
    assert (L, D) == (147, 640) and taps.size <= 16384 and abs(ref.response_db(taps, 0.0, 1.0) - 20 * np.log10(147)) < 0.01
    narrow = demod.resampler_taps(48000, 8000, transition_hz=300.0)[2]
    assert narrow.size > demod.resampler_taps()[2].size
    for args, word in [((48000, 11025), "16384"),                           # 23273 taps at the default transition
                       ((48000, 96000), "no up-sampling"), ((48000, 7999), "160"), ((48000, 48000 // 1025), "1024"),
                       ((48000, 8000, 26.0), "per phase, above 4096"),      # about 5000 taps at L = 1
                       ((0, 8000), "positive"), ((48000, 0), "positive"), ((48000, 8000, 0.0), "transition"),
                       ((48000, 8000, 4000.0), "transition"), ((48000, 8000, float("nan")), "transition")]:
        with pytest.raises(ValueError, match=re.escape(word)):
            demod.resampler_taps(*args)


# ------------------------------------------------------------------ the library without a device

def _create(lib, k, L, D, taps):
    h = ctypes.c_void_p(1)
    arr = None if taps is None else (ctypes.c_float * max(len(taps), 1))(*taps)
    rc = lib.rfa_audio_rs_create(0, k, L, D, arr, 0 if taps is None else len(taps), ctypes.byref(h))
    if rc == 0:
        lib.rfa_audio_rs_destroy(h)
    return rc, h.value


def test_argument_errors_come_before_the_device(lib):
    ok = [0.5] * 7
    assert lib.rfa_audio_rs_create(0, 4, 1, 6, (ctypes.c_float * 7)(*ok), 7, None) == INVALID
    for k in (0, -1, 1025, -2 ** 31, 2 ** 31 - 1):
        assert _create(lib, k, 1, 6, ok) == (INVALID, None), k
    for L, D in [(0, 1), (-1, 6), (161, 640), (2, 1), (1, 1025), (2, 4), (147, 147), (6, 9)]:
        assert _create(lib, 4, L, D, ok) == (INVALID, None), (L, D)
    assert _create(lib, 4, 1, 6, []) == (INVALID, None)                      # no taps, and not 1 / 1
    assert _create(lib, 4, 2, 3, None) == (INVALID, None)
    assert _create(lib, 4, 1, 6, [0.1] * 4097) == (INVALID, None)            # J above 4096
    assert _create(lib, 4, 147, 640, [0.1] * 16385) == (INVALID, None)       # T above 16384
    h = ctypes.c_void_p(1)
    assert lib.rfa_audio_rs_create(0, 4, 1, 6, None, 7, ctypes.byref(h)) == INVALID and h.value is None
    assert lib.rfa_audio_rs_create(0, 4, 1, 6, (ctypes.c_float * 7)(*ok), -1, ctypes.byref(h)) == INVALID
    for bad in (float("nan"), float("inf"), float("-inf")):
        assert _create(lib, 4, 1, 6, [0.5, bad, 0.25]) == (INVALID, None)


def test_valid_request_without_a_device_is_nodevice(lib):
    import torch
    for k, L, D, taps in [(1, 1, 1, None), (32, 1, 6, [0.5] * 219), (1024, 147, 640, [0.001] * 16384), (2, 1, 2, [0.1] * 4096)]:
        rc, h = _create(lib, k, L, D, taps)
        if not torch.cuda.is_available():
            assert (rc, h) == (NODEVICE, None)
        else:
            assert rc == 0


def test_null_handle_answers(lib):
    s = ctypes.c_void_p(0)
    v, w = ctypes.c_int32(9), ctypes.c_int32(9)
    x = (ctypes.c_float * 4)(9, 9, 9, 9)
    n = (ctypes.c_size_t * 1)(2)
    assert lib.rfa_audio_rs_destroy(None) == INVALID
    assert lib.rfa_audio_rs_last_error(None) == b"null handle"
    assert lib.rfa_audio_rs_set_stream(None, None) == INVALID
    assert lib.rfa_audio_rs_get_stream(None, ctypes.byref(s)) == INVALID
    assert lib.rfa_audio_rs_synchronize(None) == INVALID
    assert lib.rfa_audio_rs_get_channels(None, ctypes.byref(v)) == INVALID
    assert lib.rfa_audio_rs_get_ratio(None, ctypes.byref(v), ctypes.byref(w)) == INVALID
    assert lib.rfa_audio_rs_get_taps(None, x, 4, ctypes.byref(v)) == INVALID
    assert lib.rfa_audio_rs_get_offset(None, 0, ctypes.byref(v)) == INVALID
    assert lib.rfa_audio_rs_reset(None, -1) == INVALID
    assert lib.rfa_audio_rs_process(None, None, 0, n, None, 0, None, 0, None) == INVALID
    assert lib.rfa_audio_rs_process_host(None, None, 0, n, None, 0, None, 0, None) == INVALID
    assert (v.value, w.value, list(x)) == (9, 9, [9.0] * 4)


def test_constants_of_the_binding_equal_the_header():
    from rfanalyzer_amd import _lib, demod
    text = open(os.path.join(ROOT, "include", "rfa.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"#define\s+(RFA_AUDIO_RS_\w+)\s+(\d+)", text)}
    assert len(defs) == 12
    for name in ("MAX_CHANNELS", "MAX_L", "MAX_D", "MAX_TAPS", "MAX_PHASE_TAPS", "HISTORY", "MAX_TILE", "PLAN_FIELDS"):
        assert getattr(_lib, f"RFA_AUDIO_RS_{name}") == defs[f"RFA_AUDIO_RS_{name}"], name
    for i, path in enumerate(_lib.RFA_AUDIO_RS_PATHS):
        assert defs[f"RFA_AUDIO_RS_PATH_{path.upper()}"] == i
    assert tuple(_lib.RFA_AUDIO_RS_PATHS) == paths.PATHS
    assert (defs["RFA_AUDIO_RS_MAX_L"], defs["RFA_AUDIO_RS_MAX_D"], defs["RFA_AUDIO_RS_MAX_TAPS"]) == (160, 1024, 16384)
    assert defs["RFA_AUDIO_RS_HISTORY"] == ref.H == defs["RFA_AUDIO_RS_MAX_PHASE_TAPS"] - 1 == 4095
    assert len(demod.AUDIO_RS_PLAN_FIELDS) == defs["RFA_AUDIO_RS_PLAN_FIELDS"]
    declared = set(re.findall(r"\b(rfa_audio_rs_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    assert len(declared) == 16 and all(getattr(_lib.lib(), name).argtypes is not None for name in declared)


def test_resampler_bank_sits_on_the_handle_base_and_checks_before_the_device():
    from rfanalyzer_amd import demod
    cls = demod.AudioResamplerBank
    assert issubclass(cls, demod._Handle) and cls._prefix == "rfa_audio_rs"
    for name in ("close", "set_stream", "synchronize", "stream", "__enter__", "__exit__", "__del__", "_call"):
        assert name not in vars(cls), name
    for name in ("for_rates", "process", "process_tensor", "process_device", "reset", "offset", "ratio", "taps",
                 "max_outputs", "plan"):
        assert name in vars(cls), name
    for args, word in [((2, 0, 1, [1.0]), "L = 0"), ((2, 161, 640, [1.0]), "160"), ((2, 1, 1025, [1.0]), "1024"),
                       ((2, 3, 2, [1.0]), "no up-sampling"), ((2, 2, 4, [1.0]), "not reduced"),
                       ((2, 1, 6, []), "no taps"), ((2, 1, 6, None), "no taps"), ((2, 1, 6, np.ones(4097)), "4096"),
                       ((2, 147, 640, np.ones(16385)), "16384"), ((2, 1, 6, np.ones((2, 2))), "1-D"),
                       ((2, 1, 6, [1.0, np.nan]), "finite"), ((2, 1, 6, [np.inf]), "finite")]:
        with pytest.raises(ValueError, match=re.escape(word)):
            cls(*args)
    with pytest.raises(ValueError, match="16384"):
        cls.for_rates(2, 11025)


# ------------------------------------------------------------------ the audio log

def test_audio_log_writer_round_trip(tmp_path):
    from rfanalyzer_amd import recording
    rng = np.random.Generator(np.random.PCG64(9))
    calls = [[rng.integers(-32768, 32768, n).astype(np.int16) for n in ns] for ns in ((55, 0, 54), (0, 0, 55), (54, 0, 1))]
    with recording.AudioLogWriter(str(tmp_path / "log"), ["a", "b", "c"], 8000) as log:
        for arrays in calls:
            log.write(arrays)
        with pytest.raises(ValueError):
            log.write(calls[0][:2])
        with pytest.raises(ValueError):
            log.write([a.astype(np.int32) for a in calls[0]])
        done = log.close()
    assert log.close() == done                               # closing twice is harmless
    assert list(done) == ["a", "b", "c"]
    for k, name in enumerate("abc"):
        path, count = done[name]
        want = np.concatenate([c[k] for c in calls])
        assert path == str(tmp_path / "log" / f"{name}.wav") and count == want.size
        with wave.open(path, "rb") as w:
            assert (w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()) == (1, 2, 8000, want.size)
            assert np.array_equal(np.frombuffer(w.readframes(want.size), "<i2"), want)
    with pytest.raises(ValueError):
        log.write(calls[0])                                  # closed
    for names in ([], ["a", "a"], ["a/b"], [""], [".."]):
        with pytest.raises(ValueError):
            recording.AudioLogWriter(str(tmp_path / "bad"), names, 8000)
    for rate in (0, 8000.5, -1):
        with pytest.raises(ValueError):
            recording.AudioLogWriter(str(tmp_path / "bad"), ["a"], rate)


# ------------------------------------------------------------------ the chains' keyword without a device

def test_pcm_is_a_keyword_of_every_bank_chain():
    from rfanalyzer_amd import demod
    for cls in (demod.ReceiverBank, demod.TunedReceiverBank, demod.RasterReceiverBank):
        p = inspect.signature(cls.__init__).parameters["pcm"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None
    for name in ("pcm_counts", "pcm_tensor"):
        assert isinstance(vars(demod._BankChain)[name], property)
    assert "pcm" in vars(demod._BankChain) and "audio_rs" not in vars(demod._BankChain)
    assert "pcm" not in inspect.signature(demod.Receiver.__init__).parameters


def test_pcm_entries():
    from rfanalyzer_amd import demod
    assert demod._pcm_entry(None) is None
    for entry in (8000, np.int64(8000), {"out_rate": 8000}, {"out_rate": 8000, "in_rate": 48000}):
        L, D, taps = demod._pcm_entry(entry)
        assert (L, D) == (1, 6) and np.array_equal(taps, demod.resampler_taps()[2])
    L, D, taps = demod._pcm_entry({"out_rate": 16000, "transition_hz": 2000.0, "attenuation_db": 50.0})
    assert (L, D) == (1, 3) and np.array_equal(taps, demod.resampler_taps(48000, 16000, 2000.0, 50.0)[2])
    L, D, taps = demod._pcm_entry({"L": 2, "D": 3, "taps": [0.5, 0.25, 0.125]})
    assert (L, D) == (2, 3) and taps.dtype == F32 and list(taps) == [0.5, 0.25, 0.125]
    assert demod._pcm_entry({"L": 1, "D": 1, "taps": None})[2].size == 0


def test_pcm_keyword_is_checked_before_any_handle_is_made():
    """These raise on a machine with a device and on one without, before a handle exists."""
    from rfanalyzer_amd import demod
    fs, spacing = 2_400_000, 25_000
    for make in (lambda **kw: demod.ReceiverBank("u8", fs, ["nfm", "am"], **kw),
                 lambda **kw: demod.TunedReceiverBank("u8", fs, spacing, ["nfm", "am"], **kw),
                 lambda **kw: demod.RasterReceiverBank("u8", fs, spacing, ["nfm", "am"], **kw)):
        for bad in (True, False, "8000", 8000.0, [8000, 8000], 0, -8000, 96000, 11025, 7999,
                    {}, {"rate": 8000}, {"out_rate": 8000, "bass": 1}, {"out_rate": 8000, "in_rate": 44100},
                    {"out_rate": 8000, "transition_hz": 0.0}, {"L": 1, "D": 6}, {"L": 1, "D": 6, "taps": [1.0], "out_rate": 8000},
                    {"L": 2, "D": 4, "taps": [1.0]}, {"L": 1, "D": 6, "taps": []}, {"L": 1, "D": 6, "taps": [np.nan]},
                    {"L": 1, "D": 6, "taps": np.ones((2, 2))}, {"L": 1, "D": 6, "taps": np.ones(4097)}):
            with pytest.raises(ValueError):
                make(pcm=bad)


def test_valid_pcm_without_a_device_fails_at_the_device():
    import torch
    if torch.cuda.is_available():
        return                                              # with a device tests/test_gpu_audio_rs.py builds these chains
    from rfanalyzer_amd import _lib, demod
    with pytest.raises(_lib.RfaError) as e:
        demod.ReceiverBank("u8", 2_400_000, ["nfm"] * 2, pcm=8000)
    assert e.value.status == NODEVICE


def test_host_check_program_passes_under_sanitizers(lib):
    """tools/audio_rs_host_check: audio_rs.hip's host side built with -fsanitize=address,undefined into a
    stand-alone program that walks the counts rule, the plan and the error paths."""
    exe = os.path.join(ROOT, "tools", "audio_rs_host_check")
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tools"), exe], capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "audio_rs_host_check ok" in r.stdout
