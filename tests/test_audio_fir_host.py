"""CPU: the host-only side of the audio FIR bank -- the restatement (tests/audio_fir_ref.py) against a
literal per-sample loop, demod.voice_taps against an independent float64 design, rfa_audio_fir_plan and
the case table of the device tests, the argument checks of rfa_audio_fir_* that come before the device
is looked for, the chains' ``audio_filter`` keyword without a device, the prototypes and constants of
_lib.py against the header, and tools/audio_fir_host_check (the same host paths under ASan + UBSan)."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import audio_fir_paths as paths
import audio_fir_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, NODEVICE = -1, -4
RATE = 48000


@pytest.fixture(scope="module")
def lib():
    import rfanalyzer_amd
    rfanalyzer_amd.build()
    return rfanalyzer_amd.lib()


# ------------------------------------------------------------------ the restatement

@pytest.mark.parametrize("t", [1, 2, 3, 7, 64, 65])
def test_restatement_equals_the_literal_loop(t):
    x = ref.rows(1, 300, seed=t)[0]
    taps = ref.taps_of(t)
    hist = ref.rows(1, ref.H, seed=100 + t)[0]
    y, after = ref.fir(taps, x, hist)
    assert y.dtype == np.float32 and ref.bits_equal(y, ref.fir_literal(taps, x, hist))
    assert ref.bits_equal(after, np.concatenate([hist, x])[-ref.H:])
    # zeros before the first call, and a row cut anywhere gives the row given whole
    whole, _ = ref.fir(taps, x)
    assert ref.bits_equal(whole, ref.fir_literal(taps, x))
    s = ref.Slot(taps)
    cut = np.concatenate([s.process(x[:1]), s.process(x[1:t + 1]), s.process(x[t + 1:])])
    assert ref.bits_equal(cut, whole)


def test_restatement_order_of_the_sum_and_special_values():
    # (0 + t0 x[i]) + t1 x[i-1]: the first product is added to +0.0, so -0.0 reads +0.0
    y, _ = ref.fir([1.0, 1.0], np.array([-0.0, -0.0], np.float32))
    assert not np.signbit(y).any()
    # the order is visible: 1e8 + 1 - 1e8 in float32 is 0 one way and 1 the other
    x = np.array([1.0, 1.0, 1.0], np.float32)
    assert ref.fir([-1e8, 1.0, 1e8], x)[0][2] == 0.0 and ref.fir([1e8, -1e8, 1.0], x)[0][2] == 1.0
    # a NaN reaches the T outputs it is a term of
    x = ref.rows(1, 40)[0].copy()
    x[10] = np.nan
    y, _ = ref.fir(ref.taps_of(5), x)
    assert list(np.flatnonzero(np.isnan(y))) == [10, 11, 12, 13, 14]
    # no taps: the bits as they are, NaN payloads included
    odd = np.array([0x7fc00001, 0xffc12345, 0x7f800001, 0x80000000, 0x00000001], np.uint32).view(np.float32)
    y, after = ref.fir([], odd)
    assert ref.bits_equal(y, odd) and ref.bits_equal(after[-5:], odd)


def test_restated_history_is_the_last_4095_inputs_whatever_the_taps():
    x = ref.rows(1, 3 * ref.H + 11)[0]
    s = ref.Slot(ref.taps_of(3))
    s.process(x[:ref.H + 5])
    assert ref.bits_equal(s.hist, x[5:ref.H + 5])
    s.taps = ref.taps_of(4096)
    y = s.process(x[ref.H + 5:])
    assert ref.bits_equal(y[:50], ref.fir(ref.taps_of(4096), x)[0][ref.H + 5:ref.H + 55])


# ------------------------------------------------------------------ voice_taps

def test_voice_taps_shape():
    from rfanalyzer_amd import demod
    t = demod.voice_taps()
    assert t.dtype == np.float32 and t.ndim == 1 and t.size == 1309 and t.size % 2 == 1
    assert np.array_equal(t, t[::-1])
    dc = abs(float(np.sum(t.astype(np.float64))))
    print(f"voice_taps: {t.size} taps, delay {(t.size - 1) / 2 / RATE * 1e3:.2f} ms, |sum| {dc:.3e}")
    assert dc < 1e-5
    # it is the inversion of the low-pass design
    lp = demod.create_low_pass_taps(1.0, 48000.0, 300.0, 100.0, 60.0)
    want = -lp
    want[lp.size // 2] += np.float32(1.0)
    assert np.array_equal(t, want)
    narrow = demod.voice_taps(transition_hz=60.0)
    assert narrow.size == 2181 and np.array_equal(narrow, narrow[::-1])
    assert demod.voice_taps(rate=8000, cutoff_hz=300.0, transition_hz=100.0).size % 2 == 1
    for bad in ({"transition_hz": 10.0}, {"cutoff_hz": 0.0}, {"cutoff_hz": 30000.0}, {"transition_hz": 0.0}):
        with pytest.raises(ValueError):
            demod.voice_taps(**bad)


@pytest.mark.parametrize("transition", [100.0, 60.0])
def test_voice_taps_response_against_an_independent_design(transition):
    """Within 0.5 dB of a float64 Blackman windowed-sinc of the same length wherever that design is above
    -60 dB; below it only <= -55 dB is asked."""
    from rfanalyzer_amd import demod
    t = demod.voice_taps(transition_hz=transition)
    want = ref.highpass_f64(t.size, RATE, 300.0)
    for hz in (150.0, 203.5, 225.7, 254.1, 350.0, 500.0, 3000.0):
        got_db, want_db = ref.response_db(t, hz, RATE), ref.response_db(want, hz, RATE)
        print(f"transition {transition} Hz, {t.size} taps, {hz} Hz: {got_db:.2f} dB (independent design {want_db:.2f} dB)")
        if want_db > -60.0:
            assert abs(got_db - want_db) <= 0.5, hz
        else:
            assert got_db <= -55.0, hz
    print(f"300 Hz: {ref.response_db(t, 300.0, RATE):.2f} dB, 100 Hz: {ref.response_db(t, 100.0, RATE):.2f} dB, "
          f"400 Hz: {ref.response_db(t, 400.0, RATE):.3f} dB")


# ------------------------------------------------------------------ the plan and the case table

def test_plan_paths(lib):
    from rfanalyzer_amd import demod
    T, N = paths.TILE, paths.NARROW_MAX
    assert demod.audio_fir_plan(0, 0)["path"] == "none" and demod.audio_fir_plan(1309, 0)["path"] == "none"
    assert demod.audio_fir_plan(0, 1)["path"] == "copy" and demod.audio_fir_plan(0, 5 * T)["path"] == "copy"
    assert demod.audio_fir_plan(1, 1)["path"] == "narrow" and demod.audio_fir_plan(4096, N)["path"] == "narrow"
    assert demod.audio_fir_plan(1, N + 1)["path"] == "wide" and demod.audio_fir_plan(4096, 1 << 36)["path"] == "wide"
    p = demod.audio_fir_plan(1309, 328)
    assert p == {"tile": T, "lds_bytes": p["lds_bytes"], "path": "narrow", "outputs_per_thread": 2, "workgroups": 1}
    assert 4 * (1309 + 328 + 1308) <= p["lds_bytes"] <= 4 * (1309 + 328 + 1308 + 32)
    p = demod.audio_fir_plan(4096, 2 * T + 17)
    assert (p["path"], p["outputs_per_thread"], p["workgroups"]) == ("wide", 8, 3)
    assert 4 * (4096 + T + 4095) <= p["lds_bytes"] <= 64 * 1024
    assert demod.AudioFilterBank.plan(65, 65) == demod.audio_fir_plan(65, 65)
    out = (ctypes.c_int32 * 5)()
    for t, n in ((-1, 5), (4097, 5), (5, (1 << 36) + 1)):
        assert lib.rfa_audio_fir_plan(t, n, out) == INVALID
    assert lib.rfa_audio_fir_plan(5, 5, None) == INVALID


def test_case_table_reaches_every_path(lib):
    from rfanalyzer_amd import demod
    hit = {}
    for t, n in paths.shapes():
        hit.setdefault(demod.audio_fir_plan(t, n)["path"], []).append((t, n))
    print({k: len(v) for k, v in hit.items()})
    assert set(hit) == set(paths.PATHS)
    # both compute paths with a tap count that is and is not a multiple of their step, and more than one tile
    for path, step in (("narrow", 2), ("wide", 4)):
        assert {t % step for t, _ in hit[path]} >= {0, 1}, path
    assert any(demod.audio_fir_plan(t, n)["workgroups"] > 2 for t, n in hit["wide"])
    assert set(paths.TAP_COUNTS) == {1, 2, 3, 64, 65, 1309, 4096}
    T = paths.TILE
    for t in paths.TAP_COUNTS:
        assert set(paths.counts_for(t)) == {n for n in (0, 1, t - 2, t - 1, t, T - 1, T, T + 1, 2 * T + 17) if n >= 0}
    assert sorted(t for t, _ in paths.MULTI) == [0, 1, 65, 1309, 4096]
    counts = [n for _, n in paths.MULTI]
    assert len(set(counts)) == 5 and 0 in counts


def test_history_source(lib):
    H = ref.H
    frm, idx = ctypes.c_int32(9), ctypes.c_size_t(9)
    for n in (0, 1, H - 1, H, H + 1, 3 * H, 1 << 36):
        for j in (0, 1, H // 2, H - 1):
            assert lib.rfa_audio_fir_history_source(n, j, ctypes.byref(frm), ctypes.byref(idx)) == 0
            at = n + j                                      # the position in (history ++ inputs)
            assert (frm.value, idx.value) == ((1, at - H) if at >= H else (0, at)), (n, j)
    for n, j in ((5, -1), (5, H), ((1 << 36) + 1, 0)):
        assert lib.rfa_audio_fir_history_source(n, j, ctypes.byref(frm), ctypes.byref(idx)) == INVALID


# ------------------------------------------------------------------ _lib.py against the header

_C_SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "size_t": ctypes.c_size_t}
_C_TARGETS = {"int32_t": ctypes.c_int32, "size_t": ctypes.c_size_t, "float": ctypes.c_float,
              "void *": ctypes.c_void_p, "rfa_audio_fir *": ctypes.c_void_p}


def _header():
    with open(os.path.join(ROOT, "include", "rfa.h")) as f:
        return f.read()


def _prototypes():
    """{name: (return type text, [argument type text])} of the header's rfa_audio_fir_* entries."""
    out = {}
    for ret, name, args in re.findall(r"RFA_API\s+([\w\s\*]+?)\s*\b(rfa_audio_fir_\w+)\s*\(([^)]*)\)\s*;", _header()):
        types = []
        for a in args.split(","):
            a = re.sub(r"/\*.*?\*/", "", a).strip()
            m = re.match(r"^(.*?)(\w+)$", a)                # the last word is the argument's name
            types.append(re.sub(r"\s+", " ", m.group(1).replace("const ", "")).strip())
        out[name] = (re.sub(r"\s+", " ", ret.replace("const ", "")).strip(), types)
    return out


def _matches(ctype, text: str) -> bool:
    if text in _C_SCALARS:
        return ctype is _C_SCALARS[text]
    assert text.endswith("*"), text
    if ctype is ctypes.c_void_p:                            # an address: device rows, handles, host arrays by address
        return True
    target = text[:-1].strip()
    return issubclass(ctype, ctypes._Pointer) and ctype._type_ is _C_TARGETS[target]


def test_prototypes_of_the_binding_equal_the_header(lib):
    protos = _prototypes()
    assert len(protos) == 14 and {"rfa_audio_fir_create", "rfa_audio_fir_process", "rfa_audio_fir_plan",
                                  "rfa_audio_fir_set_taps", "rfa_audio_fir_get_taps", "rfa_audio_fir_reset",
                                  "rfa_audio_fir_process_host", "rfa_audio_fir_history_source"} <= set(protos)
    for name, (ret, args) in protos.items():
        fn = getattr(lib, name)                             # exported
        assert fn.argtypes is not None and len(fn.argtypes) == len(args), name
        for i, (ctype, text) in enumerate(zip(fn.argtypes, args)):
            assert _matches(ctype, text), (name, i, text, ctype)
        if ret == "char *":
            assert fn.restype is ctypes.c_char_p, name
        else:
            assert ret == "int" and fn.restype is ctypes.c_int, name


def test_constants_of_the_binding_equal_the_header():
    from rfanalyzer_amd import _lib, demod
    defs = {k: int(v) for k, v in re.findall(r"#define\s+(RFA_AUDIO_FIR_\w+)\s+(\d+)", _header())}
    assert len(defs) == 9
    for name in ("MAX_CHANNELS", "MAX_TAPS", "TILE", "NARROW_MAX", "PLAN_FIELDS"):
        assert getattr(_lib, f"RFA_AUDIO_FIR_{name}") == defs[f"RFA_AUDIO_FIR_{name}"], name
    for i, path in enumerate(_lib.RFA_AUDIO_FIR_PATHS):
        assert defs[f"RFA_AUDIO_FIR_PATH_{path.upper()}"] == i
    assert defs["RFA_AUDIO_FIR_MAX_TAPS"] == ref.MAX_TAPS == demod.AUDIO_FIR_MAX_TAPS == 4096
    assert defs["RFA_AUDIO_FIR_MAX_CHANNELS"] == 1024 and defs["RFA_AUDIO_FIR_TILE"] == paths.TILE
    assert len(demod.AUDIO_FIR_PLAN_FIELDS) == defs["RFA_AUDIO_FIR_PLAN_FIELDS"]


# ------------------------------------------------------------------ the library without a device

def _create(lib, n_channels):
    h = ctypes.c_void_p(1)
    rc = lib.rfa_audio_fir_create(0, n_channels, ctypes.byref(h))
    if rc == 0:
        lib.rfa_audio_fir_destroy(h)
    return rc, h.value


def test_argument_errors_come_before_the_device(lib):
    assert lib.rfa_audio_fir_create(0, 4, None) == INVALID
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
    v = ctypes.c_int32(9)
    x = (ctypes.c_float * 4)(9, 9, 9, 9)
    n = (ctypes.c_size_t * 1)(2)
    assert lib.rfa_audio_fir_destroy(None) == INVALID
    assert lib.rfa_audio_fir_last_error(None) == b"null handle"
    assert lib.rfa_audio_fir_set_stream(None, None) == INVALID
    assert lib.rfa_audio_fir_get_stream(None, ctypes.byref(s)) == INVALID
    assert lib.rfa_audio_fir_synchronize(None) == INVALID
    assert lib.rfa_audio_fir_get_channels(None, ctypes.byref(v)) == INVALID
    assert lib.rfa_audio_fir_set_taps(None, 0, x, 4) == INVALID
    assert lib.rfa_audio_fir_get_taps(None, 0, x, 4, ctypes.byref(v)) == INVALID
    assert lib.rfa_audio_fir_reset(None, -1) == INVALID
    assert lib.rfa_audio_fir_process(None, None, 0, n, None, 0) == INVALID
    assert lib.rfa_audio_fir_process_host(None, None, 0, n, None, 0) == INVALID
    assert (v.value, list(x)) == (9, [9.0] * 4)


def test_filter_bank_sits_on_the_handle_base():
    from rfanalyzer_amd import demod
    assert issubclass(demod.AudioFilterBank, demod._Handle) and demod.AudioFilterBank._prefix == "rfa_audio_fir"
    for name in ("close", "set_stream", "synchronize", "stream", "__enter__", "__exit__", "__del__", "_call"):
        assert name not in vars(demod.AudioFilterBank), name
    for name in ("set_taps", "taps", "reset", "process_device", "process_tensor", "process", "plan"):
        assert name in vars(demod.AudioFilterBank), name


# ------------------------------------------------------------------ the chains' keyword without a device

def test_audio_filter_is_a_keyword_of_every_bank_chain():
    from rfanalyzer_amd import demod
    for cls in (demod.ReceiverBank, demod.TunedReceiverBank, demod.RasterReceiverBank):
        p = inspect.signature(cls.__init__).parameters["audio_filter"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None
    for name in ("audio_counts", "audio_tensor"):
        assert isinstance(vars(demod._BankChain)[name], property)
    assert "set_audio_filter" in vars(demod._BankChain)
    assert "audio_fir" not in vars(demod._BankChain)         # no handle attribute unless a chain asks for filters
    assert "audio_filter" not in inspect.signature(demod.Receiver.__init__).parameters


def test_audio_filter_keyword_is_checked_before_any_handle_is_made():
    """These raise on a machine with a device and on one without, before a handle exists."""
    from rfanalyzer_amd import demod
    fs, spacing = 2_400_000, 25_000
    for make in (lambda **kw: demod.ReceiverBank("u8", fs, ["nfm", "am"], **kw),
                 lambda **kw: demod.TunedReceiverBank("u8", fs, spacing, ["nfm", "am"], **kw),
                 lambda **kw: demod.RasterReceiverBank("u8", fs, spacing, ["nfm", "am"], **kw)):
        for bad in (True, "voice", 300.0, 3,                                   # not one entry per slot
                    ["voice"], ["voice", None, None], [],                     # a wrong entry count
                    ["voice", "bass"], [True, None], [300.0, None], [7, None],   # a wrong entry type
                    [np.zeros((2, 3), np.float32), None], [np.ones(4097, np.float32), None],
                    [[1.0, np.nan], None], [[1.0, np.inf], None], [["a", "b"], None]):
            with pytest.raises(ValueError):
                make(audio_filter=bad)


def test_audio_filter_entries():
    from rfanalyzer_amd import demod
    assert demod._audio_filter_entries(None, 3) is None
    got = demod._audio_filter_entries([None, "voice", [0.5, 0.25], np.array([], np.float32)], 4)
    assert got[0] is None and got[3] is None
    assert np.array_equal(got[1], demod.voice_taps())
    assert got[2].dtype == np.float32 and list(got[2]) == [0.5, 0.25]


def test_valid_audio_filter_without_a_device_fails_at_the_device():
    import torch
    if torch.cuda.is_available():
        return                                              # with a device tests/test_gpu_audio_fir.py builds these chains
    from rfanalyzer_amd import _lib, demod
    with pytest.raises(_lib.RfaError) as e:
        demod.ReceiverBank("u8", 2_400_000, ["nfm"] * 2, audio_filter=["voice", None])
    assert e.value.status == NODEVICE


def test_host_check_program_passes_under_sanitizers(lib):
    """tools/audio_fir_host_check: audio_fir.hip's host side built with -fsanitize=address,undefined into a
    stand-alone program that walks the host-only entries and the error paths."""
    exe = os.path.join(ROOT, "tools", "audio_fir_host_check")
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tools"), exe], capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "audio_fir_host_check ok" in r.stdout
