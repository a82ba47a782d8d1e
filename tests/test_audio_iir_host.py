"""CPU: the host-only side of the audio IIR bank -- the library's tables against the restatement
(tests/audio_iir_ref.py), the restatement's cut invariance and its accuracy against a float64 recurrence
next to a plain sequential float32 one, the closed-form designs' responses, rfa_audio_iir_plan and
rfa_audio_iir_carry_after, the argument checks of rfa_audio_iir_* that come before the device is looked
for, the chains' ``audio_iir`` keyword without a device, the prototypes and constants of _lib.py against
the header, and tools/audio_iir_host_check (the same host paths under ASan + UBSan)."""
import ctypes
import functools
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import audio_iir_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, NODEVICE = -1, -4
RATE = 48000
B = ref.B
N = 8000
CUTS = (1, 127, 128, 129, 500, 2048, 2049, N - 1)
SETS = ("cheb8", "butter6", "deemphasis", "notch", "cheb8+deemphasis")
INPUTS = ("noise + 100 Hz + DC", "DC step", "700 Hz square")


@pytest.fixture(scope="module")
def lib():
    import rfanalyzer_amd
    rfanalyzer_amd.build()
    return rfanalyzer_amd.lib()


@functools.lru_cache(maxsize=None)
def sets():
    return ref.section_sets()


@functools.lru_cache(maxsize=None)
def inputs():
    x = ref.inputs(N)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def whole(name):
    """The restatement's rows of the three inputs given whole, computed once."""
    out = np.stack([ref.blocked(sets()[name], x) for x in inputs()])
    out.setflags(write=False)
    return out


# ------------------------------------------------------------------ the tables

def test_section_sets_are_the_five_named():
    assert tuple(sets()) == SETS
    assert [len(s) for s in sets().values()] == [4, 3, 1, 1, 5]
    radius = np.sqrt(float(sets()["notch"][0, 4]))
    assert abs(radius - 0.999) < 1e-6


@pytest.mark.parametrize("name", SETS)
def test_library_tables_equal_the_restatement(lib, name):
    from rfanalyzer_amd import demod
    for c in sets()[name]:
        G, P = demod.audio_iir_tables(c[3], c[4])
        g, p = ref.tables(c[3], c[4])
        assert G.dtype == np.float32 and G.shape == (B, 2) and P.shape == (2, 2)
        assert ref.bits_equal(G, g) and ref.bits_equal(P, p)
        assert list(G[0]) == [1.0, 0.0] and list(G[1]) == [-c[3], 1.0]          # I, then A's first row
        assert np.isfinite(G).all() and np.isfinite(P).all()


def test_tables_are_powers_of_the_transition_matrix():
    """G[i] and P against A^i by numpy's own matrix power, in float64: within a few ulp of float32."""
    c = sets()["cheb8"][0]
    A = np.array([[-float(c[3]), 1.0], [-float(c[4]), 0.0]])
    G, P = ref.tables(c[3], c[4])
    for i in (0, 1, 2, 17, 127):
        np.testing.assert_allclose(G[i], np.linalg.matrix_power(A, i)[0], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(P, np.linalg.matrix_power(A, B), rtol=1e-6, atol=1e-6)


# ------------------------------------------------------------------ the restatement

@pytest.mark.parametrize("name", SETS)
def test_restatement_is_cut_invariant(name):
    sec = sets()[name]
    for r in range(3):
        x, want = inputs()[r], whole(name)[r]
        for cut in CUTS:
            assert ref.bits_equal(ref.cut_run(sec, x, [cut]), want), (INPUTS[r], cut)
    x, want = inputs()[0], whole(name)[0]
    assert ref.bits_equal(ref.cut_run(sec, x, range(B - 8, B + 9)), want), "one-sample calls across a block edge"
    assert ref.bits_equal(ref.cut_run(sec, x, [1, 2, 127, 128, 129, 255, 256, 257, 500]), want), "many cuts"


def test_restatement_is_the_step_written_out_inside_the_first_block():
    """Block 0 has s0 = 0: the blocked output is the plain float32 recurrence there, bit for bit, up to the
    sign of a zero (zs + (+0) turns -0 into +0)."""
    for name in SETS:
        got, seq = whole(name)[:, :B], ref.sequential(sets()[name], inputs()[:, :B])
        assert np.array_equal(got, seq), name
    b0 = sets()["deemphasis"][0, 0]
    assert whole("deemphasis")[0, 0] == b0 * inputs()[0, 0]


def test_restatement_special_values():
    sec = sets()["cheb8"]
    odd = np.array([0x7fc00001, 0xffc12345, 0x7f800001, 0x80000000, 0x00000001], np.uint32).view(np.float32)
    assert ref.bits_equal(ref.blocked(None, odd), odd) and ref.bits_equal(ref.blocked(np.zeros((0, 5)), odd), odd)
    x = inputs()[0].copy()
    x[3 * B + 40] = np.nan
    y = ref.blocked(sec, x)
    assert np.isfinite(y[:3 * B + 40]).all() and not np.isfinite(y[3 * B + 40:]).any()
    s = ref.Slot(sec)
    s.process(x)
    assert not np.isfinite(s.process(inputs()[1])).any()     # until the slot is reset
    s.reset()
    assert ref.bits_equal(s.process(inputs()[1]), whole("cheb8")[1])


@pytest.mark.parametrize("name", SETS)
def test_blocked_form_is_as_accurate_as_the_sequential_one(name):
    """E(x) = max |x - float64 recurrence|.  E(blocked) <= 4 E(sequential float32) + 2^-22 max(|x|, |y|): the
    factor is a cap from the blocked form doing at most a few roundings more per output than the sequential
    one, not a measurement.  Observed here: 0.52 ... 1.59 (cheb8 0.76 / 1.53 / 0.97, butter6 1.11 / 1.59 /
    1.11, deemphasis 0.60 / 0.52 / 1.26, notch 0.99 / 0.77 / 0.65, cheb8+deemphasis 0.71 / 0.81 / 0.99)."""
    sec = sets()[name]
    f64 = ref.sequential(sec, inputs(), np.float64)
    f32 = ref.sequential(sec, inputs())
    assert f32.dtype == np.float32 and f64.dtype == np.float64
    for r in range(3):
        e_model = float(np.abs(whole(name)[r].astype(np.float64) - f64[r]).max())
        e_seq = float(np.abs(f32[r].astype(np.float64) - f64[r]).max())
        peak = max(float(np.abs(inputs()[r]).max()), float(np.abs(f64[r]).max()))
        print(f"{name}, {INPUTS[r]}: E(blocked) {e_model:.3e}, E(sequential) {e_seq:.3e}, ratio "
              f"{e_model / e_seq:.2f}, E(blocked) / peak {e_model / peak:.2e}")
        assert e_model <= 4.0 * e_seq + 2.0 ** -22 * peak, INPUTS[r]


# ------------------------------------------------------------------ the designs

def test_tone_strip_response():
    from rfanalyzer_amd import demod
    sec = demod.tone_strip_sections()
    assert sec.dtype == np.float32 and sec.shape == (4, 5)
    tones = np.array(demod.CTCSS_TONES)
    at = demod.iir_response(sec, tones)
    print("tone strip at the CTCSS tones:", np.round(at, 2))
    assert (at <= -40.0).all()
    band = np.arange(330.0, 3000.5, 5.0)
    assert (demod.iir_response(sec, band) >= -1.0).all() and (demod.iir_response(sec, band) <= 0.01).all()
    for hz, want in ((254.1, -42.1), (67.0, -45.6), (330.0, -0.96), (400.0, -0.01)):
        assert abs(demod.iir_response(sec, hz) - want) < 0.06, hz
    assert abs(demod.iir_response(sec, 255.0) + 40.0) < 0.05
    radii = np.sqrt(sec[:, 4].astype(np.float64))
    assert 0.9765 < radii.min() < 0.9775 and 0.9953 < radii.max() < 0.9955
    assert isinstance(demod.iir_response(sec, 100.0), float)
    # an odd order ends in a first-order section; the stop edge is where the attenuation is reached
    odd = demod.tone_strip_sections(order=5, attenuation_db=30.0, stop_hz=200.0)
    assert odd.shape == (3, 5) and odd[2, 2] == 0.0 and odd[2, 4] == 0.0
    assert abs(demod.iir_response(odd, 200.0) + 30.0) < 0.05 and demod.iir_response(odd, 100.0) <= -30.0
    for bad in ({"stop_hz": 0.0}, {"stop_hz": 24000.0}, {"order": 0}, {"order": 17}, {"attenuation_db": 0.0},
                {"rate": 0.0}):
        with pytest.raises(ValueError):
            demod.tone_strip_sections(**bad)


def test_deemphasis_response():
    from rfanalyzer_amd import demod
    tau = 750e-6
    sec = demod.deemphasis_sections()
    assert sec.shape == (1, 5) and sec[0, 1] == 0.0 and sec[0, 2] == 0.0 and sec[0, 4] == 0.0
    p = np.exp(-1.0 / (tau * RATE))
    assert sec[0, 0] == np.float32(1.0 - p) and sec[0, 3] == np.float32(-p)
    corner = 1.0 / (2.0 * np.pi * tau)
    assert abs(demod.iir_response(sec, corner) + 3.01) <= 0.05
    assert abs(demod.iir_response(sec, 0.0)) < 1e-4
    for hz in np.arange(1000.0, 1500.5, 50.0):               # every octave that fits between 1 and 3 kHz
        fall = demod.iir_response(sec, hz) - demod.iir_response(sec, 2.0 * hz)
        assert abs(fall - 6.0) <= 0.5, hz
    us75 = demod.deemphasis_sections(tau=75e-6)
    assert abs(demod.iir_response(us75, 1.0 / (2.0 * np.pi * 75e-6)) + 3.01) <= 0.1
    for bad in ({"tau": 0.0}, {"tau": -1.0}, {"rate": 0.0}, {"tau": float("nan")}):
        with pytest.raises(ValueError):
            demod.deemphasis_sections(**bad)


def test_butterworth_response():
    from rfanalyzer_amd import demod
    for order in (1, 2, 5, 6):
        sec = demod.highpass_sections(300.0, order)
        assert sec.shape == ((order + 1) // 2, 5)
        assert abs(demod.iir_response(sec, 300.0) + 3.0103) < 0.01, order
        assert abs(demod.iir_response(sec, 30.0) + 20.0 * order) < 0.2, order          # 6 dB / octave / pole
        assert abs(demod.iir_response(sec, 6000.0)) < 0.02, order
    with pytest.raises(ValueError):
        demod.highpass_sections(300.0, 17)


def test_every_design_is_inside_the_stability_triangle(lib):
    G, P = (ctypes.c_float * (2 * B))(), (ctypes.c_float * 4)()
    for name, sec in sets().items():
        for c in sec:
            assert abs(c[4]) < 1.0 and abs(c[3]) < 1.0 + c[4], name
            assert lib.rfa_audio_iir_tables(float(c[3]), float(c[4]), G, P) == 0


# ------------------------------------------------------------------ plan, carry, the triangle's edges

def test_plan_and_carry(lib):
    from rfanalyzer_amd import _lib, demod
    NB = _lib.RFA_AUDIO_IIR_CHUNK_BLOCKS
    C = NB * B
    assert demod.audio_iir_plan(0, 0)["path"] == "none" and demod.audio_iir_plan(8, 0, 5)["path"] == "none"
    assert demod.audio_iir_plan(0, 1)["path"] == "copy" and demod.audio_iir_plan(0, 5 * C)["path"] == "copy"
    assert demod.audio_iir_plan(1, 1)["path"] == "blocked" and demod.audio_iir_plan(8, 1 << 36, 127)["path"] == "blocked"
    p = demod.audio_iir_plan(4, 328)
    assert p == {"block": B, "chunk_blocks": NB, "lds_bytes": p["lds_bytes"], "path": "blocked", "chunks": 1, "blocks": 3}
    assert 4 * 3 * (B + 1) <= p["lds_bytes"] <= 64 * 1024
    full = demod.audio_iir_plan(4, C)
    assert (full["chunks"], full["blocks"]) == (1, NB) and 4 * NB * (B + 1) <= full["lds_bytes"] <= 160 * 1024
    assert demod.audio_iir_plan(4, C, 1)["chunks"] == 2 and demod.audio_iir_plan(4, C, 1)["blocks"] == NB + 1
    assert demod.audio_iir_plan(5, 2 * C + 5)["chunks"] == 3
    assert demod.audio_iir_plan(1, 128, 0)["blocks"] == 1 and demod.audio_iir_plan(1, 128, 1)["blocks"] == 2
    assert demod.audio_iir_plan(0, 300)["lds_bytes"] == 0 and demod.audio_iir_plan(0, 300)["chunks"] == 0
    assert demod.AudioIirBank.plan(4, 328, 7) == demod.audio_iir_plan(4, 328, 7)
    for n in (0, 1, 127, 128, 129, C, 1 << 36):
        for a in (0, 1, 127):
            assert demod.audio_iir_carry_after(n, a) == (a + n) % B
    out, nxt = (ctypes.c_int32 * 6)(), ctypes.c_int32(9)
    for s, n, a in ((-1, 5, 0), (9, 5, 0), (4, (1 << 36) + 1, 0), (4, 5, -1), (4, 5, B)):
        assert lib.rfa_audio_iir_plan(s, n, a, out) == INVALID
    assert lib.rfa_audio_iir_plan(4, 5, 0, None) == INVALID
    for n, a in (((1 << 36) + 1, 0), (5, -1), (5, B)):
        assert lib.rfa_audio_iir_carry_after(n, a, ctypes.byref(nxt)) == INVALID
    assert lib.rfa_audio_iir_carry_after(5, 0, None) == INVALID and nxt.value == 9


def test_stability_triangle_edges(lib):
    from rfanalyzer_amd import demod
    G, P = (ctypes.c_float * (2 * B))(), (ctypes.c_float * 4)()
    below = float(np.nextafter(np.float32(1.0), np.float32(0.0)))
    inside = [(0.0, 0.0), (0.0, below), (0.0, -below), (below, 0.0), (-below, 0.0), (1.49, 0.5), (-1.49, 0.5), (0.49, -0.5)]
    outside = [(0.0, 1.0), (0.0, -1.0), (1.0, 0.0), (-1.0, 0.0), (1.5, 0.5), (-1.5, 0.5), (0.5, -0.5), (2.0, 1.0),
               (float("inf"), 0.0), (0.0, float("nan")), (float("nan"), 0.5)]
    for a1, a2 in inside:
        assert lib.rfa_audio_iir_tables(a1, a2, G, P) == 0, (a1, a2)
        assert demod._audio_iir_sections([[1.0, 0.0, 0.0, a1, a2]]) is not None
    for a1, a2 in outside:
        assert lib.rfa_audio_iir_tables(a1, a2, G, P) == INVALID, (a1, a2)
        with pytest.raises(ValueError):
            demod._audio_iir_sections([[1.0, 0.0, 0.0, a1, a2]])
    assert lib.rfa_audio_iir_tables(0.0, 0.0, None, P) == INVALID and lib.rfa_audio_iir_tables(0.0, 0.0, G, None) == INVALID


# ------------------------------------------------------------------ _lib.py against the header

_C_SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "size_t": ctypes.c_size_t, "float": ctypes.c_float}
_C_TARGETS = {"int32_t": ctypes.c_int32, "size_t": ctypes.c_size_t, "float": ctypes.c_float,
              "void *": ctypes.c_void_p, "rfa_audio_iir *": ctypes.c_void_p}


def _header():
    with open(os.path.join(ROOT, "include", "rfa.h")) as f:
        return f.read()


def _prototypes():
    """{name: (return type text, [argument type text])} of the header's rfa_audio_iir_* entries."""
    out = {}
    for ret, name, args in re.findall(r"RFA_API\s+([\w\s\*]+?)\s*\b(rfa_audio_iir_\w+)\s*\(([^)]*)\)\s*;", _header()):
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
    assert len(protos) == 15 and {"rfa_audio_iir_create", "rfa_audio_iir_process", "rfa_audio_iir_plan",
                                  "rfa_audio_iir_set_sections", "rfa_audio_iir_get_sections", "rfa_audio_iir_reset",
                                  "rfa_audio_iir_process_host", "rfa_audio_iir_tables",
                                  "rfa_audio_iir_carry_after"} <= set(protos)
    for name, (ret, args) in protos.items():
        fn = getattr(lib, name)                             # exported
        assert fn.argtypes is not None and len(fn.argtypes) == len(args), name
        for i, (ctype, text) in enumerate(zip(fn.argtypes, args)):
            assert _matches(ctype, text), (name, i, text, ctype)
        if ret == "char *":
            assert fn.restype is ctypes.c_char_p, name
        else:
            assert ret == "int" and fn.restype is ctypes.c_int, name


def test_every_entry_is_in_the_integration_document():
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        doc = f.read()
    for name in _prototypes():
        assert re.search(r"\b" + name + r"\(", doc), name


def test_constants_of_the_binding_equal_the_header():
    from rfanalyzer_amd import _lib, demod
    defs = {k: int(v) for k, v in re.findall(r"#define\s+(RFA_AUDIO_IIR_\w+)\s+(\d+)", _header())}
    assert len(defs) == 8
    for name in ("MAX_CHANNELS", "MAX_SECTIONS", "BLOCK", "CHUNK_BLOCKS", "PLAN_FIELDS"):
        assert getattr(_lib, f"RFA_AUDIO_IIR_{name}") == defs[f"RFA_AUDIO_IIR_{name}"], name
    for i, path in enumerate(_lib.RFA_AUDIO_IIR_PATHS):
        assert defs[f"RFA_AUDIO_IIR_PATH_{path.upper()}"] == i
    assert defs["RFA_AUDIO_IIR_MAX_SECTIONS"] == ref.MAX_SECTIONS == demod.AUDIO_IIR_MAX_SECTIONS == 8
    assert defs["RFA_AUDIO_IIR_BLOCK"] == ref.B == demod.AUDIO_IIR_BLOCK == 128
    assert defs["RFA_AUDIO_IIR_MAX_CHANNELS"] == 1024
    assert len(demod.AUDIO_IIR_PLAN_FIELDS) == defs["RFA_AUDIO_IIR_PLAN_FIELDS"]


# ------------------------------------------------------------------ the library without a device

def _create(lib, n_channels):
    h = ctypes.c_void_p(1)
    rc = lib.rfa_audio_iir_create(0, n_channels, ctypes.byref(h))
    if rc == 0:
        lib.rfa_audio_iir_destroy(h)
    return rc, h.value


def test_argument_errors_come_before_the_device(lib):
    assert lib.rfa_audio_iir_create(0, 4, None) == INVALID
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
    x = (ctypes.c_float * 5)(9, 9, 9, 9, 9)
    n = (ctypes.c_size_t * 1)(2)
    assert lib.rfa_audio_iir_destroy(None) == INVALID
    assert lib.rfa_audio_iir_last_error(None) == b"null handle"
    assert lib.rfa_audio_iir_set_stream(None, None) == INVALID
    assert lib.rfa_audio_iir_get_stream(None, ctypes.byref(s)) == INVALID
    assert lib.rfa_audio_iir_synchronize(None) == INVALID
    assert lib.rfa_audio_iir_get_channels(None, ctypes.byref(v)) == INVALID
    assert lib.rfa_audio_iir_set_sections(None, 0, x, 1) == INVALID
    assert lib.rfa_audio_iir_get_sections(None, 0, x, 1, ctypes.byref(v)) == INVALID
    assert lib.rfa_audio_iir_reset(None, -1) == INVALID
    assert lib.rfa_audio_iir_process(None, None, 0, n, None, 0) == INVALID
    assert lib.rfa_audio_iir_process_host(None, None, 0, n, None, 0) == INVALID
    assert (v.value, list(x)) == (9, [9.0] * 5)


def test_iir_bank_sits_on_the_handle_base():
    from rfanalyzer_amd import demod
    assert issubclass(demod.AudioIirBank, demod._Handle) and demod.AudioIirBank._prefix == "rfa_audio_iir"
    for name in ("close", "set_stream", "synchronize", "stream", "__enter__", "__exit__", "__del__", "_call"):
        assert name not in vars(demod.AudioIirBank), name
    for name in ("set_sections", "sections", "reset", "process_device", "process_tensor", "process", "plan"):
        assert name in vars(demod.AudioIirBank), name


# ------------------------------------------------------------------ the chains' keyword without a device

def test_audio_iir_is_a_keyword_of_every_bank_chain():
    from rfanalyzer_amd import demod
    for cls in (demod.ReceiverBank, demod.TunedReceiverBank, demod.RasterReceiverBank):
        p = inspect.signature(cls.__init__).parameters["audio_iir"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None
    assert "set_audio_iir" in vars(demod._BankChain)
    assert "audio_iir" not in vars(demod._BankChain)         # no handle attribute unless a chain asks for one
    assert "audio_iir" not in inspect.signature(demod.Receiver.__init__).parameters


def test_audio_iir_keyword_is_checked_before_any_handle_is_made():
    """These raise on a machine with a device and on one without, before a handle exists."""
    from rfanalyzer_amd import demod
    fs, spacing = 2_400_000, 25_000
    ok = [1.0, 0.0, 0.0, -0.5, 0.0]
    for make in (lambda **kw: demod.ReceiverBank("u8", fs, ["nfm", "am"], **kw),
                 lambda **kw: demod.TunedReceiverBank("u8", fs, spacing, ["nfm", "am"], **kw),
                 lambda **kw: demod.RasterReceiverBank("u8", fs, spacing, ["nfm", "am"], **kw)):
        for bad in (True, "voice", 300.0, 3,                                   # not one entry per slot
                    ["voice"], ["voice", None, None], [],                     # a wrong entry count
                    ["voice", "bass"], ["deemphasis+voice", None], [True, None], [300.0, None], [7, None],
                    [np.zeros(5, np.float32), None], [np.zeros((2, 4), np.float32), None],     # not [S, 5]
                    [[ok] * 9, None],                                          # more than 8 sections
                    [[[1.0, np.nan, 0.0, -0.5, 0.0]], None], [[[np.inf, 0.0, 0.0, -0.5, 0.0]], None],
                    [[[1.0, 0.0, 0.0, 0.0, 1.0]], None], [[[1.0, 0.0, 0.0, -1.0, 0.0]], None],   # on the triangle's edge
                    [[["a"] * 5], None]):
            with pytest.raises(ValueError):
                make(audio_iir=bad)


def test_audio_iir_entries():
    from rfanalyzer_amd import demod
    assert demod._audio_iir_entries(None, 3) is None
    got = demod._audio_iir_entries([None, "voice", "deemphasis", "voice+deemphasis", [[0.5, 0.25, 0.0, -0.5, 0.0]],
                                    np.zeros((0, 5), np.float32)], 6)
    assert got[0] is None and got[5] is None
    assert np.array_equal(got[1], demod.tone_strip_sections()) and np.array_equal(got[2], demod.deemphasis_sections())
    assert np.array_equal(got[3], np.concatenate([demod.tone_strip_sections(), demod.deemphasis_sections()]))
    assert got[4].dtype == np.float32 and got[4].shape == (1, 5) and list(got[4][0]) == [0.5, 0.25, 0.0, -0.5, 0.0]


def test_valid_audio_iir_without_a_device_fails_at_the_device():
    import torch
    if torch.cuda.is_available():
        return                                              # with a device tests/test_gpu_audio_iir.py builds these chains
    from rfanalyzer_amd import _lib, demod
    with pytest.raises(_lib.RfaError) as e:
        demod.ReceiverBank("u8", 2_400_000, ["nfm"] * 2, audio_iir=["voice", None])
    assert e.value.status == NODEVICE


def test_host_check_program_passes_under_sanitizers(lib):
    """tools/audio_iir_host_check: audio_iir.hip's host side built with -fsanitize=address,undefined into a
    stand-alone program that walks the host-only entries and the error paths."""
    exe = os.path.join(ROOT, "tools", "audio_iir_host_check")
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tools"), exe], capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "audio_iir_host_check ok" in r.stdout
