"""CPU: the host-only side of the code meter and the DCS code squelch -- the word's known answers through
demod.dcs_word and rfa_code_word, the restatement (tests/code_ref.py) against a literal per-sample loop,
rfa_code_subcell and rfa_code_merge against it, demod.CodeRule on made-up sub-cells against the restated
rule, demod.dcs_identify, the chains' ``code`` keyword without a device, the argument checks of rfa_code_*
that come before the device is looked for, and tools/code_host_check (the same host paths under ASan +
UBSan)."""
import ctypes
import inspect
import os
import subprocess

import numpy as np
import pytest

import code_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, NODEVICE = -1, -4
RATE = 48000
P = 8


@pytest.fixture(scope="module")
def lib():
    import rfanalyzer_amd
    rfanalyzer_amd.build()
    return rfanalyzer_amd.lib()


def lib_word(lib, code):
    w = ctypes.c_uint32(9)
    assert lib.rfa_code_word(code, ctypes.byref(w)) == 0
    return w.value


# ------------------------------------------------------------------ the word

def test_known_answers_of_the_word(lib):
    from rfanalyzer_amd import demod
    for fn in (demod.dcs_word, lambda c: lib_word(lib, c), code_ref.word):
        w023 = fn(0o023)
        assert w023 == 0x763813
        rot = code_ref.rotations(w023)
        assert fn(0o340) in rot and fn(0o766) in rot
        inverse = code_ref.rotations(w023 ^ 0x7FFFFF)
        assert fn(0o047) in inverse and fn(0o375) in inverse and fn(0o707) in inverse
        words = [fn(c) for c in demod.DCS_CODES]
        assert {bin(w).count("1") for w in words} == {11, 12}
        assert all(w & 0xFFF == (0x800 | c) and w < 1 << 23 for w, c in zip(words, demod.DCS_CODES))
        classes = [code_ref.rotations(w) for w in words]
        assert not [(i, j) for i in range(len(words)) for j in range(i) if words[i] in classes[j]]
        for c in range(512):                                 # every word is a multiple of the generator
            assert code_ref.gf2_remainder((fn(c) & 0xFFF) << 11 | fn(c) >> 12, 0xC75) == 0
    assert all(demod.dcs_word(c) == lib_word(lib, c) == code_ref.word(c) for c in range(512))


def test_the_other_golay_generator_is_the_wrong_one():
    from rfanalyzer_amd import demod
    assert code_ref.word(0o023, 0xAE3) == 0x7E8813 != demod.dcs_word(0o023)
    words = [code_ref.word(c, 0xAE3) for c in demod.DCS_CODES]
    classes = [code_ref.rotations(w) for w in words]
    assert sum(words[i] in classes[j] for i in range(len(words)) for j in range(i)) == 22


def test_the_table_and_the_parser(lib):
    from rfanalyzer_amd import demod
    t = demod.DCS_CODES
    assert len(t) == 104 == len(set(t)) and list(t) == sorted(t) == list(code_ref.CODES)
    assert t[0] == 0o023 and t[-1] == 0o754 and 0o047 in t and 0o340 not in t
    assert demod.dcs_parse("023") == (0o023, False) == demod.dcs_parse("023N") == demod.dcs_parse(0o023)
    assert demod.dcs_parse("023I") == (0o023, True) and demod.dcs_parse(" 754i ") == (0o754, True)
    assert demod.dcs_parse(np.int64(0o116)) == (0o116, False)
    for bad in ("23", "0234", "089", "023X", "", "N", "-23"):
        with pytest.raises(ValueError):
            demod.dcs_parse(bad)
    for bad in (-1, 512):
        with pytest.raises(ValueError):
            demod.dcs_parse(bad)
        with pytest.raises(ValueError):
            demod.dcs_word(bad)
        assert lib.rfa_code_word(bad, ctypes.byref(ctypes.c_uint32())) == INVALID
    for bad in (True, 23.0, None, b"023", [0o023]):
        with pytest.raises(TypeError):
            demod.dcs_parse(bad)
    assert lib.rfa_code_word(0o023, None) == INVALID


# ------------------------------------------------------------------ the restatement

def _samples(n, seed=5):
    rng = np.random.default_rng(seed)
    a = (rng.standard_normal(n) * 0.1).astype(np.float32)
    special = [np.nan, np.inf, -np.inf, 32768.0, -32768.0, 32768.0 - 2.0 ** -9, 1e-40, -0.0, 2.0 ** -25,
               3 * 2.0 ** -25, -(2.0 ** -25), 5 * 2.0 ** -25, 2.0 ** -26]
    a[3:3 + len(special)] = np.array(special, np.float32)
    return a


@pytest.mark.parametrize("rate,g0", [(48000, 0), (48000, 44), (48000, 45), (8000, 7), (44100, 123_456_789)])
def test_restated_sums_equal_a_literal_loop(rate, g0):
    a = _samples(400, seed=rate + g0)
    j0, s, bad = code_ref.sums(a, g0, rate)
    lj0, ls, lbad = code_ref.sums_literal(a, g0, rate)
    assert (j0, bad) == (lj0, lbad) and bad == 5 and s.dtype == np.int64
    assert [int(v) for v in s] == ls
    q, isbad = code_ref.quantise(np.array([2.0 ** -25, 3 * 2.0 ** -25, -(2.0 ** -25), 2.0 ** -24, 32768.0 - 2.0 ** -9,
                                           -0.0, 1e-40, 0.5], np.float32))
    assert list(q) == [0, 2, 0, 1, 2 ** 39 - 2 ** 15, 0, 0, 2 ** 23] and not isbad.any()


def test_subcell_index_equals_the_restatement(lib):
    j = ctypes.c_int64(9)
    for rate in (8000, 44100, 48000, 384000):
        den = 5 * rate
        gs = {0, 1, 44, 45, 2 ** 31, 2 ** 48 - 1, 2 ** 48}
        for c in (1, 2, 7, 8, 1000, 123_456_789):            # either side of a sub-cell's first sample
            first = -(-c * den // code_ref.NUM)
            gs |= {first - 1, first}
            assert code_ref.subcell(first, rate) == c and code_ref.subcell(first - 1, rate) == c - 1
        for g in sorted(gs):
            assert lib.rfa_code_subcell(rate, g, ctypes.byref(j)) == 0
            assert j.value == (672 * 8 * g) // den == code_ref.subcell(g, rate), (rate, g)
    assert 672 * 8 * 2 ** 48 < 2 ** 61
    per = np.bincount(code_ref.subcell(np.arange(480000, dtype=np.int64), RATE))
    assert set(per) == {44, 45} and per.size == 134.4 * 8 * 10
    j.value = 9
    for rate, g in ((7999, 0), (384001, 0), (0, 0), (48000, -1), (48000, 2 ** 48 + 1), (48000, 2 ** 63 - 1)):
        assert lib.rfa_code_subcell(rate, g, ctypes.byref(j)) == INVALID and j.value == 9
    assert lib.rfa_code_subcell(48000, 0, None) == INVALID


def _merge(lib, rate, g_end, j0, sums, carry):
    m = len(sums)
    arr = (ctypes.c_int64 * max(m, 1))(*[int(v) for v in sums])
    valid = ctypes.c_int32(carry is not None)
    cj, cs = ctypes.c_int64(carry[0] if carry else 0), ctypes.c_int64(carry[1] if carry else 0)
    first, count = ctypes.c_int64(-9), ctypes.c_int64(-9)
    rc = lib.rfa_code_merge(rate, g_end, j0, m, arr, ctypes.byref(valid), ctypes.byref(cj), ctypes.byref(cs),
                            ctypes.byref(first), ctypes.byref(count))
    assert rc == 0
    return first.value, list(arr)[:count.value], ((cj.value, cs.value) if valid.value else None)


@pytest.mark.parametrize("rate", [8000, 48000])
def test_merge_over_random_cuts_gives_the_whole_streams_sub_cells(lib, rate):
    rng = np.random.default_rng(rate)
    a = _samples(3000, seed=1)
    whole = code_ref.completed(a, rate)
    for trial in range(20):
        cuts = sorted(rng.integers(0, a.size + 1, rng.integers(1, 30)).tolist())
        cuts = [0] + cuts + [cuts[-1], a.size]               # zero-length calls among them
        got, ref, carry, nxt = [], code_ref.Carry(rate), None, 0
        for lo, hi in zip(cuts, cuts[1:]):
            j0, s, _ = code_ref.sums(a[lo:hi], lo, rate)
            first, done, carry = _merge(lib, rate, hi, j0, s, carry)
            rfirst, rdone, _ = ref.call(a[lo:hi])
            assert (first, done) == (rfirst, [int(v) for v in rdone]) and carry == ref.carry
            if done:
                assert first == nxt
                nxt += len(done)
            got += done
        assert np.array_equal(np.array(got, np.int64), whole)
    # argument errors: a carry that does not meet the call, NULL pointers, a rate or counter out of range
    v, c, f = ctypes.c_int32(1), ctypes.c_int64(5), ctypes.c_int64(0)
    s = (ctypes.c_int64 * 2)(1, 2)
    r = ctypes.byref
    assert lib.rfa_code_merge(rate, 100, 6, 2, s, r(v), r(c), r(f), r(f), r(f)) == INVALID
    assert lib.rfa_code_merge(rate, 100, 5, 2, None, r(v), r(c), r(f), r(f), r(f)) == INVALID
    assert lib.rfa_code_merge(7999, 100, 5, 2, s, r(v), r(c), r(f), r(f), r(f)) == INVALID
    assert lib.rfa_code_merge(rate, -1, 5, 2, s, r(v), r(c), r(f), r(f), r(f)) == INVALID
    assert lib.rfa_code_merge(rate, 100, 5, -1, s, r(v), r(c), r(f), r(f), r(f)) == INVALID
    assert lib.rfa_code_merge(rate, 100, 5, 2, s, None, r(c), r(f), r(f), r(f)) == INVALID
    assert list(s) == [1, 2] and v.value == 1 and c.value == 5


# ------------------------------------------------------------------ the rule

def _cells(w, n_sub, phase=3, start_bit=5, amp=1_300_000, dc=0, noise=0.0, seed=0):
    """n_sub sub-cells of a clean NRZ word, the first sub-cell ``phase`` sub-cells into bit ``start_bit``."""
    i = (np.arange(n_sub) + phase) // P + start_bit
    s = np.where((w >> (i % 23)) & 1, 45 * amp, -45 * amp) + 45 * dc
    if noise:
        s = s + np.random.default_rng(seed).standard_normal(n_sub) * noise * 45 * amp
    return np.rint(s).astype(np.int64)


def _feed(rule, ref, rows, piece=61, first0=0, bad=None, n=None, active=None):
    """Rows of sub-cells in calls of ``piece`` to both rules; the gates per call."""
    K = len(rows)
    gates = []
    for lo in range(0, len(rows[0]), piece):
        part = [np.asarray(r[lo:lo + piece], np.int64) for r in rows]
        first = [first0 + lo] * K
        count = [len(p) for p in part]
        b = [0] * K if bad is None else bad
        cnt = [45 * c for c in count] if n is None else n
        g = rule.update(first, count, part, b, cnt, active)
        assert list(g) == ref.update(first, part, b, cnt, active), lo
        assert np.array_equal(rule.score, np.array(ref.score), equal_nan=True) or np.allclose(
            rule.score, ref.score, rtol=0, atol=1e-12, equal_nan=True)
        gates.append(list(g))
    return np.array(gates)


def _rules(wanted, **kw):
    from rfanalyzer_amd import demod
    rule = demod.CodeRule(len(wanted), **kw)
    words = []
    for k, entry in enumerate(wanted):
        if entry is None:
            words.append(None)
            continue
        code, inv = demod.dcs_parse(entry)
        rule.set_code(k, code, inv)
        words.append(demod.dcs_word(code) ^ (0x7FFFFF if inv else 0))
    ref = code_ref.Rule(rule.words, rule.threshold, rule.hang, words)
    return rule, ref


def test_rule_opens_on_the_right_code_after_one_window_and_on_nothing_else():
    from rfanalyzer_amd import demod
    rule, ref = _rules(["023", "023", "023", "023", "023I", None], words=2)
    assert rule.need == 8 * 47 and list(rule.open) == [False] * 5 + [True]
    w023, w047, w025 = (demod.dcs_word(c) for c in (0o023, 0o047, 0o025))
    n_sub = 3 * rule.need + 10
    noise = np.rint(np.random.default_rng(4).standard_normal(n_sub) * 5e7).astype(np.int64)
    rows = [_cells(w023, n_sub, dc=400_000, noise=0.5, seed=1), _cells(w047, n_sub, phase=6), _cells(w025, n_sub),
            noise, _cells(w023 ^ 0x7FFFFF, n_sub, phase=1, start_bit=17), _cells(w023, n_sub)]
    gates = _feed(rule, ref, rows)
    first = -(-rule.need // 61) - 1                          # the call that completes the first window
    assert not gates[:first, :5].any() and gates[first:, 0].all() and gates[first:, 4].all()
    assert not gates[:, 1:4].any() and gates[:, 5].all()
    score = rule.score
    print(f"scores {score}")
    assert score[0] > 0.9 and score[4] > 0.999 and (score[1:4] < 0.7).all() and np.isnan(score[5])
    # no variance: score 0
    flat, fref = _rules(["023"], words=2)
    _feed(flat, fref, [np.full(rule.need, 12345, np.int64)])
    assert flat.score[0] == 0.0 and not flat.open[0]


def test_rule_resets_on_a_gap_a_bad_sample_an_inactive_call_and_no_samples():
    from rfanalyzer_amd import demod
    w = demod.dcs_word(0o023)
    for how in ("gap", "bad", "inactive", "empty"):
        rule, ref = _rules(["023", "023"], words=2)
        need = rule.need
        rows = [_cells(w, 2 * need), _cells(w, 2 * need)]
        g = _feed(rule, ref, [r[:need + 30] for r in rows], piece=need + 30)
        assert g[-1].all() and (rule._fill == 30).all()
        K2 = [0, 0]
        part = [r[need + 30:need + 60] for r in rows]
        args = {"gap": ([need + 31, need + 30], [30, 30], part, K2, [1350, 1350], None),
                "bad": ([need + 30] * 2, [30, 30], part, [1, 0], [1350, 1350], None),
                "inactive": ([need + 30] * 2, [30, 30], part, K2, [1350, 1350], [False, True]),
                "empty": ([need + 30] * 2, [0, 30], part, K2, [0, 1350], None)}[how]
        gate = rule.update(*args)
        assert list(gate) == ref.update(args[0], args[2], *args[3:]) == [False, True], how
        assert np.isnan(rule.score[0]) and rule.score[1] > 0.99
        assert rule._fill[0] == (30 if how == "gap" else 0) and rule._fill[1] == 60, how
        assert rule._next[0] == (need + 61 if how == "gap" else -1)
    # a call that completes no sub-cell (a few samples inside one) resets nothing
    gate = rule.update([need + 60] * 2, [0, 0], [[], []], [0, 0], [3, 3])
    assert list(gate) == [False, True] and rule._fill[1] == 60


def test_rule_honours_hang():
    from rfanalyzer_amd import demod
    w, other = demod.dcs_word(0o023), demod.dcs_word(0o025)
    for hang in (1, 2, 3):
        rule, ref = _rules(["023"], words=2, hang=hang)
        need = rule.need
        row = np.concatenate([_cells(w, need), _cells(other, 4 * need)])
        gates = _feed(rule, ref, [row], piece=need)[:, 0]
        assert list(gates) == [True] + [True] * (hang - 1) + [False] * (4 - hang + 1), hang
    rule, ref = _rules(["023"], words=2, hang=2)
    row = np.concatenate([_cells(w, need), _cells(other, need), _cells(w, need), _cells(other, need)])
    assert _feed(rule, ref, [row], piece=need)[:, 0].all()   # a detection clears the miss count
    for bad in ({"words": 0}, {"words": 1.5}, {"threshold": 1.0}, {"threshold": -0.1}, {"hang": 0}):
        with pytest.raises(ValueError):
            demod.CodeRule(2, **bad)
    with pytest.raises(ValueError):
        demod.CodeRule(0)
    with pytest.raises(ValueError):
        rule.set_code(1, 0o023)
    r = demod.CodeRule(3)
    assert (r.words, r.threshold, r.hang) == (4, 0.8, 2) and r.open.all()


def test_identify_finds_the_code_and_the_polarity():
    from rfanalyzer_amd import demod
    for code, inverted, words in ((0o023, False, 2), (0o754, False, 4), (0o025, True, 4), (0o311, True, 2)):
        w = demod.dcs_word(code) ^ (0x7FFFFF if inverted else 0)
        sub = _cells(w, P * (23 * words + 1) + 5, phase=code % 8, start_bit=code % 23, dc=-700_000, noise=0.4,
                     seed=code)
        got = demod.dcs_identify(sub, words)
        # every table code's complement is a rotation of another table code's word (023I is 047N): the
        # reading returned is the normal one, and it is the word that was sent
        assert got[2] > 0.9 and got[1] is False and got[0] in demod.DCS_CODES, (oct(code), got)
        assert demod.dcs_word(got[0]) in code_ref.rotations(w), (oct(code), got)
        if not inverted:
            assert got[0] == code
        assert got[2] == pytest.approx(demod.dcs_score(sub[:P * (23 * words + 1)], w, words), abs=1e-12)
        assert got[2] == pytest.approx(code_ref.score(sub, w, words), abs=1e-12)
    # 023 inverted is 047: the normal reading is returned
    sub = _cells(demod.dcs_word(0o023) ^ 0x7FFFFF, P * 47)
    assert demod.dcs_identify(sub, 2)[:2] == (0o047, False)
    with pytest.raises(ValueError):
        demod.dcs_identify(sub[:-1], 2)


# ------------------------------------------------------------------ the library without a device

def _create(lib, n_channels, rate=RATE):
    h = ctypes.c_void_p(1)
    rc = lib.rfa_code_create(0, n_channels, rate, ctypes.byref(h))
    if rc == 0:
        lib.rfa_code_destroy(h)
    return rc, h.value


def test_argument_errors_come_before_the_device(lib):
    import torch
    assert lib.rfa_code_create(0, 4, RATE, None) == INVALID
    for k in (0, -1, 1025, -2 ** 31, 2 ** 31 - 1):
        assert _create(lib, k) == (INVALID, None), k
    for rate in (7999, 384001, 0, -1, 2 ** 31 - 1):
        assert _create(lib, 4, rate) == (INVALID, None), rate
    for k, rate in ((1, 8000), (32, 48000), (1024, 48000)):
        rc, h = _create(lib, k, rate)
        assert rc == 0 if torch.cuda.is_available() else (rc, h) == (NODEVICE, None)


def test_null_handle_answers(lib):
    s = ctypes.c_void_p(0)
    assert lib.rfa_code_destroy(None) == INVALID
    assert lib.rfa_code_last_error(None) == b"null handle"
    assert lib.rfa_code_set_stream(None, None) == INVALID
    assert lib.rfa_code_get_stream(None, ctypes.byref(s)) == INVALID
    assert lib.rfa_code_synchronize(None) == INVALID
    v = ctypes.c_int32(9)
    d = (ctypes.c_int64 * 8)(*[9] * 8)
    n = (ctypes.c_size_t * 1)(0)
    assert lib.rfa_code_get_channels(None, ctypes.byref(v), ctypes.byref(v)) == INVALID
    assert lib.rfa_code_break(None, 0) == INVALID and lib.rfa_code_break(None, -1) == INVALID
    assert lib.rfa_code_reset(None) == INVALID
    assert lib.rfa_code_process(None, None, 0, n) == INVALID
    assert lib.rfa_code_collect(None, d, d, d, 8, d, d) == INVALID
    assert lib.rfa_code_process_host(None, None, 0, n, d, d, d, 8, d, d) == INVALID
    assert (v.value, list(d)) == (9, [9] * 8)


def test_meter_bank_sits_on_the_handle_base():
    from rfanalyzer_amd import demod
    assert issubclass(demod.CodeMeterBank, demod._Handle) and demod.CodeMeterBank._prefix == "rfa_code"
    for name in ("close", "set_stream", "synchronize", "stream", "__enter__", "__exit__", "__del__", "_call"):
        assert name not in vars(demod.CodeMeterBank), name
    for name in ("process_device", "collect", "process", "process_tensor", "break_", "reset"):
        assert name in vars(demod.CodeMeterBank), name


# ------------------------------------------------------------------ the chains' keyword without a device

def test_code_is_a_keyword_of_every_bank_chain():
    from rfanalyzer_amd import demod
    for cls in (demod.ReceiverBank, demod.TunedReceiverBank, demod.RasterReceiverBank):
        p = inspect.signature(cls.__init__).parameters["code"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None
    for name in ("code_open", "code_score"):
        assert isinstance(vars(demod._BankChain)[name], property)
    assert "set_code" in vars(demod._BankChain)
    assert "code_meter" not in vars(demod._BankChain)        # no meter attribute unless a chain asks for codes


def test_code_keyword_is_checked_before_any_handle_is_made():
    """These raise on a machine with a device and on one without, before a handle exists."""
    from rfanalyzer_amd import demod
    fs, spacing = 2_400_000, 25_000
    for make in (lambda **kw: demod.ReceiverBank("u8", fs, ["nfm", "am"], **kw),
                 lambda **kw: demod.TunedReceiverBank("u8", fs, spacing, ["nfm", "am"], **kw),
                 lambda **kw: demod.RasterReceiverBank("u8", fs, spacing, ["nfm", "am"], **kw)):
        for bad in (True, "023", 0o023, 23.0):
            with pytest.raises(TypeError):
                make(code=bad)
        for bad in (["023", 23.0], [True, None], [["023"], None], [b"023", None]):
            with pytest.raises(TypeError):
                make(code=bad)
        for bad in (["023"], ["023", None, None], ["0234", None], ["089", None], [512, None], [-1, None],
                    ["023X", None]):
            with pytest.raises(ValueError):
                make(code=bad)
        with pytest.raises(ValueError, match="both a tone and a code"):
            make(code=["023", None], tone=[100.0, None])


def test_valid_code_without_a_device_fails_at_the_device():
    import torch
    if torch.cuda.is_available():
        return                                              # with a device tests/test_gpu_code.py builds these chains
    from rfanalyzer_amd import _lib, demod
    with pytest.raises(_lib.RfaError) as e:
        demod.ReceiverBank("u8", 2_400_000, ["nfm"] * 2, code=["023", None], tone=[None, 100.0])
    assert e.value.status == NODEVICE


def test_host_check_program_passes_under_sanitizers(lib):
    """tools/code_host_check: code.hip's host side built with -fsanitize=address,undefined into a
    stand-alone program that walks the host-only entries and the error paths."""
    exe = os.path.join(ROOT, "tools", "code_host_check")
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tools"), exe], capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "code_host_check ok" in r.stdout
