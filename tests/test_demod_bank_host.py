"""CPU: the demodulator bank's host-only surface (rfa_demod_bank_*): the header declares the
entries and _lib binds them, creation arguments are rejected before the device is looked for,
and every entry answers a null handle with RFA_ERR_INVALID."""
import ctypes
import os
import re

import pytest

from rfanalyzer_amd import _lib
from rfanalyzer_amd import demod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["create", "destroy", "last_error", "get_channels", "set_mode", "get_mode", "set_channel_width",
           "get_channel_width", "set_volume", "set_audio_sink", "get_taps", "get_state", "reset", "max_outputs",
           "process", "process_host", "set_stream", "get_stream", "synchronize"]
LIMIT = 1024


def _header():
    with open(os.path.join(ROOT, "include", "rfa.h")) as f:
        return f.read()


def test_header_declares_and_lib_binds_every_entry():
    text = _header()
    L = _lib.lib()
    for e in ENTRIES:
        name = f"rfa_demod_bank_{e}"
        assert re.search(rf"RFA_API [\w ]+\*?\b{name}\(", text), name
        fn = getattr(L, name)
        assert fn.argtypes is not None, name
    declared = set(re.findall(r"\brfa_demod_bank_(\w+)\(", text))
    assert declared == set(ENTRIES)
    m = re.search(r"#define RFA_DEMOD_BANK_MAX_CHANNELS (\d+)", text)
    assert m and int(m.group(1)) == LIMIT


def _create(modes, n=None):
    h = _lib._h()
    arr = (ctypes.c_int32 * max(len(modes), 1))(*modes)
    st = _lib.lib().rfa_demod_bank_create(0, arr, len(modes) if n is None else n, ctypes.byref(h))
    if st == _lib.RFA_OK:                       # a machine with a device: not what is asked here
        _lib.lib().rfa_demod_bank_destroy(h)
    else:
        assert not h.value
    return st


@pytest.mark.parametrize("modes,n", [
    ([1, 2], 0),
    ([1, 2], -2),
    ([2] * (LIMIT + 1), None),
    ([7, 1, 2], None),                          # a bad mode first, in the middle, last
    ([1, 7, 2], None),
    ([1, 2, -1], None),
])
def test_argument_errors_come_before_the_device_check(modes, n):
    assert _create(modes, n) == _lib.RFA_ERR_INVALID


def test_null_out_and_null_modes():
    L = _lib.lib()
    arr = (ctypes.c_int32 * 2)(1, 2)
    assert L.rfa_demod_bank_create(0, arr, 2, None) == _lib.RFA_ERR_INVALID
    h = _lib._h()
    assert L.rfa_demod_bank_create(0, None, 2, ctypes.byref(h)) == _lib.RFA_ERR_INVALID
    assert not h.value


def _no_device():
    c = ctypes.c_int(0)
    return _lib.lib().rfa_device_count(ctypes.byref(c)) != _lib.RFA_OK or c.value == 0


def test_no_device_is_a_status_not_a_crash():
    if not _no_device():
        with demod.DemodulatorBank(["am", "nfm"]) as bank:      # with a device the same call works
            assert bank.n_channels == 2
        return
    assert _create([1, 2]) == _lib.RFA_ERR_NODEVICE
    assert _create([0]) == _lib.RFA_ERR_NODEVICE
    assert _create([2] * LIMIT) == _lib.RFA_ERR_NODEVICE
    with pytest.raises(_lib.RfaError) as e:
        demod.DemodulatorBank(["am", "nfm", "off"])
    assert e.value.status == _lib.RFA_ERR_NODEVICE
    with pytest.raises(ValueError):
        demod.DemodulatorBank(["am", "fm"])                     # no such mode name


def test_every_entry_rejects_a_null_handle():
    L = _lib.lib()
    i32, f32, vp = ctypes.c_int32(0), ctypes.c_float(0), _lib._vp()
    n = (ctypes.c_size_t * 4)(9, 9, 9, 9)
    bi, bf = ctypes.byref(i32), ctypes.byref(f32)
    calls = {
        "destroy": (None,),
        "get_channels": (None, bi),
        "max_outputs": (None, 16, n),
        "process": (None, None, None, 0, 0, 0, None, 0, n),
        "process_host": (None, None, None, 0, 0, 0, None, 0, n),
        "set_stream": (None, None),
        "get_stream": (None, ctypes.byref(vp)),
        "synchronize": (None,),
    }
    for k in (0, -1, 5):                        # a slot index in or out of range makes no difference
        calls.update({
            ("set_mode", k): (None, k, 1),
            ("get_mode", k): (None, k, bi),
            ("set_channel_width", k): (None, k, 5000),
            ("get_channel_width", k): (None, k, bi),
            ("set_volume", k): (None, k, 0.5),
            ("set_audio_sink", k): (None, k, 0),
            ("get_taps", k): (None, k, 0, None, None, 0, bi, bi),
            ("get_state", k): (None, k, bf, bf, bf),
            ("reset", k): (None, k),
        })
    seen = set()
    for key, args in calls.items():
        e = key if isinstance(key, str) else key[0]
        seen.add(e)
        assert getattr(L, f"rfa_demod_bank_{e}")(*args) == _lib.RFA_ERR_INVALID, key
    assert seen == set(ENTRIES) - {"create", "last_error"}
    assert list(n) == [9, 9, 9, 9]
    err = L.rfa_demod_bank_last_error(None)
    assert isinstance(err, bytes) and err == b"null handle"
