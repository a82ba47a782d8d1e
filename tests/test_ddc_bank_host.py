"""CPU: the channel bank's host-only surface (rfa_ddc_bank_*, rfa_ddc_mix_info, SURVEY.md
§8(f) row 4b) -- the mixer design against oracle/demod.py, and argument errors that must be
reported before the device is looked for.

The bank rejects a slot whose mixer table would be empty.  calcOptimalCosineLength cannot
return 0 for a folded mix frequency: with cycle = sample_rate / |mix| < 1 its first guess is 0
with error `cycle`, and the multiples i * cycle step by less than 1, so the first one past an
integer has a fractional part below `cycle` and replaces the guess with an integer >= 1; with
cycle >= 1 the first guess is already >= 1.  The grid below therefore finds no empty table
(asserted, so a change of the design code that makes one reachable shows up here)."""
import ctypes

import pytest

from oracle import demod as od
from rfanalyzer_amd import _lib
from rfanalyzer_amd import demod

FMT = {"s8": od.IN_S8, "u8": od.IN_U8, "s16": od.IN_S16LE}
CENTER = 100_000_000


def _offsets(sr):
    near = [sr - 1, sr, sr + 1, 2 * sr, 3 * sr + 7, 5 * sr // 2]
    small = [1, 17, sr // 501, sr // 500, sr // 500 + 1, sr // 499, 1000, 12_500, 130_000, sr // 3, sr // 2]
    return [0] + [s * o for o in small + near for s in (1, -1)]


@pytest.mark.parametrize("fmt", ["s8", "u8", "s16"])
@pytest.mark.parametrize("sr", [48_000, 1_000_000, 2_400_000, 2_410_000, 20_000_000])
def test_mix_info_equals_the_oracle(fmt, sr):
    lengths = []
    for off in _offsets(sr):
        want_mf = od.mix_frequency(CENTER, CENTER + off, sr)
        want_len = max(0, od.optimal_cosine_length(sr, want_mf))
        assert demod.mix_info(fmt, sr, CENTER, CENTER + off) == (want_mf, want_len), (sr, off)
        lengths.append(want_len)
    assert demod.mix_info(fmt, sr, CENTER, CENTER)[0] == sr          # offset 0 folds by +sample rate
    assert min(lengths) >= 1                                         # no empty table (module docstring)


def test_mix_info_argument_errors():
    L = _lib.lib()
    mf, n = ctypes.c_int32(0), ctypes.c_int32(0)
    args = (ctypes.byref(mf), ctypes.byref(n))
    assert L.rfa_ddc_mix_info(9, 2_400_000, CENTER, CENTER, *args) == _lib.RFA_ERR_INVALID
    assert L.rfa_ddc_mix_info(FMT["u8"], 0, CENTER, CENTER, *args) == _lib.RFA_ERR_INVALID
    assert L.rfa_ddc_mix_info(od.IN_F32_INTERLEAVED, 2_400_000, CENTER, CENTER, *args) == _lib.RFA_ERR_UNSUPPORTED
    assert L.rfa_ddc_mix_info(FMT["u8"], 2_400_000, CENTER, CENTER + 130_000, None, None) == _lib.RFA_OK
    with pytest.raises(ValueError):
        demod.mix_info("u4", 2_400_000, CENTER, CENTER)


def _create(fmt, sr, out, resampler, k):
    h = _lib._h()
    st = _lib.lib().rfa_ddc_bank_create(0, fmt, sr, out, resampler, k, ctypes.byref(h))
    if st == _lib.RFA_OK:                       # a machine with a device: not what is asked here
        _lib.lib().rfa_ddc_bank_destroy(h)
    else:
        assert not h.value
    return st


@pytest.mark.parametrize("args,status", [
    ((9, 2_400_000, 96_000, 0, 2), _lib.RFA_ERR_INVALID),                   # no such format
    ((4, 2_400_000, 96_000, 0, 2), _lib.RFA_ERR_INVALID),                   # planar float: not a ddc format
    ((od.IN_F32_INTERLEAVED, 2_400_000, 96_000, 0, 2), _lib.RFA_ERR_UNSUPPORTED),
    ((od.IN_F32_INTERLEAVED, 2_400_000, 96_000, 1, 2), _lib.RFA_ERR_UNSUPPORTED),
    ((od.IN_U8, 2_400_000, 96_000, 0, 0), _lib.RFA_ERR_INVALID),
    ((od.IN_U8, 2_400_000, 96_000, 0, -3), _lib.RFA_ERR_INVALID),
    ((od.IN_U8, 2_400_000, 96_000, 0, 1025), _lib.RFA_ERR_INVALID),         # above RFA_DDC_BANK_MAX_CHANNELS
    ((od.IN_U8, 0, 96_000, 0, 2), _lib.RFA_ERR_INVALID),
    ((od.IN_U8, 2_400_000, -1, 1, 2), _lib.RFA_ERR_INVALID),
    ((od.IN_U8, 2_400_000, 96_000, 2, 2), _lib.RFA_ERR_INVALID),            # resampler is 0 or 1
])
def test_argument_errors_come_before_the_device_check(args, status):
    assert _create(*args) == status


def test_null_arguments():
    L = _lib.lib()
    assert L.rfa_ddc_bank_create(0, od.IN_U8, 2_400_000, 96_000, 0, 2, None) == _lib.RFA_ERR_INVALID
    assert L.rfa_ddc_bank_destroy(None) == _lib.RFA_ERR_INVALID
    assert L.rfa_ddc_bank_last_error(None) == b"null handle"
    got = ctypes.c_size_t(7)
    assert L.rfa_ddc_bank_process(None, None, 0, None, None, 0, ctypes.byref(got)) == _lib.RFA_ERR_INVALID
    assert L.rfa_ddc_bank_set_frequencies(None, 0, None) == _lib.RFA_ERR_INVALID
    assert L.rfa_ddc_bank_max_outputs(None, 16, ctypes.byref(got)) == _lib.RFA_ERR_INVALID


def _no_device():
    c = ctypes.c_int(0)
    return _lib.lib().rfa_device_count(ctypes.byref(c)) != _lib.RFA_OK or c.value == 0


def test_no_device_is_a_status_not_a_crash():
    if not _no_device():
        with demod.FrontEndBank("u8", 2_400_000, 96_000, 2) as bank:   # with a device the same call works
            assert bank.n_channels == 2
        return
    assert _create(od.IN_U8, 2_400_000, 96_000, 0, 2) == _lib.RFA_ERR_NODEVICE
    assert _create(od.IN_S8, 20_000_000, 384_000, 1, 256) == _lib.RFA_ERR_NODEVICE
    with pytest.raises(_lib.RfaError) as e:
        demod.FrontEndBank("u8", 2_400_000, 96_000, 2)
    assert e.value.status == _lib.RFA_ERR_NODEVICE
