"""CPU: what the five streaming stages take from csrc/stage_common.h and demod._Handle.  The
stream entries, destroy and last_error of every family answer a null handle (and a null
out-pointer) the same way, and every Python wrapper class sits on the one handle base with a
prefix whose entries _lib binds."""
import ctypes

import pytest

from rfanalyzer_amd import _lib
from rfanalyzer_amd import demod

CLASSES = {
    "rfa_ddc": demod.FrontEnd,
    "rfa_ddc_bank": demod.FrontEndBank,
    "rfa_demod": demod.Demodulator,
    "rfa_demod_bank": demod.DemodulatorBank,
    "rfa_pfb": demod.Channelizer,
}
SHARED = ["set_stream", "get_stream", "synchronize", "destroy", "last_error"]


@pytest.mark.parametrize("prefix", sorted(CLASSES))
def test_shared_entries_reject_a_null_handle(prefix):
    L = _lib.lib()
    vp = _lib._vp(0x55)
    assert getattr(L, f"{prefix}_set_stream")(None, None) == _lib.RFA_ERR_INVALID
    assert getattr(L, f"{prefix}_get_stream")(None, ctypes.byref(vp)) == _lib.RFA_ERR_INVALID
    assert vp.value == 0x55                     # nothing written
    assert getattr(L, f"{prefix}_get_stream")(None, None) == _lib.RFA_ERR_INVALID
    assert getattr(L, f"{prefix}_synchronize")(None) == _lib.RFA_ERR_INVALID
    assert getattr(L, f"{prefix}_destroy")(None) == _lib.RFA_ERR_INVALID
    err = getattr(L, f"{prefix}_last_error")(None)
    assert isinstance(err, bytes) and err == b"null handle"


@pytest.mark.parametrize("prefix", sorted(CLASSES))
def test_wrapper_class_sits_on_the_handle_base(prefix):
    cls = CLASSES[prefix]
    assert issubclass(cls, demod._Handle)
    assert cls._prefix == prefix
    L = _lib.lib()
    for e in SHARED + ["process", "process_host"]:
        fn = getattr(L, f"{prefix}_{e}")
        assert fn.argtypes is not None, f"{prefix}_{e}"
    for name in ("close", "__enter__", "__exit__", "__del__", "set_stream", "synchronize", "stream",
                 "_follow_torch_stream", "_call"):
        assert name not in vars(cls), f"{cls.__name__} restates {name}"
        assert hasattr(cls, name)


def test_fir_filter_is_a_front_end_handle():
    assert issubclass(demod.FirFilter, demod.FrontEnd) and demod.FirFilter._prefix == "rfa_ddc"
