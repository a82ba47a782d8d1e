"""ctypes binding of librfa.so (include/rfa.h).

The library is built in-tree (``python -m rfanalyzer_amd.build`` or
``__graft_entry__.build()``).  There is no CPU fallback anywhere in this
package: if the library is missing or no HIP device is visible, calls raise.
"""
from __future__ import annotations

import ctypes
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
# RFA_LIB: load an alternative build (A/B experiments, scripts/); default in-tree librfa.so
LIB_PATH = os.environ.get("RFA_LIB") or os.path.join(HERE, "librfa.so")
CSRC = os.path.join(HERE, "csrc")

RFA_OK = 0
RFA_ERR_INVALID = -1
RFA_ERR_SIZE = -2
RFA_ERR_UNSUPPORTED = -3
RFA_ERR_NODEVICE = -4
RFA_ERR_NOMEM = -5
RFA_ERR_HIP = -6
RFA_ERR_STATE = -7

RFA_PFB_MAX_INTERPOLATION = 64      # include/rfa.h
RFA_PFB_TUNE_MAX_STEPS = 1 << 20    # include/rfa.h
RFA_AUDIO_FIR_MAX_CHANNELS = 1024   # include/rfa.h
RFA_AUDIO_FIR_MAX_TAPS = 4096
RFA_AUDIO_FIR_TILE = 2048
RFA_AUDIO_FIR_NARROW_MAX = 512
RFA_AUDIO_FIR_PATHS = ("none", "copy", "narrow", "wide")    # RFA_AUDIO_FIR_PATH_* in order
RFA_AUDIO_FIR_PLAN_FIELDS = 5
RFA_AUDIO_RS_MAX_CHANNELS = 1024
RFA_AUDIO_RS_MAX_L = 160
RFA_AUDIO_RS_MAX_D = 1024
RFA_AUDIO_RS_MAX_TAPS = 16384
RFA_AUDIO_RS_MAX_PHASE_TAPS = 4096
RFA_AUDIO_RS_HISTORY = 4095
RFA_AUDIO_RS_MAX_TILE = 1024
RFA_AUDIO_RS_PATHS = ("none", "convert", "decimate", "polyphase")   # RFA_AUDIO_RS_PATH_* in order
RFA_AUDIO_RS_PLAN_FIELDS = 5
RFA_AUDIO_IIR_MAX_CHANNELS = 1024
RFA_AUDIO_IIR_MAX_SECTIONS = 8
RFA_AUDIO_IIR_BLOCK = 128
RFA_AUDIO_IIR_CHUNK_BLOCKS = 256
RFA_AUDIO_IIR_PATHS = ("none", "copy", "blocked")   # RFA_AUDIO_IIR_PATH_* in order
RFA_AUDIO_IIR_PLAN_FIELDS = 6

WINDOWS = {"blackman": 0, "hann": 1, "none": 2}
FORMATS = {"s8": 0, "u8": 1, "s16": 2, "f32": 3, "f32p": 4}
BYTES_PER_SAMPLE = {0: 2, 1: 2, 2: 4, 3: 8, 4: 8}
AVG_MODES = {"none": 0, "boxcar": 1, "ema": 2}


class RfaError(RuntimeError):
    def __init__(self, status: int, where: str, detail: str = ""):
        self.status = status
        msg = f"{where}: {status_string(status)} ({status})"
        if detail:
            msg += f": {detail}"
        super().__init__(msg)


class RfaConfig(ctypes.Structure):
    _fields_ = [
        ("fft_size", ctypes.c_int32),
        ("window", ctypes.c_int32),
        ("input_format", ctypes.c_int32),
        ("avg_mode", ctypes.c_int32),
        ("avg_length", ctypes.c_int32),
        ("ema_alpha", ctypes.c_float),
        ("peak_hold", ctypes.c_int32),
        ("ring_rows", ctypes.c_int32),
        ("device_id", ctypes.c_int32),
    ]


_lib = None
_fp = ctypes.POINTER(ctypes.c_float)
_vp = ctypes.c_void_p
_h = ctypes.c_void_p


def build(force: bool = False) -> str:
    """Compile librfa.so for gfx950 with hipcc (csrc/Makefile, incremental)."""
    if force:
        subprocess.run(["make", "-s", "-C", CSRC, "clean"], check=True)
    subprocess.run(["make", "-s", "-C", CSRC, "-j4"], check=True)
    return LIB_PATH


class RfaDrawParams(ctypes.Structure):
    """rfa_draw_params (include/rfa.h): AnalyzerSurface.drawPreprocessing inputs."""
    _fields_ = [("width", ctypes.c_int32), ("fft_height", ctypes.c_int32),
                ("viewport_frequency", ctypes.c_int64), ("viewport_sample_rate", ctypes.c_int64),
                ("min_db", ctypes.c_float), ("max_db", ctypes.c_float), ("average_length", ctypes.c_int32),
                ("colormap_size", ctypes.c_int32), ("colormap", ctypes.POINTER(ctypes.c_uint32))]


def _declare(lib: ctypes.CDLL) -> None:
    sig = {
        "rfa_abi_version": (ctypes.c_int, []),
        "rfa_device_count": (ctypes.c_int, [ctypes.POINTER(ctypes.c_int)]),
        "rfa_status_string": (ctypes.c_char_p, [ctypes.c_int]),
        "rfa_default_config": (None, [ctypes.POINTER(RfaConfig)]),
        "rfa_create": (ctypes.c_int, [ctypes.POINTER(RfaConfig), ctypes.POINTER(_h)]),
        "rfa_destroy": (ctypes.c_int, [_h]),
        "rfa_get_config": (ctypes.c_int, [_h, ctypes.POINTER(RfaConfig)]),
        "rfa_last_error": (ctypes.c_char_p, [_h]),
        "rfa_set_stream": (ctypes.c_int, [_h, _vp]),
        "rfa_get_stream": (ctypes.c_int, [_h, ctypes.POINTER(_vp)]),
        "rfa_use_own_stream": (ctypes.c_int, [_h]),
        "rfa_synchronize": (ctypes.c_int, [_h]),
        "rfa_set_pipelined": (ctypes.c_int, [_h, ctypes.c_int32]),
        "rfa_join": (ctypes.c_int, [_h]),
        "rfa_process": (ctypes.c_int, [_h, _vp, ctypes.c_size_t, ctypes.c_size_t, _vp]),
        "rfa_process_host": (ctypes.c_int, [_h, _vp, ctypes.c_size_t, ctypes.c_size_t, _vp]),
        "rfa_process_batches": (ctypes.c_int, [_h, _vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t,
                                               ctypes.c_size_t, _vp]),
        "rfa_set_tuning": (ctypes.c_int, [_h, ctypes.c_int64, ctypes.c_int64]),
        "rfa_push_packet": (ctypes.c_int, [_h, _vp, ctypes.c_size_t, ctypes.c_int64, ctypes.c_int64, _vp,
                                           ctypes.POINTER(ctypes.c_int32)]),
        "rfa_pending_samples": (ctypes.c_int, [_h, ctypes.POINTER(ctypes.c_int64)]),
        "rfa_get_state_generation": (ctypes.c_int, [_h, ctypes.POINTER(ctypes.c_int64)]),
        "rfa_get_peaks": (ctypes.c_int, [_h, _fp]),
        "rfa_get_ema": (ctypes.c_int, [_h, _fp]),
        "rfa_get_boxcar": (ctypes.c_int, [_h, ctypes.c_int32, _fp]),
        "rfa_get_ring": (ctypes.c_int, [_h, _fp, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]),
        "rfa_reset_state": (ctypes.c_int, [_h]),
        "rfa_set_ring_rows": (ctypes.c_int, [_h, ctypes.c_int32]),
        "rfa_set_fft_size": (ctypes.c_int, [_h, ctypes.c_int32]),
        "rfa_get_device_state": (ctypes.c_int, [_h, ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_vp)]),
        "rfa_get_ring_order": (ctypes.c_int, [_h, ctypes.POINTER(ctypes.c_int32)]),
        "rfa_get_ring_positions": (ctypes.c_int, [_h, ctypes.POINTER(ctypes.c_int32), ctypes.c_size_t]),
        "rfa_stream_copy": (ctypes.c_int, [_vp, _vp, ctypes.c_size_t, _vp]),
        "rfa_ddc_get_format": (ctypes.c_int, [_h, ctypes.POINTER(ctypes.c_int32)]),
        "rfa_windowed_fft_mag_planar": (ctypes.c_int, [_h, _fp, _fp, _fp, ctypes.c_size_t]),
        "rfa_fft_logmag_interleaved": (ctypes.c_int, [_h, _fp, _fp, ctypes.c_size_t]),
        "rfa_fft_ordered": (ctypes.c_int, [_h, _fp, _fp, ctypes.c_size_t]),
        "rfa_seam_supported": (ctypes.c_int, [ctypes.c_int32]),
        "rfa_seam_create": (ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(_h)]),
        "rfa_seam_destroy": (ctypes.c_int, [_h]),
        "rfa_seam_last_error": (ctypes.c_char_p, [_h]),
        "rfa_seam_get_plan": (ctypes.c_int, [_h, ctypes.POINTER(ctypes.c_int32), ctypes.c_int32,
                                             ctypes.POINTER(ctypes.c_int32)]),
        "rfa_seam_windowed_fft_mag_planar": (ctypes.c_int, [_h, _fp, _fp, _fp, ctypes.c_size_t]),
        "rfa_seam_fft_logmag_interleaved": (ctypes.c_int, [_h, _fp, _fp, ctypes.c_size_t]),
        "rfa_seam_fft_ordered": (ctypes.c_int, [_h, _fp, _fp, ctypes.c_size_t]),
        "rfa_set_profiling": (ctypes.c_int, [_h, ctypes.c_int]),
        "rfa_get_kernel_time": (ctypes.c_int, [_h, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64)]),
        "rfa_main_kernel_name": (ctypes.c_char_p, [_h]),
        "rfa_retune_offset": (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int, ctypes.c_int64]),
        "rfa_set_channel": (ctypes.c_int, [_h, ctypes.c_int64, ctypes.c_int64]),
        "rfa_draw_preprocess": (ctypes.c_int, [_h, ctypes.POINTER(RfaDrawParams), _vp, _fp, _fp, _fp]),
        "rfa_row_window_stats": (ctypes.c_int, [_h, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32),
                                                ctypes.c_size_t, _fp, _fp]),
        "rfa_set_windows": (ctypes.c_int, [_h, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32),
                                           ctypes.c_size_t]),
        "rfa_get_window_stats": (ctypes.c_int, [_h, _fp, _fp, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t),
                                                ctypes.POINTER(ctypes.c_size_t)]),
        "rfa_get_window_stats_device": (ctypes.c_int, [_h, ctypes.POINTER(_vp), ctypes.POINTER(_vp),
                                                       ctypes.POINTER(ctypes.c_size_t),
                                                       ctypes.POINTER(ctypes.c_size_t)]),
        "rfa_ring_window_stats": (ctypes.c_int, [_h, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32),
                                                 ctypes.c_size_t, ctypes.c_int32, _fp, _fp]),
        "rfa_get_channel_means": (ctypes.c_int, [_h, ctypes.POINTER(ctypes.c_float), ctypes.c_size_t,
                                                 ctypes.POINTER(ctypes.c_size_t)]),
        # demod front end (rfanalyzer_amd/demod.py)
        "rfa_ddc_create": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int32, ctypes.c_int32,
                                          ctypes.POINTER(_h)]),
        "rfa_ddc_create_resampler": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int32, ctypes.c_int32,
                                                    ctypes.POINTER(_h)]),
        "rfa_ddc_create_fir": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int32, _fp, ctypes.c_int32,
                                              ctypes.c_int32, ctypes.POINTER(_h)]),
        "rfa_ddc_set_stream": (ctypes.c_int, [_h, _vp]),
        "rfa_ddc_get_ratio": (ctypes.c_int, [_h, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32),
                                             ctypes.POINTER(ctypes.c_int32)]),
        "rfa_resampler_design": (ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_float,
                                                ctypes.c_int32, ctypes.POINTER(ctypes.c_int32),
                                                ctypes.POINTER(ctypes.c_int32), _fp, ctypes.c_size_t,
                                                ctypes.POINTER(ctypes.c_int32)]),
        "rfa_ddc_destroy": (ctypes.c_int, [_h]),
        "rfa_ddc_last_error": (ctypes.c_char_p, [_h]),
        "rfa_ddc_set_sample_rate": (ctypes.c_int, [_h, ctypes.c_int32]),
        "rfa_ddc_set_frequencies": (ctypes.c_int, [_h, ctypes.c_int64, ctypes.c_int64]),
        "rfa_ddc_process": (ctypes.c_int, [_h, _vp, ctypes.c_size_t, _vp, _vp, ctypes.c_size_t,
                                           ctypes.POINTER(ctypes.c_size_t)]),
        "rfa_ddc_process_host": (ctypes.c_int, [_h, _vp, ctypes.c_size_t, _vp, _vp, ctypes.c_size_t,
                                                ctypes.POINTER(ctypes.c_size_t)]),
        "rfa_ddc_synchronize": (ctypes.c_int, [_h]),
        "rfa_ddc_get_stream": (ctypes.c_int, [_h, ctypes.POINTER(_vp)]),
        "rfa_ddc_get_taps": (ctypes.c_int, [_h, _fp, ctypes.c_size_t, ctypes.POINTER(ctypes.c_int32),
                                            ctypes.POINTER(ctypes.c_int32)]),
        "rfa_ddc_get_mixer": (ctypes.c_int, [_h, _fp, _fp, ctypes.c_size_t, ctypes.POINTER(ctypes.c_int32),
                                             ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]),
        "rfa_lowpass_taps": (ctypes.c_int, [ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float,
                                            ctypes.c_float, ctypes.c_int32, _fp, ctypes.c_size_t,
                                            ctypes.POINTER(ctypes.c_int32)]),
        # front-end channel bank (rfanalyzer_amd/demod.py FrontEndBank, ReceiverBank)
        "rfa_ddc_bank_create": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int32, ctypes.c_int32,
                                               ctypes.c_int, ctypes.c_int32, ctypes.POINTER(_h)]),
        "rfa_ddc_bank_destroy": (ctypes.c_int, [_h]),
        "rfa_ddc_bank_last_error": (ctypes.c_char_p, [_h]),
        "rfa_ddc_bank_get_channels": (ctypes.c_int, [_h, ctypes.POINTER(ctypes.c_int32)]),
        "rfa_ddc_bank_set_sample_rate": (ctypes.c_int, [_h, ctypes.c_int32]),
        "rfa_ddc_bank_set_frequencies": (ctypes.c_int, [_h, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]),
        "rfa_ddc_bank_max_outputs": (ctypes.c_int, [_h, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]),
        "rfa_ddc_bank_process": (ctypes.c_int, [_h, _vp, ctypes.c_size_t, _vp, _vp, ctypes.c_size_t,
                                                ctypes.POINTER(ctypes.c_size_t)]),
        "rfa_ddc_bank_process_host": (ctypes.c_int, [_h, _vp, ctypes.c_size_t, _vp, _vp, ctypes.c_size_t,
                                                     ctypes.POINTER(ctypes.c_size_t)]),
        "rfa_ddc_bank_get_channel": (ctypes.c_int, [_h, ctypes.c_int32] + [ctypes.POINTER(ctypes.c_int32)] * 3),
        "rfa_ddc_bank_get_ratio": (ctypes.c_int, [_h] + [ctypes.POINTER(ctypes.c_int32)] * 3),
        "rfa_ddc_bank_get_taps": (ctypes.c_int, [_h, _fp, ctypes.c_size_t, ctypes.POINTER(ctypes.c_int32),
                                                 ctypes.POINTER(ctypes.c_int32)]),
        "rfa_ddc_bank_set_stream": (ctypes.c_int, [_h, _vp]),
        "rfa_ddc_bank_get_stream": (ctypes.c_int, [_h, ctypes.POINTER(_vp)]),
        "rfa_ddc_bank_synchronize": (ctypes.c_int, [_h]),
        "rfa_ddc_mix_info": (ctypes.c_int, [ctypes.c_int, ctypes.c_int32, ctypes.c_int64, ctypes.c_int64,
                                            ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]),
        "rfa_ddc_tile_plan": (ctypes.c_int, [ctypes.c_int32] * 4 + [ctypes.POINTER(ctypes.c_int32)]),
        # polyphase channelizer (rfanalyzer_amd/demod.py Channelizer, RasterReceiverBank)
        "rfa_pfb_supported": (ctypes.c_int, [ctypes.c_int32]),
        "rfa_pfb_create": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int32, ctypes.c_int32, _fp,
                                          ctypes.c_int32, ctypes.POINTER(_h)]),
        "rfa_pfb_destroy": (ctypes.c_int, [_h]),
        "rfa_pfb_last_error": (ctypes.c_char_p, [_h]),
        "rfa_pfb_get_plan": (ctypes.c_int, [_h] + [ctypes.POINTER(ctypes.c_int32)] * 4
                             + [ctypes.c_int32, ctypes.POINTER(ctypes.c_int32)]),
        "rfa_pfb_get_taps": (ctypes.c_int, [_h, _fp, ctypes.c_size_t, ctypes.POINTER(ctypes.c_int32)]),
        "rfa_pfb_set_channels": (ctypes.c_int, [_h, ctypes.POINTER(ctypes.c_int32), ctypes.c_int32]),
        "rfa_pfb_get_channels": (ctypes.c_int, [_h, ctypes.POINTER(ctypes.c_int32), ctypes.c_size_t,
                                                ctypes.POINTER(ctypes.c_int32)]),
        "rfa_pfb_max_outputs": (ctypes.c_int, [_h, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]),
        "rfa_pfb_process": (ctypes.c_int, [_h, _vp, ctypes.c_size_t, _vp, _vp, ctypes.c_size_t,
                                           ctypes.POINTER(ctypes.c_size_t)]),
        "rfa_pfb_process_host": (ctypes.c_int, [_h, _vp, ctypes.c_size_t, _vp, _vp, ctypes.c_size_t,
                                                ctypes.POINTER(ctypes.c_size_t)]),
        "rfa_pfb_reset": (ctypes.c_int, [_h]),
        "rfa_pfb_set_stream": (ctypes.c_int, [_h, _vp]),
        "rfa_pfb_get_stream": (ctypes.c_int, [_h, ctypes.POINTER(_vp)]),
        "rfa_pfb_synchronize": (ctypes.c_int, [_h]),
        "rfa_pfb_create_rational": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int32, ctypes.c_int32,
                                                   ctypes.c_int32, _fp, ctypes.c_int32, ctypes.POINTER(_h)]),
        "rfa_pfb_get_ratio": (ctypes.c_int, [_h] + [ctypes.POINTER(ctypes.c_int32)] * 3),
        "rfa_pfb_rational_outputs": (ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.c_uint64, ctypes.c_size_t,
                                                    ctypes.POINTER(ctypes.c_size_t)]),
        "rfa_pfb_tile_plan": (ctypes.c_int, [ctypes.c_int32] * 4 + [ctypes.POINTER(ctypes.c_int32)]),
        "rfa_pfb_set_tuning": (ctypes.c_int, [_h, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32), ctypes.c_int32]),
        "rfa_pfb_get_tuning": (ctypes.c_int, [_h, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32),
                                              ctypes.c_size_t, ctypes.POINTER(ctypes.c_int32)]),
        "rfa_pfb_tuning_index": (ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.c_uint64,
                                                ctypes.POINTER(ctypes.c_int32)]),
        "rfa_pfb_tuning_table": (ctypes.c_int, [ctypes.c_int32, _fp, _fp, ctypes.c_size_t]),
        # demodulator (rfanalyzer_amd/demod.py Demodulator, Receiver)
        "rfa_demod_mode_info": (ctypes.c_int, [ctypes.c_int] + [ctypes.POINTER(ctypes.c_int32)] * 4),
        "rfa_bandpass_taps": (ctypes.c_int, [ctypes.c_float] * 6 + [_fp, _fp, ctypes.c_size_t,
                                                                    ctypes.POINTER(ctypes.c_int32)]),
        "rfa_demod_create": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.POINTER(_h)]),
        "rfa_demod_destroy": (ctypes.c_int, [_h]),
        "rfa_demod_last_error": (ctypes.c_char_p, [_h]),
        "rfa_demod_set_mode": (ctypes.c_int, [_h, ctypes.c_int]),
        "rfa_demod_get_mode": (ctypes.c_int, [_h, ctypes.POINTER(ctypes.c_int32)]),
        "rfa_demod_set_channel_width": (ctypes.c_int, [_h, ctypes.c_int32]),
        "rfa_demod_get_channel_width": (ctypes.c_int, [_h, ctypes.POINTER(ctypes.c_int32)]),
        "rfa_demod_set_volume": (ctypes.c_int, [_h, ctypes.c_float]),
        "rfa_demod_set_audio_sink": (ctypes.c_int, [_h, ctypes.c_int]),
        "rfa_demod_process": (ctypes.c_int, [_h, _vp, _vp, ctypes.c_size_t, ctypes.c_size_t, _vp, ctypes.c_size_t,
                                             ctypes.POINTER(ctypes.c_size_t)]),
        "rfa_demod_process_host": (ctypes.c_int, [_h, _vp, _vp, ctypes.c_size_t, ctypes.c_size_t, _vp,
                                                  ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]),
        "rfa_demod_max_outputs": (ctypes.c_int, [_h, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]),
        "rfa_demod_get_taps": (ctypes.c_int, [_h, ctypes.c_int, _fp, _fp, ctypes.c_size_t,
                                              ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]),
        "rfa_demod_get_state": (ctypes.c_int, [_h, _fp, _fp, _fp]),
        "rfa_demod_reset": (ctypes.c_int, [_h]),
        "rfa_demod_set_stream": (ctypes.c_int, [_h, _vp]),
        "rfa_demod_get_stream": (ctypes.c_int, [_h, ctypes.POINTER(_vp)]),
        "rfa_demod_synchronize": (ctypes.c_int, [_h]),
        # demodulator bank (rfanalyzer_amd/demod.py DemodulatorBank, ReceiverBank)
        "rfa_demod_bank_create": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(ctypes.c_int32), ctypes.c_int32,
                                                 ctypes.POINTER(_h)]),
        "rfa_demod_bank_destroy": (ctypes.c_int, [_h]),
        "rfa_demod_bank_last_error": (ctypes.c_char_p, [_h]),
        "rfa_demod_bank_get_channels": (ctypes.c_int, [_h, ctypes.POINTER(ctypes.c_int32)]),
        "rfa_demod_bank_set_mode": (ctypes.c_int, [_h, ctypes.c_int32, ctypes.c_int]),
        "rfa_demod_bank_get_mode": (ctypes.c_int, [_h, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32)]),
        "rfa_demod_bank_set_channel_width": (ctypes.c_int, [_h, ctypes.c_int32, ctypes.c_int32]),
        "rfa_demod_bank_get_channel_width": (ctypes.c_int, [_h, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32)]),
        "rfa_demod_bank_set_volume": (ctypes.c_int, [_h, ctypes.c_int32, ctypes.c_float]),
        "rfa_demod_bank_set_audio_sink": (ctypes.c_int, [_h, ctypes.c_int32, ctypes.c_int]),
        "rfa_demod_bank_get_taps": (ctypes.c_int, [_h, ctypes.c_int32, ctypes.c_int, _fp, _fp, ctypes.c_size_t,
                                                   ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]),
        "rfa_demod_bank_get_state": (ctypes.c_int, [_h, ctypes.c_int32, _fp, _fp, _fp]),
        "rfa_demod_bank_reset": (ctypes.c_int, [_h, ctypes.c_int32]),
        "rfa_demod_bank_max_outputs": (ctypes.c_int, [_h, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]),
        "rfa_demod_bank_process": (ctypes.c_int, [_h, _vp, _vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t,
                                                  _vp, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]),
        "rfa_demod_bank_process_host": (ctypes.c_int, [_h, _vp, _vp, ctypes.c_size_t, ctypes.c_size_t,
                                                       ctypes.c_size_t, _vp, ctypes.c_size_t,
                                                       ctypes.POINTER(ctypes.c_size_t)]),
        "rfa_demod_bank_set_stream": (ctypes.c_int, [_h, _vp]),
        "rfa_demod_bank_get_stream": (ctypes.c_int, [_h, ctypes.POINTER(_vp)]),
        "rfa_demod_bank_synchronize": (ctypes.c_int, [_h]),
        # squelch bank: level meter + the Scheduler's squelch rule per slot (rfanalyzer_amd/csrc/squelch.hip)
        "rfa_squelch_level": (ctypes.c_float, [ctypes.c_double, ctypes.c_size_t, ctypes.c_float]),
        "rfa_squelch_step": (ctypes.c_int, [ctypes.c_int, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32)]),
        "rfa_squelch_create": (ctypes.c_int, [ctypes.c_int, ctypes.c_int32, ctypes.POINTER(_h)]),
        "rfa_squelch_destroy": (ctypes.c_int, [_h]),
        "rfa_squelch_last_error": (ctypes.c_char_p, [_h]),
        "rfa_squelch_get_channels": (ctypes.c_int, [_h, ctypes.POINTER(ctypes.c_int32)]),
        "rfa_squelch_set": (ctypes.c_int, [_h, ctypes.c_int32, ctypes.c_int, ctypes.c_float]),
        "rfa_squelch_get": (ctypes.c_int, [_h, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32), _fp]),
        "rfa_squelch_set_debounce": (ctypes.c_int, [_h, ctypes.c_int32]),
        "rfa_squelch_get_debounce": (ctypes.c_int, [_h, ctypes.POINTER(ctypes.c_int32)]),
        "rfa_squelch_reset": (ctypes.c_int, [_h]),
        "rfa_squelch_process": (ctypes.c_int, [_h, _vp, _vp, ctypes.c_size_t, ctypes.c_size_t, _vp, _vp]),
        "rfa_squelch_process_host": (ctypes.c_int, [_h, _vp, _vp, ctypes.c_size_t, ctypes.c_size_t, _vp, _vp]),
        "rfa_squelch_get_state": (ctypes.c_int, [_h, _vp, _vp, _vp, _vp]),
        "rfa_squelch_set_stream": (ctypes.c_int, [_h, _vp]),
        "rfa_squelch_get_stream": (ctypes.c_int, [_h, ctypes.POINTER(_vp)]),
        "rfa_squelch_synchronize": (ctypes.c_int, [_h]),
        # frequency meter bank: lag-1 autocorrelation per slot (rfanalyzer_amd/csrc/freq.hip)
        "rfa_freq_error_hz": (ctypes.c_double, [ctypes.c_double, ctypes.c_double, ctypes.c_double]),
        "rfa_freq_create": (ctypes.c_int, [ctypes.c_int, ctypes.c_int32, ctypes.POINTER(_h)]),
        "rfa_freq_destroy": (ctypes.c_int, [_h]),
        "rfa_freq_last_error": (ctypes.c_char_p, [_h]),
        "rfa_freq_get_channels": (ctypes.c_int, [_h, ctypes.POINTER(ctypes.c_int32)]),
        "rfa_freq_break": (ctypes.c_int, [_h, ctypes.c_int32]),
        "rfa_freq_reset": (ctypes.c_int, [_h]),
        "rfa_freq_process": (ctypes.c_int, [_h, _vp, _vp, ctypes.c_size_t, ctypes.c_size_t]),
        "rfa_freq_collect": (ctypes.c_int, [_h, _vp, _vp, _vp]),
        "rfa_freq_process_host": (ctypes.c_int, [_h, _vp, _vp, ctypes.c_size_t, ctypes.c_size_t, _vp, _vp, _vp]),
        "rfa_freq_set_stream": (ctypes.c_int, [_h, _vp]),
        "rfa_freq_get_stream": (ctypes.c_int, [_h, ctypes.POINTER(_vp)]),
        "rfa_freq_synchronize": (ctypes.c_int, [_h]),
        # tone meter bank: probe sums of every slot's audio row (rfanalyzer_amd/csrc/tone.hip)
        "rfa_tone_phasor": (ctypes.c_int, [ctypes.c_int32, ctypes.c_int64, ctypes.POINTER(ctypes.c_double),
                                           ctypes.POINTER(ctypes.c_double)]),
        "rfa_tone_quality": (ctypes.c_double, [ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                               ctypes.c_int64]),
        "rfa_tone_create": (ctypes.c_int, [ctypes.c_int, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(_h)]),
        "rfa_tone_destroy": (ctypes.c_int, [_h]),
        "rfa_tone_last_error": (ctypes.c_char_p, [_h]),
        "rfa_tone_get_channels": (ctypes.c_int, [_h, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]),
        "rfa_tone_set_probes": (ctypes.c_int, [_h, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32)]),
        "rfa_tone_get_probes": (ctypes.c_int, [_h, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32)]),
        "rfa_tone_break": (ctypes.c_int, [_h, ctypes.c_int32]),
        "rfa_tone_reset": (ctypes.c_int, [_h]),
        "rfa_tone_process": (ctypes.c_int, [_h, _vp, ctypes.c_size_t, _vp]),
        "rfa_tone_collect": (ctypes.c_int, [_h, _vp, _vp]),
        "rfa_tone_process_host": (ctypes.c_int, [_h, _vp, ctypes.c_size_t, _vp, _vp, _vp]),
        "rfa_tone_set_stream": (ctypes.c_int, [_h, _vp]),
        "rfa_tone_get_stream": (ctypes.c_int, [_h, ctypes.POINTER(_vp)]),
        "rfa_tone_synchronize": (ctypes.c_int, [_h]),
        # code meter bank: DCS sub-cell sums of every slot's audio row (rfanalyzer_amd/csrc/code.hip)
        "rfa_code_subcell": (ctypes.c_int, [ctypes.c_int32, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]),
        "rfa_code_word": (ctypes.c_int, [ctypes.c_int32, ctypes.POINTER(ctypes.c_uint32)]),
        "rfa_code_merge": (ctypes.c_int, [ctypes.c_int32, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, _vp,
                                          ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64),
                                          ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64),
                                          ctypes.POINTER(ctypes.c_int64)]),
        "rfa_code_create": (ctypes.c_int, [ctypes.c_int, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(_h)]),
        "rfa_code_destroy": (ctypes.c_int, [_h]),
        "rfa_code_last_error": (ctypes.c_char_p, [_h]),
        "rfa_code_get_channels": (ctypes.c_int, [_h, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]),
        "rfa_code_break": (ctypes.c_int, [_h, ctypes.c_int32]),
        "rfa_code_reset": (ctypes.c_int, [_h]),
        "rfa_code_process": (ctypes.c_int, [_h, _vp, ctypes.c_size_t, _vp]),
        "rfa_code_collect": (ctypes.c_int, [_h, _vp, _vp, _vp, ctypes.c_size_t, _vp, _vp]),
        "rfa_code_process_host": (ctypes.c_int, [_h, _vp, ctypes.c_size_t, _vp, _vp, _vp, _vp, ctypes.c_size_t, _vp,
                                                 _vp]),
        "rfa_code_set_stream": (ctypes.c_int, [_h, _vp]),
        "rfa_code_get_stream": (ctypes.c_int, [_h, ctypes.POINTER(_vp)]),
        "rfa_code_synchronize": (ctypes.c_int, [_h]),
        # audio FIR bank: a real FIR per slot on the audio rows (rfanalyzer_amd/csrc/audio_fir.hip)
        "rfa_audio_fir_plan": (ctypes.c_int, [ctypes.c_int32, ctypes.c_size_t, ctypes.POINTER(ctypes.c_int32)]),
        "rfa_audio_fir_history_source": (ctypes.c_int, [ctypes.c_size_t, ctypes.c_int32,
                                                        ctypes.POINTER(ctypes.c_int32),
                                                        ctypes.POINTER(ctypes.c_size_t)]),
        "rfa_audio_fir_create": (ctypes.c_int, [ctypes.c_int, ctypes.c_int32, ctypes.POINTER(_h)]),
        "rfa_audio_fir_destroy": (ctypes.c_int, [_h]),
        "rfa_audio_fir_last_error": (ctypes.c_char_p, [_h]),
        "rfa_audio_fir_get_channels": (ctypes.c_int, [_h, ctypes.POINTER(ctypes.c_int32)]),
        "rfa_audio_fir_set_taps": (ctypes.c_int, [_h, ctypes.c_int32, _fp, ctypes.c_int32]),
        "rfa_audio_fir_get_taps": (ctypes.c_int, [_h, ctypes.c_int32, _fp, ctypes.c_size_t,
                                                  ctypes.POINTER(ctypes.c_int32)]),
        "rfa_audio_fir_reset": (ctypes.c_int, [_h, ctypes.c_int32]),
        "rfa_audio_fir_process": (ctypes.c_int, [_h, _vp, ctypes.c_size_t, _vp, _vp, ctypes.c_size_t]),
        "rfa_audio_fir_process_host": (ctypes.c_int, [_h, _vp, ctypes.c_size_t, _vp, _vp, ctypes.c_size_t]),
        "rfa_audio_fir_set_stream": (ctypes.c_int, [_h, _vp]),
        "rfa_audio_fir_get_stream": (ctypes.c_int, [_h, ctypes.POINTER(_vp)]),
        "rfa_audio_fir_synchronize": (ctypes.c_int, [_h]),
        # audio resampler bank: every slot's audio row by L / D to s16 / f32 (rfanalyzer_amd/csrc/audio_rs.hip)
        "rfa_audio_rs_counts": (ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_size_t,
                                               ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_int32)]),
        "rfa_audio_rs_max_outputs": (ctypes.c_size_t, [ctypes.c_int32, ctypes.c_int32, ctypes.c_size_t]),
        "rfa_audio_rs_plan": (ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_size_t,
                                             ctypes.POINTER(ctypes.c_int32)]),
        "rfa_audio_rs_create": (ctypes.c_int, [ctypes.c_int, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _fp,
                                               ctypes.c_int32, ctypes.POINTER(_h)]),
        "rfa_audio_rs_destroy": (ctypes.c_int, [_h]),
        "rfa_audio_rs_last_error": (ctypes.c_char_p, [_h]),
        "rfa_audio_rs_get_channels": (ctypes.c_int, [_h, ctypes.POINTER(ctypes.c_int32)]),
        "rfa_audio_rs_get_ratio": (ctypes.c_int, [_h, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]),
        "rfa_audio_rs_get_taps": (ctypes.c_int, [_h, _fp, ctypes.c_size_t, ctypes.POINTER(ctypes.c_int32)]),
        "rfa_audio_rs_reset": (ctypes.c_int, [_h, ctypes.c_int32]),
        "rfa_audio_rs_get_offset": (ctypes.c_int, [_h, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32)]),
        "rfa_audio_rs_process": (ctypes.c_int, [_h, _vp, ctypes.c_size_t, _vp, _vp, ctypes.c_size_t, _vp,
                                                ctypes.c_size_t, _vp]),
        "rfa_audio_rs_process_host": (ctypes.c_int, [_h, _vp, ctypes.c_size_t, _vp, _vp, ctypes.c_size_t, _vp,
                                                     ctypes.c_size_t, _vp]),
        "rfa_audio_rs_set_stream": (ctypes.c_int, [_h, _vp]),
        "rfa_audio_rs_get_stream": (ctypes.c_int, [_h, ctypes.POINTER(_vp)]),
        "rfa_audio_rs_synchronize": (ctypes.c_int, [_h]),
        # audio IIR bank: recursive sections per slot on the audio rows (rfanalyzer_amd/csrc/audio_iir.hip)
        "rfa_audio_iir_tables": (ctypes.c_int, [ctypes.c_float, ctypes.c_float, _fp, _fp]),
        "rfa_audio_iir_plan": (ctypes.c_int, [ctypes.c_int32, ctypes.c_size_t, ctypes.c_int32,
                                              ctypes.POINTER(ctypes.c_int32)]),
        "rfa_audio_iir_carry_after": (ctypes.c_int, [ctypes.c_size_t, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32)]),
        "rfa_audio_iir_create": (ctypes.c_int, [ctypes.c_int, ctypes.c_int32, ctypes.POINTER(_h)]),
        "rfa_audio_iir_destroy": (ctypes.c_int, [_h]),
        "rfa_audio_iir_last_error": (ctypes.c_char_p, [_h]),
        "rfa_audio_iir_get_channels": (ctypes.c_int, [_h, ctypes.POINTER(ctypes.c_int32)]),
        "rfa_audio_iir_set_sections": (ctypes.c_int, [_h, ctypes.c_int32, _fp, ctypes.c_int32]),
        "rfa_audio_iir_get_sections": (ctypes.c_int, [_h, ctypes.c_int32, _fp, ctypes.c_size_t,
                                                      ctypes.POINTER(ctypes.c_int32)]),
        "rfa_audio_iir_reset": (ctypes.c_int, [_h, ctypes.c_int32]),
        "rfa_audio_iir_process": (ctypes.c_int, [_h, _vp, ctypes.c_size_t, _vp, _vp, ctypes.c_size_t]),
        "rfa_audio_iir_process_host": (ctypes.c_int, [_h, _vp, ctypes.c_size_t, _vp, _vp, ctypes.c_size_t]),
        "rfa_audio_iir_set_stream": (ctypes.c_int, [_h, _vp]),
        "rfa_audio_iir_get_stream": (ctypes.c_int, [_h, ctypes.POINTER(_vp)]),
        "rfa_audio_iir_synchronize": (ctypes.c_int, [_h]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args


def lib() -> ctypes.CDLL:
    """Load librfa.so (raises if it has not been built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} not built: run __graft_entry__.build() (no CPU fallback exists)")
        l = ctypes.CDLL(LIB_PATH)
        _declare(l)
        _lib = l
    return _lib


def status_string(status: int) -> str:
    try:
        return lib().rfa_status_string(status).decode()
    except Exception:  # noqa: BLE001 - library not loadable: plain text
        return str(status)


def check(status: int, where: str, handle=None) -> None:
    if status != RFA_OK:
        detail = ""
        if handle is not None:
            detail = (lib().rfa_last_error(handle) or b"").decode()
        raise RfaError(status, where, detail)


def device_count() -> int:
    c = ctypes.c_int(0)
    check(lib().rfa_device_count(ctypes.byref(c)), "rfa_device_count")
    return c.value
