"""Demod-branch front end on the GPU.

Host mirror of what the reference's demodulation branch does before the
demodulator proper (paths relative to app/src/main/java/com/mantz_it/rfanalyzer/):

* ``Scheduler.run`` hands every raw packet to ``source.mixPacketIntoSamplePacket(
  packet, demodBuffer, channelFrequency)`` (analyzer/Scheduler.kt:237-245), i.e.
  ``IQConverter.mixPacketIntoSamplePacket`` (source/Signed8BitIQConverter.java:101-130,
  Unsigned8BitIQConverter.java:101-130, Signed16BitIQConverter.kt:126-181): LUT
  conversion and an NCO down-mix by ``(int)(frequency - channelFrequency)``;
* ``Decimator.downsampling`` (analyzer/Decimator.java:175-191) filters the mixed
  packet with ``FirFilter.createLowPass(decimation, 1, inRate, 0.75*out, 0.25*out, 60)``
  and keeps every decimation-th output (dsp/FirFilter.kt:63-107).

``FrontEnd`` runs both in one HIP kernel (``rfanalyzer_amd/csrc/ddc.hip``) through
the C-ABI ``rfa_ddc_*`` (include/rfa.h).  Filter and mixer state carry over between
calls exactly as in the reference, so feeding packets one by one or a whole buffer
at once gives the same samples.  There is no CPU fallback: without librfa.so or a
HIP device every call raises.

``Demodulator`` is what follows in the app -- analyzer/Demodulator.kt:151-403 with the
AudioSink's decimators (analyzer/AudioSink.java:94-97,215-237): quadrature-rate samples
to 48 kHz audio through ``rfa_demod_*`` (``rfanalyzer_amd/csrc/demod.hip``) -- and
``Receiver`` chains a ``FrontEnd`` into it, raw IQ bytes to audio on one stream.

``FrontEndBank`` is K front ends on one raw stream in two launches per call
(``rfa_ddc_bank_*``): one filter, a mixer and a delay line per slot, each slot bit for bit a
``FrontEnd``.  ``DemodulatorBank`` is K demodulators in four launches per call
(``rfa_demod_bank_*``), each slot bit for bit a ``Demodulator``; ``ReceiverBank`` chains the
two banks.

``Channelizer`` is the front end for channels on a uniform raster (``rfa_pfb_*``): a polyphase
filter bank that gives all M channels k * Fs / M of one raw stream in two launches per call,
for a cost that does not grow with the channel count; ``RasterReceiverBank`` chains it into a
``DemodulatorBank``.  ``Channelizer.for_channels`` with ``set_offsets`` receives channels that are off
the raster through their nearest raster channel (a per-slot rotation fused into the channelizer's
store); ``TunedReceiverBank`` is that chain with ``ReceiverBank``'s interface.

``SquelchBank`` is the per-channel squelch of the bank chains (``rfa_squelch_*``): a level meter
on the quadrature rows and the Scheduler's squelch rule with its debounce per slot; a bank chain
built with ``squelch=`` holds the demodulator slots whose gate is closed.

``FrequencyMeterBank`` measures where each slot's signal sits relative to its centre (``rfa_freq_*``:
the lag-1 autocorrelation of the quadrature rows, summed on the device); ``AfcRule`` is the
per-slot control rule on the host, and ``ReceiverBank`` / ``TunedReceiverBank`` built with ``afc=``
retune their slots with the two.  The reference has no counterpart.

``CodeMeterBank`` sums every slot's quantised audio over the sub-cells of the 134.4 bit/s DCS bit
(``rfa_code_*``: exact int64 sums, an incomplete sub-cell carried to the next call); ``CodeRule``
correlates the cells with the wanted 23-bit word (``dcs_word``, ``dcs_parse``, ``DCS_CODES``;
``dcs_identify`` searches the table), and a bank chain built with ``code=`` reports no audio for a
slot whose code gate is closed.  The reference has no counterpart.

``AudioFilterBank`` is a real FIR on every slot's audio row behind the demodulator bank
(``rfa_audio_fir_*``): taps, history and count per slot, one launch per call; ``voice_taps`` is the
300 Hz high-pass that takes a CTCSS tone out of the voice, and a bank chain built with
``audio_filter=`` hands out the filtered rows.  The reference has no counterpart.

``AudioResamplerBank`` is the last stage of a K-channel voice logger (``rfa_audio_rs_*``): every
slot's audio row resampled by one rational ratio L / D through one prototype FIR and written as int16
PCM, float32 or both, one launch per call; ``resampler_taps`` designs the prototype, a bank chain
built with ``pcm=8000`` leaves the PCM in ``pcm_tensor`` and hands it out through ``pcm()``, and
``recording.AudioLogWriter`` writes one WAV per slot.  The reference has no counterpart.

``AudioIirBank`` is a cascade of up to 8 second-order recursive sections on every slot's audio row
(``rfa_audio_iir_*``): a blocked recurrence that a row cut into calls anywhere reproduces to the bit,
one launch per call; ``deemphasis_sections`` is an NFM receiver's 6 dB / octave de-emphasis,
``tone_strip_sections`` the 8th-order Chebyshev II high-pass that takes a CTCSS tone out of the voice
(DESIGN.md 5.7p has its measured cost next to the FIR's), and a bank chain built with ``audio_iir=`` runs it directly behind the
demodulators.  The reference has no counterpart.
"""
from __future__ import annotations

import ctypes
import functools
import math

import numpy as np

from . import _lib

FORMATS = {"s8": 0, "u8": 1, "s16": 2, "f32": 3}     # f32: already-mixed interleaved I,Q (filter only)
BYTES_PER_SAMPLE = {0: 2, 1: 2, 2: 4, 3: 8}


def _format_id(input_format: str) -> int:
    if input_format not in FORMATS:
        raise ValueError(f"input_format must be one of {sorted(FORMATS)}")
    return FORMATS[input_format]


def _raw_bytes(data) -> np.ndarray:
    """Host bytes or any numpy array as one contiguous uint8 array."""
    return np.ascontiguousarray(np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray, memoryview))
                                else np.asarray(data).view(np.uint8).reshape(-1))


class _Handle:
    """A stage handle of the C-ABI: the entries ``{_prefix}_*`` on ``self._h``, with the lifetime
    and stream methods that every stage has in the same form."""

    _prefix = ""
    _h = None
    _stream = None            # what set_stream was last given (None: the handle's own stream)

    def _create(self, entry: str, *args) -> None:
        """``entry(*args, &handle)``: every create entry returns the handle through its last argument."""
        h = _lib._h()
        _lib.check(getattr(_lib.lib(), entry)(*args, ctypes.byref(h)), entry)
        self._h = h

    def __init_subclass__(cls, **kwargs):
        super().__init_subclass__(**kwargs)
        if "_prefix" in vars(cls):
            cls._entries = {}     # name -> the bound C entry: a per-packet call looks nothing up twice

    def _call(self, name: str, *args) -> None:
        try:
            fn = self._entries[name]
        except KeyError:
            fn = self._entries[name] = getattr(_lib.lib(), f"{self._prefix}_{name}")
        status = fn(self._h, *args)
        if status:
            detail = (getattr(_lib.lib(), f"{self._prefix}_last_error")(self._h) or b"").decode()
            raise _lib.RfaError(status, f"{self._prefix}_{name}", detail)

    def _query_floats(self, name: str, n_arrays: int, n_ints: int, *pre):
        """A size-then-fill getter ``name(*pre, float * x n_arrays, capacity, int32 * x n_ints)`` whose
        first int32 is the arrays' length: (the arrays, the other int32 values)."""
        ints = [ctypes.c_int32(0) for _ in range(n_ints)]
        refs = [ctypes.byref(v) for v in ints]
        self._call(name, *pre, *[None] * n_arrays, 0, *refs)
        arrays = [np.empty(ints[0].value, np.float32) for _ in range(n_arrays)]
        self._call(name, *pre, *[a.ctypes.data_as(_lib._fp) for a in arrays], ints[0].value, *refs)
        return arrays, [v.value for v in ints[1:]]

    def close(self) -> None:
        if self._h:
            getattr(_lib.lib(), f"{self._prefix}_destroy")(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass

    def set_stream(self, stream_ptr: int | None) -> None:
        """Enqueue on exactly this hipStream_t (None: the handle's own stream)."""
        self._call("set_stream", stream_ptr or None)
        self._stream = stream_ptr or None

    def _follow_torch_stream(self, tensor) -> None:
        """Move to torch's current stream on the tensor's device, so that a call is ordered after
        the op that produced its inputs and before any later torch op that reads its outputs."""
        import torch

        cur = torch.cuda.current_stream(tensor.device).cuda_stream
        if cur != self._stream:
            self.set_stream(cur)

    def synchronize(self) -> None:
        self._call("synchronize")

    @property
    def stream(self) -> int:
        s = _lib._vp()
        self._call("get_stream", ctypes.byref(s))
        return s.value or 0


def create_low_pass_taps(gain: float, sample_rate: float, cutoff_frequency: float, transition_width: float,
                         attenuation_db: float, max_taps: int = 0) -> np.ndarray | None:
    """FirFilter.createLowPassTaps (dsp/FirFilter.kt:134-195), Blackman window; None where
    the reference returns null.  Host-only (no device work)."""
    L = _lib.lib()
    n = ctypes.c_int32(0)
    st = L.rfa_lowpass_taps(gain, sample_rate, cutoff_frequency, transition_width, attenuation_db, max_taps,
                            None, 0, ctypes.byref(n))
    if st == _lib.RFA_ERR_INVALID:
        return None
    _lib.check(st, "rfa_lowpass_taps")
    taps = np.empty(n.value, np.float32)
    _lib.check(L.rfa_lowpass_taps(gain, sample_rate, cutoff_frequency, transition_width, attenuation_db, max_taps,
                                  taps.ctypes.data_as(_lib._fp), taps.size, ctypes.byref(n)), "rfa_lowpass_taps")
    return taps


class FrontEnd(_Handle):
    """One demodulated channel: mix + decimate raw IQ on ``device``.

    ``resampler=True`` filters with the live app's Resampler (analyzer/Resampler.kt:
    RationalResampler of limitDenominator(out, in, 10000), Kaiser taps) instead of the
    Decimator.
    ``input_format`` "s8" (HackRF), "u8" (RTL-SDR), "s16" (Airspy/HydraSDR) or "f32"
    (already-mixed interleaved floats: the Decimator alone, as ResamplerTest drives it).
    """

    _prefix = "rfa_ddc"

    def __init__(self, input_format: str, sample_rate: int, output_sample_rate: int, device: int = 0,
                 resampler: bool = False, _fir=None):
        self.fmt = _format_id(input_format)
        self.output_sample_rate = output_sample_rate
        self.resampler = resampler
        if _fir is not None:  # FirFilter(taps, decimation): see FirFilter below
            taps, decimation = _fir
            taps = np.ascontiguousarray(taps, np.float32)
            self._create("rfa_ddc_create_fir", device, self.fmt, sample_rate, taps.ctypes.data_as(_lib._fp), taps.size,
                         decimation)
        else:
            self._create("rfa_ddc_create_resampler" if resampler else "rfa_ddc_create", device, self.fmt, sample_rate,
                         output_sample_rate)

    # -- configuration (IQConverter.setSampleRate / mixPacketIntoSamplePacket's table check)
    def set_sample_rate(self, sample_rate: int) -> None:
        self._call("set_sample_rate", sample_rate)

    def set_frequencies(self, frequency: int, channel_frequency: int) -> None:
        self._call("set_frequencies", frequency, channel_frequency)

    @property
    def taps(self) -> np.ndarray:
        return self._query_floats("get_taps", 1, 2)[0][0]

    @property
    def decimation(self) -> int:
        return self.ratio()[1]

    def mixer(self):
        """(cos_t, sin_t, mix_frequency, cosine_index) of the current mixer table."""
        (c, s), (mf, ci) = self._query_floats("get_mixer", 2, 3)
        return c, s, mf, ci

    def ratio(self):
        """(interpolation, decimation, taps per output) of the filter."""
        v = [ctypes.c_int32() for _ in range(3)]
        self._call("get_ratio", *[ctypes.byref(x) for x in v])
        return tuple(x.value for x in v)

    def max_outputs(self, n_samples: int) -> int:
        i, d, _ = self.ratio()
        return n_samples * i // max(d, 1) + 2

    # -- processing
    def process(self, data, frequency: int | None = None, channel_frequency: int | None = None):
        """Host bytes / numpy in -> (re, im) float32 numpy arrays of decimated samples."""
        if frequency is not None:
            self.set_frequencies(frequency, channel_frequency)
        buf = _raw_bytes(data)
        n = buf.size // BYTES_PER_SAMPLE[self.fmt]
        cap = self.max_outputs(n)
        re = np.empty(cap, np.float32)
        im = np.empty(cap, np.float32)
        got = ctypes.c_size_t(0)
        self._call("process_host", buf.ctypes.data, n, re.ctypes.data, im.ctypes.data, cap, ctypes.byref(got))
        return re[:got.value], im[:got.value]

    def process_device(self, in_ptr: int, n_samples: int, re_ptr: int, im_ptr: int, capacity: int) -> int:
        """Device pointers; asynchronous on the handle's stream; returns the output count."""
        got = ctypes.c_size_t(0)
        self._call("process", in_ptr, n_samples, re_ptr, im_ptr, capacity, ctypes.byref(got))
        return got.value

    def process_tensor(self, raw, out_re, out_im) -> int:
        """torch.cuda tensors: raw bytes (uint8/int8/int16/float32, contiguous) -> planar float32 outputs.
        Runs on torch's current stream, so it is ordered after the op that produced ``raw``
        and before any later torch op that reads the outputs."""
        self._follow_torch_stream(raw)
        n = raw.numel() * raw.element_size() // BYTES_PER_SAMPLE[self.fmt]
        if out_re.numel() != out_im.numel():
            raise ValueError("out_re and out_im must have the same length")
        return self.process_device(raw.data_ptr(), n, out_re.data_ptr(), out_im.data_ptr(), out_re.numel())


class FirFilter(FrontEnd):
    """dsp/FirFilter.kt on the device: ``FirFilter.createLowPass(decimation, gain, sampleRate,
    cutoff, transition, attenuation)`` (FirFilter.kt:243-263) or explicit taps, then
    ``filter(re, im)`` with the reference's delay line and decimation counter
    (FirFilter.kt:63-110) carried across calls.  Already-mixed float samples in."""

    def __init__(self, taps, decimation: int, sample_rate: int = 1, device: int = 0):
        super().__init__("f32", int(sample_rate), max(1, int(sample_rate) // max(1, int(decimation))), device,
                         _fir=(taps, int(decimation)))

    @classmethod
    def createLowPass(cls, decimation: int, gain: float, sample_rate: float, cutoff_frequency: float,  # noqa: N802
                      transition_width: float, attenuation_db: float, device: int = 0):
        taps = create_low_pass_taps(gain, sample_rate, cutoff_frequency, transition_width, attenuation_db)
        if taps is None:
            return None
        return cls(taps, decimation, max(1, int(sample_rate)), device)

    @property
    def numberOfTaps(self) -> int:  # noqa: N802
        return int(self.taps.size)

    def filter(self, re, im):
        """Planar float32 in -> (re, im) outputs (FirFilter.filter over a whole packet)."""
        re = np.asarray(re, np.float32)
        im = np.asarray(im, np.float32)
        iq = np.empty(2 * re.size, np.float32)
        iq[0::2], iq[1::2] = re, im
        return self.process(iq)


def mix_info(input_format: str, sample_rate: int, frequency: int, channel_frequency: int):
    """(folded mix frequency, mixer table length) that ``set_frequencies`` would build for one
    channel; length 0 is the empty table a ``FrontEndBank`` rejects.  Host-only."""
    mf, n = ctypes.c_int32(0), ctypes.c_int32(0)
    _lib.check(_lib.lib().rfa_ddc_mix_info(_format_id(input_format), sample_rate, frequency, channel_frequency,
                                           ctypes.byref(mf), ctypes.byref(n)), "rfa_ddc_mix_info")
    return mf.value, n.value


TILE_PLAN_FIELDS = ("P", "threads", "KC", "chunks", "pad", "row", "lds_bytes")   # rfa_ddc_plan_field order


def tile_plan(taps_per_output: int, interpolation: int, decimation: int, table_length: int) -> dict:
    """The workgroup tile plan of a front-end filter (``rfa_ddc_tile_plan``): outputs per
    workgroup ``P``, ``threads``, taps per LDS pass ``KC`` and the number of passes ``chunks``,
    ``pad`` (1: rows of ``row`` samples at an odd pitch, 0: linear), ``row`` and ``lds_bytes``.
    Arguments as ``FrontEnd.ratio()`` and the mixer table length give them (0 for "f32"; a bank
    plans with its longest table).  Host-only."""
    out = (ctypes.c_int32 * len(TILE_PLAN_FIELDS))()
    _lib.check(_lib.lib().rfa_ddc_tile_plan(taps_per_output, interpolation, decimation, table_length, out),
               "rfa_ddc_tile_plan")
    return dict(zip(TILE_PLAN_FIELDS, (int(v) for v in out)))


class FrontEndBank(_Handle):
    """``n_channels`` channels out of one raw IQ stream per call (``rfa_ddc_bank_*``): the slots
    share format, rates and filter, each has its own mixer and delay line, and slot k gives
    bit for bit what a ``FrontEnd`` with the same arguments and calls gives.  One call is two
    kernel launches whatever the channel count (up to 256; two per 256 beyond).  A channel
    whose mixer table would be empty (``mix_info`` length 0) is rejected at ``set_frequencies``."""

    _prefix = "rfa_ddc_bank"

    def __init__(self, input_format: str, sample_rate: int, output_sample_rate: int, n_channels: int,
                 device: int = 0, resampler: bool = False):
        self.fmt = _format_id(input_format)
        self.output_sample_rate = output_sample_rate
        self.resampler = resampler
        self.n_channels = int(n_channels)
        self._create("rfa_ddc_bank_create", device, self.fmt, sample_rate, output_sample_rate, 1 if resampler else 0,
                     self.n_channels)

    # -- configuration
    def set_sample_rate(self, sample_rate: int) -> None:
        self._call("set_sample_rate", sample_rate)

    def set_frequencies(self, frequency: int, channel_frequencies) -> None:
        """``FrontEnd.set_frequencies(frequency, channel_frequencies[k])`` on every slot, all or
        nothing: if one channel is rejected no slot changes."""
        ch = [int(c) for c in channel_frequencies]
        if len(ch) != self.n_channels:
            raise ValueError(f"{self.n_channels} channel frequencies expected, got {len(ch)}")
        arr = (ctypes.c_int64 * len(ch))(*ch)
        self._call("set_frequencies", int(frequency), arr)

    def channel(self, k: int):
        """(mix_frequency, table_length, cosine_index) of slot k's mixer."""
        v = [ctypes.c_int32(0) for _ in range(3)]
        self._call("get_channel", k, *[ctypes.byref(x) for x in v])
        return tuple(x.value for x in v)

    @property
    def taps(self) -> np.ndarray:
        return self._query_floats("get_taps", 1, 2)[0][0]

    def ratio(self):
        """(interpolation, decimation, taps per output) of the shared filter."""
        v = [ctypes.c_int32() for _ in range(3)]
        self._call("get_ratio", *[ctypes.byref(x) for x in v])
        return tuple(x.value for x in v)

    def max_outputs(self, n_samples: int) -> int:
        """Upper bound of one call's outputs per channel."""
        n = ctypes.c_size_t(0)
        self._call("max_outputs", n_samples, ctypes.byref(n))
        return n.value

    # -- processing
    def process(self, data):
        """Host bytes / numpy in -> (re[K, n], im[K, n]) float32 numpy arrays."""
        buf = _raw_bytes(data)
        n = buf.size // BYTES_PER_SAMPLE[self.fmt]
        cap = self.max_outputs(n)
        re = np.empty((self.n_channels, cap), np.float32)
        im = np.empty((self.n_channels, cap), np.float32)
        got = ctypes.c_size_t(0)
        self._call("process_host", buf.ctypes.data, n, re.ctypes.data, im.ctypes.data, cap, ctypes.byref(got))
        return re[:, :got.value], im[:, :got.value]

    def process_device(self, in_ptr: int, n_samples: int, re_ptr: int, im_ptr: int, channel_stride: int) -> int:
        """Device pointers, outputs [K][channel_stride] floats; asynchronous on the bank's stream;
        returns the output count per channel."""
        got = ctypes.c_size_t(0)
        self._call("process", in_ptr, n_samples, re_ptr, im_ptr, channel_stride, ctypes.byref(got))
        return got.value

    def process_tensor(self, raw, out_re, out_im) -> int:
        """torch.cuda tensors: raw bytes (contiguous) -> float32 outputs of shape [K, stride], on
        torch's current stream (see ``FrontEnd.process_tensor``)."""
        self._follow_torch_stream(raw)
        n = raw.numel() * raw.element_size() // BYTES_PER_SAMPLE[self.fmt]
        if out_re.shape != out_im.shape or out_re.dim() != 2 or out_re.shape[0] != self.n_channels:
            raise ValueError(f"out_re and out_im must both have shape [{self.n_channels}, stride]")
        if not (out_re.is_contiguous() and out_im.is_contiguous()):
            raise ValueError("out_re and out_im must be contiguous")
        return self.process_device(raw.data_ptr(), n, out_re.data_ptr(), out_im.data_ptr(), out_re.shape[1])


# ---------------------------------------------------------------- demodulator proper

MODES = {"off": 0, "am": 1, "nfm": 2, "wfm": 3, "lsb": 4, "usb": 5, "cw": 6}
TAPS = {"user": 0, "bandpass": 1, "audio1": 2, "audio2": 3}
AUDIO_RATE = 48000


def _mode_id(mode) -> int:
    if isinstance(mode, str):
        if mode.lower() not in MODES:
            raise ValueError(f"mode must be one of {sorted(MODES)}")
        return MODES[mode.lower()]
    return int(mode)


def mode_info(mode):
    """(quadrature rate, min, max, default channel width) of a DemodulationMode
    (analyzer/Demodulator.kt:52-61).  Host-only."""
    v = [ctypes.c_int32(0) for _ in range(4)]
    _lib.check(_lib.lib().rfa_demod_mode_info(_mode_id(mode), *[ctypes.byref(x) for x in v]), "rfa_demod_mode_info")
    return tuple(x.value for x in v)


def create_band_pass_taps(gain: float, sample_rate: float, low_cutoff: float, high_cutoff: float,
                          transition_width: float, attenuation_db: float):
    """ComplexFirFilter.createBandPass's taps (dsp/ComplexFirFilter.java:186-262) as (re, im);
    None where the reference returns null.  Host-only."""
    L = _lib.lib()
    n = ctypes.c_int32(0)
    args = (gain, sample_rate, low_cutoff, high_cutoff, transition_width, attenuation_db)
    st = L.rfa_bandpass_taps(*args, None, None, 0, ctypes.byref(n))
    if st == _lib.RFA_ERR_INVALID:
        return None
    _lib.check(st, "rfa_bandpass_taps")
    re = np.empty(n.value, np.float32)
    im = np.empty(n.value, np.float32)
    _lib.check(L.rfa_bandpass_taps(*args, re.ctypes.data_as(_lib._fp), im.ctypes.data_as(_lib._fp), re.size,
                                   ctypes.byref(n)), "rfa_bandpass_taps")
    return re, im


class Demodulator(_Handle):
    """analyzer/Demodulator.kt with its AudioSink on ``device``: quadrature-rate planar IQ
    in, 48 kHz float audio out (``rfanalyzer_amd/csrc/demod.hip`` through ``rfa_demod_*``).

    ``demodulationMode``, ``channelWidth`` and ``audioVolumeLevel`` behave as the Kotlin
    properties: setting the mode sets the width to the mode's default, the width is coerced
    into the mode's range, and every filter, AGC and carry-over state survives both.  A call
    may carry several packets (``packet_samples``); the result equals the reference run
    packet by packet.  ``audio_sink=False`` returns the demodulator's own audio buffer at the
    packet rate instead of the AudioSink's 48 kHz stream."""

    _prefix = "rfa_demod"

    def __init__(self, mode="off", device: int = 0, audio_sink: bool = True):
        self._create("rfa_demod_create", device, _mode_id(mode))
        if not audio_sink:
            self.audio_sink = False

    # -- the Kotlin properties
    @property
    def demodulationMode(self) -> int:  # noqa: N802
        m = ctypes.c_int32(0)
        self._call("get_mode", ctypes.byref(m))
        return m.value

    @demodulationMode.setter
    def demodulationMode(self, mode) -> None:  # noqa: N802
        self._call("set_mode", _mode_id(mode))

    @property
    def channelWidth(self) -> int:  # noqa: N802
        w = ctypes.c_int32(0)
        self._call("get_channel_width", ctypes.byref(w))
        return w.value

    @channelWidth.setter
    def channelWidth(self, width: int) -> None:  # noqa: N802
        self._call("set_channel_width", int(width))

    @property
    def audioVolumeLevel(self) -> float:  # noqa: N802
        return getattr(self, "_volume", 1.0)

    @audioVolumeLevel.setter
    def audioVolumeLevel(self, v: float) -> None:  # noqa: N802
        self._call("set_volume", float(v))
        self._volume = float(np.float32(v))

    @property
    def audio_sink(self) -> bool:
        return getattr(self, "_sink", True)

    @audio_sink.setter
    def audio_sink(self, enable: bool) -> None:
        self._call("set_audio_sink", 1 if enable else 0)
        self._sink = bool(enable)

    @property
    def quadrature_rate(self) -> int:
        return mode_info(self.demodulationMode)[0]

    # -- inspection
    def taps(self, which: str):
        """("user" | "bandpass" | "audio1" | "audio2") -> (re, im, decimation); empty before a
        packet has built the user or band-pass filter."""
        (re, im), (d,) = self._query_floats("get_taps", 2, 2, TAPS[which])
        return re, im, d

    def state(self):
        """(lastMax, carryOverSamplesRe, carryOverSamplesIm) as numpy float32; drains the stream."""
        v = [ctypes.c_float(0) for _ in range(3)]
        self._call("get_state", *[ctypes.byref(x) for x in v])
        return tuple(np.float32(x.value) for x in v)

    def reset(self) -> None:
        self._call("reset")

    def max_outputs(self, n_samples: int) -> int:
        n = ctypes.c_size_t(0)
        self._call("max_outputs", n_samples, ctypes.byref(n))
        return n.value

    # -- processing
    def process(self, re, im, packet_samples: int | None = None) -> np.ndarray:
        """Host planar float32 in -> float32 audio."""
        re = np.ascontiguousarray(re, np.float32)
        im = np.ascontiguousarray(im, np.float32)
        if re.shape != im.shape or re.ndim != 1:
            raise ValueError("re and im must be one-dimensional and of the same length")
        cap = self.max_outputs(re.size)
        out = np.empty(max(cap, 1), np.float32)
        got = ctypes.c_size_t(0)
        self._call("process_host", re.ctypes.data, im.ctypes.data, re.size, packet_samples or 0, out.ctypes.data, cap,
                   ctypes.byref(got))
        return out[:got.value].copy()

    def process_device(self, re_ptr: int, im_ptr: int, n_samples: int, audio_ptr: int, capacity: int,
                       packet_samples: int | None = None) -> int:
        """Device pointers; asynchronous on the handle's stream; returns the audio sample count."""
        got = ctypes.c_size_t(0)
        self._call("process", re_ptr, im_ptr, n_samples, packet_samples or 0, audio_ptr, capacity, ctypes.byref(got))
        return got.value

    def process_tensor(self, re, im, out, packet_samples: int | None = None) -> int:
        """torch.cuda float32 tensors; runs on torch's current stream, ordered after the op that
        produced ``re``/``im`` and before any later torch op that reads ``out``."""
        self._follow_torch_stream(re)
        if re.numel() != im.numel():
            raise ValueError("re and im must have the same length")
        return self.process_device(re.data_ptr(), im.data_ptr(), re.numel(), out.data_ptr(), out.numel(),
                                   packet_samples)


class DemodulatorBank(_Handle):
    """``len(modes)`` demodulators, each with its AudioSink, in one handle (``rfa_demod_bank_*``):
    one stream and one set of launches -- four kernels and one copy of the slots' launch
    records per call, whatever the slot count.  Slot k gives bit for bit what a ``Demodulator``
    with the same settings and calls gives; the per-slot methods behave as its properties do.
    Modes of different quadrature rates may share a bank; an "off" slot returns no audio and
    keeps its state."""

    _prefix = "rfa_demod_bank"

    def __init__(self, modes, device: int = 0, audio_sink: bool = True):
        ids = [_mode_id(m) for m in modes]
        self.n_channels = len(ids)
        arr = (ctypes.c_int32 * max(len(ids), 1))(*ids)
        self._create("rfa_demod_bank_create", device, arr, len(ids))
        self._counts = (ctypes.c_size_t * self.n_channels)()
        self._held = {}                           # slot -> (mode, width) put aside by set_hold
        if not audio_sink:
            for k in range(self.n_channels):
                self.set_audio_sink(k, False)

    # -- per slot, as the Demodulator's properties
    def mode(self, k: int) -> int:
        if k in self._held:
            return self._held[k][0]
        m = ctypes.c_int32(0)
        self._call("get_mode", k, ctypes.byref(m))
        return m.value

    def set_mode(self, k: int, mode) -> None:
        if k in self._held:                       # applied when the hold is released
            self._held[k] = (_mode_id(mode), mode_info(mode)[3])
        else:
            self._call("set_mode", k, _mode_id(mode))

    def channel_width(self, k: int) -> int:
        if k in self._held:
            return self._held[k][1]
        w = ctypes.c_int32(0)
        self._call("get_channel_width", k, ctypes.byref(w))
        return w.value

    def set_channel_width(self, k: int, width: int) -> None:
        if k in self._held:                       # coerced into the slot's own mode's limits, as the handle does
            mode, _ = self._held[k]
            _, lo, hi, _ = mode_info(mode)
            self._held[k] = (mode, min(max(int(width), lo), hi))
        else:
            self._call("set_channel_width", k, int(width))

    def set_hold(self, k: int, on: bool) -> None:
        """Hold slot k: until released, a call passes it over exactly as it passes over an "off"
        slot -- no audio, a count of 0 (``max_outputs`` too), no filter designed, every state and
        filter counter kept -- so the slot equals a ``Demodulator`` that was given only the calls
        made while it was not held.  The bank has one way of passing a slot over, its "off" mode:
        a hold puts the slot's mode and width aside, switches the slot off, and puts both back on
        release (a filter is stale by mode and width alone, so nothing is rebuilt that would not
        have been); ``mode``, ``set_mode``, ``channel_width`` and ``set_channel_width`` of a held
        slot read and change what is put aside."""
        if not 0 <= k < self.n_channels:
            raise _lib.RfaError(_lib.RFA_ERR_INVALID, "DemodulatorBank.set_hold", "no such slot")
        if on and k not in self._held:
            saved = (self.mode(k), self.channel_width(k))
            self._call("set_mode", k, MODES["off"])
            self._held[k] = saved
        elif not on and k in self._held:
            mode, width = self._held.pop(k)
            self._call("set_mode", k, mode)
            self._call("set_channel_width", k, width)

    def hold(self, k: int) -> bool:
        if not 0 <= k < self.n_channels:
            raise _lib.RfaError(_lib.RFA_ERR_INVALID, "DemodulatorBank.hold", "no such slot")
        return k in self._held

    def set_volume(self, k: int, v: float) -> None:
        self._call("set_volume", k, float(v))

    def set_audio_sink(self, k: int, on: bool) -> None:
        self._call("set_audio_sink", k, 1 if on else 0)

    def taps(self, k: int, which: str):
        """Slot k's ("user" | "bandpass" | "audio1" | "audio2") -> (re, im, decimation)."""
        (re, im), (d,) = self._query_floats("get_taps", 2, 2, k, TAPS[which])
        return re, im, d

    def state(self, k: int):
        """Slot k's (lastMax, carryOverSamplesRe, carryOverSamplesIm); drains the stream."""
        v = [ctypes.c_float(0) for _ in range(3)]
        self._call("get_state", k, *[ctypes.byref(x) for x in v])
        return tuple(np.float32(x.value) for x in v)

    def reset(self, k: int) -> None:
        self._call("reset", k)

    def max_outputs(self, n_samples: int) -> list[int]:
        """Every slot's audio sample count for the next call of ``n_samples``."""
        n = (ctypes.c_size_t * self.n_channels)()
        self._call("max_outputs", n_samples, n)
        return list(n)

    # -- processing
    def process(self, re, im, packet_samples: int | None = None) -> list[np.ndarray]:
        """Host planar float32 [K, n] in -> K float32 audio arrays."""
        re = np.ascontiguousarray(re, np.float32)
        im = np.ascontiguousarray(im, np.float32)
        if re.shape != im.shape or re.ndim != 2 or re.shape[0] != self.n_channels:
            raise ValueError(f"re and im must both have shape [{self.n_channels}, n]")
        n = re.shape[1]
        cap = max(self.max_outputs(n))
        out = np.empty((self.n_channels, max(cap, 1)), np.float32)
        self._call("process_host", re.ctypes.data, im.ctypes.data, n, n, packet_samples or 0, out.ctypes.data,
                   out.shape[1], self._counts)
        return [out[k, :g].copy() for k, g in enumerate(self._counts)]

    def process_device(self, re_ptr: int, im_ptr: int, channel_stride: int, n_samples: int, audio_ptr: int,
                       audio_stride: int, packet_samples: int | None = None) -> list[int]:
        """Device pointers, rows ``channel_stride`` / ``audio_stride`` floats apart; asynchronous on
        the bank's stream; returns every slot's audio sample count."""
        self._call("process", re_ptr, im_ptr, channel_stride, n_samples, packet_samples or 0, audio_ptr, audio_stride,
                   self._counts)
        return list(self._counts)

    def process_tensor(self, re, im, out, packet_samples: int | None = None) -> list[int]:
        """torch.cuda float32 tensors [K, n] (rows may be slices of wider tensors: unit stride
        along n) -> ``out`` [K, capacity]; on torch's current stream (see
        ``Demodulator.process_tensor``)."""
        self._follow_torch_stream(re)
        K = self.n_channels
        if re.shape != im.shape or re.dim() != 2 or re.shape[0] != K or out.dim() != 2 or out.shape[0] != K:
            raise ValueError(f"re, im and out must have shape [{K}, .]")
        for t in (re, im, out):
            if t.shape[1] > 1 and t.stride(1) != 1:
                raise ValueError("rows must be contiguous")
        if K > 1 and re.stride(0) != im.stride(0):
            raise ValueError("re and im must have the same row stride")
        stride = re.stride(0) if K > 1 else re.shape[1]
        ostride = out.stride(0) if K > 1 else out.shape[1]
        if K > 1 and ostride < out.shape[1]:
            raise ValueError("out's rows overlap")
        if ostride > out.shape[1] and max(self.max_outputs(re.shape[1])) > out.shape[1]:
            # rows of a wider tensor: the C entry's capacity is the row pitch, the view is narrower
            raise _lib.RfaError(_lib.RFA_ERR_SIZE, "rfa_demod_bank_process", "out's rows are too short for a slot")
        return self.process_device(re.data_ptr(), im.data_ptr(), stride, re.shape[1], out.data_ptr(), ostride,
                                   packet_samples)


class SquelchBank(_Handle):
    """Level meter and squelch gate for ``n_channels`` slots (``rfa_squelch_*``,
    ``rfanalyzer_amd/csrc/squelch.hip``).  A call measures every slot's quadrature row,
    ``level = 5 * log10(mean(re^2 + im^2))`` -- the reference's magnitude-dB, 10 * log10(A) for a
    tone of amplitude A -- and steps the Scheduler's rule per slot (Scheduler.kt:161-165,237):
    a slot is open while its level is above its threshold, and for ``debounce - 1`` more calls.
    A slot without a threshold is always open.  The sums are bit-identical from run to run and
    for any placement of the rows."""

    _prefix = "rfa_squelch"

    def __init__(self, n_channels: int, device: int = 0):
        self.n_channels = int(n_channels)
        self._create("rfa_squelch_create", device, self.n_channels)
        self._levels = np.full(self.n_channels, -999.0, np.float32)
        self._open = np.ones(self.n_channels, np.uint8)

    def set(self, k: int, threshold_db: float | None) -> None:
        """Slot k's threshold in dB; None disables its squelch (always open)."""
        self._call("set", k, 0 if threshold_db is None else 1, 0.0 if threshold_db is None else float(threshold_db))

    def get(self, k: int) -> float | None:
        on, thr = ctypes.c_int32(0), ctypes.c_float(0)
        self._call("get", k, ctypes.byref(on), ctypes.byref(thr))
        return float(thr.value) if on.value else None

    @property
    def debounce(self) -> int:
        v = ctypes.c_int32(0)
        self._call("get_debounce", ctypes.byref(v))
        return v.value

    @debounce.setter
    def debounce(self, calls: int) -> None:
        self._call("set_debounce", int(calls))

    def reset(self) -> None:
        """Counters to 0 and levels to -999; thresholds and debounce stay."""
        self._call("reset")

    def _result(self):
        return self._levels.copy(), self._open.astype(bool)

    def process_device(self, re_ptr: int, im_ptr: int, channel_stride: int, n_samples: int):
        """Device pointers, rows ``channel_stride`` floats apart -> (levels float32[K], open
        bool[K]).  Enqueued on the handle's stream; returns once the K sums have arrived, which
        is after everything enqueued on that stream before it."""
        self._call("process", re_ptr, im_ptr, channel_stride, n_samples, self._levels.ctypes.data,
                   self._open.ctypes.data)
        return self._result()

    def process(self, re, im):
        """Host planar float32 [K, n] -> (levels, open)."""
        re = np.ascontiguousarray(re, np.float32)
        im = np.ascontiguousarray(im, np.float32)
        if re.shape != im.shape or re.ndim != 2 or re.shape[0] != self.n_channels:
            raise ValueError(f"re and im must both have shape [{self.n_channels}, n]")
        n = re.shape[1]
        self._call("process_host", re.ctypes.data, im.ctypes.data, n, n, self._levels.ctypes.data,
                   self._open.ctypes.data)
        return self._result()

    def process_tensor(self, re, im):
        """torch.cuda float32 tensors [K, n] (rows may be slices of wider tensors) -> (levels,
        open); on torch's current stream."""
        self._follow_torch_stream(re)
        K = self.n_channels
        if re.shape != im.shape or re.dim() != 2 or re.shape[0] != K:
            raise ValueError(f"re and im must have shape [{K}, n]")
        if re.dtype != im.dtype or str(re.dtype) != "torch.float32":
            raise ValueError("re and im must be float32")
        for t in (re, im):
            if t.shape[1] > 1 and t.stride(1) != 1:
                raise ValueError("rows must be contiguous")
        if K > 1 and re.stride(0) != im.stride(0):
            raise ValueError("re and im must have the same row stride")
        stride = re.stride(0) if K > 1 else re.shape[1]
        return self.process_device(re.data_ptr(), im.data_ptr(), stride, re.shape[1])

    def state(self) -> dict:
        """The last call's ``sums`` (float64), ``levels``, ``counters`` and ``open``, per slot."""
        K = self.n_channels
        sums, levels = np.empty(K, np.float64), np.empty(K, np.float32)
        counters, opn = np.empty(K, np.int32), np.empty(K, np.uint8)
        self._call("get_state", sums.ctypes.data, levels.ctypes.data, counters.ctypes.data, opn.ctypes.data)
        return {"sums": sums, "levels": levels, "counters": counters, "open": opn.astype(bool)}


def frequency_error_hz(re: float, im: float, rate: float) -> float:
    """``atan2(im, re) * rate / (2 pi)`` of a lag-1 autocorrelation (``rfa_freq_error_hz``): how far
    above the slot's centre its signal sits.  0 for R1 = 0, NaN where a sum is not finite.  Host only."""
    return float(_lib.lib().rfa_freq_error_hz(float(re), float(im), float(rate)))


class FrequencyMeterBank(_Handle):
    """Frequency-error meter for ``n_channels`` slots (``rfa_freq_*``, ``rfanalyzer_amd/csrc/freq.hip``).
    A call sums every slot's lag-1 autocorrelation ``R1 = sum x[i] * conj(x[i-1])`` over its quadrature
    row, in double, with the slot's last sample of the previous call as ``x[-1]`` (kept on the device;
    ``break_`` drops it).  ``frequency_error_hz`` turns a pair of sums into Hz.  The sums are
    bit-identical from run to run and for any placement of the rows.  ``process_device`` is
    asynchronous; ``collect`` waits for its copy of the sums alone."""

    _prefix = "rfa_freq"

    def __init__(self, n_channels: int, device: int = 0):
        self.n_channels = int(n_channels)
        self._create("rfa_freq_create", device, self.n_channels)
        self._re = np.zeros(self.n_channels, np.float64)
        self._im = np.zeros(self.n_channels, np.float64)
        self._terms = np.zeros(self.n_channels, np.int64)

    def _out(self):
        return self._re.ctypes.data, self._im.ctypes.data, self._terms.ctypes.data

    def _result(self):
        return self._re.copy(), self._im.copy(), self._terms.copy()

    def break_(self, k: int | None = None) -> None:
        """Drop slot k's carried sample (None: every slot's): its next call has one term less and no
        predecessor.  For a slot whose phase is about to jump.  Ordered on the stream, no wait."""
        self._call("break", -1 if k is None else int(k))

    def reset(self) -> None:
        """Drop every carry and the last results."""
        self._call("reset")

    def process_device(self, re_ptr: int, im_ptr: int, channel_stride: int, n_samples: int) -> None:
        """Device pointers, rows ``channel_stride`` floats apart.  Enqueues the sums and their copy on
        the handle's stream and returns; ``collect`` hands them out."""
        self._call("process", re_ptr, im_ptr, channel_stride, n_samples)

    def collect(self):
        """(r1_re float64[K], r1_im float64[K], terms int64[K]) of the last ``process_device``; waits
        for that call's copy and nothing else."""
        self._call("collect", *self._out())
        return self._result()

    def process(self, re, im):
        """Host planar float32 [K, n] -> (r1_re, r1_im, terms)."""
        re = np.ascontiguousarray(re, np.float32)
        im = np.ascontiguousarray(im, np.float32)
        if re.shape != im.shape or re.ndim != 2 or re.shape[0] != self.n_channels:
            raise ValueError(f"re and im must both have shape [{self.n_channels}, n]")
        n = re.shape[1]
        self._call("process_host", re.ctypes.data, im.ctypes.data, n, n, *self._out())
        return self._result()

    def process_tensor(self, re, im):
        """torch.cuda float32 tensors [K, n] (rows may be slices of wider tensors) -> (r1_re, r1_im,
        terms); on torch's current stream."""
        self._follow_torch_stream(re)
        K = self.n_channels
        if re.shape != im.shape or re.dim() != 2 or re.shape[0] != K:
            raise ValueError(f"re and im must have shape [{K}, n]")
        if re.dtype != im.dtype or str(re.dtype) != "torch.float32":
            raise ValueError("re and im must be float32")
        for t in (re, im):
            if t.shape[1] > 1 and t.stride(1) != 1:
                raise ValueError("rows must be contiguous")
        if K > 1 and re.stride(0) != im.stride(0):
            raise ValueError("re and im must have the same row stride")
        stride = re.stride(0) if K > 1 else re.shape[1]
        self.process_device(re.data_ptr(), im.data_ptr(), stride, re.shape[1])
        return self.collect()


class AfcRule:
    """Automatic frequency control for ``n_channels`` slots at quadrature rate ``rate``: what to do
    with the sums of a ``FrequencyMeterBank``.  Host arithmetic only, no device.

    ``update(r1_re, r1_im, active)`` adds the sums of the active slots into one double accumulator
    pair per slot and counts the call.  On every ``interval``-th call each slot that was active at
    least once turns its accumulated R1 into an error estimate ``err`` (``frequency_error_hz``); a
    slot whose R1 is 0 or whose estimate is not finite is passed over.  ``err`` was measured while
    the slot's applied correction ``a`` was in force, so the signal sits at ``a + err``, and the
    rule moves its estimate ``c`` towards that: ``c <- clamp(c + gain * (a + err - c), +-limit_hz)``
    -- for ``gain = 1`` the new estimate itself, and ``c + gain * err`` where ``c`` is what was
    applied.  The applied correction is ``c`` rounded to the nearest multiple of ``step_hz`` (a tie
    goes up), so a residual below half a step moves nothing and the output cannot hunt between two
    multiples.  ``update`` returns the slots whose applied correction changed (an empty list
    between intervals) and clears the accumulators.

    ``step_hz = 25``, ``interval = 8`` and ``gain = 1`` are parameters chosen by hand, not
    measurements: a step well below any mode's filter width, an interval of a few packets.
    ``limit_hz`` (a number or one per slot) has no default here; the chains use half the mode's
    default width."""

    def __init__(self, n_channels: int, rate: float, *, step_hz: float = 25, limit_hz, interval: int = 8,
                 gain: float = 1.0):
        K = int(n_channels)
        if K < 1:
            raise ValueError("at least one slot")
        if not (math.isfinite(rate) and rate > 0):
            raise ValueError("rate must be positive")
        if not (math.isfinite(step_hz) and step_hz > 0):
            raise ValueError("step_hz must be positive")
        if int(interval) != interval or interval < 1:
            raise ValueError("interval must be a whole number of calls, at least 1")
        if not (math.isfinite(gain) and 0 < gain <= 1):
            raise ValueError("gain must lie in (0, 1]")
        limit = np.array(np.broadcast_to(np.asarray(limit_hz, np.float64), (K,)))
        if not (limit >= 0).all():
            raise ValueError("limit_hz must be zero or more")
        self.n_channels, self.rate = K, float(rate)
        self.step_hz, self.interval, self.gain = float(step_hz), int(interval), float(gain)
        self.limit_hz = limit
        self._acc_re, self._acc_im = np.zeros(K), np.zeros(K)
        self._seen = np.zeros(K, bool)
        self._estimate, self._applied = np.zeros(K), np.zeros(K)
        self._errors = np.full(K, np.nan)
        self._calls = 0

    @property
    def corrections(self) -> np.ndarray:
        """The applied correction per slot in Hz, multiples of ``step_hz`` (float64[K])."""
        return self._applied.copy()

    @property
    def errors_hz(self) -> np.ndarray:
        """Every slot's last error estimate in Hz (float64[K]); NaN before its first."""
        return self._errors.copy()

    def reset(self, k: int | None = None) -> None:
        """Slot k (None: every slot, and the call count) back to no correction and no estimate."""
        s = slice(None) if k is None else self._slot(k)
        for a, v in ((self._acc_re, 0.0), (self._acc_im, 0.0), (self._seen, False), (self._estimate, 0.0),
                     (self._applied, 0.0), (self._errors, np.nan)):
            a[s] = v
        if k is None:
            self._calls = 0

    def _slot(self, k: int) -> int:
        if not 0 <= int(k) < self.n_channels:
            raise ValueError(f"no slot {k}")
        return int(k)

    def update(self, r1_re, r1_im, active=None) -> list[int]:
        K = self.n_channels
        r1_re, r1_im = np.asarray(r1_re, np.float64), np.asarray(r1_im, np.float64)
        act = np.ones(K, bool) if active is None else np.asarray(active, bool)
        if r1_re.shape != (K,) or r1_im.shape != (K,) or act.shape != (K,):
            raise ValueError(f"{K} sums and flags expected")
        with np.errstate(all="ignore"):
            self._acc_re[act] += r1_re[act]
            self._acc_im[act] += r1_im[act]
        self._seen |= act
        self._calls += 1
        if self._calls % self.interval:
            return []
        changed = []
        for k in np.flatnonzero(self._seen):
            re, im = self._acc_re[k], self._acc_im[k]
            if re == 0.0 and im == 0.0:
                continue
            err = frequency_error_hz(re, im, self.rate)
            if not math.isfinite(err):
                continue
            self._errors[k] = err
            lim = self.limit_hz[k]
            c = self._estimate[k] + self.gain * (self._applied[k] + err - self._estimate[k])
            c = self._estimate[k] = min(max(c, -lim), lim)
            applied = self.step_hz * math.floor(c / self.step_hz + 0.5)
            if applied != self._applied[k]:
                self._applied[k] = applied
                changed.append(int(k))
        self._acc_re[:] = 0.0
        self._acc_im[:] = 0.0
        self._seen[:] = False
        return changed


AFC_MODES = ("am", "nfm", "wfm")          # modes with a carrier at the slot's centre
_AFC_MODE_IDS = frozenset(MODES[m] for m in AFC_MODES)


def _afc_rule(afc, modes, rate: int):
    """The ``afc=`` keyword of a bank chain -> (an ``AfcRule`` or None, whether ``limit_hz`` is the
    default).  Host only: a wrong keyword raises before any handle is made."""
    if afc is None or afc is False:
        return None, False
    if afc is True:
        afc = {}
    if not isinstance(afc, dict):
        raise TypeError("afc must be None, True or a dict of AfcRule's keywords")
    kw = dict(afc)
    default_limit = "limit_hz" not in kw
    if default_limit:
        kw["limit_hz"] = [mode_info(m)[3] / 2 for m in modes]
    return AfcRule(len(modes), rate, **kw), default_limit


# ---------------------------------------------------------------- CTCSS tone squelch

# The 50 standard CTCSS tones in Hz (TIA-603 and the common extensions); neighbours are 2.3 ... 7.6 Hz apart.
CTCSS_TONES = (67.0, 69.3, 71.9, 74.4, 77.0, 79.7, 82.5, 85.4, 88.5, 91.5, 94.8, 97.4, 100.0, 103.5, 107.2, 110.9,
               114.8, 118.8, 123.0, 127.3, 131.8, 136.5, 141.3, 146.2, 151.4, 156.7, 159.8, 162.2, 165.5, 167.9,
               171.3, 173.8, 177.3, 179.9, 183.5, 186.2, 189.9, 192.8, 196.6, 199.5, 203.5, 206.5, 210.7, 218.1,
               225.7, 229.1, 233.6, 241.8, 250.3, 254.1)
TONE_SUMS = 8                    # RFA_TONE_SUMS: Sc0 Ss0 Sc1 Ss1 Sc2 Ss2 P S1
TONE_PROBES = 3


def tone_guards(hz: float) -> tuple[float, float]:
    """The two guard frequencies of a wanted tone: for a tone of ``CTCSS_TONES`` (to 0.05 Hz) its table
    neighbours -- what another user of the channel would send -- and for any other tone, or at the
    table's ends, ``hz * 0.965`` and ``hz * 1.035`` rounded to 0.1 Hz."""
    hz = float(hz)
    for i in range(1, len(CTCSS_TONES) - 1):
        if abs(CTCSS_TONES[i] - hz) <= 0.05:
            return CTCSS_TONES[i - 1], CTCSS_TONES[i + 1]
    return round(hz * 0.965 * 10) / 10, round(hz * 1.035 * 10) / 10


def tone_quality(sc: float, ss: float, p: float, s1: float, n: int) -> float:
    """``2 (sc^2 + ss^2) / (n p - s1^2)`` (``rfa_tone_quality``): the share of a row's AC power that is
    coherent at a probe.  0 where the denominator is <= 0, NaN where a sum is not finite.  Host only."""
    return float(_lib.lib().rfa_tone_quality(float(sc), float(ss), float(p), float(s1), int(n)))


def _tone_probes(hz, rate: int = AUDIO_RATE) -> list[int]:
    """A wanted tone in Hz (None: no tone) -> its three probes in tenths of a hertz, guards included."""
    if hz is None:
        return [0] * TONE_PROBES
    if isinstance(hz, (bool, str, bytes)) or not isinstance(hz, (int, float, np.integer, np.floating)):
        raise TypeError("a tone is a frequency in Hz or None")
    if not math.isfinite(hz):
        raise ValueError("a tone must be finite")
    f10 = [int(round(float(f) * 10)) for f in (hz, *tone_guards(hz))]
    if not all(1 <= f < 5 * rate for f in f10):
        raise ValueError(f"tone {hz} Hz or a guard of it lies outside 0.1 Hz ... {rate / 2} Hz")
    return f10


def _tone_entries(tone, n_channels: int):
    """The ``tone=`` keyword of a bank chain -> None or the probes of every slot.  Host only: a wrong
    keyword raises before any handle is made."""
    if tone is None:
        return None
    if isinstance(tone, (bool, str, bytes, int, float)) or not hasattr(tone, "__iter__"):
        raise TypeError("tone must be None or one entry per slot (a frequency in Hz or None)")
    entries = list(tone)
    if len(entries) != n_channels:
        raise ValueError(f"{n_channels} tones expected, got {len(entries)}")
    return [_tone_probes(hz) for hz in entries]


class ToneMeterBank(_Handle):
    """Tone meter for ``n_channels`` slots of audio at ``sample_rate`` (``rfa_tone_*``,
    ``rfanalyzer_amd/csrc/tone.hip``).  Every slot has up to three probes in tenths of a hertz -- the
    wanted tone and two guards -- and a call sums its audio row, ``n[k]`` samples, into 8 doubles:
    ``Sc_j, Ss_j`` (the row against probe j's cosine and sine, phase-continuous over calls through a
    sample counter per slot that ``break_`` zeroes), ``P`` (power) and ``S1`` (plain sum).  The sums
    are bit-identical from run to run and for any placement of the rows.  ``process_device`` is
    asynchronous; ``collect`` waits for its copy of the sums alone."""

    _prefix = "rfa_tone"

    def __init__(self, n_channels: int, sample_rate: int = AUDIO_RATE, device: int = 0):
        self.n_channels, self.sample_rate = int(n_channels), int(sample_rate)
        self._create("rfa_tone_create", device, self.n_channels, self.sample_rate)
        self._sums = np.zeros((TONE_SUMS, self.n_channels), np.float64)
        self._n = np.zeros(self.n_channels, np.int64)

    def set_probes(self, k: int, f10) -> None:
        """Slot k's probes in tenths of a hertz, up to three, 0 for an unused one; the counter stays."""
        f10 = [int(f) for f in f10]
        if len(f10) > TONE_PROBES:
            raise ValueError(f"at most {TONE_PROBES} probes")
        arr = (ctypes.c_int32 * TONE_PROBES)(*f10)
        self._call("set_probes", int(k), arr)

    def probes(self, k: int) -> list[int]:
        arr = (ctypes.c_int32 * TONE_PROBES)()
        self._call("get_probes", int(k), arr)
        return list(arr)

    def break_(self, k: int | None = None) -> None:
        """Slot k's sample counter (None: every slot's) back to 0.  Host only."""
        self._call("break", -1 if k is None else int(k))

    def reset(self) -> None:
        """Every counter and the last results to 0; the probes stay."""
        self._call("reset")

    def _count_array(self, counts):
        if isinstance(counts, ctypes.c_size_t * self.n_channels):
            return counts
        counts = [int(c) for c in counts]
        if len(counts) != self.n_channels or min(counts) < 0:
            raise ValueError(f"{self.n_channels} counts of zero or more expected")
        return (ctypes.c_size_t * self.n_channels)(*counts)

    def _result(self):
        return self._sums.copy(), self._n.copy()

    def process_device(self, audio_ptr: int, audio_stride: int, counts) -> None:
        """Device rows ``audio_stride`` floats apart, one count per slot (``DemodulatorBank``'s).
        Enqueues the sums and their copy on the handle's stream and returns; ``collect`` hands them out."""
        self._call("process", audio_ptr, audio_stride, self._count_array(counts))

    def collect(self):
        """(sums float64[8, K], n int64[K]) of the last ``process_device``; waits for that call's copy
        and nothing else."""
        self._call("collect", self._sums.ctypes.data, self._n.ctypes.data)
        return self._result()

    def process(self, audio, counts=None):
        """Host float32 [K, width] rows and one count per slot (default: the width) -> (sums, n)."""
        audio = np.ascontiguousarray(audio, np.float32)
        if audio.ndim != 2 or audio.shape[0] != self.n_channels:
            raise ValueError(f"audio must have shape [{self.n_channels}, n]")
        counts = self._count_array([audio.shape[1]] * self.n_channels if counts is None else counts)
        if max(counts) > audio.shape[1]:
            raise ValueError("a count above the rows' length")
        self._call("process_host", audio.ctypes.data, audio.shape[1], counts, self._sums.ctypes.data,
                   self._n.ctypes.data)
        return self._result()

    def process_tensor(self, audio, counts):
        """A torch.cuda float32 tensor [K, width] (rows may be slices of a wider tensor) and one count
        per slot -> (sums, n); on torch's current stream."""
        self._follow_torch_stream(audio)
        K = self.n_channels
        if audio.dim() != 2 or audio.shape[0] != K or str(audio.dtype) != "torch.float32":
            raise ValueError(f"audio must be float32 of shape [{K}, n]")
        if audio.shape[1] > 1 and audio.stride(1) != 1:
            raise ValueError("rows must be contiguous")
        counts = self._count_array(counts)
        if max(counts) > audio.shape[1]:
            raise ValueError("a count above the rows' length")
        self.process_device(audio.data_ptr(), audio.stride(0) if K > 1 else audio.shape[1], counts)
        return self.collect()


class ToneRule:
    """Tone squelch for ``n_channels`` slots of audio at ``rate``: what to do with the sums of a
    ``ToneMeterBank``.  Host arithmetic only, no device.

    Per slot the rule accumulates the eight sums and the sample count.  ``update(sums, n, active)``
    adds the values of the active slots; a slot that is inactive or has ``n = 0`` is reset
    (accumulators to 0, gate closed).  Once a slot has accumulated ``n >= window_s * rate`` samples
    it is evaluated and its accumulators are cleared: ``q`` is ``tone_quality`` of probe 0, and the
    tone is detected where q is finite, ``q > threshold`` and probe 0's power ``Sc^2 + Ss^2`` exceeds
    ``guard_ratio`` times that of every used guard.  A detection opens the gate and clears the miss
    count, a miss increments it, ``hang`` misses in a row close the gate.  A slot whose probe 0 is
    unused (``set_used``) has no tone squelch: it is never evaluated and reads open.

    ``window_s = 0.5``, ``threshold = 0.01``, ``guard_ratio = 4`` and ``hang = 2`` are parameters
    chosen by hand on a simulation, not measurements of off-air audio."""

    def __init__(self, n_channels: int, rate: float = AUDIO_RATE, *, window_s: float = 0.5, threshold: float = 0.01,
                 guard_ratio: float = 4.0, hang: int = 2):
        K = int(n_channels)
        if K < 1:
            raise ValueError("at least one slot")
        if not (math.isfinite(rate) and rate > 0):
            raise ValueError("rate must be positive")
        if not (math.isfinite(window_s) and window_s > 0):
            raise ValueError("window_s must be positive")
        if not (math.isfinite(threshold) and threshold >= 0):
            raise ValueError("threshold must be zero or more")
        if not (math.isfinite(guard_ratio) and guard_ratio >= 0):
            raise ValueError("guard_ratio must be zero or more")
        if int(hang) != hang or hang < 1:
            raise ValueError("hang must be a whole number of windows, at least 1")
        self.n_channels, self.rate = K, float(rate)
        self.window_s, self.threshold, self.guard_ratio, self.hang = (float(window_s), float(threshold),
                                                                      float(guard_ratio), int(hang))
        self._acc = np.zeros((TONE_SUMS, K))
        self._acc_n = np.zeros(K, np.int64)
        self._gate = np.zeros(K, bool)
        self._misses = np.zeros(K, np.int64)
        self._quality = np.full(K, np.nan)
        self._used = np.ones((K, TONE_PROBES), bool)

    def _slot(self, k: int) -> int:
        if not 0 <= int(k) < self.n_channels:
            raise ValueError(f"no slot {k}")
        return int(k)

    def set_used(self, k: int, used) -> None:
        """Which of slot k's three probes are in use; the slot starts again (``reset(k)``)."""
        k = self._slot(k)
        used = [bool(u) for u in used]
        if len(used) != TONE_PROBES:
            raise ValueError(f"{TONE_PROBES} flags expected")
        self._used[k] = used
        self.reset(k)

    @property
    def open(self) -> np.ndarray:
        """The gate per slot (bool[K]); a slot without a wanted tone reads open."""
        return self._gate | ~self._used[:, 0]

    @property
    def quality(self) -> np.ndarray:
        """Every slot's q of its last evaluated window (float64[K]); NaN before its first."""
        return self._quality.copy()

    def reset(self, k: int | None = None) -> None:
        """Slot k (None: every slot): accumulators to 0, gate closed, no quality."""
        s = slice(None) if k is None else self._slot(k)
        self._acc[:, s] = 0.0
        for a, v in ((self._acc_n, 0), (self._gate, False), (self._misses, 0), (self._quality, np.nan)):
            a[s] = v

    def update(self, sums, n, active=None) -> np.ndarray:
        """One call's sums [8, K] and counts [K] -> ``open``."""
        K = self.n_channels
        sums, n = np.asarray(sums, np.float64), np.asarray(n, np.int64)
        act = np.ones(K, bool) if active is None else np.asarray(active, bool)
        if sums.shape != (TONE_SUMS, K) or n.shape != (K,) or act.shape != (K,):
            raise ValueError(f"[{TONE_SUMS}, {K}] sums, {K} counts and flags expected")
        # every slot at once -- this runs per packet; only a slot whose window is full takes the loop below
        live = self._used[:, 0] & act & (n > 0)
        with np.errstate(all="ignore"):
            if live.all():
                self._acc += sums
                self._acc_n += n
            else:
                dead = self._used[:, 0] & ~live
                self._acc[:, dead] = 0.0
                for a, v in ((self._acc_n, 0), (self._gate, False), (self._misses, 0), (self._quality, np.nan)):
                    a[dead] = v
                self._acc += np.where(live, sums, 0.0)
                self._acc_n += np.where(live, n, 0)
        due = live & (self._acc_n >= self.window_s * self.rate)
        for k in np.flatnonzero(due) if due.any() else ():
            a = self._acc[:, k].copy()
            q = tone_quality(a[0], a[1], a[6], a[7], int(self._acc_n[k]))
            self._acc[:, k] = 0.0
            self._acc_n[k] = 0
            self._quality[k] = q
            with np.errstate(all="ignore"):
                c0 = a[0] * a[0] + a[1] * a[1]
                hit = bool(math.isfinite(q) and q > self.threshold)
                for j in (1, 2):
                    if hit and self._used[k, j]:
                        hit = bool(c0 > self.guard_ratio * (a[2 * j] * a[2 * j] + a[2 * j + 1] * a[2 * j + 1]))
            if hit:
                self._gate[k] = True
                self._misses[k] = 0
            else:
                self._misses[k] += 1
                if self._misses[k] >= self.hang:
                    self._gate[k] = False
        return self.open


# ---------------------------------------------------------------- DCS code squelch

# The 104 standard DCS codes (three octal digits each).
DCS_CODES = tuple(int(c, 8) for c in (
    "023 025 026 031 032 036 043 047 051 053 054 065 071 072 073 074 114 115 116 122 125 131 132 134 143 145 152 "
    "155 156 162 165 172 174 205 212 223 225 226 243 244 245 246 251 252 255 261 263 265 266 271 274 306 311 315 "
    "325 331 332 343 346 351 356 364 365 371 411 412 413 423 431 432 445 446 452 454 455 462 464 465 466 503 506 "
    "516 523 526 532 546 565 606 612 624 627 631 632 654 662 664 703 712 723 731 732 734 743 754").split())
CODE_SUBCELLS = 8                # RFA_CODE_SUBCELLS: P, sub-cells per bit
CODE_WORD_BITS = 23
_CODE_NUM = 672 * CODE_SUBCELLS  # s(g) = _CODE_NUM * g // (5 * rate)


def dcs_word(code: int) -> int:
    """The 23-bit word of a 9-bit code, bit i being bit i on the air: the code in bits 0 ... 8, 0, 0, 1 in
    bits 9 ... 11 and in bits 12 ... 22 the parity of the systematic Golay (23,12) code with generator
    ``0xC75`` -- the remainder of ``d x^11`` by it over GF(2).  ``dcs_word(0o023) == 0x763813``.  Host only."""
    code = int(code)
    if not 0 <= code <= 0x1FF:
        raise ValueError("a DCS code has 9 bits (three octal digits)")
    d = 0x800 | code
    r = d << 11
    for b in range(22, 10, -1):
        if r >> b & 1:
            r ^= 0xC75 << (b - 11)
    return d | r << 12


def dcs_parse(entry) -> tuple[int, bool]:
    """``"023"``, ``"023N"``, ``"023I"`` (three octal digits, N normal, I inverted) or an int such as
    ``0o023`` -> (code, inverted).  Any 9-bit code is taken, not only those of ``DCS_CODES``."""
    if isinstance(entry, bool) or not isinstance(entry, (str, int, np.integer)):
        raise TypeError("a DCS code is a string such as '023', '023N' or '023I', or an int such as 0o023")
    if not isinstance(entry, str):
        if not 0 <= int(entry) <= 0x1FF:
            raise ValueError("a DCS code has 9 bits (three octal digits)")
        return int(entry), False
    text = entry.strip().upper()
    inverted = text.endswith("I")
    if text.endswith(("N", "I")):
        text = text[:-1]
    if len(text) != 3 or any(c not in "01234567" for c in text):
        raise ValueError(f"DCS code {entry!r}: three octal digits and an optional N or I expected")
    return int(text, 8), inverted


@functools.lru_cache(maxsize=256)
def _dcs_patterns(word: int, words: int) -> np.ndarray:
    """The 23 rotations of a word as mean-removed +-1 cell patterns, tiled: float64 [23, 23 * words], each
    row of norm 1.  Row r, cell i: bit (i + r) mod 23."""
    bits = np.array([1.0 if word >> i & 1 else -1.0 for i in range(CODE_WORD_BITS)])
    rows = np.stack([np.tile(np.roll(bits, -r), words) for r in range(CODE_WORD_BITS)])
    rows -= rows.mean(axis=1, keepdims=True)
    rows /= np.sqrt((rows * rows).sum(axis=1, keepdims=True))
    rows.setflags(write=False)
    return rows


def _dcs_cells(subcells, words: int) -> np.ndarray:
    """``P * (23 * words + 1)`` sub-cells -> the mean-removed, normalised cell values of the P timing
    phases, float64 [P, 23 * words]; a phase without variance is a row of zeros."""
    P, n = CODE_SUBCELLS, CODE_WORD_BITS * words
    sub = np.asarray(subcells, np.float64)
    x = np.stack([sub[p:p + P * n].reshape(n, P).sum(axis=1) for p in range(P)])
    x -= x.mean(axis=1, keepdims=True)
    norm = np.sqrt((x * x).sum(axis=1, keepdims=True))
    return np.divide(x, norm, out=np.zeros_like(x), where=norm > 0)


def dcs_score(subcells, word: int, words: int) -> float:
    """The largest signed normalised correlation of the cells with ``word`` over the P timing phases
    and the 23 rotations; 0 where the cells have no variance."""
    return float((_dcs_cells(subcells, words) @ _dcs_patterns(int(word), int(words)).T).max())


@functools.lru_cache(maxsize=4)
def _dcs_table(words: int) -> np.ndarray:
    out = np.concatenate([_dcs_patterns(dcs_word(c), words) for c in DCS_CODES])
    out.setflags(write=False)
    return out


def dcs_identify(subcells, words: int) -> tuple[int, bool, float]:
    """The search for an unknown code: the best (code, inverted, rho) over ``DCS_CODES`` and both
    polarities on ``P * (23 * words + 1)`` sub-cells (more are ignored).  An inverted word is another
    code's normal word (023I is 047N), and the complement of every code of ``DCS_CODES`` is in the table:
    the normal reading is returned unless the inverted one scores higher by more than 1e-9."""
    words = int(words)
    need = CODE_SUBCELLS * (CODE_WORD_BITS * words + 1)
    sub = np.asarray(subcells)
    if sub.ndim != 1 or sub.size < need:
        raise ValueError(f"{need} sub-cells expected for {words} words")
    rho = (_dcs_cells(sub[:need], words) @ _dcs_table(words).T).reshape(CODE_SUBCELLS, len(DCS_CODES), CODE_WORD_BITS)
    per_code = rho.max(axis=(0, 2)), (-rho).max(axis=(0, 2))
    best = [int(np.argmax(p)) for p in per_code]
    inverted = bool(per_code[1][best[1]] > per_code[0][best[0]] + 1e-9)
    return DCS_CODES[best[inverted]], inverted, float(per_code[inverted][best[inverted]])


def _code_entries(code, n_channels: int, tone=None):
    """The ``code=`` keyword of a bank chain -> None or (code, inverted) or None per slot.  Host only: a
    wrong keyword raises before any handle is made."""
    if code is None:
        return None
    if isinstance(code, (bool, str, bytes, int, float)) or not hasattr(code, "__iter__"):
        raise TypeError("code must be None or one entry per slot (a DCS code such as '023' or None)")
    entries = list(code)
    if len(entries) != n_channels:
        raise ValueError(f"{n_channels} codes expected, got {len(entries)}")
    parsed = [None if e is None else dcs_parse(e) for e in entries]
    if tone is not None:
        for k, (c, t) in enumerate(zip(parsed, tone)):
            if c is not None and t is not None:
                raise ValueError(f"slot {k} has both a tone and a code")
    return parsed


class CodeMeterBank(_Handle):
    """Code meter for ``n_channels`` slots of audio at ``sample_rate`` (``rfa_code_*``,
    ``rfanalyzer_amd/csrc/code.hip``): per call and slot the int64 sums of the quantised audio,
    ``llrint(a * 2^24)``, over sub-cells, 8 to the 134.4 bit/s bit, indexed from the slot's last
    ``break_``; a sample that is not finite or has ``|a| >= 2^15`` adds 0 and is counted as bad.  The
    handle carries an incomplete last sub-cell to the next call, so the completed sub-cells of any
    sequence of calls are the whole stream's, bit for bit.  ``process_device`` is asynchronous and every
    call must be collected once; ``collect`` waits for that call's copy alone."""

    _prefix = "rfa_code"

    def __init__(self, n_channels: int, sample_rate: int = AUDIO_RATE, device: int = 0):
        self.n_channels, self.sample_rate = int(n_channels), int(sample_rate)
        self._create("rfa_code_create", device, self.n_channels, self.sample_rate)
        K = self.n_channels
        self._first, self._count = np.zeros(K, np.int64), np.zeros(K, np.int64)
        self._bad, self._n = np.zeros(K, np.int64), np.zeros(K, np.int64)
        self._sums = np.zeros((K, 64), np.int64)

    def max_subcells(self, n: int) -> int:
        """An upper bound of the sub-cells that ``n`` samples of a slot complete, a carry included."""
        return int(n) * _CODE_NUM // (5 * self.sample_rate) + 2

    def _room(self, n: int) -> None:
        if self._sums.shape[1] < self.max_subcells(n):
            self._sums = np.zeros((self.n_channels, self.max_subcells(n)), np.int64)

    def break_(self, k: int | None = None) -> None:
        """Slot k's sample counter (None: every slot's) back to 0, its carry dropped.  Host only."""
        self._call("break", -1 if k is None else int(k))

    def reset(self) -> None:
        """Every counter to 0, every carry dropped, no call outstanding."""
        self._call("reset")

    _count_array = ToneMeterBank._count_array

    def _out(self):
        return (self._first.ctypes.data, self._count.ctypes.data, self._sums.ctypes.data, self._sums.shape[1],
                self._bad.ctypes.data, self._n.ctypes.data)

    def _result(self):
        return (self._first.copy(), [self._sums[k, :c].copy() for k, c in enumerate(self._count)], self._bad.copy(),
                self._n.copy())

    def process_device(self, audio_ptr: int, audio_stride: int, counts) -> None:
        """Device rows ``audio_stride`` floats apart, one count per slot.  Enqueues the sums and their copy
        on the handle's stream and returns; ``RfaError`` (``RFA_ERR_STATE``) while a call is uncollected."""
        counts = self._count_array(counts)
        self._call("process", audio_ptr, audio_stride, counts)
        self._room(max(counts))

    def collect(self):
        """(first int64[K], K int64 arrays of completed sub-cell sums, bad int64[K], n int64[K]) of the
        last ``process_device``; waits for that call's copy and nothing else."""
        self._call("collect", *self._out())
        return self._result()

    def process(self, audio, counts=None):
        """Host float32 [K, width] rows and one count per slot (default: the width) -> as ``collect``."""
        audio = np.ascontiguousarray(audio, np.float32)
        if audio.ndim != 2 or audio.shape[0] != self.n_channels:
            raise ValueError(f"audio must have shape [{self.n_channels}, n]")
        counts = self._count_array([audio.shape[1]] * self.n_channels if counts is None else counts)
        if max(counts) > audio.shape[1]:
            raise ValueError("a count above the rows' length")
        self._room(max(counts))
        self._call("process_host", audio.ctypes.data, audio.shape[1], counts, *self._out())
        return self._result()

    def process_tensor(self, audio, counts):
        """A torch.cuda float32 tensor [K, width] (rows may be slices of a wider tensor) and one count
        per slot -> as ``collect``; on torch's current stream."""
        self._follow_torch_stream(audio)
        K = self.n_channels
        if audio.dim() != 2 or audio.shape[0] != K or str(audio.dtype) != "torch.float32":
            raise ValueError(f"audio must be float32 of shape [{K}, n]")
        if audio.shape[1] > 1 and audio.stride(1) != 1:
            raise ValueError("rows must be contiguous")
        counts = self._count_array(counts)
        if max(counts) > audio.shape[1]:
            raise ValueError("a count above the rows' length")
        self.process_device(audio.data_ptr(), audio.stride(0) if K > 1 else audio.shape[1], counts)
        return self.collect()


class CodeRule:
    """DCS code squelch for ``n_channels`` slots: what to do with the sub-cells of a ``CodeMeterBank``.
    Host arithmetic only, no device.

    Per slot the rule appends the completed sub-cells of every call.  A slot that is inactive, has
    ``n = 0``, ``bad > 0`` or a gap in its sub-cell index is reset (buffer cleared, gate closed; sub-cells
    that come with a gap start the new buffer).  Once a slot holds ``P * (23 * words + 1)`` sub-cells it
    is evaluated and those sub-cells are dropped: for each of the P timing phases the ``23 * words`` cell
    values (sums of P sub-cells) have their mean removed and are correlated, signed and normalised,
    with the mean-removed +-1 pattern of the wanted word (complemented for an inverted code), tiled
    ``words`` times, at each of the 23 rotations; the score is the largest of the 8 x 23 values, 0 where
    the cells have no variance, and the code is detected where the score is above ``threshold``.  A
    detection opens the gate and clears the miss count, a miss increments it, ``hang`` misses in a row
    close the gate.  A slot that is unused (``set_used``) has no code squelch and reads open.

    ``words = 4``, ``threshold = 0.8`` and ``hang = 2`` are parameters chosen by hand on a simulation
    (DESIGN.md 5.7o), not measurements of off-air audio."""

    def __init__(self, n_channels: int, *, words: int = 4, threshold: float = 0.8, hang: int = 2):
        K = int(n_channels)
        if K < 1:
            raise ValueError("at least one slot")
        if int(words) != words or not 1 <= words <= 64:
            raise ValueError("words must be a whole number of code words, 1 ... 64")
        if not (math.isfinite(threshold) and 0 <= threshold < 1):
            raise ValueError("threshold must lie in [0, 1)")
        if int(hang) != hang or hang < 1:
            raise ValueError("hang must be a whole number of windows, at least 1")
        self.n_channels, self.words, self.threshold, self.hang = K, int(words), float(threshold), int(hang)
        self.need = CODE_SUBCELLS * (CODE_WORD_BITS * self.words + 1)
        self._buf = np.zeros((K, 2 * self.need), np.int64)
        self._fill = np.zeros(K, np.int64)
        self._next = np.full(K, -1, np.int64)               # the sub-cell index the buffer goes on with; -1: none
        self._gate = np.zeros(K, bool)
        self._misses = np.zeros(K, np.int64)
        self._score = np.full(K, np.nan)
        self._used = np.zeros(K, bool)
        self._word = np.zeros(K, np.int64)

    def _slot(self, k: int) -> int:
        if not 0 <= int(k) < self.n_channels:
            raise ValueError(f"no slot {k}")
        return int(k)

    def set_code(self, k: int, code: int, inverted: bool = False) -> None:
        """Slot k's wanted code; the slot starts again (``reset(k)``)."""
        k = self._slot(k)
        word = dcs_word(code)
        self._word[k] = word ^ 0x7FFFFF if inverted else word
        self.set_used(k, True)

    def set_used(self, k: int, used: bool) -> None:
        """Whether slot k has a code squelch at all; the slot starts again."""
        k = self._slot(k)
        self._used[k] = bool(used)
        self.reset(k)

    @property
    def open(self) -> np.ndarray:
        """The gate per slot (bool[K]); a slot without a wanted code reads open."""
        return self._gate | ~self._used

    @property
    def score(self) -> np.ndarray:
        """Every slot's score of its last evaluated window (float64[K]); NaN before its first."""
        return self._score.copy()

    def reset(self, k: int | None = None) -> None:
        """Slot k (None: every slot): buffer cleared, gate closed, no score."""
        s = slice(None) if k is None else self._slot(k)
        for a, v in ((self._fill, 0), (self._next, -1), (self._gate, False), (self._misses, 0), (self._score, np.nan)):
            a[s] = v

    def update(self, first, count, sums, bad, n, active=None) -> np.ndarray:
        """One call's results as ``CodeMeterBank`` hands them out -- first[K], count[K], the sums as
        [K, >= max count] or K arrays, bad[K], n[K] -> ``open``."""
        K = self.n_channels
        first, count, bad, n = (np.asarray(a, np.int64) for a in (first, count, bad, n))
        act = np.ones(K, bool) if active is None else np.asarray(active, bool)
        if any(a.shape != (K,) for a in (first, count, bad, n, act)) or len(sums) != K or count.min() < 0:
            raise ValueError(f"{K} values of each expected")
        cmax = int(count.max())
        if not (isinstance(sums, np.ndarray) and sums.ndim == 2):
            rows, sums = sums, np.zeros((K, cmax), np.int64)
            for k in range(K):
                sums[k, :count[k]] = np.asarray(rows[k], np.int64)[:count[k]]
        if sums.shape[1] < cmax:
            raise ValueError("fewer sums than a slot's count")
        # every slot at once -- this runs per packet; only a slot whose window is full takes the loop below
        live = self._used & act & (n > 0) & (bad == 0)
        takes = live & (count > 0)
        gone = (self._used & ~live) | (takes & (self._next >= 0) & (first != self._next))
        if gone.any():
            for a, v in ((self._fill, 0), (self._next, -1), (self._gate, False), (self._misses, 0),
                         (self._score, np.nan)):
                a[gone] = v
        if not takes.any():
            return self.open
        if int(self._fill.max()) + cmax > self._buf.shape[1]:
            grown = np.zeros((K, 2 * (int(self._fill.max()) + cmax)), np.int64)
            grown[:, :self._buf.shape[1]] = self._buf
            self._buf = grown
        cols = np.arange(cmax)
        mask = (cols[None, :] < count[:, None]) & takes[:, None]
        slot, col = np.nonzero(mask)
        self._buf[slot, self._fill[slot] + col] = sums[slot, col]
        self._fill += np.where(takes, count, 0)
        self._next = np.where(takes, first + count, self._next)
        for k in np.flatnonzero(self._fill >= self.need):
            fill = int(self._fill[k])
            while fill >= self.need:
                rho = dcs_score(self._buf[k, :self.need], int(self._word[k]), self.words)
                fill -= self.need
                self._buf[k, :fill] = self._buf[k, self.need:self.need + fill].copy()
                self._score[k] = rho
                if rho > self.threshold:
                    self._gate[k] = True
                    self._misses[k] = 0
                else:
                    self._misses[k] += 1
                    if self._misses[k] >= self.hang:
                        self._gate[k] = False
            self._fill[k] = fill
        return self.open


# ---------------------------------------------------------------- audio FIR bank

AUDIO_FIR_MAX_TAPS = _lib.RFA_AUDIO_FIR_MAX_TAPS
AUDIO_FIR_PLAN_FIELDS = ("tile", "lds_bytes", "path", "outputs_per_thread", "workgroups")   # rfa_audio_fir_plan order


@functools.lru_cache(maxsize=8)
def _voice_design(rate: float, cutoff_hz: float, transition_hz: float, attenuation_db: float) -> np.ndarray:
    """``voice_taps`` of these arguments, read-only: a chain of 32 "voice" slots designs once."""
    taps = _design_voice_taps(rate, cutoff_hz, transition_hz, attenuation_db)
    taps.setflags(write=False)
    return taps


def voice_taps(rate: float = AUDIO_RATE, cutoff_hz: float = 300.0, transition_hz: float = 100.0,
               attenuation_db: float = 60.0) -> np.ndarray:
    """The high-pass that takes a CTCSS tone out of the voice: the spectral inversion of the reference's
    own low-pass design, ``lp = create_low_pass_taps(1.0, rate, cutoff_hz, transition_hz, attenuation_db)``
    (odd in length by its design), ``hp = -lp`` and ``hp[centre] += 1``, in float32.  1309 taps at the
    defaults, a delay of 654 samples.  ``ValueError`` where the design is rejected or is longer than
    ``AUDIO_FIR_MAX_TAPS``.  Host only."""
    return _voice_design(float(rate), float(cutoff_hz), float(transition_hz), float(attenuation_db)).copy()


def _design_voice_taps(rate: float, cutoff_hz: float, transition_hz: float, attenuation_db: float) -> np.ndarray:
    lp = create_low_pass_taps(1.0, float(rate), float(cutoff_hz), float(transition_hz), float(attenuation_db))
    if lp is None:
        raise ValueError("the low-pass design rejected these arguments")
    if lp.size % 2 == 0:
        raise ValueError("the low-pass design has no centre tap")
    if lp.size > AUDIO_FIR_MAX_TAPS:
        raise ValueError(f"{lp.size} taps, above {AUDIO_FIR_MAX_TAPS}: widen transition_hz")
    hp = -lp
    hp[lp.size // 2] += np.float32(1.0)
    return hp.astype(np.float32)


def _audio_filter_taps(entry):
    """One slot's ``audio_filter`` entry -> None (pass-through) or its float32 taps.  Host only."""
    if entry is None:
        return None
    if isinstance(entry, str):
        if entry != "voice":
            raise ValueError(f"audio filter {entry!r}: the one named filter is 'voice'")
        return _voice_design(float(AUDIO_RATE), 300.0, 100.0, 60.0)
    if isinstance(entry, (bool, bytes, int, float)) or not hasattr(entry, "__len__"):
        raise ValueError("an audio filter is None, 'voice' or a 1-D array of taps")
    try:
        taps = np.asarray(entry, np.float32)
    except (TypeError, ValueError) as e:
        raise ValueError("an audio filter is None, 'voice' or a 1-D array of taps") from e
    if taps.ndim != 1 or taps.size > AUDIO_FIR_MAX_TAPS or not np.isfinite(taps).all():
        raise ValueError(f"taps must be 1-D, finite and at most {AUDIO_FIR_MAX_TAPS}")
    return np.ascontiguousarray(taps) if taps.size else None


def _audio_filter_entries(audio_filter, n_channels: int):
    """The ``audio_filter=`` keyword of a bank chain -> None or every slot's taps (None: pass-through).
    Host only: a wrong entry count or type raises before any device work."""
    if audio_filter is None:
        return None
    if isinstance(audio_filter, (bool, str, bytes, int, float)) or not hasattr(audio_filter, "__iter__"):
        raise ValueError("audio_filter must be None or one entry per slot (None, 'voice' or an array of taps)")
    entries = list(audio_filter)
    if len(entries) != n_channels:
        raise ValueError(f"{n_channels} audio filters expected, got {len(entries)}")
    return [_audio_filter_taps(e) for e in entries]


def audio_fir_plan(num_taps: int, n: int) -> dict:
    """What a call of one slot with ``num_taps`` taps and ``n`` samples runs (``rfa_audio_fir_plan``):
    ``tile`` (outputs per workgroup), ``lds_bytes``, ``path`` ("none", "copy", "narrow", "wide"),
    ``outputs_per_thread`` and ``workgroups``.  Host only."""
    out = (ctypes.c_int32 * _lib.RFA_AUDIO_FIR_PLAN_FIELDS)()
    _lib.check(_lib.lib().rfa_audio_fir_plan(int(num_taps), int(n), out), "rfa_audio_fir_plan")
    plan = dict(zip(AUDIO_FIR_PLAN_FIELDS, (int(v) for v in out)))
    plan["path"] = _lib.RFA_AUDIO_FIR_PATHS[plan["path"]]
    return plan


class AudioFilterBank(_Handle):
    """A real FIR on each of ``n_channels`` audio rows (``rfa_audio_fir_*``,
    ``rfanalyzer_amd/csrc/audio_fir.hip``): every slot has its own taps (up to 4096; none: a bitwise
    pass-through), its own history of the last 4095 inputs on the device and its own count per call.
    Output i is ``((0 + t[0] x[i]) + t[1] x[i-1]) + ...`` with every product and sum rounded to
    float32, so a row cut into calls anywhere gives the bits of the row given whole.  One launch per
    call whatever the slot count; ``process_device`` is asynchronous on the handle's stream."""

    _prefix = "rfa_audio_fir"

    def __init__(self, n_channels: int, device: int = 0):
        self.n_channels = int(n_channels)
        self._create("rfa_audio_fir_create", device, self.n_channels)

    def set_taps(self, k: int, taps) -> None:
        """Slot k's taps from the next call on (None or empty: pass-through); its history stays."""
        if taps is None:
            self._call("set_taps", int(k), None, 0)
            return
        taps = np.ascontiguousarray(taps, np.float32)
        if taps.ndim != 1:
            raise ValueError("taps must be 1-D")
        self._call("set_taps", int(k), taps.ctypes.data_as(_lib._fp), taps.size)

    def taps(self, k: int) -> np.ndarray:
        return self._query_floats("get_taps", 1, 1, int(k))[0][0]

    def reset(self, k: int | None = None) -> None:
        """Slot k's history (None: every slot's) to zeros; the taps stay."""
        self._call("reset", -1 if k is None else int(k))

    @staticmethod
    def plan(num_taps: int, n: int) -> dict:
        return audio_fir_plan(num_taps, n)

    def _count_array(self, counts):
        if isinstance(counts, ctypes.c_size_t * self.n_channels):
            return counts
        counts = [int(c) for c in counts]
        if len(counts) != self.n_channels or min(counts) < 0:
            raise ValueError(f"{self.n_channels} counts of zero or more expected")
        return (ctypes.c_size_t * self.n_channels)(*counts)

    def process_device(self, in_ptr: int, in_stride: int, counts, out_ptr: int, out_stride: int) -> None:
        """Device rows in and out, strides in floats, one count per slot (``DemodulatorBank``'s).
        Enqueues on the handle's stream and returns."""
        self._call("process", in_ptr, in_stride, self._count_array(counts), out_ptr, out_stride)

    def process_tensor(self, audio, counts, out) -> None:
        """torch.cuda float32 tensors [K, width] in and out (rows may be slices of wider tensors) and one
        count per slot; on torch's current stream."""
        self._follow_torch_stream(audio)
        K = self.n_channels
        for t in (audio, out):
            if t.dim() != 2 or t.shape[0] != K or str(t.dtype) != "torch.float32":
                raise ValueError(f"audio and out must be float32 of shape [{K}, n]")
            if t.shape[1] > 1 and t.stride(1) != 1:
                raise ValueError("rows must be contiguous")
        counts = self._count_array(counts)
        if max(counts) > min(audio.shape[1], out.shape[1]):
            raise ValueError("a count above the rows' length")
        self.process_device(audio.data_ptr(), audio.stride(0) if K > 1 else audio.shape[1], counts,
                            out.data_ptr(), out.stride(0) if K > 1 else out.shape[1])

    def process(self, rows, counts=None) -> list[np.ndarray]:
        """Host float32 [K, width] rows and one count per slot (default: the width) -> K filtered arrays."""
        rows = np.ascontiguousarray(rows, np.float32)
        if rows.ndim != 2 or rows.shape[0] != self.n_channels:
            raise ValueError(f"rows must have shape [{self.n_channels}, n]")
        counts = self._count_array([rows.shape[1]] * self.n_channels if counts is None else counts)
        if max(counts) > rows.shape[1]:
            raise ValueError("a count above the rows' length")
        out = np.zeros(rows.shape, np.float32)
        self._call("process_host", rows.ctypes.data, rows.shape[1], counts, out.ctypes.data, rows.shape[1])
        return [out[k, :c].copy() for k, c in enumerate(counts)]


# ---------------------------------------------------------------- audio IIR bank

AUDIO_IIR_MAX_SECTIONS = _lib.RFA_AUDIO_IIR_MAX_SECTIONS
AUDIO_IIR_BLOCK = _lib.RFA_AUDIO_IIR_BLOCK
AUDIO_IIR_PLAN_FIELDS = ("block", "chunk_blocks", "lds_bytes", "path", "chunks", "blocks")   # rfa_audio_iir_plan order
AUDIO_IIR_NAMES = ("deemphasis", "voice", "voice+deemphasis")


def _bilinear_highpass(c0: float, c1: float, wz2: float, K: float) -> list[float]:
    """(s^2 + wz2) / (s^2 + c1 s + c0) under s = (1 - z^-1) / (K (1 + z^-1)), a0 = 1."""
    a0 = 1.0 + c1 * K + c0 * K * K
    n0 = 1.0 + wz2 * K * K
    return [n0 / a0, (2.0 * wz2 * K * K - 2.0) / a0, n0 / a0, (2.0 * c0 * K * K - 2.0) / a0,
            (1.0 - c1 * K + c0 * K * K) / a0]


def _bilinear_highpass_first(sigma: float, K: float) -> list[float]:
    """s / (s + sigma) under the same substitution, a0 = 1."""
    a0 = 1.0 + sigma * K
    return [1.0 / a0, -1.0 / a0, 0.0, (sigma * K - 1.0) / a0, 0.0]


def _check_design(edge_hz: float, order: int, rate: float) -> None:
    if not (math.isfinite(rate) and rate > 0 and math.isfinite(edge_hz) and 0.0 < edge_hz < rate / 2):
        raise ValueError("the edge must lie between 0 and half the rate")
    if not 1 <= order <= 2 * AUDIO_IIR_MAX_SECTIONS:
        raise ValueError(f"order outside 1 ... {2 * AUDIO_IIR_MAX_SECTIONS}")


def deemphasis_sections(tau: float = 750e-6, rate: float = AUDIO_RATE) -> np.ndarray:
    """The one-pole de-emphasis of an NFM receiver as a float32 ``[1, 5]`` section: p = exp(-1 / (tau rate)),
    b0 = 1 - p, a1 = -p: unit gain at DC, -3 dB at 1 / (2 pi tau), 6 dB / octave above.  Host only."""
    tau, rate = float(tau), float(rate)
    if not (math.isfinite(tau) and tau > 0 and math.isfinite(rate) and rate > 0):
        raise ValueError("tau and rate must be positive")
    p = math.exp(-1.0 / (tau * rate))
    return np.array([[1.0 - p, 0.0, 0.0, -p, 0.0]], np.float32)


def tone_strip_sections(stop_hz: float = 255.0, attenuation_db: float = 40.0, order: int = 8,
                        rate: float = AUDIO_RATE) -> np.ndarray:
    """The high-pass that takes a CTCSS tone out of the voice as float32 ``[ceil(order / 2), 5]`` sections: a
    Chebyshev II design in closed form, at most ``-attenuation_db`` from DC to ``stop_hz`` and monotonic
    above.  With eps = 1 / sqrt(10^(A / 10) - 1), mu = asinh(1 / eps) / order and theta_k = (2k - 1) pi /
    (2 order), the analog pair k has zeros +-j cos(theta_k) and poles -sinh(mu) sin(theta_k) +- j cosh(mu)
    cos(theta_k); s = (1 - z^-1) / (K (1 + z^-1)) with K = tan(pi stop / rate) maps it, normalised to
    a0 = 1.  At the defaults: -40.0 dB at 255 Hz, -0.96 dB at 330 Hz, -0.01 dB at 400 Hz, pole radii
    0.977 ... 0.9954.  Host only."""
    stop_hz, attenuation_db, order, rate = float(stop_hz), float(attenuation_db), int(order), float(rate)
    _check_design(stop_hz, order, rate)
    if not (math.isfinite(attenuation_db) and attenuation_db > 0):
        raise ValueError("attenuation_db must be positive")
    eps = 1.0 / math.sqrt(10.0 ** (attenuation_db / 10.0) - 1.0)
    mu = math.asinh(1.0 / eps) / order
    K = math.tan(math.pi * stop_hz / rate)
    out = []
    for k in range(1, order // 2 + 1):
        th = (2 * k - 1) * math.pi / (2 * order)
        re, im = -math.sinh(mu) * math.sin(th), math.cosh(mu) * math.cos(th)
        out.append(_bilinear_highpass(re * re + im * im, -2.0 * re, math.cos(th) ** 2, K))
    if order % 2:
        out.append(_bilinear_highpass_first(math.sinh(mu), K))
    return np.array(out, np.float32)


def highpass_sections(cutoff_hz: float, order: int, rate: float = AUDIO_RATE) -> np.ndarray:
    """A Butterworth high-pass of ``order`` with its -3 dB point at ``cutoff_hz`` as float32
    ``[ceil(order / 2), 5]`` sections, by the same bilinear substitution.  Host only."""
    cutoff_hz, order, rate = float(cutoff_hz), int(order), float(rate)
    _check_design(cutoff_hz, order, rate)
    K = math.tan(math.pi * cutoff_hz / rate)
    out = [_bilinear_highpass(1.0, 2.0 * math.sin((2 * k - 1) * math.pi / (2 * order)), 0.0, K)
           for k in range(1, order // 2 + 1)]
    if order % 2:
        out.append(_bilinear_highpass_first(1.0, K))
    return np.array(out, np.float32)


def iir_response(sections, hz, rate: float = AUDIO_RATE):
    """The cascade's response in dB at ``hz`` (a number or an array), from the coefficients as given,
    in float64.  Host only."""
    sec = np.asarray(sections, np.float64).reshape(-1, 5)
    z1 = np.exp(-2j * np.pi * np.asarray(hz, np.float64) / float(rate))
    h = np.ones_like(z1)
    for b0, b1, b2, a1, a2 in sec:
        h = h * (b0 + b1 * z1 + b2 * z1 * z1) / (1.0 + a1 * z1 + a2 * z1 * z1)
    with np.errstate(divide="ignore"):
        db = 20.0 * np.log10(np.abs(h))
    return float(db) if db.ndim == 0 else db


@functools.lru_cache(maxsize=4)
def _named_sections(name: str) -> np.ndarray:
    parts = {"deemphasis": (deemphasis_sections,), "voice": (tone_strip_sections,),
             "voice+deemphasis": (tone_strip_sections, deemphasis_sections)}[name]
    sec = np.concatenate([f() for f in parts])
    sec.setflags(write=False)
    return sec


def _audio_iir_sections(entry):
    """One slot's ``audio_iir`` entry -> None (pass-through) or its float32 ``[S, 5]`` sections.  Host only."""
    what = "an audio IIR entry is None, 'deemphasis', 'voice', 'voice+deemphasis' or an [S, 5] array of sections"
    if entry is None:
        return None
    if isinstance(entry, str):
        if entry not in AUDIO_IIR_NAMES:
            raise ValueError(f"audio IIR {entry!r}: the named ones are {AUDIO_IIR_NAMES}")
        return _named_sections(entry)
    if isinstance(entry, (bool, bytes, int, float)) or not hasattr(entry, "__len__"):
        raise ValueError(what)
    try:
        sec = np.asarray(entry, np.float32)
    except (TypeError, ValueError) as e:
        raise ValueError(what) from e
    if sec.size == 0:
        return None
    if sec.ndim != 2 or sec.shape[1] != 5 or sec.shape[0] > AUDIO_IIR_MAX_SECTIONS or not np.isfinite(sec).all():
        raise ValueError(f"sections must be [S, 5], finite, S at most {AUDIO_IIR_MAX_SECTIONS}")
    a1, a2 = sec[:, 3].astype(np.float64), sec[:, 4].astype(np.float64)
    if not ((np.abs(a2) < 1.0) & (np.abs(a1) < 1.0 + a2)).all():
        raise ValueError("a section's poles are not inside the unit circle (|a2| < 1 and |a1| < 1 + a2)")
    return np.ascontiguousarray(sec)


def _audio_iir_entries(audio_iir, n_channels: int):
    """The ``audio_iir=`` keyword of a bank chain -> None or every slot's sections (None: pass-through).
    Host only: a wrong entry count or type raises before any device work."""
    if audio_iir is None:
        return None
    if isinstance(audio_iir, (bool, str, bytes, int, float)) or not hasattr(audio_iir, "__iter__"):
        raise ValueError("audio_iir must be None or one entry per slot (None, a name or an [S, 5] array)")
    entries = list(audio_iir)
    if len(entries) != n_channels:
        raise ValueError(f"{n_channels} audio IIR entries expected, got {len(entries)}")
    return [_audio_iir_sections(e) for e in entries]


def audio_iir_tables(a1: float, a2: float):
    """The library's own tables of a section with these a1, a2 (``rfa_audio_iir_tables``): float32 ``G[128, 2]``
    and ``P[2, 2]``.  Host only."""
    G, P = np.empty((AUDIO_IIR_BLOCK, 2), np.float32), np.empty((2, 2), np.float32)
    _lib.check(_lib.lib().rfa_audio_iir_tables(float(a1), float(a2), G.ctypes.data_as(_lib._fp),
                                               P.ctypes.data_as(_lib._fp)), "rfa_audio_iir_tables")
    return G, P


def audio_iir_plan(num_sections: int, n: int, a_mod_b: int = 0) -> dict:
    """What a call of one slot with ``num_sections`` sections and ``n`` samples, ``a_mod_b`` samples into a
    block, runs (``rfa_audio_iir_plan``): ``block``, ``chunk_blocks``, ``lds_bytes``, ``path`` ("none", "copy",
    "blocked"), ``chunks`` and ``blocks`` (touched).  Host only."""
    out = (ctypes.c_int32 * _lib.RFA_AUDIO_IIR_PLAN_FIELDS)()
    _lib.check(_lib.lib().rfa_audio_iir_plan(int(num_sections), int(n), int(a_mod_b), out), "rfa_audio_iir_plan")
    plan = dict(zip(AUDIO_IIR_PLAN_FIELDS, (int(v) for v in out)))
    plan["path"] = _lib.RFA_AUDIO_IIR_PATHS[plan["path"]]
    return plan


def audio_iir_carry_after(n: int, a_mod_b: int) -> int:
    """(a_mod_b + n) mod 128 (``rfa_audio_iir_carry_after``).  Host only."""
    nxt = ctypes.c_int32(0)
    _lib.check(_lib.lib().rfa_audio_iir_carry_after(int(n), int(a_mod_b), ctypes.byref(nxt)), "rfa_audio_iir_carry_after")
    return nxt.value


class AudioIirBank(_Handle):
    """Up to 8 second-order recursive sections on each of ``n_channels`` audio rows (``rfa_audio_iir_*``,
    ``rfanalyzer_amd/csrc/audio_iir.hip``): every slot has its own sections (none: a bitwise
    pass-through), its own carried state on the device and its own count per call.  The recurrence is
    blocked -- 128-sample blocks, each the zero-state response plus the block-start state's zero-input
    response (include/rfa.h has the definition) -- so the blocks run in parallel and a row cut into
    calls anywhere gives the bits of the row given whole.  One launch per call whatever the slot count;
    ``process_device`` is asynchronous on the handle's stream."""

    _prefix = "rfa_audio_iir"

    def __init__(self, n_channels: int, device: int = 0):
        self.n_channels = int(n_channels)
        self._create("rfa_audio_iir_create", device, self.n_channels)

    def set_sections(self, k: int, sections) -> None:
        """Slot k's sections from the next call on (None or empty: pass-through); its carry is zeroed."""
        sec = None if sections is None else np.ascontiguousarray(sections, np.float32)
        if sec is None or sec.size == 0:
            self._call("set_sections", int(k), None, 0)
            return
        if sec.ndim != 2 or sec.shape[1] != 5:
            raise ValueError("sections must be [S, 5]")
        self._call("set_sections", int(k), sec.ctypes.data_as(_lib._fp), sec.shape[0])

    def sections(self, k: int) -> np.ndarray:
        n = ctypes.c_int32(0)
        self._call("get_sections", int(k), None, 0, ctypes.byref(n))
        sec = np.empty((n.value, 5), np.float32)
        self._call("get_sections", int(k), sec.ctypes.data_as(_lib._fp), n.value, ctypes.byref(n))
        return sec

    def reset(self, k: int | None = None) -> None:
        """Slot k's carry (None: every slot's) to zeros; the sections stay."""
        self._call("reset", -1 if k is None else int(k))

    @staticmethod
    def plan(num_sections: int, n: int, a_mod_b: int = 0) -> dict:
        return audio_iir_plan(num_sections, n, a_mod_b)

    _count_array = AudioFilterBank._count_array
    process_device = AudioFilterBank.process_device
    process_tensor = AudioFilterBank.process_tensor
    process = AudioFilterBank.process


# ---------------------------------------------------------------- audio resampler bank

AUDIO_RS_MAX_L = _lib.RFA_AUDIO_RS_MAX_L
AUDIO_RS_MAX_D = _lib.RFA_AUDIO_RS_MAX_D
AUDIO_RS_MAX_TAPS = _lib.RFA_AUDIO_RS_MAX_TAPS
AUDIO_RS_MAX_PHASE_TAPS = _lib.RFA_AUDIO_RS_MAX_PHASE_TAPS
AUDIO_RS_PLAN_FIELDS = ("tile", "lds_bytes", "path", "outputs_per_thread", "workgroups")    # rfa_audio_rs_plan order


def _check_resampler_shape(L: int, D: int, num_taps: int) -> None:
    """The limits of ``rfa_audio_rs_create`` as ``ValueError``s that name them.  Host only."""
    if not 1 <= L <= AUDIO_RS_MAX_L:
        raise ValueError(f"L = {L} outside 1 ... {AUDIO_RS_MAX_L}")
    if not L <= D <= AUDIO_RS_MAX_D:
        raise ValueError(f"D = {D} outside L = {L} ... {AUDIO_RS_MAX_D} (no up-sampling)")
    if math.gcd(L, D) != 1:
        raise ValueError(f"L / D = {L} / {D} is not reduced")
    if not 0 <= num_taps <= AUDIO_RS_MAX_TAPS:
        raise ValueError(f"{num_taps} taps, above {AUDIO_RS_MAX_TAPS}")
    if num_taps == 0 and (L, D) != (1, 1):
        raise ValueError("only L = D = 1 may have no taps")
    if -(-num_taps // L) > AUDIO_RS_MAX_PHASE_TAPS:
        raise ValueError(f"{-(-num_taps // L)} taps per phase, above {AUDIO_RS_MAX_PHASE_TAPS}")


def resampler_taps(in_rate: int = AUDIO_RATE, out_rate: int = 8000, transition_hz: float | None = None,
                   attenuation_db: float = 60.0):
    """(L, D, float32 taps) of an ``AudioResamplerBank`` from ``in_rate`` to ``out_rate``: L / D is
    out / in reduced and the prototype is the reference's own low-pass design at the rate L * in_rate
    with gain L, ``create_low_pass_taps(L, L * in_rate, (pass + stop) / 2, stop - pass, attenuation_db)``
    with the stopband edge ``stop`` at min(in, out) / 2 and the passband edge ``pass`` at 0.85 of it,
    or at ``stop - transition_hz``.  219 taps at the defaults.  That design has its -6 dB point at the
    cutoff, the middle of the transition band: the stopband edge itself is at -23 dB and the attenuation
    asked for is reached about half a band above it (DESIGN.md 5.7n has the table).  ``ValueError``,
    naming the limit, for a ratio or a tap count outside the handle's limits.  Host only."""
    in_rate, out_rate = int(in_rate), int(out_rate)
    if in_rate < 1 or out_rate < 1:
        raise ValueError("rates must be positive")
    g = math.gcd(in_rate, out_rate)
    L, D = out_rate // g, in_rate // g
    _check_resampler_shape(L, D, 1)
    stop = min(in_rate, out_rate) / 2.0
    width = 0.15 * stop if transition_hz is None else float(transition_hz)
    if not (math.isfinite(width) and 0.0 < width < stop):
        raise ValueError(f"transition_hz must lie between 0 and the stopband edge, {stop} Hz")
    taps = create_low_pass_taps(float(L), float(L) * in_rate, stop - width / 2.0, width, float(attenuation_db))
    if taps is None:
        raise ValueError("the low-pass design rejected these arguments")
    _check_resampler_shape(L, D, taps.size)
    return L, D, taps.astype(np.float32)


def audio_rs_counts(L: int, D: int, r: int, n: int) -> tuple[int, int]:
    """(outputs, next offset) of a slot at offset ``r`` given ``n`` inputs (``rfa_audio_rs_counts``).  Host only."""
    n_out, r_next = ctypes.c_size_t(0), ctypes.c_int32(0)
    _lib.check(_lib.lib().rfa_audio_rs_counts(int(L), int(D), int(r), int(n), ctypes.byref(n_out), ctypes.byref(r_next)),
               "rfa_audio_rs_counts")
    return n_out.value, r_next.value


def audio_rs_plan(L: int, D: int, num_taps: int, n: int) -> dict:
    """What a call of one slot at offset 0 with ``n`` inputs runs (``rfa_audio_rs_plan``): ``tile`` (outputs per
    workgroup), ``lds_bytes``, ``path`` ("none", "convert", "decimate", "polyphase"), ``outputs_per_thread``
    and ``workgroups``.  Host only."""
    out = (ctypes.c_int32 * _lib.RFA_AUDIO_RS_PLAN_FIELDS)()
    _lib.check(_lib.lib().rfa_audio_rs_plan(int(L), int(D), int(num_taps), int(n), out), "rfa_audio_rs_plan")
    plan = dict(zip(AUDIO_RS_PLAN_FIELDS, (int(v) for v in out)))
    plan["path"] = _lib.RFA_AUDIO_RS_PATHS[plan["path"]]
    return plan


class AudioResamplerBank(_Handle):
    """Each of ``n_channels`` audio rows resampled by L / D through one real prototype FIR and written
    as int16 PCM, float32 or both (``rfa_audio_rs_*``, ``rfanalyzer_amd/csrc/audio_rs.hip``).  A slot
    keeps its last 4095 inputs on the device and an offset r on the host; output m of a call has
    u = r + m D, i = u // L, p = u % L and is ``((0 + h[p] x[i]) + h[p+L] x[i-1]) + ...`` with every
    product and sum rounded to float32, so a stream cut into calls anywhere gives the bits and the
    count of the stream given whole.  PCM is ``rint(y * 32768)`` clipped to int16, NaN as 0.  One
    launch per call whatever the slot count; ``process_device`` is asynchronous on the handle's stream."""

    _prefix = "rfa_audio_rs"

    def __init__(self, n_channels: int, L: int, D: int, taps, device: int = 0):
        self.n_channels = int(n_channels)
        taps = np.ascontiguousarray(np.zeros(0) if taps is None else taps, np.float32)
        if taps.ndim != 1:
            raise ValueError("taps must be 1-D")
        _check_resampler_shape(int(L), int(D), taps.size)
        if not np.isfinite(taps).all():
            raise ValueError("a tap is not finite")
        self._create("rfa_audio_rs_create", device, self.n_channels, int(L), int(D),
                     taps.ctypes.data_as(_lib._fp) if taps.size else None, taps.size)
        self._ratio = (int(L), int(D))
        self._n_out = (ctypes.c_size_t * self.n_channels)()

    @classmethod
    def for_rates(cls, n_channels: int, out_rate: int, in_rate: int = AUDIO_RATE, device: int = 0, **design):
        """A bank from ``in_rate`` to ``out_rate`` with ``resampler_taps(in_rate, out_rate, **design)``."""
        return cls(n_channels, *resampler_taps(in_rate, out_rate, **design), device=device)

    @property
    def ratio(self) -> tuple[int, int]:
        """(L, D)."""
        return self._ratio

    @property
    def taps(self) -> np.ndarray:
        return self._query_floats("get_taps", 1, 1)[0][0]

    def offset(self, k: int) -> int:
        """Slot k's offset r as of the calls made so far."""
        r = ctypes.c_int32(0)
        self._call("get_offset", int(k), ctypes.byref(r))
        return r.value

    def reset(self, k: int | None = None) -> None:
        """Slot k's history (None: every slot's) to zeros and its offset to 0."""
        self._call("reset", -1 if k is None else int(k))

    def max_outputs(self, n: int) -> int:
        """ceil(n L / D): the most outputs a call of n inputs writes."""
        return int(_lib.lib().rfa_audio_rs_max_outputs(*self._ratio, int(n)))

    def plan(self, n: int, num_taps: int | None = None) -> dict:
        return audio_rs_plan(*self._ratio, self.taps.size if num_taps is None else num_taps, n)

    _count_array = AudioFilterBank._count_array

    def process_device(self, in_ptr: int, in_stride: int, counts, f32_ptr: int | None, f32_stride: int,
                       s16_ptr: int | None, s16_stride: int) -> list[int]:
        """Device rows in (stride in floats), float32 rows and / or int16 rows out (strides in elements;
        a pointer may be None, not both), one count per slot.  Enqueues on the handle's stream and returns
        every slot's output count."""
        self._call("process", in_ptr, in_stride, self._count_array(counts), f32_ptr or None, f32_stride,
                   s16_ptr or None, s16_stride, self._n_out)
        return list(self._n_out)

    def process_tensor(self, audio, counts, out_s16=None, out_f32=None) -> list[int]:
        """torch.cuda tensors [K, width]: float32 in, int16 and / or float32 out (rows may be slices of
        wider tensors) and one count per slot; on torch's current stream.  Returns the output counts."""
        self._follow_torch_stream(audio)
        K = self.n_channels
        if out_s16 is None and out_f32 is None:
            raise ValueError("out_s16, out_f32 or both")
        for t, dt in ((audio, "torch.float32"), (out_s16, "torch.int16"), (out_f32, "torch.float32")):
            if t is None:
                continue
            if t.dim() != 2 or t.shape[0] != K or str(t.dtype) != dt:
                raise ValueError(f"audio and out_f32 must be float32 and out_s16 int16, of shape [{K}, n]")
            if t.shape[1] > 1 and t.stride(1) != 1:
                raise ValueError("rows must be contiguous")
        counts = self._count_array(counts)
        if max(counts) > audio.shape[1]:
            raise ValueError("a count above the rows' length")
        need = self.max_outputs(max(counts))
        if any(t is not None and t.shape[1] < need for t in (out_s16, out_f32)):
            raise ValueError(f"output rows shorter than {need}")
        stride = lambda t: 0 if t is None else t.stride(0) if K > 1 else t.shape[1]
        return self.process_device(audio.data_ptr(), stride(audio), counts,
                                   None if out_f32 is None else out_f32.data_ptr(), stride(out_f32),
                                   None if out_s16 is None else out_s16.data_ptr(), stride(out_s16))

    def process_both(self, rows, counts=None) -> tuple[list[np.ndarray], list[np.ndarray]]:
        """Host float32 [K, width] rows and one count per slot (default: the width) -> (K int16 arrays,
        K float32 arrays) of one call that writes both outputs."""
        rows = np.ascontiguousarray(rows, np.float32)
        if rows.ndim != 2 or rows.shape[0] != self.n_channels:
            raise ValueError(f"rows must have shape [{self.n_channels}, n]")
        counts = self._count_array([rows.shape[1]] * self.n_channels if counts is None else counts)
        if max(counts) > rows.shape[1]:
            raise ValueError("a count above the rows' length")
        width = max(self.max_outputs(max(counts)), 1)
        pcm = np.zeros((self.n_channels, width), np.int16)
        f32 = np.zeros((self.n_channels, width), np.float32)
        self._call("process_host", rows.ctypes.data, rows.shape[1], counts, f32.ctypes.data, width, pcm.ctypes.data,
                   width, self._n_out)
        return ([pcm[k, :c].copy() for k, c in enumerate(self._n_out)],
                [f32[k, :c].copy() for k, c in enumerate(self._n_out)])

    def process(self, rows, counts=None, pcm: bool = True) -> list[np.ndarray]:
        """Host float32 [K, width] rows and one count per slot (default: the width) -> K int16 arrays
        (``pcm=False``: K float32 arrays)."""
        rows = np.ascontiguousarray(rows, np.float32)
        if rows.ndim != 2 or rows.shape[0] != self.n_channels:
            raise ValueError(f"rows must have shape [{self.n_channels}, n]")
        counts = self._count_array([rows.shape[1]] * self.n_channels if counts is None else counts)
        if max(counts) > rows.shape[1]:
            raise ValueError("a count above the rows' length")
        width = max(self.max_outputs(max(counts)), 1)
        out = np.zeros((self.n_channels, width), np.int16 if pcm else np.float32)
        ptrs = (None, 0, out.ctypes.data, width) if pcm else (out.ctypes.data, width, None, 0)
        self._call("process_host", rows.ctypes.data, rows.shape[1], counts, *ptrs, self._n_out)
        return [out[k, :c].copy() for k, c in enumerate(self._n_out)]


def _pcm_entry(pcm):
    """The ``pcm=`` keyword of a bank chain -> None or (L, D, taps).  Host only: a wrong entry raises
    before any device work."""
    if pcm is None:
        return None
    if isinstance(pcm, bool):
        raise ValueError("pcm must be None, an output rate in Hz or a dict of AudioResamplerBank.for_rates keywords")
    if isinstance(pcm, (int, np.integer)):
        return resampler_taps(AUDIO_RATE, int(pcm))
    if not isinstance(pcm, dict):
        raise ValueError("pcm must be None, an output rate in Hz or a dict of AudioResamplerBank.for_rates keywords")
    design = dict(pcm)
    explicit = [key in design for key in ("L", "D", "taps")]
    if any(explicit):
        if not all(explicit) or len(design) != 3:
            raise ValueError("an explicit resampler is exactly L, D and taps")
        taps = np.ascontiguousarray(np.zeros(0) if design["taps"] is None else design["taps"], np.float32)
        if taps.ndim != 1 or not np.isfinite(taps).all():
            raise ValueError("taps must be 1-D and finite")
        _check_resampler_shape(int(design["L"]), int(design["D"]), taps.size)
        return int(design["L"]), int(design["D"]), taps
    unknown = set(design) - {"out_rate", "in_rate", "transition_hz", "attenuation_db"}
    if unknown or "out_rate" not in design:
        raise ValueError(f"pcm takes out_rate, in_rate, transition_hz and attenuation_db; got {sorted(design)}")
    if int(design.get("in_rate", AUDIO_RATE)) != AUDIO_RATE:
        raise ValueError(f"a chain's audio rows run at {AUDIO_RATE} Hz")
    design.pop("in_rate", None)
    return resampler_taps(AUDIO_RATE, int(design.pop("out_rate")), **design)


class _Chain:
    """What the receiver chains share: the context manager, the audio tensor and the staging of
    one host packet.  A chain has ``front``, ``_buffers``, ``process_device`` and ``close``."""

    _raw = _re = _im = _audio = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def audio_tensor(self):
        return self._audio

    def _process_host(self, raw_bytes, demod):
        """One raw input packet (host bytes) through ``process_device``, waited for on ``demod``."""
        torch = self._torch
        buf = _raw_bytes(raw_bytes)
        n = buf.size // BYTES_PER_SAMPLE[self.front.fmt]
        self._buffers(buf.size, n)
        demod.synchronize()                           # the staging buffer's previous use is over
        self._raw[:buf.size].copy_(torch.from_numpy(buf.copy()))
        torch.cuda.synchronize(self._tdev)
        got = self.process_device(self._raw.data_ptr(), n)
        demod.synchronize()
        return got


class Receiver(_Chain):
    """Raw IQ bytes -> audio: ``FrontEnd(..., resampler=True)`` at the mode's quadrature rate
    chained into a ``Demodulator``, device to device on one stream.  One ``process`` call is
    one input packet, as the app's Scheduler feeds its Demodulator.  Changing ``mode`` retunes
    the front end's output rate (Demodulator.kt:96-100 sets ``resampler.outputSampleRate``);
    where the rate changes the resampler is built anew with an empty delay line, as
    Resampler.kt:102-110 does (and, unlike the app's IQConverter, the mixer's cosine index
    starts again with it)."""

    def __init__(self, input_format: str, sample_rate: int, mode="nfm", device: int = 0):
        import torch

        self._torch = torch
        self.input_format, self.sample_rate, self.device = input_format, int(sample_rate), device
        self._tdev = torch.device("cuda", device)
        self.demod = Demodulator(mode, device)
        self.front = None
        self._freqs = None
        self._cap_for = (None, 0)
        self._retune()

    def _retune(self) -> None:
        rate = self.demod.quadrature_rate
        if self.front is not None and self.front.output_sample_rate == rate:
            return
        if self.front is not None:
            self.front.close()
        self.front = FrontEnd(self.input_format, self.sample_rate, rate, self.device, resampler=True)
        self.front.set_stream(self.demod.stream)
        if self._freqs is not None:
            self.front.set_frequencies(*self._freqs)

    @property
    def mode(self) -> int:
        return self.demod.demodulationMode

    @mode.setter
    def mode(self, mode) -> None:
        self.demod.demodulationMode = mode
        self._retune()

    def set_frequencies(self, frequency: int, channel_frequency: int) -> None:
        self._freqs = (int(frequency), int(channel_frequency))
        self.front.set_frequencies(*self._freqs)

    def set_stream(self, stream_ptr: int | None) -> None:
        """Enqueue both stages on exactly this hipStream_t (None: the demodulator's own stream)."""
        self.demod.set_stream(stream_ptr)
        self.front.set_stream(self.demod.stream)

    def _buffers(self, nbytes: int, n: int):
        torch = self._torch
        if self._raw is None or self._raw.numel() < nbytes:
            self._raw = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=self._tdev)
        if self._cap_for[0] != (n, id(self.front)):
            self._cap_for = ((n, id(self.front)), self.front.max_outputs(n))
        cap = self._cap_for[1]
        if self._re is None or self._re.numel() < cap:
            self._re = torch.empty(cap, dtype=torch.float32, device=self._tdev)
            self._im = torch.empty(cap, dtype=torch.float32, device=self._tdev)
            self._audio = torch.empty(cap, dtype=torch.float32, device=self._tdev)
        return cap

    def process_device(self, raw_ptr: int, n_samples: int) -> int:
        """Raw samples at a device address -> audio left in ``self.audio_tensor``; asynchronous on
        the receiver's stream; returns the audio sample count."""
        cap = self._buffers(0, n_samples)
        nq = self.front.process_device(raw_ptr, n_samples, self._re.data_ptr(), self._im.data_ptr(), cap)
        return self.demod.process_device(self._re.data_ptr(), self._im.data_ptr(), nq, self._audio.data_ptr(), cap)

    def process(self, raw_bytes) -> np.ndarray:
        """One raw input packet (host bytes) -> float32 audio."""
        got = self._process_host(raw_bytes, self.demod)
        return self._audio[:got].cpu().numpy()

    def close(self) -> None:
        if self.front is not None:
            self.front.close()
            self.front = None
        self.demod.close()


def _common_rate(modes):
    """(the modes as a list, their one quadrature rate): a bank chain's slots share the front end."""
    modes = list(modes)
    if not modes:
        raise ValueError("at least one mode")
    rates = {mode_info(m)[0] for m in modes}
    if len(rates) != 1:
        raise ValueError(f"the modes' quadrature rates differ: {sorted(rates)}")
    return modes, rates.pop()


class _BankChain(_Chain):
    """Raw IQ bytes -> one audio stream per slot: a banked front end at the modes' common
    quadrature rate feeding a ``DemodulatorBank``, device to device on one stream.  A subclass
    supplies ``_make_front(*front_args)`` and ``_capacity(n)``, the rows' length for a call of n
    samples.

    ``squelch``: None (no squelch handle; a call enqueues the front end and the demodulators and
    nothing else), True, or one threshold in dB per slot, None for a slot without squelch.  With
    a squelch the chain runs front end -> ``SquelchBank`` on the front end's rows -> a hold on
    the demodulator slots whose gate is closed -> demodulator bank.  The front end runs on every
    packet for every slot (it is shared, and the level is measured on its output); only the
    demodulator slot is held, so slot k's audio is that of a demodulator fed the always-running
    front end's output on its open packets only.  With a squelch, ``process_device`` returns
    after the front end of this call has finished -- the one wait, for the K sums; the
    demodulators stay asynchronous.

    ``afc`` (the chains that can tune: ``ReceiverBank``, ``TunedReceiverBank``): None (no meter
    handle, nothing more enqueued), True, or a dict of ``AfcRule``'s keywords; ``limit_hz`` defaults
    per slot to half the mode's default width -- beyond that the carrier has left the user filter.
    The chain then owns a ``FrequencyMeterBank`` (``meter``) and an ``AfcRule``.  Per call, after the
    front end: the meter is enqueued on the front end's rows, the squelch waits as before, the
    meter's sums are collected (behind a squelch they have arrived: same stream, enqueued earlier),
    the rule is stepped, and the demodulators follow.  A slot is active in the rule only in AM, NFM
    or WFM (SSB has no carrier, CW sits off centre by design) and, with a squelch, only on calls
    where its gate is open.  The chain remembers the frequencies of ``set_frequencies`` as nominal
    and, for the slots the rule reports, retunes the front end to nominal + correction through the
    setters ``set_frequencies`` itself uses, whole Hz, from the next call on, and drops those slots'
    carried samples.  A user ``set_frequencies`` resets the rule; until the first one nothing is
    metered.  AFC is the meter and those setter calls: the audio equals a chain without AFC that
    is given the same ``set_frequencies`` calls between the same packets.

    ``tone``: None (no tone meter handle, nothing more enqueued), or one entry per slot: a CTCSS tone
    in Hz, or None for a slot without tone squelch, which is always tone-open.  The chain then owns
    a ``ToneMeterBank`` on the audio rows (``tone_meter``) and a ``ToneRule``; a slot's guards are
    ``tone_guards`` of its tone.  Per call, after the demodulator bank of call j is enqueued: the
    sums of call j-1 are collected (enqueued before call j's kernels: in steady state nothing is
    waited for), the rule is stepped -- a slot is active where its count in call j-1 was above 0 --
    the meter is enqueued on call j's audio rows with call j's counts, and call j's counts are
    returned with 0 for the slots that have a tone and a closed gate.  The audio rows stay as the
    demodulators wrote them, the gate lags by one call, and a slot that the carrier squelch reopens
    starts tone-closed until its first window has passed.

    ``code``: None (no code meter handle, nothing more enqueued), or one entry per slot: a DCS code as
    ``dcs_parse`` takes it (``"023"``, ``"023I"``, ``0o023``), or None for a slot without code squelch,
    which is always code-open; a slot with both a tone and a code is a ``ValueError``.  The chain then
    owns a ``CodeMeterBank`` on the demodulators' audio rows (``code_meter``) and a ``CodeRule``, and
    steps them in the tone meter's order: collect call j-1, step the rule (a slot is active where its
    count in call j-1 was above 0), enqueue the meter on call j's rows with the demodulator bank's
    counts, report call j's counts with 0 for the slots whose code gate is closed.  The audio rows stay
    untouched, the gate lags by one call, and ``audio_filter=`` and ``pcm=`` treat a code-closed slot
    as a tone-closed one.

    ``audio_iir``: None (no handle, no buffer, nothing more enqueued), or one entry per slot: None
    (pass-through), ``"deemphasis"`` (``deemphasis_sections()``), ``"voice"`` (``tone_strip_sections()``),
    ``"voice+deemphasis"`` or an ``[S, 5]`` array of sections.  The chain then owns an ``AudioIirBank``
    (``audio_iir``) that runs directly behind the demodulator bank on every call, with the demodulator
    bank's own counts -- the ungated ones, so the stream stays continuous across closed gates -- into a
    row tensor of its own; ``audio_filter=`` and ``pcm=`` then read those rows.  The tone and code meters
    keep reading the demodulators' rows, and the reported counts, the gates and ``pcm()`` keep their
    meaning.  ``audio_tensor`` and ``process`` return the last stage present.

    ``audio_filter``: None (no filter handle, no second audio buffer, nothing more enqueued), or one
    entry per slot: None (pass-through), ``"voice"`` (``voice_taps()``) or a 1-D float array of taps.
    The chain then owns an ``AudioFilterBank`` (``audio_fir``) that runs behind the demodulator bank
    (behind the IIR bank with ``audio_iir=``) on every call with the demodulator bank's own counts
    (``audio_counts``) -- not the tone-gated ones, so a slot's filtered stream is continuous across
    closed gates -- into a second row tensor, which ``audio_tensor`` and ``process`` then return.  The
    tone meter keeps reading the demodulators' rows: it needs the tone.  The reported counts stay as
    without the filter.

    ``pcm``: None (no resampler handle, no PCM buffer, nothing more enqueued), an output rate in Hz, or a
    dict of ``AudioResamplerBank.for_rates`` keywords (``out_rate``, ``transition_hz``,
    ``attenuation_db``) or of exactly ``L``, ``D`` and ``taps``.  The chain then owns an
    ``AudioResamplerBank`` (``audio_rs``) that runs last on every call, on the rows ``audio_tensor``
    returns and with the demodulator bank's own counts -- the ungated ones, so a slot's PCM stream
    stays continuous across closed tone gates, as the filter's does -- into an int16 ``[K, cap]``
    tensor, ``pcm_tensor``.  ``pcm_counts`` are the last call's ungated output counts; ``pcm()``
    waits for the stream and returns K int16 arrays, empty for a slot whose reported audio count in
    this call is 0 (squelch-held or tone-closed).  ``process`` and its counts stay as they are."""

    squelch = None
    _pcm = None                # the resampler's int16 rows; the handle is self.audio_rs, present only with pcm=
    _pcm_counts = None
    _reported = None           # the last call's reported counts, kept only with pcm=
    _filtered = None           # the filter's rows; the handle is self.audio_fir, present only with audio_filter=
    _iir_rows = None           # the IIR bank's rows; the handle is self.audio_iir, present only with audio_iir=
    _audio_counts = None
    _code = None               # the CodeRule; the meter handle is self.code_meter, present only with code=
    _tone = None               # the ToneRule; the meter handle is self.tone_meter, present only with tone=
    _afc = None                # the AfcRule; the meter handle is self.meter, present only with AFC
    _nominal = None            # (frequency, [channel frequencies]) of the user's set_frequencies

    def __init__(self, input_format: str, sample_rate: int, modes, rate: int, device: int, *front_args,
                 squelch=None, afc=None, tone=None, audio_filter=None, pcm=None, code=None, audio_iir=None):
        import torch

        rule, self._afc_default_limit = _afc_rule(afc, modes, rate)
        probes = _tone_entries(tone, len(modes))
        codes = _code_entries(code, len(modes), None if probes is None else list(tone))
        filters = _audio_filter_entries(audio_filter, len(modes))
        iirs = _audio_iir_entries(audio_iir, len(modes))
        resampler = _pcm_entry(pcm)
        self._torch = torch
        self.input_format, self.sample_rate, self.device = input_format, int(sample_rate), device
        self._tdev = torch.device("cuda", device)
        self.quadrature_rate = rate
        self.demods, self.front = None, None
        self._n_channels = len(modes)
        try:
            self.demods = DemodulatorBank(modes, device)
            self.front = self._make_front(*front_args)
            if squelch is not None and squelch is not False:
                self.squelch = SquelchBank(self._n_channels, device)
                self._held = np.zeros(self._n_channels, bool)
                if squelch is not True:
                    thresholds = list(squelch)
                    if len(thresholds) != self._n_channels:
                        raise ValueError(f"{self._n_channels} squelch thresholds expected, got {len(thresholds)}")
                    for k, thr in enumerate(thresholds):
                        self.squelch.set(k, thr)
            if rule is not None:
                self.meter = FrequencyMeterBank(self._n_channels, device)
                self._afc = rule
                self._afc_ok = np.array([_mode_id(m) in _AFC_MODE_IDS for m in modes])
            if probes is not None:
                self.tone_meter = ToneMeterBank(self._n_channels, AUDIO_RATE, device)
                self._tone = ToneRule(self._n_channels, AUDIO_RATE)
                for k, f10 in enumerate(probes):
                    self._set_tone_probes(k, f10)
            if codes is not None:
                self.code_meter = CodeMeterBank(self._n_channels, AUDIO_RATE, device)
                self._code = CodeRule(self._n_channels)
                for k, entry in enumerate(codes):
                    if entry is not None:
                        self._code.set_code(k, *entry)
            if iirs is not None:
                self.audio_iir = AudioIirBank(self._n_channels, device)
                for k, sec in enumerate(iirs):
                    if sec is not None:
                        self.audio_iir.set_sections(k, sec)
            if filters is not None:
                self.audio_fir = AudioFilterBank(self._n_channels, device)
                for k, taps in enumerate(filters):
                    if taps is not None:
                        self.audio_fir.set_taps(k, taps)
            if resampler is not None:
                self.audio_rs = AudioResamplerBank(self._n_channels, *resampler, device=device)
            self.set_stream(None)
        except Exception:
            self.close()
            raise

    @property
    def n_channels(self) -> int:
        return self._n_channels

    def _squelch(self) -> SquelchBank:
        if self.squelch is None:
            raise ValueError("this chain was built without a squelch (squelch=None)")
        return self.squelch

    def set_squelch(self, k: int, threshold_db: float | None) -> None:
        """Slot k's squelch threshold in dB (None: no squelch on this slot, always open)."""
        self._squelch().set(k, threshold_db)

    @property
    def squelch_debounce(self) -> int:
        """Calls a slot stays open after its level fell to or below the threshold, plus one
        (the reference's 50-packet debounce by default)."""
        return self._squelch().debounce

    @squelch_debounce.setter
    def squelch_debounce(self, calls: int) -> None:
        self._squelch().debounce = calls

    @property
    def levels(self):
        """The last call's level per slot in dB (float32[K]); None without a squelch."""
        return None if self.squelch is None else self.squelch._levels.copy()

    @property
    def open(self):
        """The last call's gate per slot (bool[K]); None without a squelch."""
        return None if self.squelch is None else self.squelch._open.astype(bool)

    @property
    def frequency_errors(self):
        """Every slot's last error estimate in Hz, relative to where it was tuned then (float64[K],
        NaN before a slot's first); None without AFC."""
        return None if self._afc is None else self._afc.errors_hz

    @property
    def corrections(self):
        """The correction applied to every slot in Hz (float64[K]); None without AFC."""
        return None if self._afc is None else self._afc.corrections

    def _tone_rule(self) -> ToneRule:
        if self._tone is None:
            raise ValueError("this chain was built without a tone squelch (tone=None)")
        return self._tone

    @property
    def tone_open(self):
        """The tone gate per slot as of the last call (bool[K]; True for a slot without a tone); None
        without ``tone=``."""
        return None if self._tone is None else self._tone.open

    @property
    def tone_quality(self):
        """Every slot's quality of its last evaluated window (float64[K], NaN before a slot's first);
        None without ``tone=``."""
        return None if self._tone is None else self._tone.quality

    def _set_tone_probes(self, k: int, f10) -> None:
        self.tone_meter.set_probes(k, f10)
        self.tone_meter.break_(k)
        self._tone.set_used(k, [f != 0 for f in f10])

    def set_tone(self, k: int, hz: float | None) -> None:
        """Slot k's wanted tone in Hz (None: no tone squelch on this slot, always tone-open): sets the
        probes, starts the slot's sample index again and resets its rule."""
        self._tone_rule()._slot(k)
        self._set_tone_probes(int(k), _tone_probes(hz))

    def _step_tone(self, counts, cap: int) -> list[int]:
        """Collect the previous call's sums, step the rule, enqueue the meter on this call's audio."""
        m = self.tone_meter
        m._call("collect", m._sums.ctypes.data, m._n.ctypes.data)
        gate = self._tone.update(m._sums, m._n)
        m._call("process", self._audio.data_ptr(), cap, self.demods._counts)
        return [c if g else 0 for c, g in zip(counts, gate)]

    def _code_rule(self) -> CodeRule:
        if self._code is None:
            raise ValueError("this chain was built without a code squelch (code=None)")
        return self._code

    @property
    def code_open(self):
        """The code gate per slot as of the last call (bool[K]; True for a slot without a code); None
        without ``code=``."""
        return None if self._code is None else self._code.open

    @property
    def code_score(self):
        """Every slot's score of its last evaluated window (float64[K], NaN before a slot's first);
        None without ``code=``."""
        return None if self._code is None else self._code.score

    def set_code(self, k: int, entry) -> None:
        """Slot k's wanted DCS code as ``dcs_parse`` takes it (None: no code squelch on this slot, always
        code-open): starts the slot's sub-cell index again and resets its rule."""
        rule = self._code_rule()
        k = rule._slot(k)
        parsed = None if entry is None else dcs_parse(entry)
        if parsed is not None and self._tone is not None and self._tone._used[k, 0]:
            raise ValueError(f"slot {k} has a tone: a slot has a tone or a code, not both")
        self.code_meter.break_(k)
        if parsed is None:
            rule.set_used(k, False)
        else:
            rule.set_code(k, *parsed)

    def _step_code(self, counts, cap: int) -> list[int]:
        """Collect the previous call's sub-cells, step the rule, enqueue the meter on this call's audio."""
        m = self.code_meter
        m._room(cap)
        m._call("collect", *m._out())
        gate = self._code.update(m._first, m._count, m._sums, m._bad, m._n)
        m._call("process", self._audio.data_ptr(), cap, self.demods._counts)
        return [c if g else 0 for c, g in zip(counts, gate)]

    @property
    def audio_tensor(self):
        """The rows of the last call, from the last stage present: the filter's with ``audio_filter=``,
        else the IIR bank's with ``audio_iir=``, else the demodulators'."""
        if self._filtered is not None:
            return self._filtered
        return self._audio if self._iir_rows is None else self._iir_rows

    @property
    def audio_counts(self):
        """The demodulator bank's counts of the last call, before any tone gate (list[int]; None before
        the first call): what the rows of ``audio_tensor`` hold."""
        return None if self._audio_counts is None else list(self._audio_counts)

    @property
    def pcm_tensor(self):
        """The int16 ``[K, cap]`` rows the resampler wrote in the last call; None without ``pcm=``."""
        return self._pcm

    @property
    def pcm_counts(self):
        """The resampler's output counts of the last call, before any gate (list[int]; None before the
        first call or without ``pcm=``): what the rows of ``pcm_tensor`` hold."""
        return None if self._pcm_counts is None else list(self._pcm_counts)

    def pcm(self) -> list[np.ndarray]:
        """The last call's PCM: waits for the stream; K int16 arrays cut to ``pcm_counts``, empty for a
        slot whose reported audio count in that call is 0."""
        if not hasattr(self, "audio_rs"):
            raise ValueError("this chain was built without a resampler (pcm=None)")
        if self._pcm_counts is None:
            return [np.zeros(0, np.int16) for _ in range(self._n_channels)]
        self.demods.synchronize()
        rows = self._pcm.cpu().numpy()
        return [rows[k, :c if g else 0].copy() for k, (c, g) in enumerate(zip(self._pcm_counts, self._reported))]

    def _audio_fir(self) -> AudioFilterBank:
        if not hasattr(self, "audio_fir"):
            raise ValueError("this chain was built without an audio filter (audio_filter=None)")
        return self.audio_fir

    def set_audio_filter(self, k: int, entry) -> None:
        """Slot k's audio filter from the next call on: None, ``"voice"`` or taps; its history stays."""
        fir = self._audio_fir()
        if not 0 <= int(k) < self._n_channels:
            raise ValueError(f"slot {k} outside 0 ... {self._n_channels - 1}")
        fir.set_taps(int(k), _audio_filter_taps(entry))

    def set_audio_iir(self, k: int, entry) -> None:
        """Slot k's audio IIR from the next call on: None, a name or ``[S, 5]`` sections; its carry is zeroed."""
        if not hasattr(self, "audio_iir"):
            raise ValueError("this chain was built without an audio IIR (audio_iir=None)")
        if not 0 <= int(k) < self._n_channels:
            raise ValueError(f"slot {k} outside 0 ... {self._n_channels - 1}")
        self.audio_iir.set_sections(int(k), _audio_iir_sections(entry))

    def _set_nominal(self, frequency: int, channel_frequencies) -> None:
        """After a user's ``set_frequencies`` went through: the rule starts again from these."""
        if self._afc is not None:
            self._nominal = (int(frequency), [int(f) for f in channel_frequencies])
            self._afc.reset()
            self.meter.break_()

    def _step_afc(self, active) -> None:
        """Collect the meter's sums, step the rule, retune the slots it reports."""
        m = self.meter
        m._call("collect", *m._out())
        rule = self._afc
        before = rule._estimate.copy(), rule._applied.copy()
        changed = rule.update(m._re, m._im, active)
        if changed:
            frequency, nominal = self._nominal
            try:
                self._tune(frequency, [f + int(round(c)) for f, c in zip(nominal, rule._applied)])
            except Exception:
                rule._estimate[:], rule._applied[:] = before      # the setters are all or nothing: so is the rule
                raise
            for k in changed:
                m.break_(k)

    def mode(self, k: int) -> int:
        return self.demods.mode(k)

    def set_mode(self, k: int, mode) -> None:
        """Slot k's DemodulationMode; only to a mode of the bank's quadrature rate."""
        if mode_info(mode)[0] != self.quadrature_rate:
            raise ValueError(f"mode {mode!r} has quadrature rate {mode_info(mode)[0]}, the bank runs at "
                             f"{self.quadrature_rate}")
        self.demods.set_mode(k, mode)
        if self._afc is not None:
            self._afc_ok[k] = _mode_id(mode) in _AFC_MODE_IDS
            if self._afc_default_limit:
                self._afc.limit_hz[k] = mode_info(mode)[3] / 2

    def set_stream(self, stream_ptr: int | None) -> None:
        """Enqueue every stage on exactly this hipStream_t (None: the demodulator bank's own)."""
        self.demods.set_stream(stream_ptr)
        self.front.set_stream(self.demods.stream)
        if self.squelch is not None:
            self.squelch.set_stream(self.demods.stream)
        if self._afc is not None:
            self.meter.set_stream(self.demods.stream)
        if self._tone is not None:
            self.tone_meter.set_stream(self.demods.stream)
        if self._code is not None:
            self.code_meter.set_stream(self.demods.stream)
        if hasattr(self, "audio_iir"):
            self.audio_iir.set_stream(self.demods.stream)
        if hasattr(self, "audio_fir"):
            self.audio_fir.set_stream(self.demods.stream)
        if hasattr(self, "audio_rs"):
            self.audio_rs.set_stream(self.demods.stream)

    def synchronize(self) -> None:
        self.demods.synchronize()

    def _buffers(self, nbytes: int, n: int) -> int:
        torch = self._torch
        if self._raw is None or self._raw.numel() < nbytes:
            self._raw = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=self._tdev)
        cap = self._capacity(n)
        if self._re is None or self._re.shape[1] < cap:
            shape = (self.n_channels, cap)
            self._re = torch.empty(shape, dtype=torch.float32, device=self._tdev)
            self._im = torch.empty(shape, dtype=torch.float32, device=self._tdev)
            self._audio = torch.empty(shape, dtype=torch.float32, device=self._tdev)
            if hasattr(self, "audio_iir"):
                self._iir_rows = torch.empty(shape, dtype=torch.float32, device=self._tdev)
            if hasattr(self, "audio_fir"):
                self._filtered = torch.empty(shape, dtype=torch.float32, device=self._tdev)
            if hasattr(self, "audio_rs"):
                self._pcm = torch.empty((self.n_channels, max(self.audio_rs.max_outputs(cap), 1)), dtype=torch.int16,
                                        device=self._tdev)
        return self._re.shape[1]

    def process_device(self, raw_ptr: int, n_samples: int) -> list[int]:
        """Raw samples at a device address -> audio left in the rows of ``self.audio_tensor``;
        asynchronous on the bank's stream (with a squelch: after the front end has finished, see
        the class); returns every slot's audio sample count, 0 for a slot whose gate is closed."""
        cap = self._buffers(0, n_samples)
        nq = self.front.process_device(raw_ptr, n_samples, self._re.data_ptr(), self._im.data_ptr(), cap)
        metered = self._nominal is not None
        if metered:
            self.meter._call("process", self._re.data_ptr(), self._im.data_ptr(), cap, nq)
        if self.squelch is not None:
            sq = self.squelch
            sq._call("process", self._re.data_ptr(), self._im.data_ptr(), cap, nq, sq._levels.ctypes.data,
                     sq._open.ctypes.data)
            closed = sq._open == 0
            for k in np.flatnonzero(closed != self._held):
                self.demods.set_hold(int(k), bool(closed[k]))
            self._held = closed
            if metered:
                self._step_afc(self._afc_ok & ~closed)
        elif metered:
            self._step_afc(self._afc_ok)
        counts = self.demods.process_device(self._re.data_ptr(), self._im.data_ptr(), cap, nq,
                                            self._audio.data_ptr(), cap)
        self._audio_counts = counts
        voice = self._audio
        if self._iir_rows is not None:
            voice = self._iir_rows
            self.audio_iir._call("process", self._audio.data_ptr(), cap, self.demods._counts, voice.data_ptr(), cap)
        if self._filtered is not None:
            self.audio_fir._call("process", voice.data_ptr(), cap, self.demods._counts,
                                 self._filtered.data_ptr(), cap)
        if self._tone is not None:
            counts = self._step_tone(counts, cap)
        if self._code is not None:
            counts = self._step_code(counts, cap)
        if self._pcm is not None:
            rs = self.audio_rs
            rs._call("process", self.audio_tensor.data_ptr(), cap, self.demods._counts, None, 0, self._pcm.data_ptr(),
                     self._pcm.shape[1], rs._n_out)
            self._pcm_counts, self._reported = list(rs._n_out), counts
        return counts

    def process(self, raw_bytes) -> list[np.ndarray]:
        """One raw input packet (host bytes) -> K float32 audio arrays."""
        got = self._process_host(raw_bytes, self.demods)
        audio = self.audio_tensor.cpu().numpy()
        return [audio[k, :g].copy() for k, g in enumerate(got)]

    def close(self) -> None:
        if self.front is not None:
            self.front.close()
            self.front = None
        if self.squelch is not None:
            self.squelch.close()
            self.squelch = None
        if self._afc is not None:
            self.meter.close()
            del self.meter
            self._afc = self._nominal = None
        if self._tone is not None:
            self.tone_meter.close()
            del self.tone_meter
            self._tone = None
        if self._code is not None:
            self.code_meter.close()
            del self.code_meter
            self._code = None
        if hasattr(self, "audio_iir"):
            self.audio_iir.close()
            del self.audio_iir
            self._iir_rows = None
        if hasattr(self, "audio_fir"):
            self.audio_fir.close()
            del self.audio_fir
            self._filtered = None
        if hasattr(self, "audio_rs"):
            self.audio_rs.close()
            del self.audio_rs
            self._pcm = None
        if self.demods is not None:
            self.demods.close()
            self.demods = None


class ReceiverBank(_BankChain):
    """Raw IQ bytes -> one audio stream per channel: a ``FrontEndBank(..., resampler=True)`` at
    the modes' quadrature rate feeding a ``DemodulatorBank``, device to device on one stream.
    Slot k's audio equals, bit for bit, a ``Receiver`` in mode ``modes[k]`` tuned to channel k
    and given the same packets.  The slots share the resampler, so every mode must have the
    same quadrature rate (``ValueError`` otherwise, at creation and in ``set_mode``).
    Both stages are banked: a packet is 2 + 4 launches whatever the channel count."""

    def __init__(self, input_format: str, sample_rate: int, modes, device: int = 0, *, squelch=None, afc=None,
                 tone=None, audio_filter=None, pcm=None, code=None, audio_iir=None):
        self._cap_for = (None, 0)
        super().__init__(input_format, sample_rate, *_common_rate(modes), device, squelch=squelch, afc=afc, tone=tone,
                         audio_filter=audio_filter, pcm=pcm, code=code, audio_iir=audio_iir)

    def _make_front(self):
        return FrontEndBank(self.input_format, self.sample_rate, self.quadrature_rate, self.n_channels, self.device,
                            resampler=True)

    def _capacity(self, n: int) -> int:
        if self._cap_for[0] != n:
            self._cap_for = (n, self.front.max_outputs(n))
        return self._cap_for[1]

    def _tune(self, frequency: int, channel_frequencies) -> None:
        self.front.set_frequencies(frequency, channel_frequencies)

    def set_frequencies(self, frequency: int, channel_frequencies) -> None:
        self._tune(frequency, channel_frequencies)
        self._set_nominal(frequency, channel_frequencies)


# ---------------------------------------------------------------- polyphase channelizer

PFB_PLAN_FIELDS = ("NT", "Mp", "run", "staged_run", "staged_taps", "rows_by_time", "stage_points", "lds_bytes",
                   "stages")                                # rfa_pfb_plan_field order; the radices follow
PFB_PLAN_MAX_STAGES = 12


def pfb_tile_plan(n_channels: int, interpolation: int, decimation: int, num_taps: int) -> dict:
    """The workgroup tile plan of a channelizer (``rfa_pfb_tile_plan``): output times per workgroup
    ``NT``, LDS row pitch ``Mp``, the ``run`` of samples a workgroup depends on, ``staged_run`` (0 / 1),
    ``staged_taps`` (integer handle: 0 / 1; rational: staged tap rows), ``rows_by_time`` (0 / 1),
    ``stage_points``, ``lds_bytes`` as launched, ``stages`` and the list ``radices``.  ``interpolation``
    0 is the handle of ``Channelizer(...)``, >= 1 that of ``Channelizer.rational``; ``num_taps`` is the
    prototype's length.  Host-only."""
    out = (ctypes.c_int32 * (len(PFB_PLAN_FIELDS) + PFB_PLAN_MAX_STAGES))()
    _lib.check(_lib.lib().rfa_pfb_tile_plan(n_channels, interpolation, decimation, num_taps, out),
               "rfa_pfb_tile_plan")
    plan = dict(zip(PFB_PLAN_FIELDS, (int(v) for v in out)))
    plan["radices"] = [int(v) for v in out[len(PFB_PLAN_FIELDS):len(PFB_PLAN_FIELDS) + plan["stages"]]]
    return plan


class Channelizer(_Handle):
    """All ``n_channels`` = M channels of the uniform raster k * Fs / M out of one raw IQ stream
    per call (``rfa_pfb_*``, ``rfanalyzer_amd/csrc/channelizer.hip``): the prototype low-pass
    ``taps`` is folded once per output time and one M-point DFT gives every channel, so a call
    is two kernel launches and costs about the same whatever the channel count.  M = 2^a 3^b 5^c,
    8 ... 4096; 1 <= ``decimation`` <= M; up to 16 * M taps.  Channel k is the stream mixed down
    by k * Fs / M (k >= M/2: the negative offsets), filtered and decimated; ``set_channels``
    picks which channels are written, slot j being channel ``channels[j]``.  The output rows are
    what ``DemodulatorBank.process_device`` reads.  A channel that is not on the raster is received
    through its nearest raster channel: ``for_channels`` widens the prototype, ``nearest_channel``
    picks the slot and ``set_offsets`` / ``set_tuning`` rotate it to DC inside the same launch."""

    _prefix = "rfa_pfb"

    def __init__(self, input_format: str, n_channels: int, decimation: int, taps, device: int = 0,
                 _interpolation: int | None = None):
        self.fmt = _format_id(input_format)
        self.n_channels = int(n_channels)
        self.interpolation = 1 if _interpolation is None else int(_interpolation)
        self.decimation = int(decimation)
        taps = np.ascontiguousarray(taps, np.float32).reshape(-1)
        if _interpolation is None:
            self._create("rfa_pfb_create", device, self.fmt, self.n_channels, self.decimation,
                         taps.ctypes.data_as(_lib._fp), taps.size)
        else:               # Channelizer.rational, L = 1 included
            self._create("rfa_pfb_create_rational", device, self.fmt, self.n_channels, self.interpolation,
                         self.decimation, taps.ctypes.data_as(_lib._fp), taps.size)
        self._n_selected = self.n_channels

    @classmethod
    def rational(cls, input_format: str, n_channels: int, interpolation: int, decimation: int, taps, device: int = 0):
        """The rational-rate channelizer (``rfa_pfb_create_rational``): the same raster at
        ``interpolation / decimation`` = L / D times the input rate, 1 <= L <= D <= L * M, gcd 1,
        L <= 64; ``taps`` is the prototype at L times the input rate, up to 16 * M * L taps.  Output
        n has phase (n * D) mod L and newest sample floor(n * D / L); after c samples ceil(c * L / D)
        outputs exist.  L = 1 keeps that convention (m_n = n * D), which is not the plain
        constructor's n * D + D - 1."""
        return cls(input_format, n_channels, decimation, taps, device, _interpolation=int(interpolation))

    @staticmethod
    def raster_ratio(sample_rate: int, spacing_hz: int, output_rate: int) -> tuple[int, int, int]:
        """(M, L, D) of ``for_raster_resampled``: M = sample_rate / spacing_hz, L / D = output_rate /
        sample_rate in lowest terms; ``ValueError`` where ``rfa_pfb_create_rational`` would refuse them.
        Host only."""
        sample_rate, spacing_hz, output_rate = int(sample_rate), int(spacing_hz), int(output_rate)
        if sample_rate <= 0 or spacing_hz <= 0 or output_rate <= 0:
            raise ValueError("rates and spacing must be positive")
        if sample_rate % spacing_hz:
            raise ValueError("sample_rate must be a whole multiple of spacing_hz")
        g = math.gcd(sample_rate, output_rate)
        M, L, D = sample_rate // spacing_hz, output_rate // g, sample_rate // g
        if L > D:
            raise ValueError("output_rate above sample_rate")
        if L > _lib.RFA_PFB_MAX_INTERPOLATION:
            raise ValueError(f"interpolation {L} above {_lib.RFA_PFB_MAX_INTERPOLATION}")
        if D > L * M:
            raise ValueError("output_rate below spacing_hz")
        if not _lib.lib().rfa_pfb_supported(M):
            raise ValueError(f"{M} channels: not 2^a 3^b 5^c within 8 ... 4096")
        return M, L, D

    @classmethod
    def for_raster_resampled(cls, input_format: str, sample_rate: int, spacing_hz: int, output_rate: int,
                             device: int = 0):
        """The channelizer of a raster at any source rate: ``sample_rate / spacing_hz`` channels (a
        whole number), each at ``output_rate`` = sample_rate * L / D in lowest terms, with the
        ``for_raster`` design moved to the interpolated rate as prototype
        (``create_low_pass_taps(L, L * sample_rate, 0.375 * spacing, 0.25 * spacing, 60)``, gain L,
        about 10.9 * M * L taps, so about 10.9 * M per output).  ``ValueError`` where a limit of
        ``rfa_pfb_create_rational`` fails."""
        M, L, D = cls.raster_ratio(sample_rate, spacing_hz, output_rate)
        taps = create_low_pass_taps(L, L * int(sample_rate), 0.375 * int(spacing_hz), 0.25 * int(spacing_hz), 60)
        if taps is None:
            raise ValueError("the low-pass design rejected the raster")
        if taps.size > 16 * M * L:
            raise ValueError(f"prototype of {taps.size} taps above 16 * {M} * {L}")
        return cls.rational(input_format, M, L, D, taps, device)

    @classmethod
    def for_raster(cls, input_format: str, sample_rate: int, spacing_hz: int, output_rate: int, device: int = 0):
        """The channelizer of a raster: ``sample_rate / spacing_hz`` channels, each at ``output_rate``,
        with the reference's own low-pass design as prototype (``create_low_pass_taps(1, sample_rate,
        0.375 * spacing, 0.25 * spacing, 60)``, about 10.9 taps per channel).  Both ratios must be
        whole numbers."""
        sample_rate, spacing_hz, output_rate = int(sample_rate), int(spacing_hz), int(output_rate)
        if sample_rate <= 0 or spacing_hz <= 0 or output_rate <= 0:
            raise ValueError("rates and spacing must be positive")
        if sample_rate % spacing_hz or sample_rate % output_rate:
            raise ValueError("sample_rate must be a whole multiple of spacing_hz and of output_rate")
        taps = create_low_pass_taps(1, sample_rate, 0.375 * spacing_hz, 0.25 * spacing_hz, 60)
        if taps is None:
            raise ValueError("the low-pass design rejected the raster")
        return cls(input_format, sample_rate // spacing_hz, sample_rate // output_rate, taps, device)

    @staticmethod
    def channels_design(sample_rate: int, spacing_hz: int, output_rate: int, passband_hz: float,
                        resample: bool = False):
        """((M, L, D), taps) of ``for_channels``: the raster of ``for_raster`` (L = 1) or
        ``for_raster_resampled``, and the prototype with pass edge fp = ``passband_hz`` and stop edge
        fs = ``output_rate / 2`` (where the output rate's own aliases begin):
        ``create_low_pass_taps(L, L * sample_rate, (fp + fs) / 2, fs - fp, 60)``.  ``ValueError``
        where fp >= fs or a channelizer limit fails.  Host only."""
        sample_rate, spacing_hz, output_rate = int(sample_rate), int(spacing_hz), int(output_rate)
        M, L, D = Channelizer.raster_ratio(sample_rate, spacing_hz, output_rate)
        if not resample and L != 1:
            raise ValueError("sample_rate must be a whole multiple of output_rate (or resample=True)")
        fp, fs = float(passband_hz), output_rate / 2
        if not 0 < fp < fs:
            raise ValueError(f"passband_hz {fp} must lie inside (0, output_rate / 2 = {fs})")
        taps = create_low_pass_taps(L, L * sample_rate, (fp + fs) / 2, fs - fp, 60)
        if taps is None:
            raise ValueError("the low-pass design rejected the raster")
        if taps.size > 16 * M * L:
            raise ValueError(f"prototype of {taps.size} taps above 16 * {M} * {L}")
        return (M, L, D), taps

    @classmethod
    def for_channels(cls, input_format: str, sample_rate: int, spacing_hz: int, output_rate: int, passband_hz: float,
                     device: int = 0, resample: bool = False):
        """The channelizer for receivers at any frequency: the raster of ``for_raster`` (or, with
        ``resample``, of ``for_raster_resampled``) with a prototype wide enough that a signal up to
        ``passband_hz`` from a raster centre passes (``channels_design``); ``set_offsets`` then moves
        it to DC and the demodulator's own filter selects the channel."""
        (M, L, D), taps = cls.channels_design(sample_rate, spacing_hz, output_rate, passband_hz, resample)
        if resample:
            return cls.rational(input_format, M, L, D, taps, device)
        return cls(input_format, M, D, taps, device)

    # -- configuration
    def set_channels(self, channels=None) -> None:
        """Slot j is channel ``channels[j]`` (any order, repeats allowed); None or empty: all
        channels in natural order.  An invalid list raises and leaves the selection as it was."""
        ch = [int(c) for c in channels] if channels is not None else []
        arr = (ctypes.c_int32 * max(len(ch), 1))(*ch)
        self._call("set_channels", arr if ch else None, len(ch))
        self._n_selected = len(ch) or self.n_channels

    @property
    def channels(self) -> list[int]:
        n = ctypes.c_int32(0)
        out = (ctypes.c_int32 * self.n_channels)()
        self._call("get_channels", out, self.n_channels, ctypes.byref(n))
        return list(out[:n.value])

    def channel_of(self, frequency: int, channel_frequency: int, sample_rate: int) -> int:
        """The channel k that holds ``channel_frequency`` when the stream is tuned to ``frequency``;
        ``ValueError`` where the offset is not on the raster."""
        num = (int(channel_frequency) - int(frequency)) * self.n_channels
        if num % int(sample_rate):
            raise ValueError(f"offset {int(channel_frequency) - int(frequency)} Hz is not on the raster of "
                             f"{sample_rate}/{self.n_channels} Hz")
        return (num // int(sample_rate)) % self.n_channels

    @staticmethod
    def nearest_raster_channel(n_channels: int, frequency: int, channel_frequency: int, sample_rate: int):
        """``nearest_channel`` for a raster of ``n_channels``, without a handle.  Host only."""
        M, fs = int(n_channels), int(sample_rate)
        if M <= 0 or fs <= 0 or fs % M:
            raise ValueError(f"the spacing {sample_rate}/{n_channels} Hz must be a whole number of Hz")
        spacing = fs // M
        offset = int(channel_frequency) - int(frequency)
        if 2 * abs(offset) > fs:
            raise ValueError(f"offset {offset} Hz is outside the stream's +-{fs / 2} Hz")
        k = (2 * offset + spacing) // (2 * spacing)                # floor((offset + spacing / 2) / spacing)
        return k % M, offset - k * spacing

    def nearest_channel(self, frequency: int, channel_frequency: int, sample_rate: int) -> tuple[int, int]:
        """(k, delta_hz): the raster channel nearest to ``channel_frequency`` when the stream is tuned
        to ``frequency``, and what is left for ``set_offsets``: k = floor((offset + spacing / 2) /
        spacing) mod M with spacing = sample_rate / n_channels (a whole number of Hz), delta = offset -
        (unwrapped k) * spacing in [-spacing / 2, spacing / 2).  ``ValueError`` where |offset| >
        sample_rate / 2.  Host only."""
        return self.nearest_raster_channel(self.n_channels, frequency, channel_frequency, sample_rate)

    @staticmethod
    def offsets_tuning(offsets_hz, output_rate: int) -> tuple[int, list[int]]:
        """(q, steps) of ``set_offsets``: g = gcd(output_rate, |offsets| ...), q = output_rate / g,
        m_j = offset_j / g, so that m_j * output_rate / q is offset_j exactly.  ``ValueError`` for a
        non-integer offset, |offset| >= output_rate, or q above ``RFA_PFB_TUNE_MAX_STEPS``.  Host only."""
        rate = int(output_rate)
        if rate <= 0:
            raise ValueError("output_rate must be positive")
        offs = []
        for o in offsets_hz:
            if int(o) != o:
                raise ValueError(f"offset {o!r} is not a whole number of Hz")
            offs.append(int(o))
        g = math.gcd(rate, *[abs(o) for o in offs])
        q = rate // g
        if q > _lib.RFA_PFB_TUNE_MAX_STEPS:
            raise ValueError(f"tuning denominator {q} above {_lib.RFA_PFB_TUNE_MAX_STEPS}")
        if any(abs(o) >= rate for o in offs):
            raise ValueError(f"an offset of {output_rate} Hz or more cannot be tuned at that output rate")
        return q, [o // g for o in offs]

    def set_tuning(self, q: int = 0, steps=None) -> None:
        """Slot j is rotated by exp(-2 pi j steps[j] n / q) on its way out, n the absolute output
        index (``rfa_pfb_set_tuning``): a signal steps[j] * output_rate / q Hz above the raster centre
        lands at DC.  One step per selected slot, -q < step < q, 1 <= q <= 2^20; q = 0 or steps None
        removes the tuning.  An invalid request raises and leaves the tuning as it was;
        ``set_channels`` removes it."""
        if steps is None or not q:
            self._call("set_tuning", 0, None, 0)
            return
        st = [int(m) for m in steps]
        arr = (ctypes.c_int32 * max(len(st), 1))(*st)
        self._call("set_tuning", int(q), arr, len(st))

    @property
    def tuning(self):
        """None, or (q, steps) as given to ``set_tuning``."""
        q, n = ctypes.c_int32(0), ctypes.c_int32(0)
        out = (ctypes.c_int32 * self.n_channels)()
        self._call("get_tuning", ctypes.byref(q), out, self.n_channels, ctypes.byref(n))
        return (q.value, list(out[:n.value])) if q.value else None

    def set_offsets(self, offsets_hz, output_rate: int) -> None:
        """Slot j receives ``offsets_hz[j]`` (whole Hz) above its raster centre: ``set_tuning`` with
        the smallest table that holds every offset exactly (``offsets_tuning``)."""
        self.set_tuning(*self.offsets_tuning(offsets_hz, output_rate))

    def plan(self) -> dict:
        """{"n_channels", "decimation", "num_taps", "radices"}: the DFT's radices in stage order."""
        v = [ctypes.c_int32(0) for _ in range(4)]
        rad = (ctypes.c_int32 * 16)()
        self._call("get_plan", ctypes.byref(v[0]), ctypes.byref(v[1]), ctypes.byref(v[2]), rad, 16, ctypes.byref(v[3]))
        return {"n_channels": v[0].value, "decimation": v[1].value, "num_taps": v[2].value,
                "radices": list(rad[:v[3].value])}

    @property
    def taps(self) -> np.ndarray:
        return self._query_floats("get_taps", 1, 1)[0][0]

    @property
    def ratio(self) -> tuple[int, int, int]:
        """(interpolation, decimation, taps per output) as ``rfa_pfb_get_ratio`` reports them:
        (1, D, T) on an integer handle, (L, D, ceil(T / L)) on a rational one."""
        v = [ctypes.c_int32(0) for _ in range(3)]
        self._call("get_ratio", *[ctypes.byref(x) for x in v])
        return v[0].value, v[1].value, v[2].value

    def max_outputs(self, n_samples: int) -> int:
        """The exact output count per channel of the next call of ``n_samples``."""
        n = ctypes.c_size_t(0)
        self._call("max_outputs", n_samples, ctypes.byref(n))
        return n.value

    # -- processing
    def process(self, data) -> list[np.ndarray]:
        """Host bytes / numpy in -> one complex64 array per selected channel."""
        buf = _raw_bytes(data)
        n = buf.size // BYTES_PER_SAMPLE[self.fmt]
        cap = max(self.max_outputs(n), 1)
        re = np.empty((self._n_selected, cap), np.float32)
        im = np.empty((self._n_selected, cap), np.float32)
        got = ctypes.c_size_t(0)
        self._call("process_host", buf.ctypes.data, n, re.ctypes.data, im.ctypes.data, cap, ctypes.byref(got))
        out = np.empty((self._n_selected, got.value), np.complex64)
        out.real, out.imag = re[:, :got.value], im[:, :got.value]
        return list(out)

    def process_device(self, in_ptr: int, n_samples: int, re_ptr: int, im_ptr: int, channel_stride: int) -> int:
        """Device pointers, outputs [selected][channel_stride] floats; asynchronous on the handle's
        stream; returns the output count per channel."""
        got = ctypes.c_size_t(0)
        self._call("process", in_ptr, n_samples, re_ptr, im_ptr, channel_stride, ctypes.byref(got))
        return got.value

    def process_tensor(self, raw, out_re, out_im) -> int:
        """torch.cuda tensors: raw bytes (contiguous) -> float32 outputs of shape [selected, stride],
        on torch's current stream (see ``FrontEnd.process_tensor``)."""
        self._follow_torch_stream(raw)
        n = raw.numel() * raw.element_size() // BYTES_PER_SAMPLE[self.fmt]
        if out_re.shape != out_im.shape or out_re.dim() != 2 or out_re.shape[0] != self._n_selected:
            raise ValueError(f"out_re and out_im must both have shape [{self._n_selected}, stride]")
        if not (out_re.is_contiguous() and out_im.is_contiguous()):
            raise ValueError("out_re and out_im must be contiguous")
        return self.process_device(raw.data_ptr(), n, out_re.data_ptr(), out_im.data_ptr(), out_re.shape[1])

    def reset(self) -> None:
        """History zeroed, sample count 0."""
        self._call("reset")


class RasterReceiverBank(_BankChain):
    """Raw IQ bytes -> one audio stream per raster channel: a ``Channelizer.for_raster`` at the
    modes' common quadrature rate feeding a ``DemodulatorBank``, device to device on one stream,
    2 + 4 launches per packet whatever the channel count.  Slot k demodulates raster channel
    ``channels[k]`` (default 0, 1, ...) in mode ``modes[k]``; its audio equals, bit for bit, a
    ``DemodulatorBank`` fed the ``Channelizer``'s own output.  Every mode must have the same
    quadrature rate (``ValueError`` otherwise, at creation and in ``set_mode``)."""

    def __init__(self, input_format: str, sample_rate: int, spacing_hz: int, modes, channels=None, device: int = 0,
                 resample: bool = False, *, squelch=None, afc=None, tone=None, audio_filter=None, pcm=None,
                 code=None, audio_iir=None):
        if afc is not None and afc is not False:
            raise ValueError("a RasterReceiverBank cannot tune: its prototype passes one raster channel per slot and "
                             "leaves no room to move; use a TunedReceiverBank for AFC")
        modes, rate = _common_rate(modes)
        channels = list(range(len(modes))) if channels is None else [int(c) for c in channels]
        if len(channels) != len(modes):
            raise ValueError(f"{len(modes)} channels expected, got {len(channels)}")
        self._resample = bool(resample)
        super().__init__(input_format, sample_rate, modes, rate, device, spacing_hz, channels, squelch=squelch,
                         tone=tone, audio_filter=audio_filter, pcm=pcm, code=code, audio_iir=audio_iir)

    def _make_front(self, spacing_hz: int, channels):
        make = Channelizer.for_raster_resampled if self._resample else Channelizer.for_raster
        front = make(self.input_format, self.sample_rate, spacing_hz, self.quadrature_rate, self.device)
        try:
            front.set_channels(channels)
        except Exception:
            front.close()
            raise
        return front

    def _capacity(self, n: int) -> int:
        if self._resample:                            # ceil(c1 L / D) - ceil(c0 L / D) <= ceil(n L / D)
            return -(-n * self.front.interpolation // self.front.decimation) + 1
        return n // self.front.decimation + 1         # an upper bound of any call of n samples

    @property
    def channels(self) -> list[int]:
        return self.front.channels


class TunedReceiverBank(_BankChain):
    """Raw IQ bytes -> one audio stream per channel at any frequency, with ``ReceiverBank``'s
    interface and the channelizer's cost: a ``Channelizer.for_channels`` on the raster of
    ``spacing_hz`` at the modes' common quadrature rate feeding a ``DemodulatorBank``, 2 + 4 launches
    per packet whatever the channel count.  ``set_frequencies`` gives every slot its nearest raster
    channel and the offset that is left (up to half a spacing) as a tuning, so the slot's signal
    sits at DC as behind a ``FrontEndBank``; the demodulator's user filter selects the channel.
    ``passband_hz`` is the prototype's pass edge: by default half a spacing plus the widest
    ``max_width`` of the modes (the widths are one-sided cut-offs, Demodulator.kt:215-226).  Slot
    k's audio equals, bit for bit, a ``DemodulatorBank`` fed the output of a ``for_channels`` handle
    with the same selection and offsets; with a squelch the level is measured on the tuned rows.
    Until ``set_frequencies`` is called the slots are raster channels 0, 1, ... untuned."""

    def __init__(self, input_format: str, sample_rate: int, spacing_hz: int, modes, device: int = 0,
                 resample: bool = False, *, squelch=None, passband_hz: float | None = None, afc=None, tone=None,
                 audio_filter=None, pcm=None, code=None, audio_iir=None):
        modes, rate = _common_rate(modes)
        if passband_hz is None:
            passband_hz = int(spacing_hz) / 2 + max(mode_info(m)[2] for m in modes)
        self.passband_hz = float(passband_hz)
        self._resample = bool(resample)
        super().__init__(input_format, sample_rate, modes, rate, device, spacing_hz, squelch=squelch, afc=afc,
                         tone=tone, audio_filter=audio_filter, pcm=pcm, code=code, audio_iir=audio_iir)

    def _make_front(self, spacing_hz: int):
        front = Channelizer.for_channels(self.input_format, self.sample_rate, spacing_hz, self.quadrature_rate,
                                         self.passband_hz, self.device, self._resample)
        try:
            front.set_channels(range(self.n_channels))
        except Exception:
            front.close()
            raise
        return front

    def _capacity(self, n: int) -> int:
        if self._resample:                            # ceil(c1 L / D) - ceil(c0 L / D) <= ceil(n L / D)
            return -(-n * self.front.interpolation // self.front.decimation) + 1
        return n // self.front.decimation + 1         # an upper bound of any call of n samples

    def set_frequencies(self, frequency: int, channel_frequencies) -> None:
        """The source's tuned frequency and one channel frequency per slot, whole Hz, each within the
        stream's +- sample_rate / 2."""
        self._tune(frequency, channel_frequencies)
        self._set_nominal(frequency, channel_frequencies)

    def _tune(self, frequency: int, channel_frequencies) -> None:
        freqs = [int(f) for f in channel_frequencies]
        if len(freqs) != self.n_channels:
            raise ValueError(f"{self.n_channels} channel frequencies expected, got {len(freqs)}")
        near = [self.front.nearest_channel(frequency, f, self.sample_rate) for f in freqs]
        tuning = Channelizer.offsets_tuning([d for _, d in near], self.quadrature_rate)   # raises before any change
        self.front.set_channels([k for k, _ in near])
        self.front.set_tuning(*tuning)

    @property
    def channels(self) -> list[int]:
        return self.front.channels

    @property
    def offsets(self) -> list[int]:
        """Every slot's offset from its raster centre in Hz."""
        t = self.front.tuning
        if t is None:
            return [0] * self.n_channels
        return [m * self.quadrature_rate // t[0] for m in t[1]]
