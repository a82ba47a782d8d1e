"""rfanalyzer_amd -- MI355X-native drop-in for RFAnalyzer's spectrum hot path.

Raw IQ bytes -> convert -> window -> FFT -> 10*log10(|X|/N) + fft-shift ->
waterfall ring / peak-hold / averaging, as hand-written gfx950 HIP kernels
behind the C-ABI in include/rfa.h (librfa.so).  The Python modules mirror the
reference's interfaces for this path:

    nativedsp.NativeDsp        nativedsp/.../NativeDsp.kt
    processor.FftProcessor     analyzer/FftProcessor.kt
    source.FileIQSource        source/FileIQSource.java (+ Scheduler framing)
    engine.SpectrumEngine      one librfa handle
    engine.SeamPlan            the legacy seams at pffft-only lengths (mixed 2/3/5, 16, 32, > 2^20)
    SpectrumEngine.draw_preprocess, scanner   AnalyzerSurface.drawPreprocessing, MainViewModel scanner
    recording                  Scheduler recording branch, file names, replay metadata
    demod.FrontEnd             IQConverter.mixPacketIntoSamplePacket + Decimator / Resampler
    demod.Demodulator          analyzer/Demodulator.kt + AudioSink.java: AM/FM/SSB/CW to 48 kHz audio
    demod.Receiver             FrontEnd chained into Demodulator, raw IQ bytes to audio
    demod.AudioFilterBank      (extension) a real FIR per bank slot on the audio rows; demod.voice_taps
    demod.AudioIirBank         (extension) recursive sections per bank slot on the audio rows: de-emphasis, tone strip;
                               demod.deemphasis_sections, demod.tone_strip_sections, audio_iir= on the bank chains
    demod.AudioResamplerBank   (extension) every bank slot's audio by L / D to 8 / 16 kHz s16 PCM; demod.resampler_taps,
                               pcm= on the bank chains, recording.AudioLogWriter
    scheduler.Scheduler       analyzer/Scheduler.kt packet fan-out

There is no CPU fallback: without librfa.so or a HIP device, calls raise.
"""
from ._lib import RfaError, build, device_count, lib  # noqa: F401
from .engine import SeamPlan, SpectrumEngine  # noqa: F401

__all__ = ["SpectrumEngine", "SeamPlan", "RfaError", "build", "device_count", "lib"]
