// audio_hist.h -- the per-slot input history that the audio stages behind the demodulator bank
// (audio_fir.hip, audio_rs.hip) keep on the device: a slot's last kAudioHist inputs, zeros at first,
// in two buffers of which a call reads one and the workgroup of tile 0 writes the other.
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/rfa.h"

constexpr int kAudioHist = RFA_AUDIO_FIR_MAX_TAPS - 1;

// Sample j of the history after a call of n inputs, as a position in (history ++ inputs):
// false and an index into the history before the call, or true and an index into the inputs.
__host__ __device__ inline bool hist_source(unsigned long long n, int j, unsigned long long &index) {
    const unsigned long long at = n + (unsigned long long)j;
    if (at < (unsigned long long)kAudioHist) {
        index = at;
        return false;
    }
    index = at - (unsigned long long)kAudioHist;
    return true;
}
