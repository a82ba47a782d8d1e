// demod.hip -- the demodulator proper on gfx950: quadrature-rate IQ (what
// rfa_ddc_process writes) -> 48 kHz float audio.  Paths relative to
// app/src/main/java/com/mantz_it/rfanalyzer/.
//
// Per packet the reference runs (analyzer/Demodulator.kt:151-187)
//   applyUserFilter (215-240)  ->  demodulateAM/FM/SSB/CW (251-403)  ->  volume
//   ->  AudioSink.applyAudioFilter (analyzer/AudioSink.java:215-237).
// Here one call carries any number of packets and runs four kernels:
//   1. demod_stage1_kernel: a workgroup owns 256 consecutive pre-gain outputs,
//      stages the inputs they depend on (plus halo and the carried history)
//      into LDS, writes the user-filtered samples back into LDS and runs the
//      mode's step from there (|x|^2, the discriminator, or the complex
//      band-pass FIR of dsp/ComplexFirFilter.java:123-170);
//   2. demod_packet_kernel: one wave per packet takes the packet's maximum and,
//      for AM, its sum in index order (loads coalesced, adds by one lane);
//   3. demod_state_kernel: one workgroup resolves the lastMax recurrence over
//      the call's packets and writes every piece of state the next call needs;
//   4. demod_audio_kernel: gain by packet index, volume, and the AudioSink's
//      one or two decimating FIRs over the continuous stream, through LDS.
// All filters are closed forms of the reference's counters: output n of a
// FirFilter built `in` samples ago has its newest input at n*D + off (off = D-1,
// or 1 for D = 1: decimationCounter starts at 1).  Output counts are computed on
// the host.  Products and sums are separately rounded in the reference's order.
//
// The bodies of the four kernels are the demod_*.inc files beside this one,
// included as text: once by the kernels above and once by the demodulator bank's
// (rfa_demod_bank_*, at the end of this file), which run K slots in one grid with
// the slot in blockIdx.y and each slot's launch record read from a device array.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "../../include/rfa.h"

#pragma clang fp contract(off)

#include "stage_common.h"

namespace {

constexpr int kTile = 256;               // outputs per workgroup
constexpr int kMaxUserTaps = 32;         // the user filter has 27
constexpr int kMaxBandTaps = 192;        // the band-pass filters have 181
constexpr int kMaxAudioTaps = 16;        // audioFilter1 has 9, audioFilter2 13
constexpr int kA1Dec = 2, kA2Dec = 4;    // AudioSink.java:94-96
constexpr int kAudioRate = 48000;

// device state, floats (two copies: a call reads one and writes the other)
constexpr int ST_UF_RE = 0, ST_UF_IM = ST_UF_RE + kMaxUserTaps;
constexpr int ST_BP_RE = ST_UF_IM + kMaxUserTaps, ST_BP_IM = ST_BP_RE + kMaxBandTaps;
constexpr int ST_A1 = ST_BP_IM + kMaxBandTaps, ST_A2 = ST_A1 + kMaxAudioTaps;
constexpr int ST_CARRY = ST_A2 + kMaxAudioTaps, ST_LMAX = ST_CARRY + 2;
constexpr int ST_SIZE = 512;
static_assert(ST_LMAX < ST_SIZE, "state layout");
// device taps
constexpr int TP_UF = 0, TP_BPR = TP_UF + kMaxUserTaps, TP_BPI = TP_BPR + kMaxBandTaps;
constexpr int TP_A1 = TP_BPI + kMaxBandTaps, TP_A2 = TP_A1 + kMaxAudioTaps, TP_SIZE = TP_A2 + kMaxAudioTaps;

enum { kKindOff = -1, kKindAm = 0, kKindFm = 1, kKindBand = 2 };   // off: bank slots only, every block returns

struct DemodLaunch {
    const float *re, *im;          // this call's input, planar
    long long n, ps, K;            // samples, packet size (>= 1), packets (>= 1)
    const float *st;               // state before the call
    float *nst;                    // state after it
    const float *taps;
    int kind;
    int Tu, Tb, T1, T2;            // taps of the user / band-pass / audio filters
    int Db, offb;                  // band-pass decimation and first-output offset (AM/FM: 1, 0)
    int skip;                      // 1: the user filter is fresh, its first input gives no output
    long long F;                   // user-filtered samples of this call: filtered f <-> input f + skip
    long long bp_in0, bp_out0;     // band-pass inputs / outputs before this call (AM/FM: 0, 0)
    long long npre;                // pre-gain values of this call
    float qgain, volume;
    int agc;                       // AM, SSB, CW
    int sink;                      // 0: none, 1: audioFilter1, 2: audioFilter1 then audioFilter2
    long long a1_in0, a1_out0, ny1, a2_in0, a2_out0, n_audio;
    float *pre, *pk_max, *pk_avg, *pk_gain, *out;
};

// ---------------------------------------------------------------- device helpers

__device__ __forceinline__ void in_at(const DemodLaunch &a, long long i, float &re, float &im) {
    if (i < 0) {
        re = a.st[ST_UF_RE + a.Tu - 1 + i];
        im = a.st[ST_UF_IM + a.Tu - 1 + i];
    } else {
        re = a.re[i];
        im = a.im[i];
    }
}

// user-filtered sample f >= 0 of this call, straight from memory (FirFilter.kt:86-95)
__device__ void filt_at(const DemodLaunch &a, long long f, float &re, float &im) {
    float sr = 0.0f, si = 0.0f;
    for (int k = 0; k < a.Tu; k++) {
        float xr, xi;
        in_at(a, f + a.skip - k, xr, xi);
        const float t = a.taps[TP_UF + k];
        sr = sr + t * xr;
        si = si + t * xi;
    }
    re = sr;
    im = si;
}

// user-filtered index of pre-gain value m: the band-pass output's newest input
__device__ __forceinline__ long long fidx(const DemodLaunch &a, long long m) {
    return (a.bp_out0 + m) * a.Db + a.offb - a.bp_in0;
}

// number of pre-gain values whose input index is below X
__device__ __forceinline__ long long pre_lower(const DemodLaunch &a, long long X) {
    const long long R = X - a.skip - a.offb + a.bp_in0;
    if (R <= 0) return 0;
    const long long c = (R + a.Db - 1) / a.Db - a.bp_out0;
    return c < 0 ? 0 : (c > a.npre ? a.npre : c);
}

// value q of the stream the AudioSink sees (after gain and volume); q < 0: audioFilter1's delay line
__device__ __forceinline__ float v_at(const DemodLaunch &a, long long q) {
    if (q < 0) return a.st[ST_A1 + a.T1 - 1 + q];
    float x = a.pre[q];
    if (a.agc) {
        long long p = (fidx(a, q) + a.skip) / a.ps;
        if (p > a.K - 1) p = a.K - 1;
        if (a.kind == kKindAm) x = (x - a.pk_avg[p]) * a.pk_gain[p];
        else x = x * a.pk_gain[p];
    }
    return x * a.volume;
}

// newest audioFilter1 input (call-relative) of its output r of this call
__device__ __forceinline__ long long c1_of(const DemodLaunch &a, long long r) {
    return (a.a1_out0 + r) * kA1Dec + (kA1Dec - 1) - a.a1_in0;
}

// audioFilter1 output r of this call; r < 0: audioFilter2's delay line
__device__ float y1_at(const DemodLaunch &a, long long r) {
    if (r < 0) return a.st[ST_A2 + a.T2 - 1 + r];
    const long long c = c1_of(a, r);
    float s = 0.0f;
    for (int k = 0; k < a.T1; k++) s = s + a.taps[TP_A1 + k] * v_at(a, c - k);
    return s;
}

// ---------------------------------------------------------------- kernel 1

constexpr int kFlMax = (kTile - 1) * 2 + kMaxBandTaps;   // user-filtered run of a tile (decimation <= 2)
constexpr int kInMax = kFlMax + kMaxUserTaps;

// The bodies of the four kernels are .inc files included as text, shared by the single
// handle's kernels and the bank's (the slot in blockIdx.y).

__global__ __launch_bounds__(kTile) void demod_stage1_kernel(DemodLaunch a) {
#define DEMOD_TILE blockIdx.x
#include "demod_stage1_tile.inc"
#undef DEMOD_TILE
}

// Bank kernels: the slot's record comes from a device array, read once before any
// store (so it stays in SGPRs); the body is the single kernel's.
__global__ __launch_bounds__(kTile) void demod_bank_stage1_kernel(const DemodLaunch *__restrict__ recs) {
    const DemodLaunch a = recs[blockIdx.y];
    // uniform over the block (a and blockIdx only): no lane is left at a barrier
    if (a.kind == kKindOff || (long long)blockIdx.x * kTile >= a.npre) return;
#define DEMOD_TILE blockIdx.x
#include "demod_stage1_tile.inc"
#undef DEMOD_TILE
}

// ---------------------------------------------------------------- kernel 2: per-packet maximum and sum


__global__ __launch_bounds__(64) void demod_packet_kernel(DemodLaunch a) {
#define DEMOD_TILE blockIdx.x
#include "demod_packet_wave.inc"
#undef DEMOD_TILE
}

__global__ __launch_bounds__(64) void demod_bank_packet_kernel(const DemodLaunch *__restrict__ recs) {
    const DemodLaunch a = recs[blockIdx.y];
    // uniform over the block: slots that are off or without AGC (the FM kinds), packets past the slot's
    if (a.kind == kKindOff || !a.agc || (long long)blockIdx.x >= a.K) return;
#define DEMOD_TILE blockIdx.x
#include "demod_packet_wave.inc"
#undef DEMOD_TILE
}

// ---------------------------------------------------------------- kernel 3: state for the next call


__global__ __launch_bounds__(kTile) void demod_state_kernel(DemodLaunch a) {
#include "demod_state_block.inc"
}

__global__ __launch_bounds__(kTile) void demod_bank_state_kernel(const DemodLaunch *__restrict__ recs) {
    const DemodLaunch a = recs[blockIdx.x];
    if (a.kind == kKindOff) return;                       // uniform over the block; the slot's state stays
#include "demod_state_block.inc"
}

// ---------------------------------------------------------------- kernel 4: gain, volume, audio FIRs

constexpr int kY1Max = (kTile - 1) * kA2Dec + kMaxAudioTaps;
constexpr int kVMax = (kY1Max - 1) * kA1Dec + kMaxAudioTaps;


__global__ __launch_bounds__(kTile) void demod_audio_kernel(DemodLaunch a) {
#define DEMOD_TILE blockIdx.x
#include "demod_audio_tile.inc"
#undef DEMOD_TILE
}

__global__ __launch_bounds__(kTile) void demod_bank_audio_kernel(const DemodLaunch *__restrict__ recs) {
    const DemodLaunch a = recs[blockIdx.y];
    // uniform over the block (a and blockIdx only): no lane is left at a barrier
    if (a.kind == kKindOff || (long long)blockIdx.x * kTile >= a.n_audio) return;
#define DEMOD_TILE blockIdx.x
#include "demod_audio_tile.inc"
#undef DEMOD_TILE
}

// ---------------------------------------------------------------- host design

// Java/Kotlin (int) of a double: truncation, saturation, NaN -> 0.
int32_t jtoint(double x) {
    if (x != x) return 0;
    if (x >= 2147483647.0) return INT32_MAX;
    if (x <= -2147483648.0) return INT32_MIN;
    return (int32_t)x;
}

// Blackman window as both filter classes compute it (WindowFunctions.kt:44-49,
// ComplexFirFilter.java:270-278): cosines in double, cast, float arithmetic.
float blackman(int n, int N) {
    const float c1 = (float)std::cos(2.0 * M_PI * n / (N - 1));
    const float c2 = (float)std::cos(4.0 * M_PI * n / (N - 1));
    return 0.42f - 0.5f * c1 + 0.08f * c2;
}

// The windowed-sinc low-pass prototype both designs share (FirFilter.kt:160-195,
// ComplexFirFilter.java:224-246), normalised to `gain` at zero frequency.
void low_pass_prototype(float gain, float fs, float fc, int ntaps, std::vector<float> &taps) {
    taps.assign(ntaps, 0.0f);
    const float pi = (float)M_PI;
    const int M = (ntaps - 1) / 2;
    const float fwT0 = 2 * pi * fc / fs;
    for (int n = -M; n <= M; n++) {
        const float w = blackman(n + M, ntaps);
        if (n == 0) taps[n + M] = fwT0 / pi * w;
        else taps[n + M] = (float)std::sin((double)((float)n * fwT0)) / ((float)n * pi) * w;
    }
    float fmx = taps[M];
    for (int n = 1; n <= M; n++) fmx += 2 * taps[n + M];
    const float g = gain / fmx;
    for (float &t : taps) t *= g;
}

// FirFilter.createLowPassTaps (FirFilter.kt:182-195, Blackman, no tap limit).
bool design_low_pass(float gain, float fs, float fc, float tw, float att, std::vector<float> &taps) {
    if (fs <= 0.0f || fc <= 0.0f || fc > fs / 2 || tw <= 0.0f) return false;
    int ntaps = jtoint((double)(att * fs) / (22.0 * (double)tw));
    if ((ntaps & 1) == 0) ntaps++;
    if (ntaps <= 0 || ntaps > (1 << 20)) return false;
    low_pass_prototype(gain, fs, fc, ntaps, taps);
    return true;
}

// ComplexFirFilter.createBandPass (ComplexFirFilter.java:186-262).
bool design_band_pass(float gain, float fs, float lo, float hi, float tw, float att, std::vector<float> &re,
                      std::vector<float> &im) {
    if (!(fs > 0.0f)) return false;
    if ((double)lo < (double)fs * -0.5 || (double)hi > (double)fs * 0.5) return false;
    if (!(lo < hi)) return false;
    if (!(tw > 0.0f)) return false;
    int ntaps = jtoint((double)(att * fs) / (22.0 * (double)tw));
    if ((ntaps & 1) == 0) ntaps++;
    if (ntaps <= 0 || ntaps > (1 << 20)) return false;
    std::vector<float> lp;
    low_pass_prototype(gain, fs, (hi - lo) / 2.0f, ntaps, lp);
    re.assign(ntaps, 0.0f);
    im.assign(ntaps, 0.0f);
    const float freq = (float)M_PI * (hi + lo) / fs;
    float phase = -freq * (float)(ntaps / 2);
    for (int i = 0; i < ntaps; i++) {
        re[i] = lp[i] * (float)std::cos((double)phase);
        im[i] = lp[i] * (float)std::sin((double)phase);
        phase += freq;
    }
    return true;
}

struct ModeInfo {
    int32_t rate, min_w, max_w, def_w;
};

// DemodulationMode's widths and Demodulator.kt:52-61.
const ModeInfo kModes[7] = {
    {2 * kAudioRate, 0, 50000, 0},             // OFF (the rate is a dummy)
    {2 * kAudioRate, 3000, 15000, 8000},       // AM
    {2 * kAudioRate, 3000, 15000, 10000},      // NFM
    {8 * kAudioRate, 30000, 150000, 100000},   // WFM
    {2 * kAudioRate, 1500, 5000, 2800},        // LSB
    {2 * kAudioRate, 1500, 5000, 2800},        // USB
    {1 * kAudioRate, 150, 800, 300},           // CW
};
constexpr int kCwOffset = 750;                 // Demodulator.kt:67

bool mode_ok(int mode) { return mode >= RFA_DEMOD_OFF && mode <= RFA_DEMOD_CW; }

long long fir_off(int D) { return D >= 2 ? D - 1 : 1; }

// outputs of a FirFilter once in_total inputs went in since it was built
long long fir_outputs(int D, long long in_total) {
    const long long lim = in_total - fir_off(D);
    return lim > 0 ? (lim + D - 1) / D : 0;
}

// One Demodulator + AudioSink as the host sees it: settings, designed taps and the
// filters' counters.  An rfa_demod is one of these with its device memory; a bank slot
// is one of these inside an rfa_demod_bank.  The plan, the staleness rules, the designs
// and the launch record below work on this part alone, so both run the same code.
struct DemodSlot {
    int mode = RFA_DEMOD_OFF;
    int32_t width = 0;
    float volume = 1.0f;
    bool sink_enabled = true;
    // userFilter (Demodulator.kt:73,215-240)
    bool uf_valid = false;
    std::vector<float> uf_taps;
    float uf_cutoff = 0.0f;
    long long uf_in = 0;
    // bandPassFilter, shared by SSB and CW (Demodulator.kt:87)
    bool bp_valid = false;
    std::vector<float> bp_re, bp_im;
    float bp_lo = 0.0f, bp_hi = 0.0f;
    int bp_dec = 1;
    long long bp_in = 0, bp_out = 0;
    // AudioSink.audioFilter1 / audioFilter2
    std::vector<float> a1_taps, a2_taps;
    long long a1_in = 0, a1_out = 0, a2_in = 0, a2_out = 0;
};

}  // namespace

struct rfa_demod : DemodSlot, StageCore {
    // device
    float *d_state[2] = {nullptr, nullptr};
    int cur = 0;
    float *d_taps = nullptr;
    float *d_pre = nullptr;
    size_t pre_cap = 0;
    float *d_pk = nullptr;         // [max K | avg K | gain K]
    size_t pk_cap = 0;
    float *d_in = nullptr, *d_out = nullptr;   // staging of the _host entry
    size_t d_in_cap = 0, d_out_cap = 0;
};

namespace {

// Demodulator.kt:217: userFilter == null || cutOffFrequency.toInt() != channelWidth
bool uf_stale(const DemodSlot *d) { return !d->uf_valid || jtoint((double)d->uf_cutoff) != d->width; }

// Demodulator.kt:321-322 (SSB) and :370 (CW), literally
bool bp_stale(const DemodSlot *d) {
    if (!d->bp_valid) return true;
    if (d->mode == RFA_DEMOD_USB) return jtoint((double)d->bp_hi) != d->width;
    if (d->mode == RFA_DEMOD_LSB) return jtoint((double)d->bp_lo) != -d->width;
    return jtoint((double)d->bp_hi) != kCwOffset + d->width / 2;
}

bool is_band(int mode) { return mode == RFA_DEMOD_LSB || mode == RFA_DEMOD_USB || mode == RFA_DEMOD_CW; }

// What one call does, from the host's counters alone.
struct Plan {
    bool uf_fresh = false, bp_fresh = false;
    int kind = kKindAm, Db = 1, sink = 0;
    long long K = 1, ps = 1, skip = 0, F = 0;
    long long bp_in0 = 0, bp_out0 = 0, npre = 0, ny1 = 0, n_audio = 0;
};

void make_plan(const DemodSlot *d, long long n, long long packet, Plan &p) {
    p.ps = packet > 0 ? packet : std::max(1LL, n);
    p.K = std::max(1LL, (n + p.ps - 1) / p.ps);
    p.uf_fresh = uf_stale(d);
    const long long uf_in = p.uf_fresh ? 0 : d->uf_in;
    p.skip = (uf_in == 0 && n > 0) ? 1 : 0;
    p.F = n - p.skip;
    int rate = kModes[d->mode].rate;
    if (is_band(d->mode)) {
        p.kind = kKindBand;
        p.bp_fresh = bp_stale(d);
        p.Db = p.bp_fresh ? (d->mode == RFA_DEMOD_CW ? 1 : 2) : d->bp_dec;
        p.bp_in0 = p.bp_fresh ? 0 : d->bp_in;
        p.bp_out0 = p.bp_fresh ? 0 : d->bp_out;
        p.npre = fir_outputs(p.Db, p.bp_in0 + p.F) - p.bp_out0;
        rate /= p.Db;
    } else {
        p.kind = d->mode == RFA_DEMOD_AM ? kKindAm : kKindFm;
        p.npre = p.F;
    }
    // AudioSink.java:182,217,229: by the packet's sample rate
    const int ratio = rate / kAudioRate;
    p.sink = !d->sink_enabled ? 0 : (ratio == 8 ? 2 : (ratio == 2 ? 1 : 0));
    p.n_audio = p.npre;
    if (p.sink >= 1) p.ny1 = p.n_audio = fir_outputs(kA1Dec, d->a1_in + p.npre) - d->a1_out;
    if (p.sink == 2) p.n_audio = fir_outputs(kA2Dec, d->a2_in + p.ny1) - d->a2_out;
}

int upload_taps(rfa_demod *d, int at, const std::vector<float> &t) {
    STAGE_HIP(d, hipMemcpyAsync(d->d_taps + at, t.data(), t.size() * sizeof(float), hipMemcpyHostToDevice, d->stream));
    STAGE_HIP(d, hipStreamSynchronize(d->stream));
    return RFA_OK;
}

// The filters a call finds stale, designed on the host; nothing of the slot changes until
// commit_design.  `why` names the rejection.
struct Design {
    bool uf = false, bp = false;
    std::vector<float> uf_taps, bp_re, bp_im;
    float bp_lo = 0.0f, bp_hi = 0.0f;
    int bp_dec = 2;
};

int design_user_filter(const DemodSlot *d, Design &g, const char *&why) {
    const float rate = (float)kModes[d->mode].rate;
    // createLowPass(1, 1f, rate, width, rate * 0.10f, 60) (Demodulator.kt:219-226)
    if (!design_low_pass(1.0f, rate, (float)d->width, rate * 0.10f, 60.0f, g.uf_taps)) {
        why = "user filter design rejected the width (createLowPass returns null)";
        return RFA_ERR_INVALID;
    }
    if (g.uf_taps.size() > (size_t)kMaxUserTaps) {
        why = "user filter longer than the kernel's limit";
        return RFA_ERR_UNSUPPORTED;
    }
    g.uf = true;
    return RFA_OK;
}

int design_band_pass_filter(const DemodSlot *d, Design &g, const char *&why) {
    const float rate = (float)kModes[d->mode].rate, w = (float)d->width;
    float lo, hi;
    int dec = 2;
    if (d->mode == RFA_DEMOD_USB) lo = 200.0f, hi = w;                 // Demodulator.kt:325-333
    else if (d->mode == RFA_DEMOD_LSB) lo = -w, hi = -200.0f;
    else lo = (float)kCwOffset - w / 2.0f, hi = (float)kCwOffset + w / 2.0f, dec = 1;   // :372-380
    if (!design_band_pass(1.0f, rate, lo, hi, rate * 0.01f, 40.0f, g.bp_re, g.bp_im)) {
        why = "band-pass design rejected the width (createBandPass returns null)";
        return RFA_ERR_INVALID;
    }
    if (g.bp_re.size() > (size_t)kMaxBandTaps) {
        why = "band-pass filter longer than the kernel's limit";
        return RFA_ERR_UNSUPPORTED;
    }
    g.bp_lo = lo;
    g.bp_hi = hi;
    g.bp_dec = dec;
    g.bp = true;
    return RFA_OK;
}

void commit_user_filter(DemodSlot *d, Design &g) {
    d->uf_taps = g.uf_taps;
    d->uf_cutoff = (float)d->width;
    d->uf_in = 0;
    d->uf_valid = true;
}

void commit_band_pass(DemodSlot *d, Design &g) {
    d->bp_re = g.bp_re;
    d->bp_im = g.bp_im;
    d->bp_lo = g.bp_lo;
    d->bp_hi = g.bp_hi;
    d->bp_dec = g.bp_dec;
    d->bp_in = d->bp_out = 0;
    d->bp_valid = true;
}

int rebuild_user_filter(rfa_demod *d) {
    Design g;
    const char *why = "";
    const int st = design_user_filter(d, g, why);
    if (st != RFA_OK) return stage_fail(d, st, why);
    STAGE_HIP(d, hipMemsetAsync(d->d_state[d->cur] + ST_UF_RE, 0, 2 * kMaxUserTaps * sizeof(float), d->stream));
    const int rc = upload_taps(d, TP_UF, g.uf_taps);
    if (rc != RFA_OK) return rc;
    commit_user_filter(d, g);
    return RFA_OK;
}

int rebuild_band_pass(rfa_demod *d) {
    Design g;
    const char *why = "";
    const int st = design_band_pass_filter(d, g, why);
    if (st != RFA_OK) return stage_fail(d, st, why);
    STAGE_HIP(d, hipMemsetAsync(d->d_state[d->cur] + ST_BP_RE, 0, 2 * kMaxBandTaps * sizeof(float), d->stream));
    int rc = upload_taps(d, TP_BPR, g.bp_re);
    if (rc == RFA_OK) rc = upload_taps(d, TP_BPI, g.bp_im);
    if (rc != RFA_OK) return rc;
    commit_band_pass(d, g);
    return RFA_OK;
}

// The launch record of one call from the slot and its plan: everything but the addresses.
void fill_launch(const DemodSlot *d, const Plan &p, long long n_samples, DemodLaunch &a) {
    a.n = n_samples;
    a.ps = p.ps;
    a.K = p.K;
    a.kind = p.kind;
    a.Tu = (int)d->uf_taps.size();
    a.Tb = p.kind == kKindBand ? (int)d->bp_re.size() : 1;
    a.T1 = (int)d->a1_taps.size();
    a.T2 = (int)d->a2_taps.size();
    a.Db = p.Db;
    a.offb = p.kind == kKindBand ? (int)fir_off(p.Db) : 0;
    a.skip = (int)p.skip;
    a.F = p.F;
    a.bp_in0 = p.bp_in0;
    a.bp_out0 = p.bp_out0;
    a.npre = p.npre;
    if (p.kind == kKindFm) {
        // quadratureRate / (2 * PI * maxDeviation).toFloat() (Demodulator.kt:176-177,257)
        const float dev = (float)d->width * (d->mode == RFA_DEMOD_NFM ? 0.75f : 0.85f);
        a.qgain = (float)kModes[d->mode].rate / (float)(2 * M_PI * (double)dev);
    }
    a.volume = d->volume;
    a.agc = p.kind != kKindFm;
    a.sink = p.sink;
    a.a1_in0 = d->a1_in;
    a.a1_out0 = d->a1_out;
    a.ny1 = p.ny1;
    a.a2_in0 = d->a2_in;
    a.a2_out0 = d->a2_out;
    a.n_audio = p.n_audio;
}

// The counters after a call that was enqueued.
void advance(DemodSlot *d, const Plan &p, long long n_samples) {
    d->uf_in += n_samples;
    if (p.kind == kKindBand) {
        d->bp_in += p.F;
        d->bp_out += p.npre;
    }
    if (p.sink >= 1) {
        d->a1_in += p.npre;
        d->a1_out += p.ny1;
    }
    if (p.sink == 2) {
        d->a2_in += p.ny1;
        d->a2_out += p.n_audio;
    }
}

void forget_filters(DemodSlot *d) {
    d->uf_valid = d->bp_valid = false;
    d->uf_in = d->bp_in = d->bp_out = 0;
    d->a1_in = d->a1_out = d->a2_in = d->a2_out = 0;
}

// AudioSink.java:94-96: createLowPass(decimation 2 / 4, gain 1, rate 1, cut-off, transition, 30 dB)
bool design_audio_filters(std::vector<float> &t1, std::vector<float> &t2) {
    return design_low_pass(1.0f, 1.0f, 0.1f, 0.15f, 30.0f, t1) && design_low_pass(1.0f, 1.0f, 0.1f, 0.1f, 30.0f, t2) &&
           t1.size() <= (size_t)kMaxAudioTaps && t2.size() <= (size_t)kMaxAudioTaps;
}

void slot_set_mode(DemodSlot *d, int mode) {
    d->mode = mode;                       // Demodulator.kt:96-100
    d->width = kModes[mode].def_w;
}

void slot_set_width(DemodSlot *d, int32_t w) {
    const ModeInfo &m = kModes[d->mode];  // Demodulator.kt:75
    d->width = std::min(std::max(w, m.min_w), m.max_w);
}

int slot_get_taps(const DemodSlot *d, int which, float *re, float *im, size_t capacity, int32_t *num_taps,
                  int32_t *decimation) {
    static const std::vector<float> none;
    const std::vector<float> *r = &none, *i = nullptr;
    int dec = 1;
    switch (which) {
    case RFA_DEMOD_TAPS_USER:
        if (d->uf_valid) r = &d->uf_taps;
        break;
    case RFA_DEMOD_TAPS_BANDPASS:
        if (d->bp_valid) r = &d->bp_re, i = &d->bp_im, dec = d->bp_dec;
        break;
    case RFA_DEMOD_TAPS_AUDIO1: r = &d->a1_taps, dec = kA1Dec; break;
    case RFA_DEMOD_TAPS_AUDIO2: r = &d->a2_taps, dec = kA2Dec; break;
    default: return RFA_ERR_INVALID;
    }
    if (num_taps) *num_taps = (int32_t)r->size();
    if (decimation) *decimation = dec;
    if (re || im) {
        if (capacity < r->size()) return RFA_ERR_SIZE;
        if (re) std::memcpy(re, r->data(), r->size() * sizeof(float));
        if (im) {
            if (i) std::memcpy(im, i->data(), i->size() * sizeof(float));
            else std::memset(im, 0, r->size() * sizeof(float));
        }
    }
    return RFA_OK;
}

// A freshly created Demodulator + AudioSink: no user or band-pass filter, zero
// carry-over and lastMax, audio filters with empty delay lines.
int fresh_state(rfa_demod *d) {
    STAGE_HIP(d, hipMemsetAsync(d->d_state[d->cur], 0, ST_SIZE * sizeof(float), d->stream));
    forget_filters(d);
    return RFA_OK;
}

}  // namespace

extern "C" {

int rfa_demod_mode_info(int mode, int32_t *quadrature_rate, int32_t *min_width, int32_t *max_width,
                        int32_t *default_width) {
    if (!mode_ok(mode)) return RFA_ERR_INVALID;
    const ModeInfo &m = kModes[mode];
    if (quadrature_rate) *quadrature_rate = m.rate;
    if (min_width) *min_width = m.min_w;
    if (max_width) *max_width = m.max_w;
    if (default_width) *default_width = m.def_w;
    return RFA_OK;
}

int rfa_bandpass_taps(float gain, float fs, float lo, float hi, float transition, float attenuation, float *re,
                      float *im, size_t capacity, int32_t *num_taps) {
    if (!num_taps) return RFA_ERR_INVALID;
    *num_taps = 0;
    std::vector<float> r, i;
    if (!design_band_pass(gain, fs, lo, hi, transition, attenuation, r, i)) return RFA_ERR_INVALID;
    *num_taps = (int32_t)r.size();
    if (re || im) {
        if (capacity < r.size()) return RFA_ERR_SIZE;
        if (re) std::memcpy(re, r.data(), r.size() * sizeof(float));
        if (im) std::memcpy(im, i.data(), i.size() * sizeof(float));
    }
    return RFA_OK;
}

int rfa_demod_create(int device, int mode, rfa_demod **out) {
    if (!out) return RFA_ERR_INVALID;
    *out = nullptr;
    if (!mode_ok(mode)) return RFA_ERR_INVALID;
    int rc = stage_check_device(device);
    if (rc != RFA_OK) return rc;
    rfa_demod *d = new (std::nothrow) rfa_demod();
    if (!d) return RFA_ERR_NOMEM;
    d->device = device;
    d->mode = mode;
    d->width = kModes[mode].def_w;
    std::vector<float> t1, t2;
    if (!design_audio_filters(t1, t2)) rc = RFA_ERR_INVALID;
    if (rc == RFA_OK) rc = stage_open(d, device);
    if (rc == RFA_OK) {
        if (hipMalloc(&d->d_state[0], ST_SIZE * sizeof(float)) != hipSuccess ||
            hipMalloc(&d->d_state[1], ST_SIZE * sizeof(float)) != hipSuccess ||
            hipMalloc(&d->d_taps, TP_SIZE * sizeof(float)) != hipSuccess)
            rc = RFA_ERR_NOMEM;
    }
    if (rc == RFA_OK && (hipMemsetAsync(d->d_taps, 0, TP_SIZE * sizeof(float), d->stream) != hipSuccess ||
                         hipMemsetAsync(d->d_state[1], 0, ST_SIZE * sizeof(float), d->stream) != hipSuccess))
        rc = RFA_ERR_HIP;
    if (rc == RFA_OK) rc = fresh_state(d);
    if (rc == RFA_OK) rc = upload_taps(d, TP_A1, t1);
    if (rc == RFA_OK) rc = upload_taps(d, TP_A2, t2);
    if (rc != RFA_OK) {
        rfa_demod_destroy(d);
        return rc;
    }
    d->a1_taps = std::move(t1);
    d->a2_taps = std::move(t2);
    *out = d;
    return RFA_OK;
}

int rfa_demod_destroy(rfa_demod *d) {
    if (!d) return RFA_ERR_INVALID;
    stage_close_stream(d);
    for (float *p : {d->d_state[0], d->d_state[1], d->d_taps, d->d_pre, d->d_pk, d->d_in, d->d_out})
        if (p) (void)hipFree(p);
    delete d;
    return RFA_OK;
}

const char *rfa_demod_last_error(const rfa_demod *d) { return stage_last_error(d); }

int rfa_demod_set_mode(rfa_demod *d, int mode) {
    if (!d) return RFA_ERR_INVALID;
    if (!mode_ok(mode)) return stage_fail(d, RFA_ERR_INVALID, "no such demodulation mode");
    slot_set_mode(d, mode);
    return RFA_OK;
}

int rfa_demod_get_mode(const rfa_demod *d, int32_t *mode) {
    if (!d || !mode) return RFA_ERR_INVALID;
    *mode = d->mode;
    return RFA_OK;
}

int rfa_demod_set_channel_width(rfa_demod *d, int32_t w) {
    if (!d) return RFA_ERR_INVALID;
    slot_set_width(d, w);
    return RFA_OK;
}

int rfa_demod_get_channel_width(const rfa_demod *d, int32_t *w) {
    if (!d || !w) return RFA_ERR_INVALID;
    *w = d->width;
    return RFA_OK;
}

int rfa_demod_set_volume(rfa_demod *d, float v) {
    if (!d) return RFA_ERR_INVALID;
    d->volume = v;
    return RFA_OK;
}

int rfa_demod_set_audio_sink(rfa_demod *d, int enable) {
    if (!d) return RFA_ERR_INVALID;
    d->sink_enabled = enable != 0;
    return RFA_OK;
}

int rfa_demod_max_outputs(const rfa_demod *d, size_t n_samples, size_t *n) {
    if (!d || !n) return RFA_ERR_INVALID;
    *n = 0;
    if (d->mode == RFA_DEMOD_OFF) return RFA_OK;
    if (n_samples > (size_t)1 << 36) return RFA_ERR_INVALID;
    Plan p;
    make_plan(d, (long long)n_samples, 0, p);
    *n = (size_t)p.n_audio;
    return RFA_OK;
}

int rfa_demod_process(rfa_demod *d, const float *re, const float *im, size_t n_samples, size_t packet_samples,
                      float *audio, size_t capacity, size_t *n_audio) {
    if (!d || !n_audio) return RFA_ERR_INVALID;
    *n_audio = 0;
    if (d->mode == RFA_DEMOD_OFF) return RFA_OK;          // Demodulator.kt:174: no output, nothing moves
    if (n_samples > (size_t)1 << 36 || packet_samples > (size_t)1 << 36)
        return stage_fail(d, RFA_ERR_INVALID, "n_samples too large");
    if (n_samples && (!re || !im)) return stage_fail(d, RFA_ERR_INVALID, "null input");
    Plan p;
    make_plan(d, (long long)n_samples, (long long)packet_samples, p);
    if ((size_t)p.n_audio > capacity) return stage_fail(d, RFA_ERR_SIZE, "audio capacity too small");
    if (p.n_audio > 0 && !audio) return stage_fail(d, RFA_ERR_INVALID, "null output");
    if (p.K > (long long)INT32_MAX || (p.npre + kTile - 1) / kTile > (long long)INT32_MAX)
        return stage_fail(d, RFA_ERR_INVALID, "call too large for one grid");
    STAGE_HIP(d, hipSetDevice(d->device));
    int rc = stage_grow(d, d->d_pre, d->pre_cap, (size_t)p.npre, "scratch");
    if (rc == RFA_OK) rc = stage_grow(d, d->d_pk, d->pk_cap, 3 * (size_t)p.K, "packet scratch");
    if (rc == RFA_OK && p.uf_fresh) rc = rebuild_user_filter(d);
    if (rc == RFA_OK && p.bp_fresh) rc = rebuild_band_pass(d);
    if (rc != RFA_OK) return rc;

    DemodLaunch a{};
    fill_launch(d, p, (long long)n_samples, a);
    a.re = re;
    a.im = im;
    a.st = d->d_state[d->cur];
    a.nst = d->d_state[d->cur ^ 1];
    a.taps = d->d_taps;
    a.pre = d->d_pre;
    a.pk_max = d->d_pk;
    a.pk_avg = d->d_pk + p.K;
    a.pk_gain = d->d_pk + 2 * p.K;
    a.out = audio;

    if (p.npre > 0) {
        hipLaunchKernelGGL(demod_stage1_kernel, dim3((unsigned)((p.npre + kTile - 1) / kTile)), dim3(kTile), 0,
                           d->stream, a);
        STAGE_HIP(d, hipGetLastError());
    }
    if (a.agc) {
        hipLaunchKernelGGL(demod_packet_kernel, dim3((unsigned)p.K), dim3(64), 0, d->stream, a);
        STAGE_HIP(d, hipGetLastError());
    }
    hipLaunchKernelGGL(demod_state_kernel, dim3(1), dim3(kTile), 0, d->stream, a);
    STAGE_HIP(d, hipGetLastError());
    if (p.n_audio > 0) {
        hipLaunchKernelGGL(demod_audio_kernel, dim3((unsigned)((p.n_audio + kTile - 1) / kTile)), dim3(kTile), 0,
                           d->stream, a);
        STAGE_HIP(d, hipGetLastError());
    }
    d->cur ^= 1;
    advance(d, p, (long long)n_samples);
    *n_audio = (size_t)p.n_audio;
    return RFA_OK;
}

int rfa_demod_process_host(rfa_demod *d, const float *re, const float *im, size_t n_samples, size_t packet_samples,
                           float *audio, size_t capacity, size_t *n_audio) {
    if (!d || !n_audio) return RFA_ERR_INVALID;
    *n_audio = 0;
    if (d->mode == RFA_DEMOD_OFF) return RFA_OK;
    if (n_samples > (size_t)1 << 36) return stage_fail(d, RFA_ERR_INVALID, "n_samples too large");
    if (n_samples && (!re || !im)) return stage_fail(d, RFA_ERR_INVALID, "null input");
    STAGE_HIP(d, hipSetDevice(d->device));
    Plan p;
    make_plan(d, (long long)n_samples, (long long)packet_samples, p);
    if ((size_t)p.n_audio > capacity) return stage_fail(d, RFA_ERR_SIZE, "audio capacity too small");
    int rc = stage_grow(d, d->d_in, d->d_in_cap, 2 * n_samples, "input staging");
    if (rc == RFA_OK) rc = stage_grow(d, d->d_out, d->d_out_cap, (size_t)p.n_audio, "output staging");
    if (rc != RFA_OK) return rc;
    if (n_samples) {
        STAGE_HIP(d, hipMemcpyAsync(d->d_in, re, n_samples * sizeof(float), hipMemcpyHostToDevice, d->stream));
        STAGE_HIP(d, hipMemcpyAsync(d->d_in + n_samples, im, n_samples * sizeof(float), hipMemcpyHostToDevice, d->stream));
    }
    size_t got = 0;
    rc = rfa_demod_process(d, d->d_in, d->d_in + n_samples, n_samples, packet_samples, d->d_out, d->d_out_cap, &got);
    if (rc != RFA_OK) return rc;
    if (got) STAGE_HIP(d, hipMemcpyAsync(audio, d->d_out, got * sizeof(float), hipMemcpyDeviceToHost, d->stream));
    STAGE_HIP(d, hipStreamSynchronize(d->stream));
    *n_audio = got;
    return RFA_OK;
}

int rfa_demod_get_taps(const rfa_demod *d, int which, float *re, float *im, size_t capacity, int32_t *num_taps,
                       int32_t *decimation) {
    if (!d) return RFA_ERR_INVALID;
    return slot_get_taps(d, which, re, im, capacity, num_taps, decimation);
}

int rfa_demod_get_state(rfa_demod *d, float *last_max, float *carry_re, float *carry_im) {
    if (!d) return RFA_ERR_INVALID;
    STAGE_HIP(d, hipSetDevice(d->device));
    float s[3] = {0.0f, 0.0f, 0.0f};
    STAGE_HIP(d, hipMemcpyAsync(s, d->d_state[d->cur] + ST_CARRY, sizeof s, hipMemcpyDeviceToHost, d->stream));
    STAGE_HIP(d, hipStreamSynchronize(d->stream));
    if (carry_re) *carry_re = s[0];
    if (carry_im) *carry_im = s[1];
    if (last_max) *last_max = s[2];
    return RFA_OK;
}

int rfa_demod_reset(rfa_demod *d) {
    if (!d) return RFA_ERR_INVALID;
    STAGE_HIP(d, hipSetDevice(d->device));
    return fresh_state(d);
}

int rfa_demod_set_stream(rfa_demod *d, void *stream) { return stage_set_stream(d, stream); }

int rfa_demod_get_stream(const rfa_demod *d, void **stream) { return stage_get_stream(d, stream); }

int rfa_demod_synchronize(rfa_demod *d) { return stage_synchronize(d); }

}  // extern "C"

// ================================================================ the demodulator bank
//
// K DemodSlots in one handle: one stream, one set of launches per call.  Slot k's state,
// taps and scratch are row k of a slab; a call fills one DemodLaunch per slot with the code
// the single handle uses (make_plan, fill_launch), copies the K records to the device and
// launches the four bank kernels over (tiles, K).
//
// The records of a call are staged in pinned host memory, in a ring of kRecRing entries of
// K records, each entry with an event recorded behind its copy.  A call waits for the
// event of the entry it is about to overwrite, so a queued copy never reads records of a
// later call; the device array is one, because copy and kernels are ordered on the stream.

constexpr int kRecRing = 8;

struct rfa_demod_bank : StageCore {
    int K = 0;
    std::vector<DemodSlot> slots;
    std::vector<int> cur;              // which copy of slot k's state is current
    std::vector<Plan> plans;           // per call, kept to allocate nothing in steady state
    float *d_state = nullptr;          // [K][2][ST_SIZE]
    float *d_taps = nullptr;           // [K][TP_SIZE]
    float *d_pre = nullptr;            // [K][pre_cap / K]
    size_t pre_cap = 0;
    float *d_pk = nullptr;             // [K][pk_cap / K]: max | avg | gain of the slot's packets
    size_t pk_cap = 0;
    DemodLaunch *d_recs = nullptr;     // [K]
    DemodLaunch *h_recs = nullptr;     // pinned, [kRecRing][K]
    hipEvent_t ev[kRecRing] = {};
    bool ev_used[kRecRing] = {};
    int ring_at = 0;
    float *d_in = nullptr, *d_out = nullptr;   // staging of the _host entry
    size_t d_in_cap = 0, d_out_cap = 0;
};

namespace {

float *bank_state(const rfa_demod_bank *b, int k, int which) {
    return b->d_state + ((size_t)k * 2 + (size_t)which) * ST_SIZE;
}

bool slot_ok(const rfa_demod_bank *b, int32_t k) { return k >= 0 && k < b->K; }

// What every slot that is not off would do with n samples.
void bank_plan(rfa_demod_bank *b, long long n, long long packet) {
    for (int k = 0; k < b->K; k++) {
        b->plans[k] = Plan{};
        if (b->slots[k].mode != RFA_DEMOD_OFF) make_plan(&b->slots[k], n, packet, b->plans[k]);
    }
}

// Every stale filter of the call: designed first (a rejection leaves all slots as they
// were), then the delay lines zeroed and the taps uploaded behind one synchronisation.
int bank_rebuild(rfa_demod_bank *b) {
    std::vector<std::pair<int, Design>> todo;
    for (int k = 0; k < b->K; k++) {
        const DemodSlot *s = &b->slots[k];
        const Plan &p = b->plans[k];
        if (s->mode == RFA_DEMOD_OFF || (!p.uf_fresh && !p.bp_fresh)) continue;
        todo.emplace_back(k, Design{});
        Design &g = todo.back().second;
        const char *why = "";
        int st = RFA_OK;
        if (p.uf_fresh) st = design_user_filter(s, g, why);
        if (st == RFA_OK && p.bp_fresh) st = design_band_pass_filter(s, g, why);
        if (st != RFA_OK) return stage_fail(b, st, "slot " + std::to_string(k) + ": " + why);
    }
    if (todo.empty()) return RFA_OK;
    for (auto &[k, g] : todo) {
        float *st = bank_state(b, k, b->cur[k]), *tp = b->d_taps + (size_t)k * TP_SIZE;
        if (g.uf) {
            STAGE_HIP(b, hipMemsetAsync(st + ST_UF_RE, 0, 2 * kMaxUserTaps * sizeof(float), b->stream));
            STAGE_HIP(b, hipMemcpyAsync(tp + TP_UF, g.uf_taps.data(), g.uf_taps.size() * sizeof(float),
                                   hipMemcpyHostToDevice, b->stream));
        }
        if (g.bp) {
            STAGE_HIP(b, hipMemsetAsync(st + ST_BP_RE, 0, 2 * kMaxBandTaps * sizeof(float), b->stream));
            STAGE_HIP(b, hipMemcpyAsync(tp + TP_BPR, g.bp_re.data(), g.bp_re.size() * sizeof(float), hipMemcpyHostToDevice,
                                   b->stream));
            STAGE_HIP(b, hipMemcpyAsync(tp + TP_BPI, g.bp_im.data(), g.bp_im.size() * sizeof(float), hipMemcpyHostToDevice,
                                   b->stream));
        }
    }
    STAGE_HIP(b, hipStreamSynchronize(b->stream));             // the designs' host copies are read by now
    for (auto &[k, g] : todo) {
        if (g.uf) commit_user_filter(&b->slots[k], g);
        if (g.bp) commit_band_pass(&b->slots[k], g);
    }
    return RFA_OK;
}

}  // namespace

extern "C" {

int rfa_demod_bank_create(int device, const int32_t *modes, int32_t n_channels, rfa_demod_bank **out) {
    if (!out) return RFA_ERR_INVALID;
    *out = nullptr;
    if (!modes || n_channels < 1 || n_channels > RFA_DEMOD_BANK_MAX_CHANNELS) return RFA_ERR_INVALID;
    for (int32_t k = 0; k < n_channels; k++)
        if (!mode_ok(modes[k])) return RFA_ERR_INVALID;
    int rc = stage_check_device(device);
    if (rc != RFA_OK) return rc;
    rfa_demod_bank *b = new (std::nothrow) rfa_demod_bank();
    if (!b) return RFA_ERR_NOMEM;
    const size_t K = (size_t)n_channels;
    b->device = device;
    b->K = n_channels;
    std::vector<float> t1, t2;
    if (!design_audio_filters(t1, t2)) rc = RFA_ERR_INVALID;
    b->slots.resize(K);
    b->cur.assign(K, 0);
    b->plans.resize(K);
    for (size_t k = 0; k < K; k++) {
        slot_set_mode(&b->slots[k], modes[k]);
        b->slots[k].a1_taps = t1;
        b->slots[k].a2_taps = t2;
    }
    if (rc == RFA_OK) rc = stage_open(b, device);
    if (rc == RFA_OK) {
        if (hipMalloc(&b->d_state, K * 2 * ST_SIZE * sizeof(float)) != hipSuccess ||
            hipMalloc(&b->d_taps, K * TP_SIZE * sizeof(float)) != hipSuccess ||
            hipMalloc(&b->d_recs, K * sizeof(DemodLaunch)) != hipSuccess ||
            hipHostMalloc(&b->h_recs, (size_t)kRecRing * K * sizeof(DemodLaunch), hipHostMallocDefault) != hipSuccess)
            rc = RFA_ERR_NOMEM;
    }
    for (int e = 0; rc == RFA_OK && e < kRecRing; e++)
        if (hipEventCreateWithFlags(&b->ev[e], hipEventDisableTiming) != hipSuccess) rc = RFA_ERR_HIP;
    // fresh Demodulators: zero state; the audio filters' taps in every slot's row
    std::vector<float> rows;
    if (rc == RFA_OK) {
        rows.assign(K * TP_SIZE, 0.0f);
        for (size_t k = 0; k < K; k++) {
            std::copy(t1.begin(), t1.end(), rows.begin() + k * TP_SIZE + TP_A1);
            std::copy(t2.begin(), t2.end(), rows.begin() + k * TP_SIZE + TP_A2);
        }
        if (hipMemsetAsync(b->d_state, 0, K * 2 * ST_SIZE * sizeof(float), b->stream) != hipSuccess ||
            hipMemcpyAsync(b->d_taps, rows.data(), rows.size() * sizeof(float), hipMemcpyHostToDevice, b->stream) !=
                hipSuccess ||
            hipStreamSynchronize(b->stream) != hipSuccess)
            rc = RFA_ERR_HIP;
    }
    if (rc != RFA_OK) {
        rfa_demod_bank_destroy(b);
        return rc;
    }
    *out = b;
    return RFA_OK;
}

int rfa_demod_bank_destroy(rfa_demod_bank *b) {
    if (!b) return RFA_ERR_INVALID;
    stage_close_stream(b);
    for (float *p : {b->d_state, b->d_taps, b->d_pre, b->d_pk, b->d_in, b->d_out})
        if (p) (void)hipFree(p);
    if (b->d_recs) (void)hipFree(b->d_recs);
    if (b->h_recs) (void)hipHostFree(b->h_recs);
    for (hipEvent_t e : b->ev)
        if (e) (void)hipEventDestroy(e);
    delete b;
    return RFA_OK;
}

const char *rfa_demod_bank_last_error(const rfa_demod_bank *b) { return stage_last_error(b); }

int rfa_demod_bank_get_channels(const rfa_demod_bank *b, int32_t *n_channels) {
    if (!b || !n_channels) return RFA_ERR_INVALID;
    *n_channels = b->K;
    return RFA_OK;
}

int rfa_demod_bank_set_mode(rfa_demod_bank *b, int32_t k, int mode) {
    if (!b) return RFA_ERR_INVALID;
    if (!slot_ok(b, k)) return stage_fail(b, RFA_ERR_INVALID, "no such slot");
    if (!mode_ok(mode)) return stage_fail(b, RFA_ERR_INVALID, "no such demodulation mode");
    slot_set_mode(&b->slots[k], mode);
    return RFA_OK;
}

int rfa_demod_bank_get_mode(const rfa_demod_bank *b, int32_t k, int32_t *mode) {
    if (!b || !mode || !slot_ok(b, k)) return RFA_ERR_INVALID;
    *mode = b->slots[k].mode;
    return RFA_OK;
}

int rfa_demod_bank_set_channel_width(rfa_demod_bank *b, int32_t k, int32_t w) {
    if (!b) return RFA_ERR_INVALID;
    if (!slot_ok(b, k)) return stage_fail(b, RFA_ERR_INVALID, "no such slot");
    slot_set_width(&b->slots[k], w);
    return RFA_OK;
}

int rfa_demod_bank_get_channel_width(const rfa_demod_bank *b, int32_t k, int32_t *w) {
    if (!b || !w || !slot_ok(b, k)) return RFA_ERR_INVALID;
    *w = b->slots[k].width;
    return RFA_OK;
}

int rfa_demod_bank_set_volume(rfa_demod_bank *b, int32_t k, float v) {
    if (!b) return RFA_ERR_INVALID;
    if (!slot_ok(b, k)) return stage_fail(b, RFA_ERR_INVALID, "no such slot");
    b->slots[k].volume = v;
    return RFA_OK;
}

int rfa_demod_bank_set_audio_sink(rfa_demod_bank *b, int32_t k, int enable) {
    if (!b) return RFA_ERR_INVALID;
    if (!slot_ok(b, k)) return stage_fail(b, RFA_ERR_INVALID, "no such slot");
    b->slots[k].sink_enabled = enable != 0;
    return RFA_OK;
}

int rfa_demod_bank_get_taps(const rfa_demod_bank *b, int32_t k, int which, float *re, float *im, size_t capacity,
                            int32_t *num_taps, int32_t *decimation) {
    if (!b || !slot_ok(b, k)) return RFA_ERR_INVALID;
    return slot_get_taps(&b->slots[k], which, re, im, capacity, num_taps, decimation);
}

int rfa_demod_bank_get_state(rfa_demod_bank *b, int32_t k, float *last_max, float *carry_re, float *carry_im) {
    if (!b) return RFA_ERR_INVALID;
    if (!slot_ok(b, k)) return stage_fail(b, RFA_ERR_INVALID, "no such slot");
    STAGE_HIP(b, hipSetDevice(b->device));
    float s[3] = {0.0f, 0.0f, 0.0f};
    STAGE_HIP(b, hipMemcpyAsync(s, bank_state(b, k, b->cur[k]) + ST_CARRY, sizeof s, hipMemcpyDeviceToHost, b->stream));
    STAGE_HIP(b, hipStreamSynchronize(b->stream));
    if (carry_re) *carry_re = s[0];
    if (carry_im) *carry_im = s[1];
    if (last_max) *last_max = s[2];
    return RFA_OK;
}

int rfa_demod_bank_reset(rfa_demod_bank *b, int32_t k) {
    if (!b) return RFA_ERR_INVALID;
    if (!slot_ok(b, k)) return stage_fail(b, RFA_ERR_INVALID, "no such slot");
    STAGE_HIP(b, hipSetDevice(b->device));
    STAGE_HIP(b, hipMemsetAsync(bank_state(b, k, b->cur[k]), 0, ST_SIZE * sizeof(float), b->stream));
    forget_filters(&b->slots[k]);
    return RFA_OK;
}

int rfa_demod_bank_max_outputs(const rfa_demod_bank *b, size_t n_samples, size_t *n) {
    if (!b || !n) return RFA_ERR_INVALID;
    for (int k = 0; k < b->K; k++) n[k] = 0;
    if (n_samples > (size_t)1 << 36) return RFA_ERR_INVALID;
    for (int k = 0; k < b->K; k++) {
        if (b->slots[k].mode == RFA_DEMOD_OFF) continue;
        Plan p;
        make_plan(&b->slots[k], (long long)n_samples, 0, p);
        n[k] = (size_t)p.n_audio;
    }
    return RFA_OK;
}

int rfa_demod_bank_process(rfa_demod_bank *b, const float *re, const float *im, size_t channel_stride,
                           size_t n_samples, size_t packet_samples, float *audio, size_t audio_stride,
                           size_t *n_audio) {
    if (!b || !n_audio) return RFA_ERR_INVALID;
    const int K = b->K;
    for (int k = 0; k < K; k++) n_audio[k] = 0;
    if (packet_samples > (size_t)1 << 36 || audio_stride > (size_t)1 << 40)
        return stage_fail(b, RFA_ERR_INVALID, "n_samples too large");
    int rc = stage_check_rows(b, (size_t)K, re, im, channel_stride, n_samples);
    if (rc != RFA_OK) return rc;
    bank_plan(b, (long long)n_samples, (long long)packet_samples);
    long long max_npre = 0, max_audio = 0, max_pk = 0;
    bool any_on = false, any_agc = false;
    for (int k = 0; k < K; k++) {
        if (b->slots[k].mode == RFA_DEMOD_OFF) continue;     // Demodulator.kt:174: no output, nothing moves
        const Plan &p = b->plans[k];
        any_on = true;
        any_agc = any_agc || p.kind != kKindFm;
        max_npre = std::max(max_npre, p.npre);
        max_audio = std::max(max_audio, p.n_audio);
        max_pk = std::max(max_pk, p.K);
    }
    if ((size_t)max_audio > audio_stride) return stage_fail(b, RFA_ERR_SIZE, "audio_stride too small for a slot");
    if (max_audio > 0 && !audio) return stage_fail(b, RFA_ERR_INVALID, "null output");
    if (max_pk > (long long)INT32_MAX || (max_npre + kTile - 1) / kTile > (long long)INT32_MAX)
        return stage_fail(b, RFA_ERR_INVALID, "call too large for one grid");
    if (!any_on) return RFA_OK;
    STAGE_HIP(b, hipSetDevice(b->device));
    rc = stage_grow(b, b->d_pre, b->pre_cap, (size_t)K * (size_t)max_npre, "scratch");
    if (rc == RFA_OK) rc = stage_grow(b, b->d_pk, b->pk_cap, (size_t)K * 3 * (size_t)max_pk, "packet scratch");
    if (rc == RFA_OK) rc = bank_rebuild(b);
    if (rc != RFA_OK) return rc;

    // this call's records: wait until the ring entry's previous copy has been made
    const int e = b->ring_at;
    if (b->ev_used[e]) STAGE_HIP(b, hipEventSynchronize(b->ev[e]));
    DemodLaunch *recs = b->h_recs + (size_t)e * (size_t)K;
    const size_t pre_row = b->pre_cap / (size_t)K, pk_row = b->pk_cap / (size_t)K;
    for (int k = 0; k < K; k++) {
        DemodLaunch a{};
        a.kind = kKindOff;
        if (b->slots[k].mode != RFA_DEMOD_OFF) {
            const Plan &p = b->plans[k];
            fill_launch(&b->slots[k], p, (long long)n_samples, a);
            a.re = re + (size_t)k * channel_stride;
            a.im = im + (size_t)k * channel_stride;
            a.st = bank_state(b, k, b->cur[k]);
            a.nst = bank_state(b, k, b->cur[k] ^ 1);
            a.taps = b->d_taps + (size_t)k * TP_SIZE;
            a.pre = b->d_pre + (size_t)k * pre_row;
            a.pk_max = b->d_pk + (size_t)k * pk_row;
            a.pk_avg = a.pk_max + p.K;
            a.pk_gain = a.pk_max + 2 * p.K;
            a.out = audio + (size_t)k * audio_stride;
        }
        recs[k] = a;
    }
    STAGE_HIP(b, hipMemcpyAsync(b->d_recs, recs, (size_t)K * sizeof(DemodLaunch), hipMemcpyHostToDevice, b->stream));
    STAGE_HIP(b, hipEventRecord(b->ev[e], b->stream));
    b->ev_used[e] = true;
    b->ring_at = (e + 1) % kRecRing;

    if (max_npre > 0) {
        hipLaunchKernelGGL(demod_bank_stage1_kernel, dim3((unsigned)((max_npre + kTile - 1) / kTile), (unsigned)K),
                           dim3(kTile), 0, b->stream, b->d_recs);
        STAGE_HIP(b, hipGetLastError());
    }
    if (any_agc) {
        hipLaunchKernelGGL(demod_bank_packet_kernel, dim3((unsigned)max_pk, (unsigned)K), dim3(64), 0, b->stream,
                           b->d_recs);
        STAGE_HIP(b, hipGetLastError());
    }
    hipLaunchKernelGGL(demod_bank_state_kernel, dim3((unsigned)K), dim3(kTile), 0, b->stream, b->d_recs);
    STAGE_HIP(b, hipGetLastError());
    if (max_audio > 0) {
        hipLaunchKernelGGL(demod_bank_audio_kernel, dim3((unsigned)((max_audio + kTile - 1) / kTile), (unsigned)K),
                           dim3(kTile), 0, b->stream, b->d_recs);
        STAGE_HIP(b, hipGetLastError());
    }
    for (int k = 0; k < K; k++) {
        if (b->slots[k].mode == RFA_DEMOD_OFF) continue;
        b->cur[k] ^= 1;
        advance(&b->slots[k], b->plans[k], (long long)n_samples);
        n_audio[k] = (size_t)b->plans[k].n_audio;
    }
    return RFA_OK;
}

int rfa_demod_bank_process_host(rfa_demod_bank *b, const float *re, const float *im, size_t channel_stride,
                                size_t n_samples, size_t packet_samples, float *audio, size_t audio_stride,
                                size_t *n_audio) {
    if (!b || !n_audio) return RFA_ERR_INVALID;
    const size_t K = (size_t)b->K;
    for (size_t k = 0; k < K; k++) n_audio[k] = 0;
    if (audio_stride > (size_t)1 << 40) return stage_fail(b, RFA_ERR_INVALID, "n_samples too large");
    int rc = stage_check_rows(b, K, re, im, channel_stride, n_samples);
    if (rc != RFA_OK) return rc;
    bank_plan(b, (long long)n_samples, (long long)packet_samples);
    size_t max_audio = 0;
    for (size_t k = 0; k < K; k++)
        if (b->slots[k].mode != RFA_DEMOD_OFF) max_audio = std::max(max_audio, (size_t)b->plans[k].n_audio);
    if (max_audio > audio_stride) return stage_fail(b, RFA_ERR_SIZE, "audio_stride too small for a slot");
    if (max_audio > 0 && !audio) return stage_fail(b, RFA_ERR_INVALID, "null output");
    rc = stage_upload_rows(b, b->d_in, b->d_in_cap, re, im, channel_stride, K, n_samples);
    if (rc == RFA_OK) rc = stage_grow(b, b->d_out, b->d_out_cap, K * max_audio, "output staging");
    if (rc != RFA_OK) return rc;
    rc = rfa_demod_bank_process(b, b->d_in, b->d_in + K * n_samples, n_samples, n_samples, packet_samples, b->d_out,
                                max_audio, n_audio);
    if (rc != RFA_OK) return rc;
    for (size_t k = 0; k < K; k++)      // a slot's row of the caller's buffer is written up to its own count
        if (n_audio[k])
            STAGE_HIP(b, hipMemcpyAsync(audio + k * audio_stride, b->d_out + k * max_audio, n_audio[k] * sizeof(float),
                                   hipMemcpyDeviceToHost, b->stream));
    STAGE_HIP(b, hipStreamSynchronize(b->stream));
    return RFA_OK;
}

// (the record ring is ordered on the bank's stream too: stage_set_stream drains it)
int rfa_demod_bank_set_stream(rfa_demod_bank *b, void *stream) { return stage_set_stream(b, stream); }

int rfa_demod_bank_get_stream(const rfa_demod_bank *b, void **stream) { return stage_get_stream(b, stream); }

int rfa_demod_bank_synchronize(rfa_demod_bank *b) { return stage_synchronize(b); }

}  // extern "C"
