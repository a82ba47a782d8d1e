// tone.hip -- per-slot tone meter on the demodulator bank's audio rows (rfa_tone_*): what a CTCSS
// tone squelch reads.
//
// Per slot and call the device sums the audio row against up to three probe frequencies -- the
// wanted tone and two guards -- and with itself:
//     Sc_j = sum a[i] * W[p_j(i)].cos,  Ss_j = sum a[i] * W[p_j(i)].sin   (j = 0, 1, 2)
//     P = sum a[i] * a[i],  S1 = sum a[i]
// in double, every product rounded once.  The host turns sums into a quality (rfa_tone_quality)
// and decides what to do with it (demod.ToneRule).  The reference has one channel, squelched by
// hand, and no counterpart of this file.
//
// Phasors.  W[p] = (cos, sin)(2 pi p / M), M = 10 * sample_rate, one table on the device, filled at
// creation in double by the host's libm through the function rfa_tone_phasor exports.  A probe is a
// whole number of tenths of a hertz, f10, so sample g of a slot's stream meets W[(f10 * g) mod M]
// exactly, in 64-bit integers: no phase accumulates an error, and a row cut into calls anywhere
// meets the phasors of the row given whole.  g = base_k + i with base_k the slot's sample counter,
// kept on the host modulo M (f10 * M is a multiple of M).
//
// The eight components are summed by the plan of slot_sum.h with a count per slot -- the
// demodulator bank's audio counts differ between slots -- through the plan's counted kernels, the
// term handing out a per-slot view that holds the slot's probes and counter.
//
// Records.  A call's counts, counters and probes must be on the device when its kernels run, while
// the host may be enqueueing the next call: they are staged in a ring of kRecRing pinned entries,
// each with an event behind its copy, as rfa_demod_bank stages its launch records.  The device
// array is one, copy and kernels being ordered on the stream.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

#include "slot_sum.h"

#pragma clang fp contract(off)

static_assert(RFA_TONE_TILE == RFA_SQUELCH_TILE, "the meters share one plan");

namespace {

constexpr int kProbes = RFA_TONE_PROBES;
constexpr int kRecRing = 8;

struct ToneSlot {
    long long base;                    // the slot's sample counter at sample 0 of this call, 0 <= base < M
    int f10[kProbes];                  // 0: unused
    int pad;
};

struct ToneTerm {
    const double2 *W;                  // [M]
    long long M;
    const ToneSlot *slots;             // [K], this call's

    struct View {
        static constexpr int C = RFA_TONE_SUMS;
        const double2 *W;
        unsigned long long M, base;
        unsigned f10[kProbes];
        struct In {
            float a;
            double2 w[kProbes];
        };
        __device__ __forceinline__ In load(const float *__restrict__ a, const float *, long long i) const {
            In x;
            x.a = a[i];
            const unsigned long long g = base + (unsigned long long)i;             // < 2^37; f10 < 2^21
#pragma unroll
            for (int j = 0; j < kProbes; j++) x.w[j] = f10[j] ? W[(f10[j] * g) % M] : double2{0.0, 0.0};
            return x;
        }
        __device__ __forceinline__ void add(double (&acc)[C], const In &x) const {
            const double a = (double)x.a;
#pragma unroll
            for (int j = 0; j < kProbes; j++)
                if (f10[j]) {                                  // the same for the whole slot
                    const double tc = a * x.w[j].x;
                    const double ts = a * x.w[j].y;
                    acc[2 * j] += tc;
                    acc[2 * j + 1] += ts;
                }
            const double tp = a * a;
            acc[2 * kProbes] += tp;
            acc[2 * kProbes + 1] += a;
        }
        __device__ __forceinline__ bool prologue(size_t, const float *, const float *, double (&)[C]) const {
            return false;
        }
        __device__ __forceinline__ void epilogue(size_t, const float *, const float *, long long) const {}
    };

    __device__ __forceinline__ View slot(size_t k) const {
        const ToneSlot s = slots[k];
        View v;
        v.W = W;
        v.M = (unsigned long long)M;
        v.base = (unsigned long long)s.base;
#pragma unroll
        for (int j = 0; j < kProbes; j++) v.f10[j] = (unsigned)s.f10[j];
        return v;
    }
};

static_assert(ToneTerm::View::C == 2 * kProbes + 2, "two sums per probe, the power and the plain sum");

// The one definition of a table entry (rfa_tone_phasor and the fill at creation).
__attribute__((noinline)) void phasor(long long M, long long p, double &c, double &s) {
    const double th = (2.0 * M_PI * (double)p) / (double)M;
    c = std::cos(th);
    s = std::sin(th);
}

bool rate_ok(int32_t rate) { return rate >= RFA_TONE_MIN_RATE && rate <= RFA_TONE_MAX_RATE; }

}  // namespace

struct rfa_tone : StageCore {
    int K = 0;
    int32_t rate = 0;
    long long M = 0;
    std::vector<int32_t> f10;          // [K][kProbes]
    std::vector<long long> base;       // [K], modulo M
    std::vector<double> sums;          // [C][K], the last collected call's
    std::vector<int64_t> n, next_n;    // that call's counts; those of the call whose copy is outstanding
    bool outstanding = false;
    SlotSums dev;                      // [C][K]; `copied` is what collect waits for
    double2 *d_w = nullptr;            // [M]
    char *d_recs = nullptr;            // long long counts[K], then ToneSlot[K]
    char *h_recs = nullptr;            // pinned, [kRecRing] of the same
    size_t rec_bytes = 0;
    hipEvent_t ev[kRecRing] = {};
    bool ev_used[kRecRing] = {};
    int ring_at = 0;
};

namespace {

void tn_zero_results(rfa_tone *t) {
    std::fill(t->sums.begin(), t->sums.end(), 0.0);
    std::fill(t->n.begin(), t->n.end(), (int64_t)0);
}

// The checks of a call; max_n is the largest count.
int tn_check(rfa_tone *t, const float *audio, size_t audio_stride, const size_t *n_audio, size_t &max_n) {
    max_n = 0;
    if (!n_audio) return stage_fail(t, RFA_ERR_INVALID, "null count array");
    if (audio_stride > (size_t)1 << 40) return stage_fail(t, RFA_ERR_INVALID, "audio_stride too large");
    for (int k = 0; k < t->K; k++) {
        if (n_audio[k] > (size_t)1 << 36) return stage_fail(t, RFA_ERR_INVALID, "count too large");
        if (t->K > 1 && n_audio[k] > audio_stride) return stage_fail(t, RFA_ERR_INVALID, "a count above audio_stride");
        max_n = std::max(max_n, n_audio[k]);
    }
    if (max_n && !audio) return stage_fail(t, RFA_ERR_INVALID, "null input");
    return RFA_OK;
}

}  // namespace

extern "C" {

int rfa_tone_phasor(int32_t sample_rate, int64_t p, double *c, double *s) {
    if (!c || !s || !rate_ok(sample_rate)) return RFA_ERR_INVALID;
    const long long M = 10LL * sample_rate;
    if (p < 0 || p >= M) return RFA_ERR_INVALID;
    phasor(M, p, *c, *s);
    return RFA_OK;
}

double rfa_tone_quality(double sc, double ss, double p, double s1, int64_t n) {
    if (!std::isfinite(sc) || !std::isfinite(ss) || !std::isfinite(p) || !std::isfinite(s1)) return std::nan("");
    const double den = (double)n * p - s1 * s1;
    if (!(den > 0.0)) return 0.0;
    return 2.0 * (sc * sc + ss * ss) / den;
}

int rfa_tone_create(int device, int32_t n_channels, int32_t sample_rate, rfa_tone **out) {
    if (!out) return RFA_ERR_INVALID;
    *out = nullptr;
    if (n_channels < 1 || n_channels > RFA_TONE_MAX_CHANNELS || !rate_ok(sample_rate)) return RFA_ERR_INVALID;
    int rc = stage_check_device(device);
    if (rc != RFA_OK) return rc;
    rfa_tone *t = new (std::nothrow) rfa_tone();
    if (!t) return RFA_ERR_NOMEM;
    const size_t K = (size_t)n_channels;
    t->device = device;
    t->K = n_channels;
    t->rate = sample_rate;
    t->M = 10LL * sample_rate;
    t->f10.assign(K * kProbes, 0);
    t->base.assign(K, 0);
    t->sums.assign(K * RFA_TONE_SUMS, 0.0);
    t->n.assign(K, 0);
    t->next_n.assign(K, 0);
    t->rec_bytes = K * (sizeof(long long) + sizeof(ToneSlot));
    rc = stage_open(t, device);
    if (rc == RFA_OK) rc = slot_sums_open(t->dev, K * RFA_TONE_SUMS);
    if (rc == RFA_OK && (hipMalloc(&t->d_w, (size_t)t->M * sizeof(double2)) != hipSuccess ||
                         hipMalloc(&t->d_recs, t->rec_bytes) != hipSuccess ||
                         hipHostMalloc(&t->h_recs, kRecRing * t->rec_bytes, hipHostMallocDefault) != hipSuccess))
        rc = RFA_ERR_NOMEM;
    for (int e = 0; rc == RFA_OK && e < kRecRing; e++)
        if (hipEventCreateWithFlags(&t->ev[e], hipEventDisableTiming) != hipSuccess) rc = RFA_ERR_HIP;
    if (rc == RFA_OK) {
        std::vector<double2> w((size_t)t->M);
        for (long long p = 0; p < t->M; p++) phasor(t->M, p, w[(size_t)p].x, w[(size_t)p].y);
        if (hipMemcpy(t->d_w, w.data(), w.size() * sizeof(double2), hipMemcpyHostToDevice) != hipSuccess)
            rc = RFA_ERR_HIP;
    }
    if (rc != RFA_OK) {
        rfa_tone_destroy(t);
        return rc;
    }
    *out = t;
    return RFA_OK;
}

int rfa_tone_destroy(rfa_tone *t) {
    if (!t) return RFA_ERR_INVALID;
    stage_close_stream(t);
    slot_sums_close(t->dev);
    if (t->d_w) (void)hipFree(t->d_w);
    if (t->d_recs) (void)hipFree(t->d_recs);
    if (t->h_recs) (void)hipHostFree(t->h_recs);
    for (hipEvent_t e : t->ev)
        if (e) (void)hipEventDestroy(e);
    delete t;
    return RFA_OK;
}

const char *rfa_tone_last_error(const rfa_tone *t) { return stage_last_error(t); }

int rfa_tone_get_channels(const rfa_tone *t, int32_t *n_channels, int32_t *sample_rate) {
    if (!t || !n_channels) return RFA_ERR_INVALID;
    *n_channels = t->K;
    if (sample_rate) *sample_rate = t->rate;
    return RFA_OK;
}

int rfa_tone_set_probes(rfa_tone *t, int32_t k, const int32_t *f10) {
    if (!t) return RFA_ERR_INVALID;
    if (k < 0 || k >= t->K) return stage_fail(t, RFA_ERR_INVALID, "no such slot");
    if (!f10) return stage_fail(t, RFA_ERR_INVALID, "null probes");
    for (int j = 0; j < kProbes; j++)
        if (f10[j] < 0 || (long long)f10[j] >= 5LL * t->rate)
            return stage_fail(t, RFA_ERR_INVALID, "a probe outside 0.1 Hz ... half the sample rate");
    for (int j = 0; j < kProbes; j++) t->f10[(size_t)k * kProbes + j] = f10[j];
    return RFA_OK;
}

int rfa_tone_get_probes(const rfa_tone *t, int32_t k, int32_t *f10) {
    if (!t || !f10 || k < 0 || k >= t->K) return RFA_ERR_INVALID;
    for (int j = 0; j < kProbes; j++) f10[j] = t->f10[(size_t)k * kProbes + j];
    return RFA_OK;
}

int rfa_tone_break(rfa_tone *t, int32_t k) {
    if (!t) return RFA_ERR_INVALID;
    if (k < -1 || k >= t->K) return stage_fail(t, RFA_ERR_INVALID, "no such slot");
    const size_t first = k < 0 ? 0 : (size_t)k, count = k < 0 ? (size_t)t->K : 1;
    for (size_t j = first; j < first + count; j++) t->base[j] = 0;
    return RFA_OK;
}

int rfa_tone_reset(rfa_tone *t) {
    if (!t) return RFA_ERR_INVALID;
    std::fill(t->base.begin(), t->base.end(), 0LL);
    t->outstanding = false;            // a later copy into h_sums is ordered behind this one on the stream
    tn_zero_results(t);
    return RFA_OK;
}

int rfa_tone_process(rfa_tone *t, const float *audio, size_t audio_stride, const size_t *n_audio) {
    if (!t) return RFA_ERR_INVALID;
    size_t max_n = 0;
    int rc = tn_check(t, audio, audio_stride, n_audio, max_n);
    if (rc != RFA_OK) return rc;
    if (max_n == 0) {                                      // nothing launched, the counters stay
        t->outstanding = false;
        tn_zero_results(t);
        return RFA_OK;
    }
    const size_t K = (size_t)t->K;
    STAGE_HIP(t, hipSetDevice(t->device));
    // this call's records: wait until the ring entry's previous copy has been made
    const int e = t->ring_at;
    if (t->ev_used[e]) STAGE_HIP(t, hipEventSynchronize(t->ev[e]));
    char *entry = t->h_recs + (size_t)e * t->rec_bytes;
    long long *counts = reinterpret_cast<long long *>(entry);
    ToneSlot *slots = reinterpret_cast<ToneSlot *>(entry + K * sizeof(long long));
    for (size_t k = 0; k < K; k++) {
        counts[k] = (long long)n_audio[k];
        ToneSlot s{};
        s.base = t->base[k];
        for (int j = 0; j < kProbes; j++) s.f10[j] = t->f10[k * kProbes + j];
        slots[k] = s;
    }
    STAGE_HIP(t, hipMemcpyAsync(t->d_recs, entry, t->rec_bytes, hipMemcpyHostToDevice, t->stream));
    STAGE_HIP(t, hipEventRecord(t->ev[e], t->stream));
    t->ev_used[e] = true;
    t->ring_at = (e + 1) % kRecRing;

    const long long *d_counts = reinterpret_cast<const long long *>(t->d_recs);
    const ToneSlot *d_slots = reinterpret_cast<const ToneSlot *>(t->d_recs + K * sizeof(long long));
    // the term reads one row: the audio stands for both rows of the plan
    rc = slot_sums_enqueue_counted(t, t->dev, ToneTerm{t->d_w, t->M, d_slots}, audio, audio, audio_stride, d_counts,
                                   max_n);
    if (t->dev.launched)                                   // the sums are those of this call whatever followed
        for (size_t k = 0; k < K; k++) {
            t->next_n[k] = (int64_t)n_audio[k];
            t->base[k] = (long long)(((unsigned long long)t->base[k] + n_audio[k]) % (unsigned long long)t->M);
        }
    if (rc != RFA_OK) return rc;
    t->outstanding = true;
    return RFA_OK;
}

int rfa_tone_collect(rfa_tone *t, double *sums, int64_t *n) {
    if (!t) return RFA_ERR_INVALID;
    if (t->outstanding) {
        STAGE_HIP(t, hipSetDevice(t->device));
        STAGE_HIP(t, hipEventSynchronize(t->dev.copied));  // this copy, not what else the stream holds
        t->outstanding = false;
        std::memcpy(t->sums.data(), t->dev.h_sums, t->sums.size() * sizeof(double));
        t->n = t->next_n;
    }
    if (sums) std::memcpy(sums, t->sums.data(), t->sums.size() * sizeof(double));
    if (n) std::memcpy(n, t->n.data(), t->n.size() * sizeof(int64_t));
    return RFA_OK;
}

int rfa_tone_process_host(rfa_tone *t, const float *audio, size_t audio_stride, const size_t *n_audio, double *sums,
                          int64_t *n) {
    if (!t) return RFA_ERR_INVALID;
    size_t max_n = 0;
    int rc = tn_check(t, audio, audio_stride, n_audio, max_n);
    if (rc != RFA_OK) return rc;
    if (max_n == 0) {
        rc = rfa_tone_process(t, nullptr, 0, n_audio);
    } else {
        const size_t K = (size_t)t->K;
        STAGE_HIP(t, hipSetDevice(t->device));
        rc = stage_grow(t, t->dev.d_in, t->dev.d_in_cap, K * max_n, "input staging");
        if (rc != RFA_OK) return rc;
        for (size_t k = 0; k < K; k++)                     // row k holds n_audio[k] floats and no more
            if (n_audio[k])
                STAGE_HIP(t, hipMemcpyAsync(t->dev.d_in + k * max_n, audio + k * audio_stride,
                                            n_audio[k] * sizeof(float), hipMemcpyHostToDevice, t->stream));
        rc = rfa_tone_process(t, t->dev.d_in, max_n, n_audio);
    }
    if (rc != RFA_OK) return rc;
    return rfa_tone_collect(t, sums, n);
}

int rfa_tone_set_stream(rfa_tone *t, void *stream) { return stage_set_stream(t, stream); }

int rfa_tone_get_stream(const rfa_tone *t, void **stream) { return stage_get_stream(t, stream); }

int rfa_tone_synchronize(rfa_tone *t) { return stage_synchronize(t); }

}  // extern "C"
