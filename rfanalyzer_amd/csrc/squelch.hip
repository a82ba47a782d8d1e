// squelch.hip -- per-slot level meter and squelch rule for the receiver banks (rfa_squelch_*).
//
// The level of a slot is the mean power of its quadrature row in the reference's magnitude-dB,
// 5 * log10(sum(re^2 + im^2) / n); the rule is the Scheduler's per-packet gate with its debounce
// (analyzer/Scheduler.kt:52,161-165,237; database/AppStateRepository.kt:318-324), kept per slot.
// The device sums; the host turns K sums into K levels and steps K counters.
//
// Term.  term[i] = re[i]^2 + im[i]^2 in float -- the two products and their sum each rounded on
// its own -- then widened: one double component per slot.  No prologue, no epilogue.  How the terms
// of a row are added, in how many launches, and what the handle owns for it: slot_sum.h.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <new>
#include <vector>

#include "slot_sum.h"

#pragma clang fp contract(off)

namespace {

struct PowerTerm {
    static constexpr int C = 1;
    struct In {
        float r, q;
    };
    __device__ __forceinline__ In load(const float *__restrict__ re, const float *__restrict__ im, long long i) const {
        return In{re[i], im[i]};
    }
    __device__ __forceinline__ void add(double (&acc)[C], In x) const {
        const float rr = x.r * x.r, qq = x.q * x.q;
        const float term = rr + qq;
        acc[0] += (double)term;
    }
    __device__ __forceinline__ bool prologue(size_t, const float *, const float *, double (&)[C]) const { return false; }
    __device__ __forceinline__ void epilogue(size_t, const float *, const float *, long long) const {}
};

}  // namespace

struct rfa_squelch : StageCore {
    int K = 0;
    int32_t debounce = RFA_SQUELCH_DEFAULT_DEBOUNCE;
    std::vector<uint8_t> enabled, open;
    std::vector<float> threshold, level;
    std::vector<int32_t> counter;
    std::vector<double> sums;          // the last call's
    SlotSums dev;                      // [K]
};

namespace {

bool sq_slot_ok(const rfa_squelch *s, int32_t k) { return k >= 0 && k < s->K; }

// Levels from the K sums of a call of n samples, one step of the rule per slot, the outputs.
void sq_commit(rfa_squelch *s, const double *sums, size_t n, float *level_db, uint8_t *open) {
    for (int k = 0; k < s->K; k++) {
        s->sums[k] = n ? sums[k] : 0.0;
        s->level[k] = rfa_squelch_level(s->sums[k], n, s->level[k]);
        const int satisfied = !s->enabled[k] || s->level[k] > s->threshold[k];
        s->open[k] = (uint8_t)rfa_squelch_step(satisfied, s->debounce, &s->counter[k]);
        if (level_db) level_db[k] = s->level[k];
        if (open) open[k] = s->open[k];
    }
}

}  // namespace

extern "C" {

float rfa_squelch_level(double sum, size_t n, float previous) {
    if (n == 0) return previous;
    return (float)(5.0 * std::log10(sum / (double)n));
}

// Scheduler.kt:161-165 and :237 as written.
int rfa_squelch_step(int satisfied, int32_t debounce, int32_t *counter) {
    int32_t local = 0;
    int32_t &ctr = counter ? *counter : local;
    if (debounce < 0) debounce = 0;
    if (satisfied) ctr = 0;
    else if (ctr < debounce) ctr++;
    return satisfied || ctr < debounce;
}

int rfa_squelch_create(int device, int32_t n_channels, rfa_squelch **out) {
    if (!out) return RFA_ERR_INVALID;
    *out = nullptr;
    if (n_channels < 1 || n_channels > RFA_SQUELCH_MAX_CHANNELS) return RFA_ERR_INVALID;
    int rc = stage_check_device(device);
    if (rc != RFA_OK) return rc;
    rfa_squelch *s = new (std::nothrow) rfa_squelch();
    if (!s) return RFA_ERR_NOMEM;
    const size_t K = (size_t)n_channels;
    s->device = device;
    s->K = n_channels;
    s->enabled.assign(K, 0);
    s->open.assign(K, 1);
    s->threshold.assign(K, 0.0f);
    s->level.assign(K, RFA_SQUELCH_INITIAL_LEVEL);
    s->counter.assign(K, 0);
    s->sums.assign(K, 0.0);
    rc = stage_open(s, device);
    if (rc == RFA_OK) rc = slot_sums_open(s->dev, K * PowerTerm::C);
    if (rc != RFA_OK) {
        rfa_squelch_destroy(s);
        return rc;
    }
    *out = s;
    return RFA_OK;
}

int rfa_squelch_destroy(rfa_squelch *s) {
    if (!s) return RFA_ERR_INVALID;
    stage_close_stream(s);
    slot_sums_close(s->dev);
    delete s;
    return RFA_OK;
}

const char *rfa_squelch_last_error(const rfa_squelch *s) { return stage_last_error(s); }

int rfa_squelch_get_channels(const rfa_squelch *s, int32_t *n_channels) {
    if (!s || !n_channels) return RFA_ERR_INVALID;
    *n_channels = s->K;
    return RFA_OK;
}

int rfa_squelch_set(rfa_squelch *s, int32_t k, int enabled, float threshold_db) {
    if (!s) return RFA_ERR_INVALID;
    if (!sq_slot_ok(s, k)) return stage_fail(s, RFA_ERR_INVALID, "no such slot");
    if (std::isnan(threshold_db)) return stage_fail(s, RFA_ERR_INVALID, "threshold is not a number");
    s->enabled[k] = enabled != 0;
    s->threshold[k] = threshold_db;
    return RFA_OK;
}

int rfa_squelch_get(const rfa_squelch *s, int32_t k, int32_t *enabled, float *threshold_db) {
    if (!s || !sq_slot_ok(s, k)) return RFA_ERR_INVALID;
    if (enabled) *enabled = s->enabled[k];
    if (threshold_db) *threshold_db = s->threshold[k];
    return RFA_OK;
}

int rfa_squelch_set_debounce(rfa_squelch *s, int32_t debounce) {
    if (!s) return RFA_ERR_INVALID;
    if (debounce < 0) return stage_fail(s, RFA_ERR_INVALID, "negative debounce");
    s->debounce = debounce;
    for (int32_t &c : s->counter) c = std::min(c, debounce);
    return RFA_OK;
}

int rfa_squelch_get_debounce(const rfa_squelch *s, int32_t *debounce) {
    if (!s || !debounce) return RFA_ERR_INVALID;
    *debounce = s->debounce;
    return RFA_OK;
}

int rfa_squelch_reset(rfa_squelch *s) {
    if (!s) return RFA_ERR_INVALID;
    for (int k = 0; k < s->K; k++) {
        s->counter[k] = 0;
        s->level[k] = RFA_SQUELCH_INITIAL_LEVEL;
        s->sums[k] = 0.0;
        s->open[k] = 1;
    }
    return RFA_OK;
}

int rfa_squelch_process(rfa_squelch *s, const float *re, const float *im, size_t channel_stride, size_t n_samples,
                        float *level_db, uint8_t *open) {
    if (!s) return RFA_ERR_INVALID;
    int rc = stage_check_rows(s, (size_t)s->K, re, im, channel_stride, n_samples);
    if (rc != RFA_OK) return rc;
    if (n_samples == 0) {                                  // nothing measured: the rule still steps
        sq_commit(s, nullptr, 0, level_db, open);
        return RFA_OK;
    }
    rc = slot_sums_enqueue(s, s->dev, PowerTerm{}, re, im, channel_stride, n_samples);
    if (rc != RFA_OK) return rc;
    STAGE_HIP(s, hipEventSynchronize(s->dev.copied));       // this copy, not what else the stream holds
    sq_commit(s, s->dev.h_sums, n_samples, level_db, open);
    return RFA_OK;
}

int rfa_squelch_process_host(rfa_squelch *s, const float *re, const float *im, size_t channel_stride, size_t n_samples,
                             float *level_db, uint8_t *open) {
    if (!s) return RFA_ERR_INVALID;
    const size_t K = (size_t)s->K;
    int rc = stage_check_rows(s, K, re, im, channel_stride, n_samples);
    if (rc != RFA_OK) return rc;
    if (n_samples == 0) return rfa_squelch_process(s, nullptr, nullptr, 0, 0, level_db, open);
    rc = stage_upload_rows(s, s->dev.d_in, s->dev.d_in_cap, re, im, channel_stride, K, n_samples);
    if (rc != RFA_OK) return rc;
    return rfa_squelch_process(s, s->dev.d_in, s->dev.d_in + K * n_samples, n_samples, n_samples, level_db, open);
}

int rfa_squelch_get_state(const rfa_squelch *s, double *sums, float *level_db, int32_t *counter, uint8_t *open) {
    if (!s) return RFA_ERR_INVALID;
    for (int k = 0; k < s->K; k++) {
        if (sums) sums[k] = s->sums[k];
        if (level_db) level_db[k] = s->level[k];
        if (counter) counter[k] = s->counter[k];
        if (open) open[k] = s->open[k];
    }
    return RFA_OK;
}

int rfa_squelch_set_stream(rfa_squelch *s, void *stream) { return stage_set_stream(s, stream); }

int rfa_squelch_get_stream(const rfa_squelch *s, void **stream) { return stage_get_stream(s, stream); }

int rfa_squelch_synchronize(rfa_squelch *s) { return stage_synchronize(s); }

}  // extern "C"
