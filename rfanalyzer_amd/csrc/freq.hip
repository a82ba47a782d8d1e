// freq.hip -- per-slot frequency-error meter for the receiver banks (rfa_freq_*).
//
// The meter of a slot is the lag-1 autocorrelation of its quadrature row,
//     R1 = sum over i of x[i] * conj(x[i-1]),
// whose argument is the mean phase advance per sample: a carrier f Hz off the slot's centre
// gives arg R1 = 2 pi f / rate.  The device sums; the host turns a pair of sums into Hz
// (rfa_freq_error_hz) and decides what to do with it (demod.AfcRule).  The reference tunes one
// channel by hand and has no counterpart of this file.
//
// Terms.  term_re[i] = xr*pr + xi*pi, term_im[i] = xi*pr - xr*pi with (pr, pi) = x[i-1], every
// product formed in double from the float inputs.  Such a product is exact, so a term is the
// exact two-product sum rounded once, whether or not the compiler contracts it into an fma.
//
// The two components are summed by the plan of slot_sum.h: a slot's sums are a function of its
// values, n and the carried sample alone, bit for bit.
//
// The carried sample.  The term for i = 0 needs the slot's last sample of the previous call:
// carry[k] (re, im) with valid[k] on the device.  Without a valid carry the term is left out.
// The plan's prologue reads the carry and adds term 0, its epilogue writes the new carry,
// x[n-1]; slot_sum.h says why the write is ordered after the read in either launch plan.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <new>
#include <vector>

#include "slot_sum.h"

#pragma clang fp contract(off)

namespace {

struct R1Term {
    static constexpr int C = 2;        // re, im
    float *carry;                      // [K][2]
    int *valid;                        // [K]
    struct In {
        float xr, xi, pr, pi;
    };
    __device__ __forceinline__ In load(const float *__restrict__ re, const float *__restrict__ im, long long i) const {
        return In{re[i], im[i], re[i - 1], im[i - 1]};
    }
    __device__ __forceinline__ void add(double (&acc)[C], In x) const {
        const double a = (double)x.xr, b = (double)x.xi, c = (double)x.pr, d = (double)x.pi;
        const double tr = a * c + b * d;
        const double ti = b * c - a * d;
        acc[0] += tr;
        acc[1] += ti;
    }
    __device__ __forceinline__ bool prologue(size_t k, const float *re, const float *im, double (&acc)[C]) const {
        if (valid[k]) add(acc, In{re[0], im[0], carry[2 * k], carry[2 * k + 1]});
        return true;
    }
    __device__ __forceinline__ void epilogue(size_t k, const float *re, const float *im, long long n) const {
        carry[2 * k] = re[n - 1];
        carry[2 * k + 1] = im[n - 1];
        valid[k] = 1;
    }
};

}  // namespace

struct rfa_freq : StageCore {
    int K = 0;
    std::vector<double> r1_re, r1_im;  // the last collected call's
    std::vector<int64_t> terms;
    std::vector<uint8_t> carried;      // host mirror of d_valid, in call order (= stream order)
    std::vector<int64_t> next_terms;   // of the call whose copy is outstanding
    bool outstanding = false;          // a copy into h_sums has been enqueued and not collected
    SlotSums dev;                      // [2][K]: re then im; `copied` is what collect waits for
    float *d_carry = nullptr;          // [K][2]
    int *d_valid = nullptr;            // [K]
};

namespace {

void fq_zero_results(rfa_freq *f) {
    for (int k = 0; k < f->K; k++) {
        f->r1_re[k] = f->r1_im[k] = 0.0;
        f->terms[k] = 0;
    }
}

}  // namespace

extern "C" {

double rfa_freq_error_hz(double r1_re, double r1_im, double rate) {
    if (!std::isfinite(r1_re) || !std::isfinite(r1_im)) return std::nan("");
    if (r1_re == 0.0 && r1_im == 0.0) return 0.0;
    return std::atan2(r1_im, r1_re) * rate / (2.0 * M_PI);
}

int rfa_freq_create(int device, int32_t n_channels, rfa_freq **out) {
    if (!out) return RFA_ERR_INVALID;
    *out = nullptr;
    if (n_channels < 1 || n_channels > RFA_FREQ_MAX_CHANNELS) return RFA_ERR_INVALID;
    int rc = stage_check_device(device);
    if (rc != RFA_OK) return rc;
    rfa_freq *f = new (std::nothrow) rfa_freq();
    if (!f) return RFA_ERR_NOMEM;
    const size_t K = (size_t)n_channels;
    f->device = device;
    f->K = n_channels;
    f->r1_re.assign(K, 0.0);
    f->r1_im.assign(K, 0.0);
    f->terms.assign(K, 0);
    f->next_terms.assign(K, 0);
    f->carried.assign(K, 0);
    rc = stage_open(f, device);
    if (rc == RFA_OK) rc = slot_sums_open(f->dev, K * R1Term::C);
    if (rc == RFA_OK && (hipMalloc(&f->d_carry, 2 * K * sizeof(float)) != hipSuccess ||
                         hipMalloc(&f->d_valid, K * sizeof(int)) != hipSuccess))
        rc = RFA_ERR_NOMEM;
    if (rc == RFA_OK && (hipMemsetAsync(f->d_valid, 0, K * sizeof(int), f->stream) != hipSuccess ||
                         hipMemsetAsync(f->d_carry, 0, 2 * K * sizeof(float), f->stream) != hipSuccess))
        rc = RFA_ERR_HIP;
    if (rc != RFA_OK) {
        rfa_freq_destroy(f);
        return rc;
    }
    *out = f;
    return RFA_OK;
}

int rfa_freq_destroy(rfa_freq *f) {
    if (!f) return RFA_ERR_INVALID;
    stage_close_stream(f);
    slot_sums_close(f->dev);
    if (f->d_carry) (void)hipFree(f->d_carry);
    if (f->d_valid) (void)hipFree(f->d_valid);
    delete f;
    return RFA_OK;
}

const char *rfa_freq_last_error(const rfa_freq *f) { return stage_last_error(f); }

int rfa_freq_get_channels(const rfa_freq *f, int32_t *n_channels) {
    if (!f || !n_channels) return RFA_ERR_INVALID;
    *n_channels = f->K;
    return RFA_OK;
}

int rfa_freq_break(rfa_freq *f, int32_t k) {
    if (!f) return RFA_ERR_INVALID;
    if (k < -1 || k >= f->K) return stage_fail(f, RFA_ERR_INVALID, "no such slot");
    STAGE_HIP(f, hipSetDevice(f->device));
    const size_t first = k < 0 ? 0 : (size_t)k, count = k < 0 ? (size_t)f->K : 1;
    STAGE_HIP(f, hipMemsetAsync(f->d_valid + first, 0, count * sizeof(int), f->stream));
    for (size_t j = first; j < first + count; j++) f->carried[j] = 0;
    return RFA_OK;
}

int rfa_freq_reset(rfa_freq *f) {
    if (!f) return RFA_ERR_INVALID;
    const int rc = rfa_freq_break(f, -1);
    if (rc != RFA_OK) return rc;
    f->outstanding = false;            // a later copy into h_sums is ordered behind this one on the stream
    fq_zero_results(f);
    return RFA_OK;
}

int rfa_freq_process(rfa_freq *f, const float *re, const float *im, size_t channel_stride, size_t n_samples) {
    if (!f) return RFA_ERR_INVALID;
    int rc = stage_check_rows(f, (size_t)f->K, re, im, channel_stride, n_samples);
    if (rc != RFA_OK) return rc;
    if (n_samples == 0) {                                  // nothing launched, the carry stays
        f->outstanding = false;
        fq_zero_results(f);
        return RFA_OK;
    }
    rc = slot_sums_enqueue(f, f->dev, R1Term{f->d_carry, f->d_valid}, re, im, channel_stride, n_samples);
    if (f->dev.launched)                                   // the device's flags are set whatever followed
        for (int k = 0; k < f->K; k++) {
            f->next_terms[k] = (int64_t)n_samples - (f->carried[k] ? 0 : 1);
            f->carried[k] = 1;
        }
    if (rc != RFA_OK) return rc;
    f->outstanding = true;
    return RFA_OK;
}

int rfa_freq_collect(rfa_freq *f, double *r1_re, double *r1_im, int64_t *terms) {
    if (!f) return RFA_ERR_INVALID;
    if (f->outstanding) {
        STAGE_HIP(f, hipSetDevice(f->device));
        STAGE_HIP(f, hipEventSynchronize(f->dev.copied));  // this copy, not what else the stream holds
        f->outstanding = false;
        for (int k = 0; k < f->K; k++) {
            f->r1_re[k] = f->dev.h_sums[k];
            f->r1_im[k] = f->dev.h_sums[f->K + k];
            f->terms[k] = f->next_terms[k];
        }
    }
    for (int k = 0; k < f->K; k++) {
        if (r1_re) r1_re[k] = f->r1_re[k];
        if (r1_im) r1_im[k] = f->r1_im[k];
        if (terms) terms[k] = f->terms[k];
    }
    return RFA_OK;
}

int rfa_freq_process_host(rfa_freq *f, const float *re, const float *im, size_t channel_stride, size_t n_samples,
                          double *r1_re, double *r1_im, int64_t *terms) {
    if (!f) return RFA_ERR_INVALID;
    const size_t K = (size_t)f->K;
    int rc = stage_check_rows(f, K, re, im, channel_stride, n_samples);
    if (rc != RFA_OK) return rc;
    if (n_samples == 0) {
        rc = rfa_freq_process(f, nullptr, nullptr, 0, 0);
    } else {
        rc = stage_upload_rows(f, f->dev.d_in, f->dev.d_in_cap, re, im, channel_stride, K, n_samples);
        if (rc != RFA_OK) return rc;
        rc = rfa_freq_process(f, f->dev.d_in, f->dev.d_in + K * n_samples, n_samples, n_samples);
    }
    if (rc != RFA_OK) return rc;
    return rfa_freq_collect(f, r1_re, r1_im, terms);
}

int rfa_freq_set_stream(rfa_freq *f, void *stream) { return stage_set_stream(f, stream); }

int rfa_freq_get_stream(const rfa_freq *f, void **stream) { return stage_get_stream(f, stream); }

int rfa_freq_synchronize(rfa_freq *f) { return stage_synchronize(f); }

}  // extern "C"
