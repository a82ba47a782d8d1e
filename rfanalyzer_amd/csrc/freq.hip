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
// Summation plan: the squelch's (squelch.hip).  Samples are cut into tiles of kFqTile = 16384,
// a workgroup of 256 threads sums one tile: thread t adds the terms at tile_start + t + 256*m,
// m ascending, into two doubles; a wave folds its 64 accumulators with wave_reduce, the four
// waves are added in wave order, tiles in ascending order.  No atomics, nothing looks at the
// row's address, the stride or K: a slot's sums are a function of its values, n and the carried
// sample alone, bit for bit.
//   n <= kFqTile: one launch, grid (K).
//   n >  kFqTile: freq_partials_kernel over (tiles, K), then freq_fold_kernel over (K).
//
// The carried sample.  The term for i = 0 needs the slot's last sample of the previous call:
// carry[k] (re, im) with valid[k] on the device.  Without a valid carry the term is left out.
// Only the workgroup of tile 0 reads the carry (its thread 0).  The new carry, x[n-1], is
// written by something ordered after that read: in the one-launch kernel by thread 0 after the
// workgroup's barrier, in the two-launch case by the fold kernel -- a later launch on the same
// stream -- and never by a partials workgroup, whose tile n-1 may run before tile 0.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <new>
#include <vector>

#include "stage_common.h"
#include "wave.h"

#pragma clang fp contract(off)

namespace {

constexpr int kFqThreads = 256;
constexpr long long kFqTile = RFA_FREQ_TILE;
static_assert(kFqTile % (4 * kFqThreads) == 0, "the unrolled loop covers whole tiles");

struct Sum2 {
    double re, im;
};

__device__ __forceinline__ void add_term(Sum2 &acc, float xr, float xi, float pr, float pi) {
    const double a = (double)xr, b = (double)xi, c = (double)pr, d = (double)pi;
    const double tr = a * c + b * d;
    const double ti = b * c - a * d;
    acc.re += tr;
    acc.im += ti;
}

// Sum of the terms i in [lo, hi) of one row, hi - lo <= kFqTile; term 0 takes its predecessor
// from (cr, ci) where have_carry, and is left out otherwise.  Valid in thread 0, after a barrier.
__device__ __forceinline__ Sum2 tile_sum(const float *__restrict__ re, const float *__restrict__ im, long long lo,
                                         long long hi, const float *carry, const int *valid) {
    __shared__ double wave_re[kFqThreads / 64], wave_im[kFqThreads / 64];
    const int t = (int)threadIdx.x;
    Sum2 acc{0.0, 0.0};
    long long i = lo + t;
    if (i == 0 && i < hi) {                                    // thread 0 of tile 0
        if (*valid) add_term(acc, re[0], im[0], carry[0], carry[1]);
        i += kFqThreads;
    }
    // four independent groups of loads in flight, added in index order
    for (; i + 3 * kFqThreads < hi; i += 4 * kFqThreads) {
        float r[4], q[4], pr[4], pq[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            r[u] = re[i + u * kFqThreads];
            q[u] = im[i + u * kFqThreads];
            pr[u] = re[i + u * kFqThreads - 1];
            pq[u] = im[i + u * kFqThreads - 1];
        }
#pragma unroll
        for (int u = 0; u < 4; u++) add_term(acc, r[u], q[u], pr[u], pq[u]);
    }
    for (; i < hi; i += kFqThreads) add_term(acc, re[i], im[i], re[i - 1], im[i - 1]);
    const double wr = rfa::wave_reduce(acc.re, [](double a, double b) { return a + b; });
    const double wi = rfa::wave_reduce(acc.im, [](double a, double b) { return a + b; });
    if ((t & 63) == 0) {
        wave_re[t >> 6] = wr;
        wave_im[t >> 6] = wi;
    }
    __syncthreads();
    Sum2 s{0.0, 0.0};
    if (t == 0) {
        s.re = wave_re[0];
        s.im = wave_im[0];
#pragma unroll
        for (int v = 1; v < kFqThreads / 64; v++) {
            s.re += wave_re[v];
            s.im += wave_im[v];
        }
    }
    return s;
}

// grid (K): 1 <= n <= kFqTile.  sums[k] = re, sums[K + k] = im.
__global__ __launch_bounds__(kFqThreads) void freq_r1_kernel(const float *__restrict__ re,
                                                              const float *__restrict__ im, size_t stride,
                                                              long long n, float *__restrict__ carry,
                                                              int *__restrict__ valid, double *__restrict__ sums) {
    const size_t k = blockIdx.x;
    const float *xr = re + k * stride, *xi = im + k * stride;
    const Sum2 s = tile_sum(xr, xi, 0, n, carry + 2 * k, valid + k);
    if (threadIdx.x == 0) {                                    // behind tile_sum's barrier
        sums[k] = s.re;
        sums[gridDim.x + k] = s.im;
        carry[2 * k] = xr[n - 1];
        carry[2 * k + 1] = xi[n - 1];
        valid[k] = 1;
    }
}

// grid (tiles, K): partials[(k * tiles + j) * 2 + {0, 1}]; reads the carry, writes none
__global__ __launch_bounds__(kFqThreads) void freq_partials_kernel(const float *__restrict__ re,
                                                                    const float *__restrict__ im, size_t stride,
                                                                    long long n, const float *__restrict__ carry,
                                                                    const int *__restrict__ valid,
                                                                    double *__restrict__ partials) {
    const size_t k = blockIdx.y;
    const long long lo = (long long)blockIdx.x * kFqTile;
    const long long hi = lo + kFqTile < n ? lo + kFqTile : n;
    const Sum2 s = tile_sum(re + k * stride, im + k * stride, lo, hi, carry + 2 * k, valid + k);
    if (threadIdx.x == 0) {
        double *p = partials + (k * (size_t)gridDim.x + blockIdx.x) * 2;
        p[0] = s.re;
        p[1] = s.im;
    }
}

// grid (K), one wave: the slot's tiles in ascending order, then the new carry.  Lanes fetch 64
// partial pairs at a time, lane 0 adds them one by one.
__global__ __launch_bounds__(64) void freq_fold_kernel(const double *__restrict__ partials, long long tiles,
                                                       const float *__restrict__ re, const float *__restrict__ im,
                                                       size_t stride, long long n, float *__restrict__ carry,
                                                       int *__restrict__ valid, double *__restrict__ sums) {
    const size_t k = blockIdx.x;
    const double *p = partials + k * (size_t)tiles * 2;
    const int lane = (int)threadIdx.x;
    double sr = 0.0, si = 0.0;
    for (long long base = 0; base < tiles; base += 64) {
        const bool mine = base + lane < tiles;
        const double mr = mine ? p[(base + lane) * 2] : 0.0;
        const double mi = mine ? p[(base + lane) * 2 + 1] : 0.0;
        const int cnt = tiles - base < 64 ? (int)(tiles - base) : 64;
        for (int j = 0; j < cnt; j++) {
            const double vr = rfa::readlane_t(mr, j), vi = rfa::readlane_t(mi, j);
            const bool first = base == 0 && j == 0;
            sr = first ? vr : sr + vr;
            si = first ? vi : si + vi;
        }
    }
    if (lane == 0) {
        sums[k] = sr;
        sums[gridDim.x + k] = si;
        carry[2 * k] = re[k * stride + (n - 1)];
        carry[2 * k + 1] = im[k * stride + (n - 1)];
        valid[k] = 1;
    }
}

}  // namespace

struct rfa_freq : StageCore {
    int K = 0;
    std::vector<double> r1_re, r1_im;  // the last collected call's
    std::vector<int64_t> terms;
    std::vector<uint8_t> carried;      // host mirror of d_valid, in call order (= stream order)
    std::vector<int64_t> next_terms;   // of the call whose copy is outstanding
    bool outstanding = false;          // a copy into h_sums has been enqueued and not collected
    double *d_sums = nullptr;          // [2K]: re then im
    double *h_sums = nullptr;          // pinned, [2K]
    double *d_partials = nullptr;      // [K][tiles][2] of a call above one tile
    size_t partials_cap = 0;
    float *d_carry = nullptr;          // [K][2]
    int *d_valid = nullptr;            // [K]
    hipEvent_t copied = nullptr;       // behind the copy of the sums: what collect waits for
    float *d_in = nullptr;             // staging of the _host entry
    size_t d_in_cap = 0;
};

namespace {

int fq_check_rows(rfa_freq *f, const float *re, const float *im, size_t channel_stride, size_t n_samples) {
    if (n_samples > (size_t)1 << 36 || channel_stride > (size_t)1 << 40)
        return stage_fail(f, RFA_ERR_INVALID, "n_samples too large");
    if (n_samples && (!re || !im)) return stage_fail(f, RFA_ERR_INVALID, "null input");
    if (f->K > 1 && channel_stride < n_samples) return stage_fail(f, RFA_ERR_INVALID, "channel_stride below n_samples");
    return RFA_OK;
}

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
    if (rc == RFA_OK && (hipMalloc(&f->d_sums, 2 * K * sizeof(double)) != hipSuccess ||
                         hipMalloc(&f->d_carry, 2 * K * sizeof(float)) != hipSuccess ||
                         hipMalloc(&f->d_valid, K * sizeof(int)) != hipSuccess ||
                         hipHostMalloc(&f->h_sums, 2 * K * sizeof(double), hipHostMallocDefault) != hipSuccess))
        rc = RFA_ERR_NOMEM;
    if (rc == RFA_OK && (hipMemsetAsync(f->d_valid, 0, K * sizeof(int), f->stream) != hipSuccess ||
                         hipMemsetAsync(f->d_carry, 0, 2 * K * sizeof(float), f->stream) != hipSuccess))
        rc = RFA_ERR_HIP;
    if (rc == RFA_OK && hipEventCreateWithFlags(&f->copied, hipEventDisableTiming) != hipSuccess) rc = RFA_ERR_HIP;
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
    if (f->d_sums) (void)hipFree(f->d_sums);
    if (f->d_partials) (void)hipFree(f->d_partials);
    if (f->d_carry) (void)hipFree(f->d_carry);
    if (f->d_valid) (void)hipFree(f->d_valid);
    if (f->d_in) (void)hipFree(f->d_in);
    if (f->h_sums) (void)hipHostFree(f->h_sums);
    if (f->copied) (void)hipEventDestroy(f->copied);
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
    int rc = fq_check_rows(f, re, im, channel_stride, n_samples);
    if (rc != RFA_OK) return rc;
    const size_t K = (size_t)f->K;
    if (n_samples == 0) {                                  // nothing launched, the carry stays
        f->outstanding = false;
        fq_zero_results(f);
        return RFA_OK;
    }
    const long long n = (long long)n_samples;
    STAGE_HIP(f, hipSetDevice(f->device));
    if (n <= kFqTile) {
        hipLaunchKernelGGL(freq_r1_kernel, dim3((unsigned)K), dim3(kFqThreads), 0, f->stream, re, im, channel_stride, n,
                           f->d_carry, f->d_valid, f->d_sums);
        STAGE_HIP(f, hipGetLastError());
    } else {
        const long long tiles = (n + kFqTile - 1) / kFqTile;           // <= 2^22
        rc = stage_grow(f, f->d_partials, f->partials_cap, 2 * K * (size_t)tiles, "partial sums");
        if (rc != RFA_OK) return rc;
        hipLaunchKernelGGL(freq_partials_kernel, dim3((unsigned)tiles, (unsigned)K), dim3(kFqThreads), 0, f->stream,
                           re, im, channel_stride, n, f->d_carry, f->d_valid, f->d_partials);
        STAGE_HIP(f, hipGetLastError());
        hipLaunchKernelGGL(freq_fold_kernel, dim3((unsigned)K), dim3(64), 0, f->stream, f->d_partials, tiles, re, im,
                           channel_stride, n, f->d_carry, f->d_valid, f->d_sums);
        STAGE_HIP(f, hipGetLastError());
    }
    // from here on the device's flags are set whatever follows
    for (size_t k = 0; k < K; k++) {
        f->next_terms[k] = (int64_t)n_samples - (f->carried[k] ? 0 : 1);
        f->carried[k] = 1;
    }
    STAGE_HIP(f, hipMemcpyAsync(f->h_sums, f->d_sums, 2 * K * sizeof(double), hipMemcpyDeviceToHost, f->stream));
    STAGE_HIP(f, hipEventRecord(f->copied, f->stream));
    f->outstanding = true;
    return RFA_OK;
}

int rfa_freq_collect(rfa_freq *f, double *r1_re, double *r1_im, int64_t *terms) {
    if (!f) return RFA_ERR_INVALID;
    if (f->outstanding) {
        STAGE_HIP(f, hipSetDevice(f->device));
        STAGE_HIP(f, hipEventSynchronize(f->copied));      // this copy, not what else the stream holds
        f->outstanding = false;
        for (int k = 0; k < f->K; k++) {
            f->r1_re[k] = f->h_sums[k];
            f->r1_im[k] = f->h_sums[f->K + k];
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
    int rc = fq_check_rows(f, re, im, channel_stride, n_samples);
    if (rc != RFA_OK) return rc;
    const size_t K = (size_t)f->K;
    if (n_samples == 0) {
        rc = rfa_freq_process(f, nullptr, nullptr, 0, 0);
    } else {
        STAGE_HIP(f, hipSetDevice(f->device));
        rc = stage_grow(f, f->d_in, f->d_in_cap, 2 * K * n_samples, "input staging");
        if (rc != RFA_OK) return rc;
        float *d_re = f->d_in, *d_im = f->d_in + K * n_samples;
        const size_t row = n_samples * sizeof(float), pitch = (K > 1 ? channel_stride : n_samples) * sizeof(float);
        STAGE_HIP(f, hipMemcpy2DAsync(d_re, row, re, pitch, row, K, hipMemcpyHostToDevice, f->stream));
        STAGE_HIP(f, hipMemcpy2DAsync(d_im, row, im, pitch, row, K, hipMemcpyHostToDevice, f->stream));
        rc = rfa_freq_process(f, d_re, d_im, n_samples, n_samples);
    }
    if (rc != RFA_OK) return rc;
    return rfa_freq_collect(f, r1_re, r1_im, terms);
}

int rfa_freq_set_stream(rfa_freq *f, void *stream) { return stage_set_stream(f, stream); }

int rfa_freq_get_stream(const rfa_freq *f, void **stream) { return stage_get_stream(f, stream); }

int rfa_freq_synchronize(rfa_freq *f) { return stage_synchronize(f); }

}  // extern "C"
