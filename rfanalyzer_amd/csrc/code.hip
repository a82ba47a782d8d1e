// code.hip -- per-slot code meter on the demodulator bank's audio rows (rfa_code_*): what a DCS
// (digital-coded squelch) decoder reads.
//
// DCS is a 134.4 bit/s NRZ word under the voice.  Per slot and call the device sums the quantised
// audio over sub-cells, P = RFA_CODE_SUBCELLS to the bit:
//     s(g) = floor(672 * P * g / (5 * sample_rate))          the sub-cell of the slot's sample g
//     q(a) = llrint((double)a * 2^24)                        0 (and counted as bad) where a is not
//                                                            finite or |a| >= 2^15
//     S[j] = sum of q(a[i]) over the call's samples with s(g0 + i) = j          (int64)
// The host carries the last sub-cell across calls where it is incomplete (rfa_code_merge) and the
// rule correlates cells with the wanted word (demod.CodeRule).  The reference has one channel,
// squelched by hand, and no counterpart of this file.
//
// The sums are exact integers (|q| < 2^39, a sub-cell holds at most 358 samples), so their value
// does not depend on the order of the additions, on the tiling, on K, the stride or the address:
// bit-identical from run to run, and a row cut into calls anywhere gives the sub-cells of the row
// given whole.  No atomics and no doubles past the quantisation.
//
// Kernel.  One launch per call: the grid is (blocks of kBlockCells sub-cells of the slot that
// touches most, K); a workgroup whose slot has no such block returns at once.  The work is cut by
// sub-cells, so none is shared between workgroups or waves: wave w of a workgroup owns 64
// sub-cells and walks their run of samples 64 at a time, coalesced.  The lanes' sub-cell indices
// are non-decreasing, so a segmented inclusive scan over the wave (6 shuffle steps) leaves each
// sub-cell's share of the 64 samples in the last lane of its segment, which adds it to the wave's
// own LDS accumulator -- one lane per accumulator and step, the wave's LDS operations in program
// order.  The sub-cell of a lane is the wave's quotient, one 64-bit division at its first sample,
// plus a 32-bit division of the lane's remainder.
//
// Records.  A call's counters, counts and output offsets are staged through a ring of kRecRing
// pinned entries with an event behind each copy, as tone.hip stages its records.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

#include "stage_common.h"
#include "wave.h"

namespace {

constexpr int kRecRing = 8;
constexpr int kBlockCells = 256;       // sub-cells of one workgroup, 64 to the wave
constexpr int kThreads = 256;
constexpr long long kNum = 672LL * RFA_CODE_SUBCELLS;          // s(g) = kNum * g / (5 * rate)
constexpr long long kMaxG = 1LL << 48;                         // kNum * g < 2^61

static_assert(kBlockCells == kThreads, "one accumulator per thread");

struct CodeSlot {
    long long g0;                      // the slot's counter at sample 0 of this call
    long long n;                       // samples
    long long j0;                      // s(g0)
    long long m;                       // touched sub-cells: s(g0 + n - 1) - j0 + 1, 0 where n = 0
    long long off;                     // of S[j0] in the call's output
};

bool rate_ok(int32_t rate) { return rate >= RFA_CODE_MIN_RATE && rate <= RFA_CODE_MAX_RATE; }

// The one definition of s(g) on the host; 0 <= g <= 2^48.
inline long long subcell(int32_t rate, long long g) { return (kNum * g) / (5LL * rate); }

// The first sample of sub-cell c: the smallest g with s(g) >= c.
__host__ __device__ __forceinline__ long long first_sample(long long c, long long den) {
    return (c * den + (kNum - 1)) / kNum;
}

__device__ __forceinline__ long long quantise(float a, int &bad) {
    if (!(fabsf(a) < 32768.0f)) {      // NaN, inf and |a| >= 2^15
        bad++;
        return 0;
    }
    return llrint((double)a * 16777216.0);                     // the product is exact; ties to even
}

// out: [K * gridDim.x] bad counts per (slot, block), then the sums at each slot's `off`.
__global__ __launch_bounds__(kThreads) void code_subcell_kernel(const float *__restrict__ audio, size_t audio_stride,
                                                               const CodeSlot *__restrict__ slots, unsigned den,
                                                               long long *__restrict__ out_bad,
                                                               long long *__restrict__ out) {
    const CodeSlot s = slots[blockIdx.y];
    const long long cb = (long long)blockIdx.x * kBlockCells;  // the block's first sub-cell, from j0
    if (cb >= s.m) return;                                     // this slot has no such block
    __shared__ long long acc[kBlockCells];
    __shared__ int wave_bad[kThreads / 64];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    acc[tid] = 0;
    __syncthreads();

    const float *__restrict__ row = audio + (size_t)blockIdx.y * audio_stride;
    const long long cw = cb + 64LL * wave;                     // the wave's sub-cells: [c0, c1)
    int bad = 0;
    if (cw < s.m) {
        const long long c0 = s.j0 + cw, c1 = s.j0 + (cw + 64 < s.m ? cw + 64 : s.m);
        long long lo = first_sample(c0, den), hi = first_sample(c1, den);
        if (lo < s.g0) lo = s.g0;
        if (hi > s.g0 + s.n) hi = s.g0 + s.n;
        // kNum * lo = (c0 + qb) * den + rb: one 64-bit division per wave
        const unsigned long long num = (unsigned long long)kNum * (unsigned long long)lo;
        unsigned qb = (unsigned)(num / den - (unsigned long long)c0);
        unsigned rb = (unsigned)(num % den);
        for (long long gb = lo; gb < hi; gb += 64) {
            const long long g = gb + lane;
            const bool valid = g < hi;
            long long v = 0;
            int cell = 64;                                     // past the wave's: a segment of its own
            if (valid) {
                v = quantise(row[g - s.g0], bad);
                cell = (int)(qb + (rb + (unsigned)kNum * (unsigned)lane) / den);  // < den + 64 kNum < 2^32
            }
            // segmented inclusive scan: equal keys are neighbours
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const long long vu = __shfl_up(v, d, 64);
                const int cu = __shfl_up(cell, d, 64);
                if (lane >= d && cu == cell) v += vu;
            }
            const int next = __shfl_down(cell, 1, 64);
            if (valid && (lane == 63 || next != cell) && (unsigned)cell < 64u) acc[64 * wave + cell] += v;
            const unsigned r = rb + (unsigned)kNum * 64u;
            qb += r / den;
            rb = r % den;
        }
    }
    bad = rfa::wave_reduce(bad, [](int a, int b) { return a + b; });
    if (lane == 0) wave_bad[wave] = bad;
    __syncthreads();
    if (tid == 0) {
        long long b = 0;
        for (int w = 0; w < kThreads / 64; w++) b += wave_bad[w];
        out_bad[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = b;
    }
    if (cb + tid < s.m) out[s.off + cb + tid] = acc[tid];
}

}  // namespace

struct rfa_code : StageCore {
    int K = 0;
    int32_t rate = 0;
    std::vector<long long> g;          // [K], every slot's counter
    std::vector<int32_t> carry_valid;  // [K]
    std::vector<int64_t> carry_j, carry_sum;
    std::vector<uint8_t> dropped;      // [K]: a break since the outstanding call was enqueued
    // the outstanding call
    bool outstanding = false;
    std::vector<CodeSlot> call;        // [K]
    size_t grid_x = 0, out_count = 0;  // blocks per slot; int64 values of the call's output
    // the last collected call
    std::vector<int64_t> res_first, res_count, res_bad, res_n;
    std::vector<std::vector<int64_t>> res_sums;
    long long *d_out = nullptr, *h_out = nullptr;
    size_t d_out_cap = 0, h_out_cap = 0;
    float *d_in = nullptr;             // rfa_code_process_host's rows
    size_t d_in_cap = 0;
    CodeSlot *d_recs = nullptr;        // [K]
    CodeSlot *h_recs = nullptr;        // pinned, [kRecRing][K]
    hipEvent_t ev[kRecRing] = {};
    bool ev_used[kRecRing] = {};
    int ring_at = 0;
    hipEvent_t copied = nullptr;
};

namespace {

void cd_zero_results(rfa_code *t) {
    for (int k = 0; k < t->K; k++) {
        t->res_first[(size_t)k] = subcell(t->rate, t->g[(size_t)k]);
        t->res_count[(size_t)k] = t->res_bad[(size_t)k] = t->res_n[(size_t)k] = 0;
        t->res_sums[(size_t)k].clear();
    }
}

// The checks of a call; max_n is the largest count.
int cd_check(rfa_code *t, const float *audio, size_t audio_stride, const size_t *n_audio, size_t &max_n) {
    max_n = 0;
    if (!n_audio) return stage_fail(t, RFA_ERR_INVALID, "null count array");
    if (audio_stride > (size_t)1 << 40) return stage_fail(t, RFA_ERR_INVALID, "audio_stride too large");
    for (int k = 0; k < t->K; k++) {
        if (n_audio[k] > (size_t)1 << 36) return stage_fail(t, RFA_ERR_INVALID, "count too large");
        if (t->K > 1 && n_audio[k] > audio_stride) return stage_fail(t, RFA_ERR_INVALID, "a count above audio_stride");
        if (t->g[(size_t)k] + (long long)n_audio[k] > kMaxG)
            return stage_fail(t, RFA_ERR_INVALID, "a slot's counter would pass 2^48: rfa_code_break");
        max_n = std::max(max_n, n_audio[k]);
    }
    if (max_n && !audio) return stage_fail(t, RFA_ERR_INVALID, "null input");
    return RFA_OK;
}

int cd_hand_out(rfa_code *t, int64_t *first, int64_t *count, int64_t *sums, size_t sums_stride, int64_t *bad,
                int64_t *n) {
    const size_t K = (size_t)t->K;
    if (sums)
        for (size_t k = 0; k < K; k++)
            if ((size_t)t->res_count[k] > sums_stride)
                return stage_fail(t, RFA_ERR_SIZE, "sums_stride below a slot's completed sub-cells");
    for (size_t k = 0; k < K; k++) {
        if (first) first[k] = t->res_first[k];
        if (count) count[k] = t->res_count[k];
        if (bad) bad[k] = t->res_bad[k];
        if (n) n[k] = t->res_n[k];
        if (sums && t->res_count[k])
            std::memcpy(sums + k * sums_stride, t->res_sums[k].data(), (size_t)t->res_count[k] * sizeof(int64_t));
    }
    return RFA_OK;
}

}  // namespace

extern "C" {

int rfa_code_subcell(int32_t sample_rate, int64_t g, int64_t *j) {
    if (!j || !rate_ok(sample_rate) || g < 0 || g > kMaxG) return RFA_ERR_INVALID;
    *j = subcell(sample_rate, g);
    return RFA_OK;
}

int rfa_code_word(int32_t code, uint32_t *word) {
    if (!word || code < 0 || code > 0x1ff) return RFA_ERR_INVALID;
    const uint32_t d = 0x800u | (uint32_t)code;
    uint32_t r = d << 11;                                      // d * x^11 modulo the generator, over GF(2)
    for (int b = 22; b >= 11; b--)
        if (r & (1u << b)) r ^= 0xC75u << (b - 11);
    *word = d | (r << 12);
    return RFA_OK;
}

int rfa_code_merge(int32_t sample_rate, int64_t g_end, int64_t j0, int64_t m, int64_t *sums, int32_t *carry_valid,
                   int64_t *carry_j, int64_t *carry_sum, int64_t *first, int64_t *count) {
    if (!rate_ok(sample_rate) || g_end < 0 || g_end > kMaxG || j0 < 0 || m < 0 || (m && !sums) || !carry_valid ||
        !carry_j || !carry_sum || !first || !count)
        return RFA_ERR_INVALID;
    *first = j0;
    *count = 0;
    if (m == 0) return RFA_OK;                                 // no samples: the carry stays
    if (*carry_valid) {
        if (*carry_j != j0) return RFA_ERR_INVALID;            // a carry is the sub-cell the next sample falls into
        sums[0] = (int64_t)((uint64_t)sums[0] + (uint64_t)*carry_sum);
    }
    const int64_t last = j0 + m - 1;
    if (subcell(sample_rate, g_end) == last) {                 // the next sample still falls into it: hold it back
        *carry_valid = 1;
        *carry_j = last;
        *carry_sum = sums[m - 1];
        *count = m - 1;
    } else {
        *carry_valid = 0;
        *carry_j = *carry_sum = 0;
        *count = m;
    }
    return RFA_OK;
}

int rfa_code_create(int device, int32_t n_channels, int32_t sample_rate, rfa_code **out) {
    if (!out) return RFA_ERR_INVALID;
    *out = nullptr;
    if (n_channels < 1 || n_channels > RFA_CODE_MAX_CHANNELS || !rate_ok(sample_rate)) return RFA_ERR_INVALID;
    int rc = stage_check_device(device);
    if (rc != RFA_OK) return rc;
    rfa_code *t = new (std::nothrow) rfa_code();
    if (!t) return RFA_ERR_NOMEM;
    const size_t K = (size_t)n_channels;
    t->device = device;
    t->K = n_channels;
    t->rate = sample_rate;
    t->g.assign(K, 0);
    t->carry_valid.assign(K, 0);
    t->carry_j.assign(K, 0);
    t->carry_sum.assign(K, 0);
    t->dropped.assign(K, 0);
    t->call.assign(K, CodeSlot{});
    t->res_first.assign(K, 0);
    t->res_count.assign(K, 0);
    t->res_bad.assign(K, 0);
    t->res_n.assign(K, 0);
    t->res_sums.assign(K, {});
    rc = stage_open(t, device);
    if (rc == RFA_OK && (hipMalloc(&t->d_recs, K * sizeof(CodeSlot)) != hipSuccess ||
                         hipHostMalloc(&t->h_recs, kRecRing * K * sizeof(CodeSlot), hipHostMallocDefault) != hipSuccess))
        rc = RFA_ERR_NOMEM;
    for (int e = 0; rc == RFA_OK && e < kRecRing; e++)
        if (hipEventCreateWithFlags(&t->ev[e], hipEventDisableTiming) != hipSuccess) rc = RFA_ERR_HIP;
    if (rc == RFA_OK && hipEventCreateWithFlags(&t->copied, hipEventDisableTiming) != hipSuccess) rc = RFA_ERR_HIP;
    if (rc != RFA_OK) {
        rfa_code_destroy(t);
        return rc;
    }
    *out = t;
    return RFA_OK;
}

int rfa_code_destroy(rfa_code *t) {
    if (!t) return RFA_ERR_INVALID;
    stage_close_stream(t);
    if (t->d_out) (void)hipFree(t->d_out);
    if (t->h_out) (void)hipHostFree(t->h_out);
    if (t->d_in) (void)hipFree(t->d_in);
    if (t->d_recs) (void)hipFree(t->d_recs);
    if (t->h_recs) (void)hipHostFree(t->h_recs);
    for (hipEvent_t e : t->ev)
        if (e) (void)hipEventDestroy(e);
    if (t->copied) (void)hipEventDestroy(t->copied);
    delete t;
    return RFA_OK;
}

const char *rfa_code_last_error(const rfa_code *t) { return stage_last_error(t); }

int rfa_code_get_channels(const rfa_code *t, int32_t *n_channels, int32_t *sample_rate) {
    if (!t || !n_channels) return RFA_ERR_INVALID;
    *n_channels = t->K;
    if (sample_rate) *sample_rate = t->rate;
    return RFA_OK;
}

int rfa_code_break(rfa_code *t, int32_t k) {
    if (!t) return RFA_ERR_INVALID;
    if (k < -1 || k >= t->K) return stage_fail(t, RFA_ERR_INVALID, "no such slot");
    const size_t first = k < 0 ? 0 : (size_t)k, count = k < 0 ? (size_t)t->K : 1;
    for (size_t j = first; j < first + count; j++) {
        t->g[j] = 0;
        t->carry_valid[j] = 0;
        t->carry_j[j] = t->carry_sum[j] = 0;
        if (t->outstanding) t->dropped[j] = 1;                 // that call's sub-cells belong to the stream before
    }
    return RFA_OK;
}

int rfa_code_reset(rfa_code *t) {
    if (!t) return RFA_ERR_INVALID;
    std::fill(t->g.begin(), t->g.end(), 0LL);
    std::fill(t->carry_valid.begin(), t->carry_valid.end(), 0);
    std::fill(t->carry_j.begin(), t->carry_j.end(), (int64_t)0);
    std::fill(t->carry_sum.begin(), t->carry_sum.end(), (int64_t)0);
    std::fill(t->dropped.begin(), t->dropped.end(), (uint8_t)0);
    t->outstanding = false;            // a later copy into h_out is ordered behind this one on the stream
    cd_zero_results(t);
    return RFA_OK;
}

int rfa_code_process(rfa_code *t, const float *audio, size_t audio_stride, const size_t *n_audio) {
    if (!t) return RFA_ERR_INVALID;
    if (t->outstanding) return stage_fail(t, RFA_ERR_STATE, "the previous call has not been collected");
    size_t max_n = 0;
    int rc = cd_check(t, audio, audio_stride, n_audio, max_n);
    if (rc != RFA_OK) return rc;
    if (max_n == 0) {                                          // nothing launched, counters and carries stay
        cd_zero_results(t);
        return RFA_OK;
    }
    const size_t K = (size_t)t->K;
    std::vector<CodeSlot> &call = t->call;
    long long max_m = 0, total = 0;
    for (size_t k = 0; k < K; k++) {
        CodeSlot s{};
        s.g0 = t->g[k];
        s.n = (long long)n_audio[k];
        s.j0 = subcell(t->rate, s.g0);
        s.m = s.n ? subcell(t->rate, s.g0 + s.n - 1) - s.j0 + 1 : 0;
        s.off = total;
        total += s.m;
        max_m = std::max(max_m, s.m);
        call[k] = s;
    }
    const size_t grid_x = (size_t)((max_m + kBlockCells - 1) / kBlockCells);
    const size_t n_bad = K * grid_x, out_count = n_bad + (size_t)total;
    STAGE_HIP(t, hipSetDevice(t->device));
    rc = stage_grow(t, t->d_out, t->d_out_cap, out_count, "sub-cell sums");
    if (rc != RFA_OK) return rc;
    if (out_count > t->h_out_cap) {
        STAGE_HIP(t, hipStreamSynchronize(t->stream));
        if (t->h_out) (void)hipHostFree(t->h_out);
        t->h_out = nullptr;
        t->h_out_cap = 0;
        const size_t want = std::max(out_count, (size_t)4096);
        if (hipHostMalloc(&t->h_out, want * sizeof(long long), hipHostMallocDefault) != hipSuccess)
            return stage_fail(t, RFA_ERR_NOMEM, "hipHostMalloc sub-cell sums");
        t->h_out_cap = want;
    }
    // this call's records: wait until the ring entry's previous copy has been made
    const int e = t->ring_at;
    if (t->ev_used[e]) STAGE_HIP(t, hipEventSynchronize(t->ev[e]));
    CodeSlot *entry = t->h_recs + (size_t)e * K;
    std::memcpy(entry, call.data(), K * sizeof(CodeSlot));
    STAGE_HIP(t, hipMemcpyAsync(t->d_recs, entry, K * sizeof(CodeSlot), hipMemcpyHostToDevice, t->stream));
    STAGE_HIP(t, hipEventRecord(t->ev[e], t->stream));
    t->ev_used[e] = true;
    t->ring_at = (e + 1) % kRecRing;

    hipLaunchKernelGGL(code_subcell_kernel, dim3((unsigned)grid_x, (unsigned)K), dim3(kThreads), 0, t->stream, audio,
                       audio_stride, t->d_recs, (unsigned)(5 * t->rate), t->d_out, t->d_out + n_bad);
    STAGE_HIP(t, hipGetLastError());
    // launched: the slots' counters are those behind this call whatever follows
    for (size_t k = 0; k < K; k++) t->g[k] += call[k].n;
    std::fill(t->dropped.begin(), t->dropped.end(), (uint8_t)0);
    t->grid_x = grid_x;
    t->out_count = out_count;
    t->outstanding = true;
    STAGE_HIP(t, hipMemcpyAsync(t->h_out, t->d_out, out_count * sizeof(long long), hipMemcpyDeviceToHost, t->stream));
    STAGE_HIP(t, hipEventRecord(t->copied, t->stream));
    return RFA_OK;
}

int rfa_code_collect(rfa_code *t, int64_t *first, int64_t *count, int64_t *sums, size_t sums_stride, int64_t *bad,
                     int64_t *n) {
    if (!t) return RFA_ERR_INVALID;
    if (t->outstanding) {
        STAGE_HIP(t, hipSetDevice(t->device));
        STAGE_HIP(t, hipEventSynchronize(t->copied));          // this copy, not what else the stream holds
        t->outstanding = false;
        const size_t K = (size_t)t->K;
        const long long *h_bad = t->h_out, *h_sums = t->h_out + K * t->grid_x;
        for (size_t k = 0; k < K; k++) {
            const CodeSlot &s = t->call[k];
            std::vector<int64_t> &out = t->res_sums[k];
            t->res_n[k] = s.n;
            if (t->dropped[k]) {                               // a break came in between: nothing of it counts
                t->res_first[k] = subcell(t->rate, t->g[k]);
                t->res_count[k] = t->res_bad[k] = t->res_n[k] = 0;
                out.clear();
                continue;
            }
            out.assign(h_sums + s.off, h_sums + s.off + s.m);
            int64_t b = 0;
            const size_t blocks = (size_t)((s.m + kBlockCells - 1) / kBlockCells);
            for (size_t x = 0; x < blocks; x++) b += h_bad[k * t->grid_x + x];
            t->res_bad[k] = b;
            const int rc = rfa_code_merge(t->rate, s.g0 + s.n, s.j0, s.m, out.data(), &t->carry_valid[k],
                                          &t->carry_j[k], &t->carry_sum[k], &t->res_first[k], &t->res_count[k]);
            if (rc != RFA_OK) return stage_fail(t, RFA_ERR_STATE, "a slot's carry does not meet its call");
            out.resize((size_t)t->res_count[k]);
        }
        std::fill(t->dropped.begin(), t->dropped.end(), (uint8_t)0);
    }
    return cd_hand_out(t, first, count, sums, sums_stride, bad, n);
}

int rfa_code_process_host(rfa_code *t, const float *audio, size_t audio_stride, const size_t *n_audio, int64_t *first,
                          int64_t *count, int64_t *sums, size_t sums_stride, int64_t *bad, int64_t *n) {
    if (!t) return RFA_ERR_INVALID;
    if (t->outstanding) return stage_fail(t, RFA_ERR_STATE, "the previous call has not been collected");
    size_t max_n = 0;
    int rc = cd_check(t, audio, audio_stride, n_audio, max_n);
    if (rc != RFA_OK) return rc;
    if (max_n == 0) {
        rc = rfa_code_process(t, nullptr, 0, n_audio);
    } else {
        const size_t K = (size_t)t->K;
        STAGE_HIP(t, hipSetDevice(t->device));
        rc = stage_grow(t, t->d_in, t->d_in_cap, K * max_n, "input staging");
        if (rc != RFA_OK) return rc;
        for (size_t k = 0; k < K; k++)                         // row k holds n_audio[k] floats and no more
            if (n_audio[k])
                STAGE_HIP(t, hipMemcpyAsync(t->d_in + k * max_n, audio + k * audio_stride, n_audio[k] * sizeof(float),
                                            hipMemcpyHostToDevice, t->stream));
        rc = rfa_code_process(t, t->d_in, max_n, n_audio);
    }
    if (rc != RFA_OK) return rc;
    return rfa_code_collect(t, first, count, sums, sums_stride, bad, n);
}

int rfa_code_set_stream(rfa_code *t, void *stream) { return stage_set_stream(t, stream); }

int rfa_code_get_stream(const rfa_code *t, void **stream) { return stage_get_stream(t, stream); }

int rfa_code_synchronize(rfa_code *t) { return stage_synchronize(t); }

}  // extern "C"
