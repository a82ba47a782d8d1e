// audio_fir.hip -- a real FIR on every bank slot's audio row (rfa_audio_fir_*): what follows the
// demodulator bank, e.g. the 300 Hz high-pass that takes a CTCSS tone out of the voice.
//
// Definition.  Slot k with taps t[0 ... T-1] and n inputs x[0 ... n-1] writes
//     y[i] = (((+0.0f + t[0] * x[i]) + t[1] * x[i-1]) + ... + t[T-1] * x[i-T+1])
// every product and every sum rounded to float32, in this order, nothing contracted -- the
// reference's real FIR (dsp/FirFilter.kt:121-163) summed from the newest sample on.  T = 0 copies
// the row bit for bit.  x[j], j < 0, is the slot's history: its last kHist = MAX_TAPS - 1 inputs,
// whatever T is, zeros at first.
//
// Kernel.  One workgroup per (slot, tile of kTile outputs), one grid for all slots; a workgroup
// whose tile its slot does not have returns at once.  The tile's inputs and T-1 samples before
// them are staged in LDS once (from the row, or from the history where the row has not begun),
// the taps beside them.  A thread keeps R consecutive outputs in registers and walks the taps in
// steps of U: one vector read of U taps -- every lane at one address, a broadcast -- and one
// vector read of the U samples that enter its window feed R * U multiplies and R * U adds in R
// independent chains.  The window lives in a register ring of R + U entries whose phase is a
// template parameter, so nothing is moved.  LDS image: lx[pad + (T-1) + o - j] is the sample
// that tap j of output o meets, pad = (-T) mod 4, which makes every vector read aligned.  v_pk_mul_f32
// and v_pk_add_f32 are IEEE per lane: the compiler may pair adjacent outputs without changing a bit.
//     wide   (n > kNarrowMax): R = 8, U = 4 (ds_read_b128)
//     narrow (n <= kNarrowMax): R = 2, U = 2 (ds_read_b64): four times the threads for a short row,
//            whose cost is the latency of one wave's T dependent additions, not throughput
//
// History.  Two buffers per slot; a call reads buffer cur_k and the workgroup of tile 0 writes
// the other one -- the last kHist samples of (history ++ inputs), hist_source() below -- so no
// tile can meet a history that this call has already advanced, in one launch.  The host flips
// cur_k for the slots that had samples.
//
// Records.  A call's counts, tap counts and cur_k are staged in a ring of kRecRing pinned entries
// with an event behind each copy, as rfa_tone_process stages its records.  Taps are uploaded by
// rfa_audio_fir_set_taps through one pinned stage on the handle's stream: calls enqueued before
// it read the old taps, calls after it the new ones.  The stage is one: a set_taps waits for the
// event behind the previous upload, so the second of two set_taps behind queued calls waits until
// those calls and the first upload are done -- a run of them drains the stream.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

#include "audio_hist.h"
#include "stage_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kMaxTaps = RFA_AUDIO_FIR_MAX_TAPS;
constexpr int kHist = kAudioHist;               // hist_source(), audio_hist.h
constexpr int kTile = RFA_AUDIO_FIR_TILE;
constexpr int kNarrowMax = RFA_AUDIO_FIR_NARROW_MAX;
constexpr int kThreads = 256;
constexpr int kWideR = 8, kNarrowR = 2;
constexpr int kSlack = 16;             // floats behind the staged samples that a window may read and not use
constexpr int kRecRing = 8;
constexpr size_t kMaxCount = (size_t)1 << 36;

static_assert(kHist == kMaxTaps - 1, "the history holds what the longest filter reaches back");
static_assert(kThreads * kWideR == kTile && kThreads * kNarrowR == kNarrowMax, "a thread's outputs fill the tile");

struct FirSlot {
    long long n;                       // this call's samples
    int taps;                          // T
    int cur;                           // the history buffer this call reads (it writes the other one)
};

inline int round4(int v) { return (v + 3) & ~3; }

// Floats of LDS for taps and for samples of a launch whose longest filter has max_taps taps and
// whose longest row has max_n samples.
inline int lds_tap_floats(int max_taps) { return round4(max_taps); }
inline int lds_sample_floats(int max_taps, size_t max_n) {
    return round4((int)std::min(max_n, (size_t)kTile) + max_taps + kSlack);
}

template <int U> struct VecOf;
template <> struct VecOf<2> { typedef float type __attribute__((ext_vector_type(2))); };
template <> struct VecOf<4> { typedef float type __attribute__((ext_vector_type(4))); };

// U taps at tp against the window: ring entry (i + N - U * P) % N holds window sample i, i = 0 the
// oldest; xs points at the U samples that enter.  Per output the taps are added in rising order.
template <int R, int U, int P>
__device__ __forceinline__ void fir_step(float (&w)[R + U], float (&acc)[R], const float *xs, const float *tp) {
    constexpr int N = R + U, ROT = (N - U * P) % N;
    using V = typename VecOf<U>::type;
    const V nw = *reinterpret_cast<const V *>(xs);
    const V t = *reinterpret_cast<const V *>(tp);
#pragma unroll
    for (int u = 0; u < U; u++) w[(u + ROT) % N] = nw[u];
#pragma unroll
    for (int u = 0; u < U; u++)
#pragma unroll
        for (int r = 0; r < R; r++) {
            const float p = t[u] * w[(U - 1 + r - u + ROT) % N];
            acc[r] = acc[r] + p;
        }
}

template <int R, int U, int P = 0>
__device__ __forceinline__ void fir_round(float (&w)[R + U], float (&acc)[R], const float *xs, const float *tp) {
    if constexpr (P < (R + U) / U) {
        fir_step<R, U, P>(w, acc, xs - P * U, tp + P * U);
        fir_round<R, U, P + 1>(w, acc, xs, tp);
    }
}

template <int R, int U, int P = 0>
__device__ __forceinline__ void fir_tail(float (&w)[R + U], float (&acc)[R], const float *xs, const float *tp,
                                         int left) {
    if constexpr (P + 1 < (R + U) / U) {
        if (left > P) {
            fir_step<R, U, P>(w, acc, xs - P * U, tp + P * U);
            fir_tail<R, U, P + 1>(w, acc, xs, tp, left);
        }
    }
}

// This thread's R outputs of a tile of m, from the LDS image.
template <int R, int U>
__device__ __forceinline__ void fir_outputs(const float *lt, const float *lx, int T, int pad, int m, float *y) {
    constexpr int N = R + U, PERIOD = N / U;
    using V = typename VecOf<U>::type;
    static_assert(R % U == 0, "a thread's window begins on a vector");
    const int o0 = (int)threadIdx.x * R;
    if (o0 >= m) return;
    float acc[R], w[N];
#pragma unroll
    for (int r = 0; r < R; r++) acc[r] = 0.0f;
    const int c0 = o0 + pad + T - 1;                       // lx[c0 + r - j]: tap j of output o0 + r
#pragma unroll
    for (int v = 1; v < PERIOD; v++) {                      // window samples U ... N-1 of the first step
        const V x = *reinterpret_cast<const V *>(lx + c0 + 1 + (v - 1) * U);
#pragma unroll
        for (int u = 0; u < U; u++) w[v * U + u] = x[u];
    }
    const int G = T / U;
    const float *xs = lx + c0 - (U - 1);
    int g = 0;
    for (; g + PERIOD <= G; g += PERIOD) fir_round<R, U>(w, acc, xs - g * U, lt + g * U);
    fir_tail<R, U>(w, acc, xs - g * U, lt + g * U, G - g);
    for (int j = G * U; j < T; j++) {                       // T mod U taps
        const float tap = lt[j];
#pragma unroll
        for (int r = 0; r < R; r++) {
            const float p = tap * lx[c0 + r - j];
            acc[r] = acc[r] + p;
        }
    }
#pragma unroll
    for (int r = 0; r < R; r++)
        if (o0 + r < m) y[o0 + r] = acc[r];
}

// grid (tiles of the longest row, K).  taps [K][kMaxTaps]; hist [2][K][kHist]; x_off: floats of
// LDS before the samples.
__global__ __launch_bounds__(kThreads) void audio_fir_kernel(const float *__restrict__ in, size_t in_stride,
                                                            float *__restrict__ out, size_t out_stride,
                                                            const FirSlot *__restrict__ slots,
                                                            const float *__restrict__ taps, float *hist, int K,
                                                            int x_off) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const size_t k = blockIdx.y;
    const FirSlot s = slots[k];
    const long long start = (long long)blockIdx.x * kTile;
    if (start >= s.n) return;
    const int m = s.n - start < kTile ? (int)(s.n - start) : kTile;
    const int T = s.taps;
    const float *x = in + k * in_stride;
    const float *h_old = hist + ((size_t)s.cur * (size_t)K + k) * kHist;
    float *h_new = hist + ((size_t)(s.cur ^ 1) * (size_t)K + k) * kHist;
    const int tid = (int)threadIdx.x;

    if (T == 0) {                                          // the bits as they are
        const unsigned *xb = reinterpret_cast<const unsigned *>(x + start);
        unsigned *yb = reinterpret_cast<unsigned *>(out + k * out_stride + start);
        for (int i = tid; i < m; i += kThreads) yb[i] = xb[i];
    } else {
        float *lt = lds, *lx = lds + x_off;
        const int pad = (4 - (T & 3)) & 3;
        const int staged = pad + T - 1 + m, lim = pad + T + m + 12;
        const float *tk = taps + k * kMaxTaps;
        for (int j = tid; j < T; j += kThreads) lt[j] = tk[j];
        for (int q = tid; q < lim; q += kThreads) {
            const long long g = start + q - pad - (T - 1);
            float v = 0.0f;
            if (q < staged) {
                if (g >= 0) v = x[g];
                else if (g >= -(long long)kHist) v = h_old[kHist + g];
            }
            lx[q] = v;
        }
        __syncthreads();
        float *y = out + k * out_stride + start;
        if (s.n <= kNarrowMax) fir_outputs<kNarrowR, 2>(lt, lx, T, pad, m, y);
        else fir_outputs<kWideR, 4>(lt, lx, T, pad, m, y);
    }

    if (blockIdx.x == 0) {                                 // the slot's history after this call
        const unsigned *xb = reinterpret_cast<const unsigned *>(x);
        const unsigned *hb = reinterpret_cast<const unsigned *>(h_old);
        unsigned *nb = reinterpret_cast<unsigned *>(h_new);
        for (int j = tid; j < kHist; j += kThreads) {
            unsigned long long idx;
            nb[j] = hist_source((unsigned long long)s.n, j, idx) ? xb[idx] : hb[idx];
        }
    }
}

}  // namespace

struct rfa_audio_fir : StageCore {
    int K = 0;
    std::vector<std::vector<float>> taps;  // [K], the host's copy
    std::vector<int> cur;                  // [K], the buffer that holds the slot's history
    float *d_taps = nullptr;               // [K][kMaxTaps]
    float *d_hist = nullptr;               // [2][K][kHist]
    float *h_tap_stage = nullptr;          // pinned, [kMaxTaps]: one upload in flight
    hipEvent_t tap_ev = nullptr;
    bool tap_ev_used = false;
    FirSlot *d_recs = nullptr;             // [K]
    FirSlot *h_recs = nullptr;             // pinned, [kRecRing][K]
    hipEvent_t ev[kRecRing] = {};
    bool ev_used[kRecRing] = {};
    int ring_at = 0;
    float *d_in = nullptr, *d_out = nullptr;   // rfa_audio_fir_process_host's rows
    size_t d_in_cap = 0, d_out_cap = 0;
};

namespace {

bool ranges_overlap(const float *a, size_t na, const float *b, size_t nb) {
    const uintptr_t a0 = (uintptr_t)a, a1 = a0 + na * sizeof(float), b0 = (uintptr_t)b, b1 = b0 + nb * sizeof(float);
    return na && nb && a0 < b1 && b0 < a1;
}

// The checks of a call that come before the rows are looked at; max_n is the largest count.
int af_check_counts(rfa_audio_fir *f, const size_t *n_audio, size_t in_stride, size_t out_stride, size_t &max_n) {
    max_n = 0;
    if (!n_audio) return stage_fail(f, RFA_ERR_INVALID, "null count array");
    if (in_stride > (size_t)1 << 40 || out_stride > (size_t)1 << 40)
        return stage_fail(f, RFA_ERR_INVALID, "stride too large");
    for (int k = 0; k < f->K; k++) {
        if (n_audio[k] > kMaxCount) return stage_fail(f, RFA_ERR_INVALID, "count too large");
        if (f->K > 1 && (n_audio[k] > in_stride || n_audio[k] > out_stride))
            return stage_fail(f, RFA_ERR_INVALID, "a count above a stride");
        max_n = std::max(max_n, n_audio[k]);
    }
    return RFA_OK;
}

int af_check_rows(rfa_audio_fir *f, const float *in, size_t in_stride, const size_t *n_audio, const float *out,
                  size_t out_stride, size_t max_n) {
    if (max_n == 0) return RFA_OK;
    if (!in || !out) return stage_fail(f, RFA_ERR_INVALID, "null row");
    const size_t K = (size_t)f->K;
    // the whole spans first: apart in every steady-state call
    if (!ranges_overlap(in, (K - 1) * in_stride + max_n, out, (K - 1) * out_stride + max_n)) return RFA_OK;
    for (size_t a = 0; a < K; a++)
        for (size_t b = 0; b < K; b++)
            if (ranges_overlap(in + a * in_stride, n_audio[a], out + b * out_stride, n_audio[b]))
                return stage_fail(f, RFA_ERR_INVALID, "input and output rows overlap");
    return RFA_OK;
}

}  // namespace

extern "C" {

int rfa_audio_fir_plan(int32_t num_taps, size_t n, int32_t *plan) {
    if (!plan || num_taps < 0 || num_taps > kMaxTaps || n > kMaxCount) return RFA_ERR_INVALID;
    const bool work = n > 0 && num_taps > 0;
    plan[0] = kTile;
    plan[1] = work ? (int32_t)((lds_tap_floats(num_taps) + lds_sample_floats(num_taps, n)) * sizeof(float)) : 0;
    plan[2] = n == 0          ? RFA_AUDIO_FIR_PATH_NONE
              : num_taps == 0 ? RFA_AUDIO_FIR_PATH_COPY
              : n <= (size_t)kNarrowMax ? RFA_AUDIO_FIR_PATH_NARROW
                                        : RFA_AUDIO_FIR_PATH_WIDE;
    plan[3] = !work ? 0 : n <= (size_t)kNarrowMax ? kNarrowR : kWideR;
    plan[4] = (int32_t)((n + kTile - 1) / kTile);
    return RFA_OK;
}

int rfa_audio_fir_history_source(size_t n, int32_t j, int32_t *from_input, size_t *index) {
    if (!from_input || !index || j < 0 || j >= kHist || n > kMaxCount) return RFA_ERR_INVALID;
    unsigned long long idx = 0;
    *from_input = hist_source((unsigned long long)n, j, idx) ? 1 : 0;
    *index = (size_t)idx;
    return RFA_OK;
}

int rfa_audio_fir_create(int device, int32_t n_channels, rfa_audio_fir **out) {
    if (!out) return RFA_ERR_INVALID;
    *out = nullptr;
    if (n_channels < 1 || n_channels > RFA_AUDIO_FIR_MAX_CHANNELS) return RFA_ERR_INVALID;
    int rc = stage_check_device(device);
    if (rc != RFA_OK) return rc;
    rfa_audio_fir *f = new (std::nothrow) rfa_audio_fir();
    if (!f) return RFA_ERR_NOMEM;
    const size_t K = (size_t)n_channels;
    f->device = device;
    f->K = n_channels;
    f->taps.resize(K);
    f->cur.assign(K, 0);
    rc = stage_open(f, device);
    if (rc == RFA_OK && (hipMalloc(&f->d_taps, K * kMaxTaps * sizeof(float)) != hipSuccess ||
                         hipMalloc(&f->d_hist, 2 * K * kHist * sizeof(float)) != hipSuccess ||
                         hipMalloc(&f->d_recs, K * sizeof(FirSlot)) != hipSuccess ||
                         hipHostMalloc(&f->h_tap_stage, kMaxTaps * sizeof(float), hipHostMallocDefault) != hipSuccess ||
                         hipHostMalloc(&f->h_recs, kRecRing * K * sizeof(FirSlot), hipHostMallocDefault) != hipSuccess))
        rc = RFA_ERR_NOMEM;
    if (rc == RFA_OK && hipEventCreateWithFlags(&f->tap_ev, hipEventDisableTiming) != hipSuccess) rc = RFA_ERR_HIP;
    for (int e = 0; rc == RFA_OK && e < kRecRing; e++)
        if (hipEventCreateWithFlags(&f->ev[e], hipEventDisableTiming) != hipSuccess) rc = RFA_ERR_HIP;
    if (rc == RFA_OK && hipMemsetAsync(f->d_hist, 0, 2 * K * kHist * sizeof(float), f->stream) != hipSuccess)
        rc = RFA_ERR_HIP;
    if (rc != RFA_OK) {
        rfa_audio_fir_destroy(f);
        return rc;
    }
    *out = f;
    return RFA_OK;
}

int rfa_audio_fir_destroy(rfa_audio_fir *f) {
    if (!f) return RFA_ERR_INVALID;
    stage_close_stream(f);
    if (f->d_taps) (void)hipFree(f->d_taps);
    if (f->d_hist) (void)hipFree(f->d_hist);
    if (f->d_recs) (void)hipFree(f->d_recs);
    if (f->d_in) (void)hipFree(f->d_in);
    if (f->d_out) (void)hipFree(f->d_out);
    if (f->h_tap_stage) (void)hipHostFree(f->h_tap_stage);
    if (f->h_recs) (void)hipHostFree(f->h_recs);
    if (f->tap_ev) (void)hipEventDestroy(f->tap_ev);
    for (hipEvent_t e : f->ev)
        if (e) (void)hipEventDestroy(e);
    delete f;
    return RFA_OK;
}

const char *rfa_audio_fir_last_error(const rfa_audio_fir *f) { return stage_last_error(f); }

int rfa_audio_fir_get_channels(const rfa_audio_fir *f, int32_t *n_channels) {
    if (!f || !n_channels) return RFA_ERR_INVALID;
    *n_channels = f->K;
    return RFA_OK;
}

int rfa_audio_fir_set_taps(rfa_audio_fir *f, int32_t k, const float *taps, int32_t num_taps) {
    if (!f) return RFA_ERR_INVALID;
    if (k < 0 || k >= f->K) return stage_fail(f, RFA_ERR_INVALID, "no such slot");
    if (num_taps < 0 || num_taps > kMaxTaps) return stage_fail(f, RFA_ERR_INVALID, "tap count outside 0 ... 4096");
    if (num_taps && !taps) return stage_fail(f, RFA_ERR_INVALID, "null taps");
    for (int j = 0; j < num_taps; j++)
        if (!std::isfinite(taps[j])) return stage_fail(f, RFA_ERR_INVALID, "a tap is not finite");
    if (num_taps) {
        STAGE_HIP(f, hipSetDevice(f->device));
        if (f->tap_ev_used) STAGE_HIP(f, hipEventSynchronize(f->tap_ev));      // the stage's previous upload is over
        std::memcpy(f->h_tap_stage, taps, (size_t)num_taps * sizeof(float));
        STAGE_HIP(f, hipMemcpyAsync(f->d_taps + (size_t)k * kMaxTaps, f->h_tap_stage, (size_t)num_taps * sizeof(float),
                                    hipMemcpyHostToDevice, f->stream));
        STAGE_HIP(f, hipEventRecord(f->tap_ev, f->stream));
        f->tap_ev_used = true;
    }
    f->taps[(size_t)k].assign(taps, taps + num_taps);
    return RFA_OK;
}

int rfa_audio_fir_get_taps(const rfa_audio_fir *f, int32_t k, float *taps, size_t capacity, int32_t *num_taps) {
    if (!f || !num_taps || k < 0 || k >= f->K) return RFA_ERR_INVALID;
    const std::vector<float> &t = f->taps[(size_t)k];
    *num_taps = (int32_t)t.size();
    if (taps && capacity >= t.size() && !t.empty()) std::memcpy(taps, t.data(), t.size() * sizeof(float));
    return RFA_OK;
}

int rfa_audio_fir_reset(rfa_audio_fir *f, int32_t k) {
    if (!f) return RFA_ERR_INVALID;
    if (k < -1 || k >= f->K) return stage_fail(f, RFA_ERR_INVALID, "no such slot");
    STAGE_HIP(f, hipSetDevice(f->device));
    const size_t K = (size_t)f->K;
    if (k < 0) {
        STAGE_HIP(f, hipMemsetAsync(f->d_hist, 0, 2 * K * kHist * sizeof(float), f->stream));
    } else {
        float *h = f->d_hist + ((size_t)f->cur[(size_t)k] * K + (size_t)k) * kHist;
        STAGE_HIP(f, hipMemsetAsync(h, 0, kHist * sizeof(float), f->stream));
    }
    return RFA_OK;
}

int rfa_audio_fir_process(rfa_audio_fir *f, const float *in, size_t in_stride, const size_t *n_audio, float *out,
                          size_t out_stride) {
    if (!f) return RFA_ERR_INVALID;
    size_t max_n = 0;
    int rc = af_check_counts(f, n_audio, in_stride, out_stride, max_n);
    if (rc == RFA_OK) rc = af_check_rows(f, in, in_stride, n_audio, out, out_stride, max_n);
    if (rc != RFA_OK || max_n == 0) return rc;             // no samples: nothing launched, the histories stay
    const size_t K = (size_t)f->K;
    STAGE_HIP(f, hipSetDevice(f->device));
    // this call's records: wait until the ring entry's previous copy has been made
    const int e = f->ring_at;
    if (f->ev_used[e]) STAGE_HIP(f, hipEventSynchronize(f->ev[e]));
    FirSlot *recs = f->h_recs + (size_t)e * K;
    int max_taps = 0;
    for (size_t k = 0; k < K; k++) {
        recs[k] = FirSlot{(long long)n_audio[k], (int)f->taps[k].size(), f->cur[k]};
        if (n_audio[k]) max_taps = std::max(max_taps, recs[k].taps);
    }
    STAGE_HIP(f, hipMemcpyAsync(f->d_recs, recs, K * sizeof(FirSlot), hipMemcpyHostToDevice, f->stream));
    STAGE_HIP(f, hipEventRecord(f->ev[e], f->stream));
    f->ev_used[e] = true;
    f->ring_at = (e + 1) % kRecRing;

    const int x_off = lds_tap_floats(max_taps);
    const size_t lds_bytes = max_taps ? (size_t)(x_off + lds_sample_floats(max_taps, max_n)) * sizeof(float) : 0;
    const dim3 grid((unsigned)((max_n + kTile - 1) / kTile), (unsigned)K);
    hipLaunchKernelGGL(audio_fir_kernel, grid, dim3(kThreads), lds_bytes, f->stream, in, in_stride, out, out_stride,
                       f->d_recs, f->d_taps, f->d_hist, f->K, x_off);
    STAGE_HIP(f, hipGetLastError());
    for (size_t k = 0; k < K; k++)
        if (n_audio[k]) f->cur[k] ^= 1;
    return RFA_OK;
}

int rfa_audio_fir_process_host(rfa_audio_fir *f, const float *in, size_t in_stride, const size_t *n_audio, float *out,
                               size_t out_stride) {
    if (!f) return RFA_ERR_INVALID;
    size_t max_n = 0;
    int rc = af_check_counts(f, n_audio, in_stride, out_stride, max_n);
    if (rc != RFA_OK || max_n == 0) return rc;
    if (!in || !out) return stage_fail(f, RFA_ERR_INVALID, "null row");
    const size_t K = (size_t)f->K;
    STAGE_HIP(f, hipSetDevice(f->device));
    rc = stage_grow(f, f->d_in, f->d_in_cap, K * max_n, "input staging");
    if (rc == RFA_OK) rc = stage_grow(f, f->d_out, f->d_out_cap, K * max_n, "output staging");
    if (rc != RFA_OK) return rc;
    for (size_t k = 0; k < K; k++)                         // row k holds n_audio[k] floats and no more
        if (n_audio[k])
            STAGE_HIP(f, hipMemcpyAsync(f->d_in + k * max_n, in + k * in_stride, n_audio[k] * sizeof(float),
                                        hipMemcpyHostToDevice, f->stream));
    rc = rfa_audio_fir_process(f, f->d_in, max_n, n_audio, f->d_out, max_n);
    if (rc != RFA_OK) return rc;
    for (size_t k = 0; k < K; k++)
        if (n_audio[k])
            STAGE_HIP(f, hipMemcpyAsync(out + k * out_stride, f->d_out + k * max_n, n_audio[k] * sizeof(float),
                                        hipMemcpyDeviceToHost, f->stream));
    STAGE_HIP(f, hipStreamSynchronize(f->stream));
    return RFA_OK;
}

int rfa_audio_fir_set_stream(rfa_audio_fir *f, void *stream) { return stage_set_stream(f, stream); }

int rfa_audio_fir_get_stream(const rfa_audio_fir *f, void **stream) { return stage_get_stream(f, stream); }

int rfa_audio_fir_synchronize(rfa_audio_fir *f) { return stage_synchronize(f); }

}  // extern "C"
