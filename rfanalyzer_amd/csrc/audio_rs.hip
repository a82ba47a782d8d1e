// audio_rs.hip -- every bank slot's audio row resampled by one rational ratio L / D and written as
// int16 PCM, float32 or both (rfa_audio_rs_*): what follows the audio FIR, e.g. 48 kHz float to the
// 8 kHz s16 of a voice logger.
//
// Definition.  Handle constants: L and D with 1 <= L <= 160, L <= D <= 1024, gcd(L, D) = 1; taps
// h[0 ... T-1], finite, T <= 16384, J = ceil(T / L) with 1 <= J <= 4096; L = D = 1 may have T = 0.
// Per slot: a history of its last kAudioHist = 4095 inputs, zeros at first, and an offset r,
// 0 <= r < D, on the host, 0 at first: where the slot's next output lies relative to the next input
// it will receive, in ticks of the rate L * f_in.  A call gives slot k n inputs x[0 ... n-1]; its
// outputs are m = 0, 1, ... while r + m * D < n * L.  Output m has u = r + m * D, i = floor(u / L),
// p = u mod L and
//     y = (((+0.0f + h[p] * x[i]) + h[p+L] * x[i-1]) + ... + h[p+(J-1)L] * x[i-J+1])
// taps at or beyond T counting as +0.0f and still multiplied and added, every product and every sum
// rounded to float32 in this order, nothing contracted; x[j], j < 0, is the history.  Afterwards
// r <- r + n_out * D - n * L and the history advances by n; a slot with n = 0 keeps everything.  So
// n_out = ceil((n * L - r) / D) for n * L > r, else 0 (rs_counts), a stream cut into calls anywhere
// gives the bits and the count of the stream given whole, and T = 0 gives y = x bitwise.
// PCM (pcm_of): v = y * 32768.0f; NaN -> 0; v >= 32767 -> 32767; v <= -32768 -> -32768; otherwise
// (int16_t)rintf(v), ties to even.
//
// Kernel.  One grid of (output tiles of the longest row, K) workgroups of 256 threads; a workgroup
// whose slot lacks its tile returns at once.  The tile is fixed per handle (rs_geom): 1024 outputs,
// halved until the tile's inputs and the taps fit the LDS.  The tile's input span -- from J - 1
// samples before its first output's input to its last output's input -- is staged once, from the row
// or, before the row begins, from the history; the taps beside it in phase-major order,
// g[p][j] = h[p + j L].  Thread t computes outputs t, t + 256, ... of the tile in independent chains.
//     convert  (T = 0)  no LDS: the conversion of the row
//     decimate (L = 1)  all outputs share the one tap row, read at one address by every lane (a
//                       broadcast).  Adjacent outputs' windows are D samples apart, so the samples are
//                       staged de-interleaved by D: sample q at lx[(q mod D) * rs + q / D].  Tap j of
//                       output o meets q = o D + (J - 1 - j): one residue row for all lanes and
//                       consecutive addresses across lanes -- no bank conflict at any D.
//     polyphase (L > 1) output o reads its own phase row g[p_o] (row stride J | 1, odd, so that
//                       different phases start on different banks) against samples in natural order.
// The workgroup of tile 0 writes the slot's new history into the buffer the call does not read
// (hist_source, audio_hist.h), also where the slot has inputs and no output.  int16 results are
// stored one sample per lane: any 2-byte-aligned row works.
//
// Records.  A call's counts, offsets and history buffers are staged in a ring of kRecRing pinned
// entries with an event behind each copy, as rfa_audio_fir_process stages its records.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>
#include <numeric>
#include <vector>

#include "audio_hist.h"
#include "stage_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kHist = kAudioHist;
constexpr int kMaxTile = RFA_AUDIO_RS_MAX_TILE;
constexpr int kThreads = 256;
constexpr int kMaxR = kMaxTile / kThreads;                 // outputs per thread, at most
constexpr int kRecRing = 8;
constexpr size_t kMaxCount = (size_t)1 << 36;
constexpr int kLdsFloats = 16384;                          // 64 KiB: what a launch gets without asking
constexpr int kLdsMaxFloats = 40000;                       // below the CU's 160 KiB: a launch that asked for it
constexpr int kMinPlainTile = 64;                          // a handle whose tile of this size fits 64 KiB stays in them

static_assert(kHist == RFA_AUDIO_RS_HISTORY && kHist >= RFA_AUDIO_RS_MAX_PHASE_TAPS - 1,
              "the history holds what the longest phase reaches back");
static_assert(kMaxTile % kThreads == 0 && kMaxR == 4, "rs_tile dispatches 1, 2 or 4 outputs per thread");

struct RsSlot {
    long long n;                       // this call's inputs
    long long n_out;                   // ... and outputs
    int r;                             // the offset the call starts at
    int cur;                           // the history buffer this call reads (it writes the other one)
};

inline int round4(int v) { return (v + 3) & ~3; }

__host__ __device__ inline int16_t pcm_of(float y) {
    const float v = y * 32768.0f;
    if (v != v) return 0;
    if (v >= 32767.0f) return 32767;
    if (v <= -32768.0f) return -32768;
    return (int16_t)rintf(v);
}

bool rs_ratio_ok(int L, int D) {
    return L >= 1 && L <= RFA_AUDIO_RS_MAX_L && D >= L && D <= RFA_AUDIO_RS_MAX_D && std::gcd(L, D) == 1;
}

bool rs_shape_ok(int L, int D, int T) {
    if (!rs_ratio_ok(L, D) || T < 0 || T > RFA_AUDIO_RS_MAX_TAPS) return false;
    if (T == 0) return L == 1 && D == 1;
    return (T + L - 1) / L <= RFA_AUDIO_RS_MAX_PHASE_TAPS;
}

// The call rule.  n * L < 2^44 and n_out * D < 2^44 + 2^10 for n up to 2^36.
void rs_counts(int L, int D, int r, unsigned long long n, unsigned long long &n_out, int &r_next) {
    const unsigned long long ticks = n * (unsigned long long)L;
    n_out = ticks > (unsigned long long)r ? (ticks - (unsigned long long)r + (unsigned long long)D - 1) / (unsigned long long)D : 0;
    r_next = (int)((unsigned long long)r + n_out * (unsigned long long)D - ticks);
}

// What is fixed per handle: taps per phase, the tap image's row stride, the output tile and the LDS
// image.  Samples of a tile: from J - 1 before the first output's input to the last output's input.
struct RsGeom {
    int J = 0, Jp = 0;                 // taps per phase; floats between phase rows of the tap image
    int tile = kMaxTile;
    int tap_floats = 0;                // LDS floats before the samples
    int span = 0;                      // samples a full tile stages, at most
    int rs = 0;                        // decimate: floats between residue rows of the sample image
    int x_floats = 0;                  // LDS floats of the sample image
    int lds_floats() const { return tap_floats + x_floats; }
};

RsGeom rs_geom_at(int L, int D, int T, int tile) {
    RsGeom g;
    g.J = (T + L - 1) / L;
    g.tile = tile;
    if (T == 0) return g;
    g.Jp = L == 1 ? g.J : (g.J | 1);
    g.tap_floats = round4(L == 1 ? g.J : L * g.Jp);
    g.span = (int)(((long long)(L - 1) + (long long)(tile - 1) * D) / L) + g.J;
    if (L == 1) {
        g.rs = (g.span + D - 1) / D + 1;
        g.x_floats = round4(D * g.rs);
    } else {
        g.x_floats = round4(g.span);
    }
    return g;
}

RsGeom rs_geom(int L, int D, int T) {
    // 64 KiB where a tile of kMinPlainTile fits them, else what a launch may ask for
    const int budget = rs_geom_at(L, D, T, kMinPlainTile).lds_floats() <= kLdsFloats ? kLdsFloats : kLdsMaxFloats;
    int tile = kMaxTile;
    RsGeom g = rs_geom_at(L, D, T, tile);
    while (g.lds_floats() > budget && tile > 1) g = rs_geom_at(L, D, T, tile /= 2);
    return g;
}

struct RsArgs {
    const float *in;
    size_t in_stride;
    float *out_f32;
    size_t f32_stride;
    int16_t *out_s16;
    size_t s16_stride;
    const RsSlot *slots;
    const float *g;                    // [L][Jp] phase-major taps, zeros beyond T; L = 1: h itself
    float *hist;                       // [2][K][kHist]
    int K, L, D, J, Jp, tile, x_off, rs;
};

__device__ __forceinline__ void rs_store(const RsArgs &a, size_t k, long long at, float y) {
    if (a.out_f32) a.out_f32[k * a.f32_stride + (size_t)at] = y;
    if (a.out_s16) a.out_s16[k * a.s16_stride + (size_t)at] = pcm_of(y);
}

// Outputs tid, tid + 256, ... (R of them) of a tile of m outputs that begins at output m0, input i0
// and phase p0, from the LDS image.  A thread whose output the tile lacks computes the tile's last one
// again and stores nothing: every read stays inside what was staged.
template <int R>
__device__ __forceinline__ void rs_tile(const RsArgs &a, const float *lt, const float *lx, size_t k, long long m0,
                                        int p0, int m) {
    const int tid = (int)threadIdx.x, J = a.J;
    float acc[R];
    int oc[R];
#pragma unroll
    for (int r = 0; r < R; r++) {
        acc[r] = 0.0f;
        oc[r] = tid + r * kThreads < m ? tid + r * kThreads : m - 1;
    }
    if (a.L == 1) {
        // tap j meets sample q = o D + e, e = J - 1 - j: residue row e mod D, place o + e / D
        int e = J - 1;
        int row = e % a.D, at = row * a.rs + e / a.D;
        for (int j = 0; j < J; j++) {
            const float t = lt[j];
#pragma unroll
            for (int r = 0; r < R; r++) {
                const float p = t * lx[at + oc[r]];
                acc[r] = acc[r] + p;
            }
            if (row == 0) {
                row = a.D - 1;
                at += (a.D - 1) * a.rs - 1;
            } else {
                row--;
                at -= a.rs;
            }
        }
    } else {
        const float *tp[R], *xq[R];
#pragma unroll
        for (int r = 0; r < R; r++) {
            const int rel = p0 + oc[r] * a.D;              // below 160 + 1024 * 1024
            tp[r] = lt + (rel % a.L) * a.Jp;
            xq[r] = lx + rel / a.L + (J - 1);               // the output's newest input
        }
        for (int j = 0; j < J; j++) {
#pragma unroll
            for (int r = 0; r < R; r++) {
                const float p = tp[r][j] * xq[r][-j];
                acc[r] = acc[r] + p;
            }
        }
    }
#pragma unroll
    for (int r = 0; r < R; r++)
        if (tid + r * kThreads < m) rs_store(a, k, m0 + tid + r * kThreads, acc[r]);
}

// grid (tiles of the longest output row, K)
__global__ __launch_bounds__(kThreads) void audio_rs_kernel(const RsArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const size_t k = blockIdx.y;
    const RsSlot s = a.slots[k];
    if (s.n == 0) return;
    const long long m0 = (long long)blockIdx.x * a.tile;
    if (m0 >= s.n_out && blockIdx.x != 0) return;
    const int tid = (int)threadIdx.x;
    const float *x = a.in + k * a.in_stride;
    const float *h_old = a.hist + ((size_t)s.cur * (size_t)a.K + k) * kHist;
    float *h_new = a.hist + ((size_t)(s.cur ^ 1) * (size_t)a.K + k) * kHist;

    if (m0 < s.n_out) {
        const int m = s.n_out - m0 < a.tile ? (int)(s.n_out - m0) : a.tile;
        if (a.J == 0) {                                    // no filter: output m is input m
            for (int o = tid; o < m; o += kThreads) {
                const long long at = m0 + o;
                if (a.out_f32)
                    reinterpret_cast<unsigned *>(a.out_f32 + k * a.f32_stride)[at] = reinterpret_cast<const unsigned *>(x)[at];
                if (a.out_s16) a.out_s16[k * a.s16_stride + (size_t)at] = pcm_of(x[at]);
            }
        } else {
            float *lt = lds, *lx = lds + a.x_off;
            const long long u0 = (long long)s.r + m0 * a.D;
            const long long i0 = u0 / a.L;
            const int p0 = (int)(u0 - i0 * a.L);
            const long long first = i0 - (a.J - 1);        // the input staged as sample 0
            const int cnt = (p0 + (m - 1) * a.D) / a.L + a.J;
            const int tap_floats = a.L == 1 ? a.J : a.L * a.Jp;
            for (int j = tid; j < tap_floats; j += kThreads) lt[j] = a.g[j];
            for (int q = tid; q < cnt; q += kThreads) {
                const long long gi = first + q;
                const float v = gi >= 0 ? x[gi] : h_old[kHist + gi];
                lx[a.L == 1 ? (q % a.D) * a.rs + q / a.D : q] = v;
            }
            __syncthreads();
            if (m <= kThreads) rs_tile<1>(a, lt, lx, k, m0, p0, m);
            else if (m <= 2 * kThreads) rs_tile<2>(a, lt, lx, k, m0, p0, m);
            else rs_tile<4>(a, lt, lx, k, m0, p0, m);
        }
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

struct rfa_audio_rs : StageCore {
    int K = 0, L = 1, D = 1;
    std::vector<float> taps;               // h, the host's copy
    RsGeom geom;
    bool big_lds = false;                  // the kernel may be launched with more than 64 KiB of LDS
    std::vector<int> r;                    // [K], every slot's offset
    std::vector<int> cur;                  // [K], the buffer that holds the slot's history
    std::vector<size_t> call_out;          // [K], a call's output counts and
    std::vector<int> call_r;               // ... next offsets: a call allocates nothing
    float *d_g = nullptr;                  // the tap image
    float *d_hist = nullptr;               // [2][K][kHist]
    RsSlot *d_recs = nullptr;              // [K]
    RsSlot *h_recs = nullptr;              // pinned, [kRecRing][K]
    hipEvent_t ev[kRecRing] = {};
    bool ev_used[kRecRing] = {};
    int ring_at = 0;
    float *d_in = nullptr, *d_f32 = nullptr;   // rfa_audio_rs_process_host's rows
    int16_t *d_s16 = nullptr;
    size_t d_in_cap = 0, d_f32_cap = 0, d_s16_cap = 0;
};

namespace {

struct Span {
    uintptr_t lo, hi;
};

Span span_of(const void *p, size_t elems, size_t elem_bytes) { return Span{(uintptr_t)p, (uintptr_t)p + elems * elem_bytes}; }

bool overlap(Span a, Span b) { return a.lo < a.hi && b.lo < b.hi && a.lo < b.hi && b.lo < a.hi; }

// One of a call's three row sets: K rows of count[k] elements, stride elements apart.
struct Rows {
    const void *base;
    size_t stride, elem;
    const size_t *count;
    size_t max_count;
    Span whole(size_t K) const { return span_of(base, base ? (K - 1) * stride + max_count : 0, elem); }
    Span row(size_t k) const { return span_of((const char *)base + k * stride * elem, count[k], elem); }
};

bool rows_overlap(const Rows &a, const Rows &b, size_t K) {
    if (!a.base || !b.base || !overlap(a.whole(K), b.whole(K))) return false;   // apart in every steady-state call
    for (size_t i = 0; i < K; i++)
        for (size_t j = 0; j < K; j++)
            if (overlap(a.row(i), b.row(j))) return true;
    return false;
}

// Everything of a call that is checked before anything is consumed; fills n_out and r_next.
int rs_check(rfa_audio_rs *s, const float *in, size_t in_stride, const size_t *n_audio, const float *out_f32,
             size_t f32_stride, const int16_t *out_s16, size_t s16_stride, std::vector<size_t> &n_out,
             std::vector<int> &r_next, size_t &max_n, size_t &max_out) {
    max_n = max_out = 0;
    if (!n_audio) return stage_fail(s, RFA_ERR_INVALID, "null count array");
    if (in_stride > (size_t)1 << 40 || f32_stride > (size_t)1 << 40 || s16_stride > (size_t)1 << 40)
        return stage_fail(s, RFA_ERR_INVALID, "stride too large");
    const size_t K = (size_t)s->K;
    for (size_t k = 0; k < K; k++) {
        if (n_audio[k] > kMaxCount) return stage_fail(s, RFA_ERR_INVALID, "count too large");
        unsigned long long m = 0;
        rs_counts(s->L, s->D, s->r[k], n_audio[k], m, r_next[k]);
        n_out[k] = (size_t)m;
        if (K > 1 && n_audio[k] > in_stride) return stage_fail(s, RFA_ERR_INVALID, "an input count above in_stride");
        if (K > 1 && ((out_f32 && n_out[k] > f32_stride) || (out_s16 && n_out[k] > s16_stride)))
            return stage_fail(s, RFA_ERR_INVALID, "an output count above an output stride");
        max_n = std::max(max_n, n_audio[k]);
        max_out = std::max(max_out, n_out[k]);
    }
    if (max_n == 0) return RFA_OK;
    if (!in) return stage_fail(s, RFA_ERR_INVALID, "null input row");
    if (!out_f32 && !out_s16) return stage_fail(s, RFA_ERR_INVALID, "both outputs null");
    if (((uintptr_t)in | (uintptr_t)out_f32) & 3u) return stage_fail(s, RFA_ERR_INVALID, "a float row off a 4-byte boundary");
    if ((uintptr_t)out_s16 & 1u) return stage_fail(s, RFA_ERR_INVALID, "the int16 rows off a 2-byte boundary");
    const Rows ri{in, in_stride, sizeof(float), n_audio, max_n};
    const Rows rf{out_f32, f32_stride, sizeof(float), n_out.data(), max_out};
    const Rows rp{out_s16, s16_stride, sizeof(int16_t), n_out.data(), max_out};
    if (rows_overlap(ri, rf, K) || rows_overlap(ri, rp, K))
        return stage_fail(s, RFA_ERR_INVALID, "an output range overlaps the input");
    if (rows_overlap(rf, rp, K)) return stage_fail(s, RFA_ERR_INVALID, "the output ranges overlap");
    return RFA_OK;
}

int rs_path(int L, int T, size_t n) {
    return n == 0 ? RFA_AUDIO_RS_PATH_NONE : T == 0 ? RFA_AUDIO_RS_PATH_CONVERT : L == 1 ? RFA_AUDIO_RS_PATH_DECIMATE
                                                                                         : RFA_AUDIO_RS_PATH_POLYPHASE;
}

// Enqueue one call whose checks have passed.
int rs_launch(rfa_audio_rs *s, const float *in, size_t in_stride, const size_t *n_audio, float *out_f32, size_t f32_stride,
              int16_t *out_s16, size_t s16_stride, const std::vector<size_t> &n_out, const std::vector<int> &r_next,
              size_t max_out) {
    const size_t K = (size_t)s->K;
    const RsGeom &g = s->geom;
    const size_t lds_bytes = (size_t)g.lds_floats() * sizeof(float);
    if (lds_bytes > (size_t)kLdsFloats * sizeof(float) && !s->big_lds)
        return stage_fail(s, RFA_ERR_UNSUPPORTED, "these taps need more LDS than a launch on this device may have");
    STAGE_HIP(s, hipSetDevice(s->device));
    // this call's records: wait until the ring entry's previous copy has been made
    const int e = s->ring_at;
    if (s->ev_used[e]) STAGE_HIP(s, hipEventSynchronize(s->ev[e]));
    RsSlot *recs = s->h_recs + (size_t)e * K;
    for (size_t k = 0; k < K; k++) recs[k] = RsSlot{(long long)n_audio[k], (long long)n_out[k], s->r[k], s->cur[k]};
    STAGE_HIP(s, hipMemcpyAsync(s->d_recs, recs, K * sizeof(RsSlot), hipMemcpyHostToDevice, s->stream));
    STAGE_HIP(s, hipEventRecord(s->ev[e], s->stream));
    s->ev_used[e] = true;
    s->ring_at = (e + 1) % kRecRing;

    const RsArgs a{in, in_stride, out_f32, f32_stride, out_s16, s16_stride, s->d_recs, s->d_g, s->d_hist,
                   s->K, s->L, s->D, g.J, g.Jp, g.tile, g.tap_floats, g.rs};
    const size_t tiles = std::max((max_out + (size_t)g.tile - 1) / (size_t)g.tile, (size_t)1);
    const dim3 grid((unsigned)tiles, (unsigned)K);
    hipLaunchKernelGGL(audio_rs_kernel, grid, dim3(kThreads), lds_bytes, s->stream, a);
    STAGE_HIP(s, hipGetLastError());
    for (size_t k = 0; k < K; k++)
        if (n_audio[k]) {
            s->cur[k] ^= 1;
            s->r[k] = r_next[k];
        }
    return RFA_OK;
}

}  // namespace

extern "C" {

int rfa_audio_rs_counts(int32_t L, int32_t D, int32_t r, size_t n, size_t *n_out, int32_t *r_next) {
    if (!n_out || !r_next || !rs_ratio_ok(L, D) || r < 0 || r >= D || n > kMaxCount) return RFA_ERR_INVALID;
    unsigned long long m = 0;
    int rn = 0;
    rs_counts(L, D, r, n, m, rn);
    *n_out = (size_t)m;
    *r_next = rn;
    return RFA_OK;
}

size_t rfa_audio_rs_max_outputs(int32_t L, int32_t D, size_t n) {
    if (!rs_ratio_ok(L, D) || n > kMaxCount) return 0;
    return (size_t)((n * (unsigned long long)L + (unsigned long long)D - 1) / (unsigned long long)D);
}

int rfa_audio_rs_plan(int32_t L, int32_t D, int32_t num_taps, size_t n, int32_t *plan) {
    if (!plan || !rs_shape_ok(L, D, num_taps) || n > kMaxCount) return RFA_ERR_INVALID;
    const RsGeom g = rs_geom(L, D, num_taps);
    const size_t n_out = rfa_audio_rs_max_outputs(L, D, n);
    const size_t in_tile = std::min(n_out, (size_t)g.tile);
    plan[0] = g.tile;
    plan[1] = n ? (int32_t)(g.lds_floats() * sizeof(float)) : 0;
    plan[2] = rs_path(L, num_taps, n);
    plan[3] = in_tile <= (size_t)kThreads ? (int32_t)(in_tile ? 1 : 0) : in_tile <= 2 * (size_t)kThreads ? 2 : kMaxR;
    plan[4] = (int32_t)std::min((n_out + (size_t)g.tile - 1) / (size_t)g.tile, (size_t)INT32_MAX);
    return RFA_OK;
}

int rfa_audio_rs_create(int device, int32_t n_channels, int32_t L, int32_t D, const float *taps, int32_t num_taps,
                        rfa_audio_rs **out) {
    if (!out) return RFA_ERR_INVALID;
    *out = nullptr;
    if (n_channels < 1 || n_channels > RFA_AUDIO_RS_MAX_CHANNELS || !rs_shape_ok(L, D, num_taps)) return RFA_ERR_INVALID;
    if (num_taps && !taps) return RFA_ERR_INVALID;
    for (int j = 0; j < num_taps; j++)
        if (!std::isfinite(taps[j])) return RFA_ERR_INVALID;
    int rc = stage_check_device(device);
    if (rc != RFA_OK) return rc;
    rfa_audio_rs *s = new (std::nothrow) rfa_audio_rs();
    if (!s) return RFA_ERR_NOMEM;
    const size_t K = (size_t)n_channels;
    s->device = device;
    s->K = n_channels;
    s->L = L;
    s->D = D;
    s->taps.assign(taps, taps + num_taps);
    s->geom = rs_geom(L, D, num_taps);
    s->r.assign(K, 0);
    s->cur.assign(K, 0);
    s->call_out.assign(K, 0);
    s->call_r.assign(K, 0);
    // the tap image: g[p][j] = h[p + j L], zeros beyond T and between J and the row stride
    const RsGeom &g = s->geom;
    std::vector<float> image((size_t)std::max(g.tap_floats, 4), 0.0f);
    for (int t = 0; t < num_taps; t++) image[L == 1 ? (size_t)t : (size_t)(t % L) * (size_t)g.Jp + (size_t)(t / L)] = taps[t];
    rc = stage_open(s, device);
    if (rc == RFA_OK && (hipMalloc(&s->d_g, image.size() * sizeof(float)) != hipSuccess ||
                         hipMalloc(&s->d_hist, 2 * K * kHist * sizeof(float)) != hipSuccess ||
                         hipMalloc(&s->d_recs, K * sizeof(RsSlot)) != hipSuccess ||
                         hipHostMalloc(&s->h_recs, kRecRing * K * sizeof(RsSlot), hipHostMallocDefault) != hipSuccess))
        rc = RFA_ERR_NOMEM;
    for (int e = 0; rc == RFA_OK && e < kRecRing; e++)
        if (hipEventCreateWithFlags(&s->ev[e], hipEventDisableTiming) != hipSuccess) rc = RFA_ERR_HIP;
    if (rc == RFA_OK && (hipMemcpy(s->d_g, image.data(), image.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
                         hipMemsetAsync(s->d_hist, 0, 2 * K * kHist * sizeof(float), s->stream) != hipSuccess))
        rc = RFA_ERR_HIP;
    if (rc == RFA_OK && g.lds_floats() > kLdsFloats) {
        s->big_lds = hipFuncSetAttribute(reinterpret_cast<const void *>(audio_rs_kernel),
                                         hipFuncAttributeMaxDynamicSharedMemorySize,
                                         kLdsMaxFloats * (int)sizeof(float)) == hipSuccess;
        (void)hipGetLastError();
    }
    if (rc != RFA_OK) {
        rfa_audio_rs_destroy(s);
        return rc;
    }
    *out = s;
    return RFA_OK;
}

int rfa_audio_rs_destroy(rfa_audio_rs *s) {
    if (!s) return RFA_ERR_INVALID;
    stage_close_stream(s);
    if (s->d_g) (void)hipFree(s->d_g);
    if (s->d_hist) (void)hipFree(s->d_hist);
    if (s->d_recs) (void)hipFree(s->d_recs);
    if (s->d_in) (void)hipFree(s->d_in);
    if (s->d_f32) (void)hipFree(s->d_f32);
    if (s->d_s16) (void)hipFree(s->d_s16);
    if (s->h_recs) (void)hipHostFree(s->h_recs);
    for (hipEvent_t e : s->ev)
        if (e) (void)hipEventDestroy(e);
    delete s;
    return RFA_OK;
}

const char *rfa_audio_rs_last_error(const rfa_audio_rs *s) { return stage_last_error(s); }

int rfa_audio_rs_get_channels(const rfa_audio_rs *s, int32_t *n_channels) {
    if (!s || !n_channels) return RFA_ERR_INVALID;
    *n_channels = s->K;
    return RFA_OK;
}

int rfa_audio_rs_get_ratio(const rfa_audio_rs *s, int32_t *L, int32_t *D) {
    if (!s || !L || !D) return RFA_ERR_INVALID;
    *L = s->L;
    *D = s->D;
    return RFA_OK;
}

int rfa_audio_rs_get_taps(const rfa_audio_rs *s, float *taps, size_t capacity, int32_t *num_taps) {
    if (!s || !num_taps) return RFA_ERR_INVALID;
    *num_taps = (int32_t)s->taps.size();
    if (taps && capacity >= s->taps.size() && !s->taps.empty())
        std::memcpy(taps, s->taps.data(), s->taps.size() * sizeof(float));
    return RFA_OK;
}

int rfa_audio_rs_reset(rfa_audio_rs *s, int32_t k) {
    if (!s) return RFA_ERR_INVALID;
    if (k < -1 || k >= s->K) return stage_fail(s, RFA_ERR_INVALID, "no such slot");
    STAGE_HIP(s, hipSetDevice(s->device));
    const size_t K = (size_t)s->K;
    if (k < 0) {
        STAGE_HIP(s, hipMemsetAsync(s->d_hist, 0, 2 * K * kHist * sizeof(float), s->stream));
        std::fill(s->r.begin(), s->r.end(), 0);
    } else {
        float *h = s->d_hist + ((size_t)s->cur[(size_t)k] * K + (size_t)k) * kHist;
        STAGE_HIP(s, hipMemsetAsync(h, 0, kHist * sizeof(float), s->stream));
        s->r[(size_t)k] = 0;
    }
    return RFA_OK;
}

int rfa_audio_rs_get_offset(const rfa_audio_rs *s, int32_t k, int32_t *r) {
    if (!s || !r || k < 0 || k >= s->K) return RFA_ERR_INVALID;
    *r = s->r[(size_t)k];
    return RFA_OK;
}

int rfa_audio_rs_process(rfa_audio_rs *s, const float *in, size_t in_stride, const size_t *n_audio, float *out_f32,
                         size_t f32_stride, int16_t *out_s16, size_t s16_stride, size_t *n_out) {
    if (!s) return RFA_ERR_INVALID;
    std::vector<size_t> &m = s->call_out;
    std::vector<int> &r_next = s->call_r;
    size_t max_n = 0, max_out = 0;
    const int rc = rs_check(s, in, in_stride, n_audio, out_f32, f32_stride, out_s16, s16_stride, m, r_next, max_n, max_out);
    if (rc != RFA_OK) return rc;
    if (n_out) std::copy(m.begin(), m.end(), n_out);
    if (max_n == 0) return RFA_OK;                         // no samples: nothing launched, every slot keeps its state
    return rs_launch(s, in, in_stride, n_audio, out_f32, f32_stride, out_s16, s16_stride, m, r_next, max_out);
}

int rfa_audio_rs_process_host(rfa_audio_rs *s, const float *in, size_t in_stride, const size_t *n_audio, float *out_f32,
                              size_t f32_stride, int16_t *out_s16, size_t s16_stride, size_t *n_out) {
    if (!s) return RFA_ERR_INVALID;
    std::vector<size_t> &m = s->call_out;
    std::vector<int> &r_next = s->call_r;
    size_t max_n = 0, max_out = 0;
    // the host rows' strides and ranges are checked as the device rows' are
    int rc = rs_check(s, in, in_stride, n_audio, out_f32, f32_stride, out_s16, s16_stride, m, r_next, max_n, max_out);
    if (rc != RFA_OK) return rc;
    if (n_out) std::copy(m.begin(), m.end(), n_out);
    if (max_n == 0) return RFA_OK;
    const size_t K = (size_t)s->K, out_w = std::max(max_out, (size_t)1);
    STAGE_HIP(s, hipSetDevice(s->device));
    rc = stage_grow(s, s->d_in, s->d_in_cap, K * max_n, "input staging");
    if (rc == RFA_OK && out_f32) rc = stage_grow(s, s->d_f32, s->d_f32_cap, K * out_w, "float output staging");
    if (rc == RFA_OK && out_s16) rc = stage_grow(s, s->d_s16, s->d_s16_cap, K * out_w, "int16 output staging");
    if (rc != RFA_OK) return rc;
    for (size_t k = 0; k < K; k++)                         // row k holds n_audio[k] floats and no more
        if (n_audio[k])
            STAGE_HIP(s, hipMemcpyAsync(s->d_in + k * max_n, in + k * in_stride, n_audio[k] * sizeof(float),
                                        hipMemcpyHostToDevice, s->stream));
    rc = rs_launch(s, s->d_in, max_n, n_audio, out_f32 ? s->d_f32 : nullptr, out_w, out_s16 ? s->d_s16 : nullptr, out_w, m,
                   r_next, max_out);
    if (rc != RFA_OK) return rc;
    for (size_t k = 0; k < K; k++) {
        if (!m[k]) continue;
        if (out_f32)
            STAGE_HIP(s, hipMemcpyAsync(out_f32 + k * f32_stride, s->d_f32 + k * out_w, m[k] * sizeof(float),
                                        hipMemcpyDeviceToHost, s->stream));
        if (out_s16)
            STAGE_HIP(s, hipMemcpyAsync(out_s16 + k * s16_stride, s->d_s16 + k * out_w, m[k] * sizeof(int16_t),
                                        hipMemcpyDeviceToHost, s->stream));
    }
    STAGE_HIP(s, hipStreamSynchronize(s->stream));
    return RFA_OK;
}

int rfa_audio_rs_set_stream(rfa_audio_rs *s, void *stream) { return stage_set_stream(s, stream); }

int rfa_audio_rs_get_stream(const rfa_audio_rs *s, void **stream) { return stage_get_stream(s, stream); }

int rfa_audio_rs_synchronize(rfa_audio_rs *s) { return stage_synchronize(s); }

}  // extern "C"
