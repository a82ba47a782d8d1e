// audio_iir.hip -- a cascade of second-order recursive sections on every bank slot's audio row
// (rfa_audio_iir_*): the de-emphasis of an NFM receiver, the 8th-order high-pass that takes a
// CTCSS tone out of the voice.  The reference has no counterpart.
//
// Definition (include/rfa.h has it in full).  Section q of slot k has (b0, b1, b2, a1, a2), a0 = 1,
// and filters the output of section q-1.  A slot counts its samples a = 0, 1, ... since its last
// reset / set_sections; sample a lies in block a / B at offset i = a % B, B = 128.  One step:
//     v = (b0*u) + z1;   z1' = ((b1*u) - (a1*v)) + z2;   z2' = (b2*u) - (a2*v)
// Per block j with block-start state s0_j: zs[i] is that recurrence run from z = (0, 0) over the
// block's inputs (the zero-state response), z_end its state after the block, and
//     y[i]       = zs[i] + ((G[i][0]*s0_j[0]) + (G[i][1]*s0_j[1]))
//     s0_{j+1}[r] = ((P[r][0]*s0_j[0]) + (P[r][1]*s0_j[1])) + z_end[r]
// with G[i] the first row of A^i and P = A^B, A = [[-a1, 1], [-a2, 0]], computed in double and
// rounded once.  Every product and sum is rounded to float32 in this order, nothing contracted.
// The blocks of a slot are independent but for the short chain of s0, so a row cut into calls
// anywhere gives the bits of the row given whole: a call that ends inside a block leaves s0 and
// the running z, and the next call goes on from them.
//
// Kernel.  One workgroup per slot, one grid for all slots.  The workgroup walks the row in chunks
// of kChunkBlocks blocks.  A chunk is staged in LDS with coalesced loads, kLd in flight per lane,
// block b at row stride B + 1 floats, so the lanes of a wave -- one block each -- meet 64 different
// banks at every offset.  Per section: (1) lane b runs the zero-state recurrence over its block in
// place, kU steps to a round of LDS reads, without a branch: only the waves that hold the call's head
// or tail block select per step whether the offset is the call's; its input is the staged row for
// section 0 and zs + the zero-input term of the section before for the others, added as it is read
// (the G of a step is one LDS address for the whole wave: a broadcast); (2) lane 0 advances s0
// block by block in block order -- one step per block -- and leaves every block's s0 in LDS.  The
// store to the output row adds the last section's zero-input term, coalesced again; 256 being a
// multiple of B, a lane meets one offset only and keeps its G in registers.  The carried state (s0
// and z per section) is read at the start and written at the end by the slot's own workgroup.
//
// Records go through a ring of kRecRing pinned entries with an event behind each copy, tables
// through one pinned stage on the handle's stream, both as audio_fir.hip does it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

#include "stage_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kB = RFA_AUDIO_IIR_BLOCK;
constexpr int kMaxS = RFA_AUDIO_IIR_MAX_SECTIONS;
constexpr int kChunkBlocks = RFA_AUDIO_IIR_CHUNK_BLOCKS;
constexpr int kThreads = 256;
constexpr int kRow = kB + 1;                    // floats between two blocks' rows in LDS
constexpr int kHead = 12;                       // floats of a section's table before G: b0 b1 b2 a1 a2, P[4], 3 unused
constexpr int kSecFloats = kHead + 2 * kB;      // one section's table on the device
constexpr int kCarry = 4;                       // s0[2], z[2] per section
constexpr int kU = 8;                           // steps whose LDS reads are issued together
constexpr int kLd = 8;                          // global loads a lane keeps in flight
constexpr int kRecRing = 8;
constexpr size_t kMaxCount = (size_t)1 << 36;

static_assert(kThreads == kChunkBlocks, "one lane per block of a chunk");
static_assert(kB % kU == 0 && kChunkBlocks % kU == 0 && (kB & (kB - 1)) == 0, "whole rounds; offsets by mask");
static_assert(kThreads % kB == 0 && kB == 128, "a lane stores one offset of every block; block index by >> 7");
static_assert(kMaxS * kCarry <= kThreads, "the carry is moved by one pass of the workgroup");

struct IirSlot {
    long long n;                       // this call's samples
    int sections;                      // S
    int a0;                            // the slot's a mod B before this call
};

inline int round_u(int v) { return (v + kU - 1) / kU * kU; }

// Floats of LDS of a launch whose widest chunk has nb blocks: the rows (to an even count), z_end[nb][2],
// s0[nb][2] (both rounded up to whole rounds of the scan), the slot's carry and its sections' G.
inline size_t lds_floats(int nb) {
    return (((size_t)nb * kRow + 1) & ~(size_t)1) + 4 * (size_t)round_u(nb) + kMaxS * kCarry + (size_t)kMaxS * 2 * kB;
}

inline long long blocks_touched(size_t n, int a0) { return n ? (long long)(((size_t)a0 + n + kB - 1) / kB) : 0; }

__device__ __forceinline__ void df2t(float b0, float b1, float b2, float a1, float a2, float u, float &z1, float &z2,
                                     float &v) {
    v = (b0 * u) + z1;
    const float t = (b1 * u) - (a1 * v);
    const float w = (b2 * u) - (a2 * v);
    z1 = t + z2;
    z2 = w;
}

// One lane's zero-state pass over its block's row r, in place, kU steps to a round of LDS reads.
// ZI: the input is the section before's zs plus its zero-input term, G of that section at gl and
// its block-start state (p0, p1).  PRED: the block is the call's head or tail and only offsets
// lo ... hi-1 are the call's; the others are computed and dropped (nothing reads what they leave).
template <bool ZI, bool PRED>
__device__ __forceinline__ void block_pass(float *r, const float *gl, float p0, float p1, float b0, float b1,
                                           float b2, float a1, float a2, int lo, int hi, float &z1, float &z2) {
    for (int i0 = 0; i0 < kB; i0 += kU) {
        float u[kU];
#pragma unroll
        for (int j = 0; j < kU; j++) u[j] = r[i0 + j];
        if constexpr (ZI) {
#pragma unroll
            for (int j = 0; j < kU; j++) {
                const float2 g = *reinterpret_cast<const float2 *>(gl + 2 * (i0 + j));
                const float zi = (g.x * p0) + (g.y * p1);
                u[j] = u[j] + zi;
            }
        }
#pragma unroll
        for (int j = 0; j < kU; j++) {
            float n1 = z1, n2 = z2, v;
            df2t(b0, b1, b2, a1, a2, u[j], n1, n2, v);
            if constexpr (PRED) {
                const bool on = i0 + j >= lo && i0 + j < hi;
                z1 = on ? n1 : z1;
                z2 = on ? n2 : z2;
            } else {
                z1 = n1;
                z2 = n2;
            }
            r[i0 + j] = v;
        }
    }
}

// grid (K).  tab [K][kMaxS][kSecFloats]; carry [K][kMaxS][kCarry]; nb_lds: the blocks the launch's LDS holds.
__global__ __launch_bounds__(kThreads) void audio_iir_kernel(const float *__restrict__ in, size_t in_stride,
                                                            float *__restrict__ out, size_t out_stride,
                                                            const IirSlot *__restrict__ slots,
                                                            const float *__restrict__ tab, float *carry, int nb_lds) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const size_t k = blockIdx.x;
    const IirSlot s = slots[k];
    if (s.n <= 0) return;                                  // the slot keeps everything
    const float *x = in + k * in_stride;
    float *y = out + k * out_stride;
    const int tid = (int)threadIdx.x;
    const int S = s.sections;

    if (S == 0) {                                          // the bits as they are, kLd loads in flight per lane
        const unsigned *xb = reinterpret_cast<const unsigned *>(x);
        unsigned *yb = reinterpret_cast<unsigned *>(y);
        for (long long base = 0; base < s.n; base += kThreads * kLd) {
            unsigned v[kLd];
#pragma unroll
            for (int j = 0; j < kLd; j++) {
                const long long i = base + j * kThreads + tid;
                v[j] = xb[i < s.n ? i : s.n - 1];
            }
#pragma unroll
            for (int j = 0; j < kLd; j++) {
                const long long i = base + j * kThreads + tid;
                if (i < s.n) yb[i] = v[j];
            }
        }
        return;
    }

    const int nb_u = (nb_lds + kU - 1) / kU * kU;
    float *row = lds, *zend = lds + ((nb_lds * kRow + 1) & ~1), *s0s = zend + 2 * nb_u, *cst = s0s + 2 * nb_u;
    float *gl = cst + kMaxS * kCarry;                      // [S][kB][2]
    const float *tk = tab + k * (size_t)(kMaxS * kSecFloats);
    float *ck = carry + k * (size_t)(kMaxS * kCarry);
    if (tid < S * kCarry) cst[tid] = ck[tid];
    for (int idx = tid; idx < S * 2 * kB; idx += kThreads)
        gl[idx] = tk[(idx >> 8) * kSecFloats + kHead + (idx & (2 * kB - 1))];
    const int o = tid & (kB - 1);                          // this lane's offset in every block it stores
    const float gout0 = tk[(S - 1) * kSecFloats + kHead + 2 * o], gout1 = tk[(S - 1) * kSecFloats + kHead + 2 * o + 1];
    const int wave = __builtin_amdgcn_readfirstlane(tid) >> 6;

    const long long a0 = s.a0, total = a0 + s.n;           // the call's samples sit at grid positions a0 ... total-1
    const long long touched = (total + kB - 1) / kB;
    const bool tail_partial = (total & (kB - 1)) != 0;

    for (long long c0 = 0; c0 < touched; c0 += kChunkBlocks) {
        const int nblk = touched - c0 < kChunkBlocks ? (int)(touched - c0) : kChunkBlocks;
        const int cells = nblk * kB;
        const long long gbase = c0 * kB;
        const bool last = c0 + nblk == touched;
        const int ncomplete = last && tail_partial ? nblk - 1 : nblk;
        // the waves that hold the call's head block or its incomplete tail block
        const bool pred = (c0 == 0 && a0 > 0 && wave == 0) || (last && tail_partial && wave == (nblk - 1) >> 6);
        __syncthreads();                                   // the chunk before has left the rows; carry and G are in
        for (int base = 0; base < cells; base += kThreads * kLd) {
            float v[kLd];
#pragma unroll
            for (int j = 0; j < kLd; j++) {                // an address inside the row whatever the cell
                const long long i = gbase + base + j * kThreads + tid - a0;
                v[j] = x[i < 0 ? 0 : i < s.n ? i : s.n - 1];
            }
#pragma unroll
            for (int j = 0; j < kLd; j++) {
                const int idx = base + j * kThreads + tid;
                if (idx < cells) row[(idx >> 7) * kRow + o] = v[j];
            }
        }
        __syncthreads();

        for (int q = 0; q < S; q++) {
            const float *sec = tk + q * kSecFloats;
            if (tid < nblk) {
                const float b0 = sec[0], b1 = sec[1], b2 = sec[2], a1 = sec[3], a2 = sec[4];
                const long long bstart = gbase + (long long)tid * kB;
                const int lo = bstart < a0 ? (int)(a0 - bstart) : 0;                   // the call's head block
                const int hi = total - bstart < kB ? (int)(total - bstart) : kB;
                float z1 = 0.0f, z2 = 0.0f;
                if (c0 == 0 && tid == 0) {                 // the head block goes on from the carried z
                    z1 = cst[q * kCarry + 2];
                    z2 = cst[q * kCarry + 3];
                }
                float *r = row + tid * kRow;
                if (q == 0) {
                    if (pred) block_pass<false, true>(r, nullptr, 0.0f, 0.0f, b0, b1, b2, a1, a2, lo, hi, z1, z2);
                    else block_pass<false, false>(r, nullptr, 0.0f, 0.0f, b0, b1, b2, a1, a2, lo, hi, z1, z2);
                } else {
                    const float *g = gl + (q - 1) * 2 * kB;                            // the section before
                    const float p0 = s0s[2 * tid], p1 = s0s[2 * tid + 1];
                    if (pred) block_pass<true, true>(r, g, p0, p1, b0, b1, b2, a1, a2, lo, hi, z1, z2);
                    else block_pass<true, false>(r, g, p0, p1, b0, b1, b2, a1, a2, lo, hi, z1, z2);
                }
                zend[2 * tid] = z1;
                zend[2 * tid + 1] = z2;
            }
            __syncthreads();
            if (tid == 0) {                                // s0 of every block, in block order
                const float p00 = sec[5], p01 = sec[6], p10 = sec[7], p11 = sec[8];
                float c0s = cst[q * kCarry], c1s = cst[q * kCarry + 1];
                int j0 = 0;
                for (; j0 + kU <= ncomplete; j0 += kU) {   // whole rounds: kU z_end read together
                    float2 e[kU];
#pragma unroll
                    for (int j = 0; j < kU; j++) e[j] = *reinterpret_cast<const float2 *>(zend + 2 * (j0 + j));
#pragma unroll
                    for (int j = 0; j < kU; j++) {
                        *reinterpret_cast<float2 *>(s0s + 2 * (j0 + j)) = float2{c0s, c1s};
                        const float n0 = ((p00 * c0s) + (p01 * c1s)) + e[j].x;
                        const float n1 = ((p10 * c0s) + (p11 * c1s)) + e[j].y;
                        c0s = n0;
                        c1s = n1;
                    }
                }
                for (; j0 < nblk; j0++) {
                    s0s[2 * j0] = c0s;
                    s0s[2 * j0 + 1] = c1s;
                    if (j0 < ncomplete) {
                        const float n0 = ((p00 * c0s) + (p01 * c1s)) + zend[2 * j0];
                        const float n1 = ((p10 * c0s) + (p11 * c1s)) + zend[2 * j0 + 1];
                        c0s = n0;
                        c1s = n1;
                    }
                }
                cst[q * kCarry] = c0s;
                cst[q * kCarry + 1] = c1s;
                if (last) {                                // an incomplete block leaves its running z
                    cst[q * kCarry + 2] = tail_partial ? zend[2 * (nblk - 1)] : 0.0f;
                    cst[q * kCarry + 3] = tail_partial ? zend[2 * (nblk - 1) + 1] : 0.0f;
                }
            }
            __syncthreads();
        }

        for (int base = 0; base < cells; base += kThreads * kLd) {     // the last section's zero-input term, and out
            float v[kLd];
#pragma unroll
            for (int j = 0; j < kLd; j++) {
                const int idx = base + j * kThreads + tid;
                const int b = idx < cells ? idx >> 7 : nblk - 1;
                const float g = (gout0 * s0s[2 * b]) + (gout1 * s0s[2 * b + 1]);
                v[j] = row[b * kRow + o] + g;
            }
#pragma unroll
            for (int j = 0; j < kLd; j++) {
                const int idx = base + j * kThreads + tid;
                const long long i = gbase + idx - a0;
                if (idx < cells && i >= 0 && i < s.n) y[i] = v[j];
            }
        }
    }
    __syncthreads();
    if (tid < S * kCarry) ck[tid] = cst[tid];
}

// Finite, and the poles inside the unit circle: |a2| < 1 and |a1| < 1 + a2.
bool section_ok(const float *c) {
    for (int j = 0; j < 5; j++)
        if (!std::isfinite(c[j])) return false;
    const double a1 = c[3], a2 = c[4];
    return std::fabs(a2) < 1.0 && std::fabs(a1) < 1.0 + a2;
}

// G[i] = first row of A^i, i = 0 ... B-1, and P = A^B, A = [[-a1, 1], [-a2, 0]]: double, rounded once.
void make_tables(float a1f, float a2f, float *G, float *P) {
    const double A[2][2] = {{-(double)a1f, 1.0}, {-(double)a2f, 0.0}};
    double R[2][2] = {{1.0, 0.0}, {0.0, 1.0}};
    for (int i = 0; i < kB; i++) {
        G[2 * i] = (float)R[0][0];
        G[2 * i + 1] = (float)R[0][1];
        double N[2][2];
        for (int r = 0; r < 2; r++)
            for (int c = 0; c < 2; c++) N[r][c] = (R[r][0] * A[0][c]) + (R[r][1] * A[1][c]);
        std::memcpy(R, N, sizeof(R));
    }
    P[0] = (float)R[0][0];
    P[1] = (float)R[0][1];
    P[2] = (float)R[1][0];
    P[3] = (float)R[1][1];
}

}  // namespace

struct rfa_audio_iir : StageCore {
    int K = 0;
    std::vector<std::vector<float>> coeffs;    // [K][5 S], the host's copy
    std::vector<int> amod;                     // [K], a mod B as of the calls made
    float *d_tab = nullptr;                    // [K][kMaxS][kSecFloats]
    float *d_carry = nullptr;                  // [K][kMaxS][kCarry]
    float *h_tab_stage = nullptr;              // pinned, [kMaxS][kSecFloats]: one upload in flight
    hipEvent_t tab_ev = nullptr;
    bool tab_ev_used = false;
    IirSlot *d_recs = nullptr;                 // [K]
    IirSlot *h_recs = nullptr;                 // pinned, [kRecRing][K]
    hipEvent_t ev[kRecRing] = {};
    bool ev_used[kRecRing] = {};
    int ring_at = 0;
    float *d_in = nullptr, *d_out = nullptr;   // rfa_audio_iir_process_host's rows
    size_t d_in_cap = 0, d_out_cap = 0;
};

namespace {

bool ranges_overlap(const float *a, size_t na, const float *b, size_t nb) {
    const uintptr_t a0 = (uintptr_t)a, a1 = a0 + na * sizeof(float), b0 = (uintptr_t)b, b1 = b0 + nb * sizeof(float);
    return na && nb && a0 < b1 && b0 < a1;
}

// The checks of a call that come before the rows are looked at; max_n is the largest count.
int ai_check_counts(rfa_audio_iir *f, const size_t *n_audio, size_t in_stride, size_t out_stride, size_t &max_n) {
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

int ai_check_rows(rfa_audio_iir *f, const float *in, size_t in_stride, const size_t *n_audio, const float *out,
                  size_t out_stride, size_t max_n) {
    if (max_n == 0) return RFA_OK;
    if (!in || !out) return stage_fail(f, RFA_ERR_INVALID, "null row");
    const size_t K = (size_t)f->K;
    if (!ranges_overlap(in, (K - 1) * in_stride + max_n, out, (K - 1) * out_stride + max_n)) return RFA_OK;
    for (size_t a = 0; a < K; a++)
        for (size_t b = 0; b < K; b++)
            if (ranges_overlap(in + a * in_stride, n_audio[a], out + b * out_stride, n_audio[b]))
                return stage_fail(f, RFA_ERR_INVALID, "input and output rows overlap");
    return RFA_OK;
}

}  // namespace

extern "C" {

int rfa_audio_iir_tables(float a1, float a2, float *G, float *P) {
    const float c[5] = {0.0f, 0.0f, 0.0f, a1, a2};
    if (!G || !P || !section_ok(c)) return RFA_ERR_INVALID;
    make_tables(a1, a2, G, P);
    return RFA_OK;
}

int rfa_audio_iir_plan(int32_t num_sections, size_t n, int32_t a_mod_B, int32_t *plan) {
    if (!plan || num_sections < 0 || num_sections > kMaxS || n > kMaxCount || a_mod_B < 0 || a_mod_B >= kB)
        return RFA_ERR_INVALID;
    const bool work = n > 0 && num_sections > 0;
    const long long touched = blocks_touched(n, a_mod_B);
    plan[0] = kB;
    plan[1] = kChunkBlocks;
    plan[2] = work ? (int32_t)(lds_floats((int)std::min<long long>(touched, kChunkBlocks)) * sizeof(float)) : 0;
    plan[3] = n == 0 ? RFA_AUDIO_IIR_PATH_NONE : num_sections == 0 ? RFA_AUDIO_IIR_PATH_COPY : RFA_AUDIO_IIR_PATH_BLOCKED;
    plan[4] = work ? (int32_t)((touched + kChunkBlocks - 1) / kChunkBlocks) : 0;
    plan[5] = (int32_t)touched;
    return RFA_OK;
}

int rfa_audio_iir_carry_after(size_t n, int32_t a_mod_B, int32_t *next) {
    if (!next || n > kMaxCount || a_mod_B < 0 || a_mod_B >= kB) return RFA_ERR_INVALID;
    *next = (int32_t)(((size_t)a_mod_B + n) % kB);
    return RFA_OK;
}

int rfa_audio_iir_create(int device, int32_t n_channels, rfa_audio_iir **out) {
    if (!out) return RFA_ERR_INVALID;
    *out = nullptr;
    if (n_channels < 1 || n_channels > RFA_AUDIO_IIR_MAX_CHANNELS) return RFA_ERR_INVALID;
    int rc = stage_check_device(device);
    if (rc != RFA_OK) return rc;
    rfa_audio_iir *f = new (std::nothrow) rfa_audio_iir();
    if (!f) return RFA_ERR_NOMEM;
    const size_t K = (size_t)n_channels;
    f->device = device;
    f->K = n_channels;
    f->coeffs.resize(K);
    f->amod.assign(K, 0);
    rc = stage_open(f, device);
    const size_t tab_bytes = (size_t)kMaxS * kSecFloats * sizeof(float), carry_bytes = K * kMaxS * kCarry * sizeof(float);
    if (rc == RFA_OK && (hipMalloc(&f->d_tab, K * tab_bytes) != hipSuccess ||
                         hipMalloc(&f->d_carry, carry_bytes) != hipSuccess ||
                         hipMalloc(&f->d_recs, K * sizeof(IirSlot)) != hipSuccess ||
                         hipHostMalloc(&f->h_tab_stage, tab_bytes, hipHostMallocDefault) != hipSuccess ||
                         hipHostMalloc(&f->h_recs, kRecRing * K * sizeof(IirSlot), hipHostMallocDefault) != hipSuccess))
        rc = RFA_ERR_NOMEM;
    if (rc == RFA_OK && hipEventCreateWithFlags(&f->tab_ev, hipEventDisableTiming) != hipSuccess) rc = RFA_ERR_HIP;
    for (int e = 0; rc == RFA_OK && e < kRecRing; e++)
        if (hipEventCreateWithFlags(&f->ev[e], hipEventDisableTiming) != hipSuccess) rc = RFA_ERR_HIP;
    if (rc == RFA_OK && hipMemsetAsync(f->d_carry, 0, carry_bytes, f->stream) != hipSuccess) rc = RFA_ERR_HIP;
    // a full chunk's rows are above the default dynamic-LDS limit of a launch
    if (rc == RFA_OK && hipFuncSetAttribute(reinterpret_cast<const void *>(audio_iir_kernel),
                                            hipFuncAttributeMaxDynamicSharedMemorySize,
                                            (int)(lds_floats(kChunkBlocks) * sizeof(float))) != hipSuccess)
        rc = RFA_ERR_HIP;
    if (rc != RFA_OK) {
        rfa_audio_iir_destroy(f);
        return rc;
    }
    *out = f;
    return RFA_OK;
}

int rfa_audio_iir_destroy(rfa_audio_iir *f) {
    if (!f) return RFA_ERR_INVALID;
    stage_close_stream(f);
    if (f->d_tab) (void)hipFree(f->d_tab);
    if (f->d_carry) (void)hipFree(f->d_carry);
    if (f->d_recs) (void)hipFree(f->d_recs);
    if (f->d_in) (void)hipFree(f->d_in);
    if (f->d_out) (void)hipFree(f->d_out);
    if (f->h_tab_stage) (void)hipHostFree(f->h_tab_stage);
    if (f->h_recs) (void)hipHostFree(f->h_recs);
    if (f->tab_ev) (void)hipEventDestroy(f->tab_ev);
    for (hipEvent_t e : f->ev)
        if (e) (void)hipEventDestroy(e);
    delete f;
    return RFA_OK;
}

const char *rfa_audio_iir_last_error(const rfa_audio_iir *f) { return stage_last_error(f); }

int rfa_audio_iir_get_channels(const rfa_audio_iir *f, int32_t *n_channels) {
    if (!f || !n_channels) return RFA_ERR_INVALID;
    *n_channels = f->K;
    return RFA_OK;
}

int rfa_audio_iir_set_sections(rfa_audio_iir *f, int32_t k, const float *coeffs, int32_t num_sections) {
    if (!f) return RFA_ERR_INVALID;
    if (k < 0 || k >= f->K) return stage_fail(f, RFA_ERR_INVALID, "no such slot");
    if (num_sections < 0 || num_sections > kMaxS) return stage_fail(f, RFA_ERR_INVALID, "section count outside 0 ... 8");
    if (num_sections && !coeffs) return stage_fail(f, RFA_ERR_INVALID, "null coefficients");
    for (int q = 0; q < num_sections; q++)
        if (!section_ok(coeffs + 5 * q))
            return stage_fail(f, RFA_ERR_INVALID, "a section is not finite or not inside the stability triangle");
    STAGE_HIP(f, hipSetDevice(f->device));
    if (num_sections) {
        if (f->tab_ev_used) STAGE_HIP(f, hipEventSynchronize(f->tab_ev));      // the stage's previous upload is over
        for (int q = 0; q < num_sections; q++) {
            float *sec = f->h_tab_stage + (size_t)q * kSecFloats;
            const float *c = coeffs + 5 * q;
            std::memcpy(sec, c, 5 * sizeof(float));
            make_tables(c[3], c[4], sec + kHead, sec + 5);
            sec[9] = sec[10] = sec[11] = 0.0f;
        }
        STAGE_HIP(f, hipMemcpyAsync(f->d_tab + (size_t)k * kMaxS * kSecFloats, f->h_tab_stage,
                                    (size_t)num_sections * kSecFloats * sizeof(float), hipMemcpyHostToDevice, f->stream));
        STAGE_HIP(f, hipEventRecord(f->tab_ev, f->stream));
        f->tab_ev_used = true;
    }
    // the slot starts again: a zero carry, and its block grid at the next sample
    STAGE_HIP(f, hipMemsetAsync(f->d_carry + (size_t)k * kMaxS * kCarry, 0, kMaxS * kCarry * sizeof(float), f->stream));
    f->amod[(size_t)k] = 0;
    f->coeffs[(size_t)k].assign(coeffs, coeffs + 5 * (size_t)num_sections);
    return RFA_OK;
}

int rfa_audio_iir_get_sections(const rfa_audio_iir *f, int32_t k, float *coeffs, size_t capacity,
                               int32_t *num_sections) {
    if (!f || !num_sections || k < 0 || k >= f->K) return RFA_ERR_INVALID;
    const std::vector<float> &c = f->coeffs[(size_t)k];
    *num_sections = (int32_t)(c.size() / 5);
    if (!coeffs) return RFA_OK;                            // asked for the count
    if (capacity < c.size() / 5) return RFA_ERR_INVALID;   // the count is there, nothing is copied
    if (!c.empty()) std::memcpy(coeffs, c.data(), c.size() * sizeof(float));
    return RFA_OK;
}

int rfa_audio_iir_reset(rfa_audio_iir *f, int32_t k) {
    if (!f) return RFA_ERR_INVALID;
    if (k < -1 || k >= f->K) return stage_fail(f, RFA_ERR_INVALID, "no such slot");
    STAGE_HIP(f, hipSetDevice(f->device));
    const size_t slot = kMaxS * kCarry;
    if (k < 0) {
        STAGE_HIP(f, hipMemsetAsync(f->d_carry, 0, (size_t)f->K * slot * sizeof(float), f->stream));
        std::fill(f->amod.begin(), f->amod.end(), 0);
    } else {
        STAGE_HIP(f, hipMemsetAsync(f->d_carry + (size_t)k * slot, 0, slot * sizeof(float), f->stream));
        f->amod[(size_t)k] = 0;
    }
    return RFA_OK;
}

int rfa_audio_iir_process(rfa_audio_iir *f, const float *in, size_t in_stride, const size_t *n_audio, float *out,
                          size_t out_stride) {
    if (!f) return RFA_ERR_INVALID;
    size_t max_n = 0;
    int rc = ai_check_counts(f, n_audio, in_stride, out_stride, max_n);
    if (rc == RFA_OK) rc = ai_check_rows(f, in, in_stride, n_audio, out, out_stride, max_n);
    if (rc != RFA_OK || max_n == 0) return rc;             // no samples: nothing launched, every carry stays
    const size_t K = (size_t)f->K;
    STAGE_HIP(f, hipSetDevice(f->device));
    // this call's records: wait until the ring entry's previous copy has been made
    const int e = f->ring_at;
    if (f->ev_used[e]) STAGE_HIP(f, hipEventSynchronize(f->ev[e]));
    IirSlot *recs = f->h_recs + (size_t)e * K;
    long long max_blocks = 0;
    for (size_t k = 0; k < K; k++) {
        recs[k] = IirSlot{(long long)n_audio[k], (int)(f->coeffs[k].size() / 5), f->amod[k]};
        if (recs[k].sections) max_blocks = std::max(max_blocks, blocks_touched(n_audio[k], f->amod[k]));
    }
    STAGE_HIP(f, hipMemcpyAsync(f->d_recs, recs, K * sizeof(IirSlot), hipMemcpyHostToDevice, f->stream));
    STAGE_HIP(f, hipEventRecord(f->ev[e], f->stream));
    f->ev_used[e] = true;
    f->ring_at = (e + 1) % kRecRing;

    const int nb_lds = (int)std::min<long long>(max_blocks, kChunkBlocks);
    const size_t lds_bytes = nb_lds ? lds_floats(nb_lds) * sizeof(float) : 0;
    hipLaunchKernelGGL(audio_iir_kernel, dim3((unsigned)K), dim3(kThreads), lds_bytes, f->stream, in, in_stride, out,
                       out_stride, f->d_recs, f->d_tab, f->d_carry, nb_lds);
    STAGE_HIP(f, hipGetLastError());
    for (size_t k = 0; k < K; k++) f->amod[k] = (int)(((size_t)f->amod[k] + n_audio[k]) % kB);
    return RFA_OK;
}

int rfa_audio_iir_process_host(rfa_audio_iir *f, const float *in, size_t in_stride, const size_t *n_audio, float *out,
                               size_t out_stride) {
    if (!f) return RFA_ERR_INVALID;
    size_t max_n = 0;
    int rc = ai_check_counts(f, n_audio, in_stride, out_stride, max_n);
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
    rc = rfa_audio_iir_process(f, f->d_in, max_n, n_audio, f->d_out, max_n);
    if (rc != RFA_OK) return rc;
    for (size_t k = 0; k < K; k++)
        if (n_audio[k])
            STAGE_HIP(f, hipMemcpyAsync(out + k * out_stride, f->d_out + k * max_n, n_audio[k] * sizeof(float),
                                        hipMemcpyDeviceToHost, f->stream));
    STAGE_HIP(f, hipStreamSynchronize(f->stream));
    return RFA_OK;
}

int rfa_audio_iir_set_stream(rfa_audio_iir *f, void *stream) { return stage_set_stream(f, stream); }

int rfa_audio_iir_get_stream(const rfa_audio_iir *f, void **stream) { return stage_get_stream(f, stream); }

int rfa_audio_iir_synchronize(rfa_audio_iir *f) { return stage_synchronize(f); }

}  // extern "C"
