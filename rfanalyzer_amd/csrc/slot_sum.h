// slot_sum.h -- the summation plan of the per-slot meters (squelch.hip, freq.hip, tone.hip), device and host.
//
// A meter sums one term per sample of each of K planar rows into C doubles per slot.  Samples are
// cut into tiles of kTile = 16384: tile j is [j*kTile, min(n, (j+1)*kTile)).  A workgroup of 256
// threads sums one tile: thread t adds the terms at tile_start + t + 256*m, m ascending, into
// doubles that start at +0.0; a wave folds its 64 accumulators with wave_reduce (fixed butterfly),
// the four waves are added in wave order starting from wave 0's sum.  Tiles are added in ascending
// order starting from tile 0's sum.  Each component is folded on its own.  None of this looks at
// the row's address, the stride or K, and nothing is atomic, so a sum is a function of the row's
// values and n (and of what the term's prologue reads) alone, bit for bit; tests/slot_sum_plan.py
// restates the order and the device tests compare with it.
//   n <= kTile (RFA_SQUELCH_ONE_LAUNCH_MAX): slot_sum_kernel, grid (K), the tile's sum is the slot's.
//   n >  kTile: slot_partials_kernel over (tiles, K), then slot_fold_kernel over (K).
// A packet of the banks is a few hundred samples per slot and a 2^24-sample call of 32 slots about
// 671 K, 41 tiles per slot: the threshold keeps every per-packet call at one launch, and a
// one-workgroup sum of 16384 samples (128 KiB out of L2) stays well below the front end's time for
// the raw samples that produce them (DESIGN 5.7i has the measured lines).
//
// A term is a small struct passed to the kernels by value:
//   static constexpr int C                    components;
//   struct In; In load(re, im, i) const       what term i reads of its row;
//   void add(double (&acc)[C], In) const      acc += term, component by component;
//   bool prologue(k, re, im, acc) const       thread 0 of tile 0, before its loop: true where it has
//                                             dealt with term 0 itself (added or left out);
//   void epilogue(k, re, im, n) const         once per slot, behind the whole sum.
// Ordering of the hooks.  Only the workgroup of tile 0 runs the prologue.  The epilogue runs in
// something ordered after that: in the one-launch kernel in thread 0 behind tile_sum's barrier, in
// the two-launch case in the fold kernel -- a later launch on the same stream -- and never in a
// partials workgroup, whose tile n-1 may run before tile 0.  So an epilogue may write what the
// prologue reads (freq.hip's carried sample).
#pragma once

#include <hip/hip_runtime.h>

#include "stage_common.h"
#include "wave.h"

#pragma clang fp contract(off)

constexpr int kSlotThreads = 256;
constexpr long long kSlotTile = RFA_SQUELCH_TILE;
static_assert(RFA_SQUELCH_ONE_LAUNCH_MAX == RFA_SQUELCH_TILE, "one launch is the one-tile case of the tile sum");
static_assert(RFA_FREQ_TILE == RFA_SQUELCH_TILE, "the meters share one plan");
static_assert(kSlotTile % (4 * kSlotThreads) == 0, "the unrolled loop covers whole tiles");

// ---------------------------------------------------------------- device

// Sum of the terms i in [lo, hi) of slot k's row, hi - lo <= kSlotTile; valid in thread 0, after a barrier.
template <class Term>
__device__ __forceinline__ void tile_sum(const Term &term, size_t k, const float *__restrict__ re,
                                         const float *__restrict__ im, long long lo, long long hi,
                                         double (&s)[Term::C]) {
    constexpr int C = Term::C;
    __shared__ double wave_sum[C][kSlotThreads / 64];
    const int t = (int)threadIdx.x;
    double acc[C];
#pragma unroll
    for (int c = 0; c < C; c++) acc[c] = 0.0;
    long long i = lo + t;
    if (i == 0 && i < hi && term.prologue(k, re, im, acc)) i += kSlotThreads;     // thread 0 of tile 0
    // four independent groups of loads in flight, added in index order
    for (; i + 3 * kSlotThreads < hi; i += 4 * kSlotThreads) {
        typename Term::In x[4];
#pragma unroll
        for (int u = 0; u < 4; u++) x[u] = term.load(re, im, i + u * kSlotThreads);
#pragma unroll
        for (int u = 0; u < 4; u++) term.add(acc, x[u]);
    }
    for (; i < hi; i += kSlotThreads) term.add(acc, term.load(re, im, i));
    double w[C];
#pragma unroll
    for (int c = 0; c < C; c++) w[c] = rfa::wave_reduce(acc[c], [](double a, double b) { return a + b; });
    if ((t & 63) == 0) {
#pragma unroll
        for (int c = 0; c < C; c++) wave_sum[c][t >> 6] = w[c];
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < C; c++) {
        s[c] = 0.0;
        if (t == 0) {
            s[c] = wave_sum[c][0];
#pragma unroll
            for (int v = 1; v < kSlotThreads / 64; v++) s[c] += wave_sum[c][v];
        }
    }
}

// grid (K): 1 <= n <= kSlotTile.  sums[c * K + k].
template <class Term>
__global__ __launch_bounds__(kSlotThreads) void slot_sum_kernel(Term term, const float *__restrict__ re,
                                                                const float *__restrict__ im, size_t stride,
                                                                long long n, double *__restrict__ sums) {
    const size_t k = blockIdx.x;
    const float *xr = re + k * stride, *xi = im + k * stride;
    double s[Term::C];
    tile_sum(term, k, xr, xi, 0, n, s);
    if (threadIdx.x == 0) {                                    // behind tile_sum's barrier
#pragma unroll
        for (int c = 0; c < Term::C; c++) sums[c * gridDim.x + k] = s[c];
        term.epilogue(k, xr, xi, n);
    }
}

// grid (tiles, K): partials[(k * tiles + j) * C + c]; runs the prologue (tile 0), never the epilogue
template <class Term>
__global__ __launch_bounds__(kSlotThreads) void slot_partials_kernel(Term term, const float *__restrict__ re,
                                                                     const float *__restrict__ im, size_t stride,
                                                                     long long n, double *__restrict__ partials) {
    const size_t k = blockIdx.y;
    const long long lo = (long long)blockIdx.x * kSlotTile;
    const long long hi = lo + kSlotTile < n ? lo + kSlotTile : n;
    double s[Term::C];
    tile_sum(term, k, re + k * stride, im + k * stride, lo, hi, s);
    if (threadIdx.x == 0) {
        double *p = partials + (k * (size_t)gridDim.x + blockIdx.x) * Term::C;
#pragma unroll
        for (int c = 0; c < Term::C; c++) p[c] = s[c];
    }
}

// grid (K), one wave: the slot's tiles in ascending order, then the epilogue.  Lanes fetch 64
// partials at a time, lane 0 adds them one by one.
template <class Term>
__global__ __launch_bounds__(64) void slot_fold_kernel(Term term, const double *__restrict__ partials, long long tiles,
                                                       const float *__restrict__ re, const float *__restrict__ im,
                                                       size_t stride, long long n, double *__restrict__ sums) {
    constexpr int C = Term::C;
    const size_t k = blockIdx.x;
    const double *p = partials + k * (size_t)tiles * C;
    const int lane = (int)threadIdx.x;
    double s[C];
#pragma unroll
    for (int c = 0; c < C; c++) s[c] = 0.0;
    for (long long base = 0; base < tiles; base += 64) {
        double mine[C];
#pragma unroll
        for (int c = 0; c < C; c++) mine[c] = base + lane < tiles ? p[(base + lane) * C + c] : 0.0;
        const int cnt = tiles - base < 64 ? (int)(tiles - base) : 64;
        for (int j = 0; j < cnt; j++) {
            const bool first = base == 0 && j == 0;
#pragma unroll
            for (int c = 0; c < C; c++) {
                const double v = rfa::readlane_t(mine[c], j);
                s[c] = first ? v : s[c] + v;
            }
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < C; c++) sums[c * gridDim.x + k] = s[c];
        term.epilogue(k, re + k * stride, im + k * stride, n);
    }
}

// ---------------------------------------------------------------- device, a count per slot
//
// The same plan where slot k has its own n = counts[k] >= 0, read from a device array (tone.hip:
// the demodulator bank's audio counts).  Tile j of slot k is [j*kTile, min(n_k, (j+1)*kTile)) and is
// summed by tile_sum itself, so a slot's sums are a function of its values and n_k (and of what its
// term reads) alone, as above.  A slot with n_k = 0 gets +0.0 sums and runs no hook.  The term
// passed to these kernels hands out a per-slot view of itself,
//   struct View; View slot(k) const           what implements the term interface above for slot k,
// for a term that needs more of its slot than the row (tone.hip: probes and sample index).

// grid (K): every counts[k] <= kSlotTile.  sums[c * K + k].
template <class Term>
__global__ __launch_bounds__(kSlotThreads) void slot_counted_sum_kernel(Term term, const float *__restrict__ re,
                                                                        const float *__restrict__ im, size_t stride,
                                                                        const long long *__restrict__ counts,
                                                                        double *__restrict__ sums) {
    using View = typename Term::View;
    const size_t k = blockIdx.x;
    const long long n = counts[k];
    const float *xr = re + k * stride, *xi = im + k * stride;
    double s[View::C];
    if (n > 0) {                                               // the same for the whole workgroup
        const View view = term.slot(k);
        tile_sum(view, k, xr, xi, 0, n, s);
        if (threadIdx.x == 0) view.epilogue(k, xr, xi, n);     // behind tile_sum's barrier
    } else {
#pragma unroll
        for (int c = 0; c < View::C; c++) s[c] = 0.0;
    }
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < View::C; c++) sums[c * gridDim.x + k] = s[c];
    }
}

// grid (tiles of the largest count, K): partials[(k * gridDim.x + j) * C + c] for the tiles slot k has
template <class Term>
__global__ __launch_bounds__(kSlotThreads) void slot_counted_partials_kernel(Term term, const float *__restrict__ re,
                                                                             const float *__restrict__ im,
                                                                             size_t stride,
                                                                             const long long *__restrict__ counts,
                                                                             double *__restrict__ partials) {
    using View = typename Term::View;
    const size_t k = blockIdx.y;
    const long long n = counts[k];
    const long long lo = (long long)blockIdx.x * kSlotTile;
    if (lo >= n) return;                                       // the whole workgroup: slot k has no such tile
    const long long hi = lo + kSlotTile < n ? lo + kSlotTile : n;
    double s[View::C];
    tile_sum(term.slot(k), k, re + k * stride, im + k * stride, lo, hi, s);
    if (threadIdx.x == 0) {
        double *p = partials + (k * (size_t)gridDim.x + blockIdx.x) * View::C;
#pragma unroll
        for (int c = 0; c < View::C; c++) p[c] = s[c];
    }
}

// grid (K), one wave: slot k's own tiles of the partials' `tiles_max` per slot, folded as slot_fold_kernel does
template <class Term>
__global__ __launch_bounds__(64) void slot_counted_fold_kernel(Term term, const double *__restrict__ partials,
                                                               long long tiles_max, const float *__restrict__ re,
                                                               const float *__restrict__ im, size_t stride,
                                                               const long long *__restrict__ counts,
                                                               double *__restrict__ sums) {
    using View = typename Term::View;
    constexpr int C = View::C;
    const size_t k = blockIdx.x;
    const long long n = counts[k];
    const long long tiles = (n + kSlotTile - 1) / kSlotTile;   // <= tiles_max
    const double *p = partials + k * (size_t)tiles_max * C;
    const int lane = (int)threadIdx.x;
    double s[C];
#pragma unroll
    for (int c = 0; c < C; c++) s[c] = 0.0;
    for (long long base = 0; base < tiles; base += 64) {
        double mine[C];
#pragma unroll
        for (int c = 0; c < C; c++) mine[c] = base + lane < tiles ? p[(base + lane) * C + c] : 0.0;
        const int cnt = tiles - base < 64 ? (int)(tiles - base) : 64;
        for (int j = 0; j < cnt; j++) {
            const bool first = base == 0 && j == 0;
#pragma unroll
            for (int c = 0; c < C; c++) {
                const double v = rfa::readlane_t(mine[c], j);
                s[c] = first ? v : s[c] + v;
            }
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < C; c++) sums[c * gridDim.x + k] = s[c];
        if (n > 0) term.slot(k).epilogue(k, re + k * stride, im + k * stride, n);
    }
}

// ---------------------------------------------------------------- host

// What a meter's handle owns for the plan.
struct SlotSums {
    size_t count = 0;                  // C * K
    double *d_sums = nullptr;          // [C][K]
    double *h_sums = nullptr;          // pinned, [C][K]: the last enqueued call's, once `copied` has passed
    double *d_partials = nullptr;      // [K][tiles][C] of a call above one tile
    size_t partials_cap = 0;
    hipEvent_t copied = nullptr;       // behind the copy of the sums: what a caller waits for
    bool launched = false;             // the last enqueue got as far as its kernels (the epilogue will run)
    float *d_in = nullptr;             // staging of the _host entries (stage_upload_rows)
    size_t d_in_cap = 0;
};

inline int slot_sums_open(SlotSums &m, size_t count) {
    m.count = count;
    if (hipMalloc(&m.d_sums, count * sizeof(double)) != hipSuccess ||
        hipHostMalloc(&m.h_sums, count * sizeof(double), hipHostMallocDefault) != hipSuccess)
        return RFA_ERR_NOMEM;
    if (hipEventCreateWithFlags(&m.copied, hipEventDisableTiming) != hipSuccess) return RFA_ERR_HIP;
    return RFA_OK;
}

inline void slot_sums_close(SlotSums &m) {
    if (m.d_sums) (void)hipFree(m.d_sums);
    if (m.d_partials) (void)hipFree(m.d_partials);
    if (m.d_in) (void)hipFree(m.d_in);
    if (m.h_sums) (void)hipHostFree(m.h_sums);
    if (m.copied) (void)hipEventDestroy(m.copied);
    m = SlotSums{};
}

// One call of n_samples >= 1 on the handle's stream: one launch or two, the copy of the C * K sums
// into h_sums and the event behind it.  Waiting for the event is the caller's.
template <class Term, class H>
int slot_sums_enqueue(H *h, SlotSums &m, const Term &term, const float *re, const float *im, size_t channel_stride,
                      size_t n_samples) {
    const size_t K = m.count / Term::C;
    const long long n = (long long)n_samples;
    m.launched = false;
    STAGE_HIP(h, hipSetDevice(h->device));
    if (n <= kSlotTile) {
        hipLaunchKernelGGL(slot_sum_kernel<Term>, dim3((unsigned)K), dim3(kSlotThreads), 0, h->stream, term, re, im,
                           channel_stride, n, m.d_sums);
        STAGE_HIP(h, hipGetLastError());
    } else {
        const long long tiles = (n + kSlotTile - 1) / kSlotTile;       // <= 2^22
        const int rc = stage_grow(h, m.d_partials, m.partials_cap, m.count * (size_t)tiles, "partial sums");
        if (rc != RFA_OK) return rc;
        hipLaunchKernelGGL(slot_partials_kernel<Term>, dim3((unsigned)tiles, (unsigned)K), dim3(kSlotThreads), 0,
                           h->stream, term, re, im, channel_stride, n, m.d_partials);
        STAGE_HIP(h, hipGetLastError());
        hipLaunchKernelGGL(slot_fold_kernel<Term>, dim3((unsigned)K), dim3(64), 0, h->stream, term, m.d_partials, tiles,
                           re, im, channel_stride, n, m.d_sums);
        STAGE_HIP(h, hipGetLastError());
    }
    m.launched = true;
    STAGE_HIP(h, hipMemcpyAsync(m.h_sums, m.d_sums, m.count * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    STAGE_HIP(h, hipEventRecord(m.copied, h->stream));
    return RFA_OK;
}

// The same with a count per slot: d_counts[K] is on the device once the stream gets here, max_n >= 1
// is the largest of them.  One launch where max_n <= kSlotTile, else partials sized by max_n and a fold.
template <class Term, class H>
int slot_sums_enqueue_counted(H *h, SlotSums &m, const Term &term, const float *re, const float *im,
                              size_t channel_stride, const long long *d_counts, size_t max_n) {
    using View = typename Term::View;
    const size_t K = m.count / View::C;
    m.launched = false;
    STAGE_HIP(h, hipSetDevice(h->device));
    if ((long long)max_n <= kSlotTile) {
        hipLaunchKernelGGL(slot_counted_sum_kernel<Term>, dim3((unsigned)K), dim3(kSlotThreads), 0, h->stream, term, re,
                           im, channel_stride, d_counts, m.d_sums);
        STAGE_HIP(h, hipGetLastError());
    } else {
        const long long tiles = ((long long)max_n + kSlotTile - 1) / kSlotTile;      // <= 2^22
        const int rc = stage_grow(h, m.d_partials, m.partials_cap, m.count * (size_t)tiles, "partial sums");
        if (rc != RFA_OK) return rc;
        hipLaunchKernelGGL(slot_counted_partials_kernel<Term>, dim3((unsigned)tiles, (unsigned)K), dim3(kSlotThreads),
                           0, h->stream, term, re, im, channel_stride, d_counts, m.d_partials);
        STAGE_HIP(h, hipGetLastError());
        hipLaunchKernelGGL(slot_counted_fold_kernel<Term>, dim3((unsigned)K), dim3(64), 0, h->stream, term,
                           m.d_partials, tiles, re, im, channel_stride, d_counts, m.d_sums);
        STAGE_HIP(h, hipGetLastError());
    }
    m.launched = true;
    STAGE_HIP(h, hipMemcpyAsync(m.h_sums, m.d_sums, m.count * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    STAGE_HIP(h, hipEventRecord(m.copied, h->stream));
    return RFA_OK;
}
