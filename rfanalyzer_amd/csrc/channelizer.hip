// channelizer.hip -- polyphase channelizer on gfx950 (rfa_pfb_*): all M raster
// channels k * Fs / M of one raw IQ stream per call, for about the cost of two
// or three slots of the front-end channel bank (ddc.hip) whatever M is.
//
// Channel k of output n (newest input i_n = n * D + D - 1) is
//   y_k[n] = sum_t h[t] * x[i_n - t] * exp(-j 2 pi k (i_n - t) / M)
// computed as a fold and one forward DFT:
//   u_n[r] = sum of h[t] * x[i_n - t] over the t with (i_n - t) mod M == r
//   y_k[n] = sum_r u_n[r] * exp(-j 2 pi k r / M)
// The phase is absolute in the sample count, so it never drifts and no rotation
// follows the DFT.
//
// Two launches per call.  pfb_kernel: a workgroup owns NT consecutive output
// times.  Where the (NT-1) * D + T converted samples they depend on and the taps
// fit kPfbStageBytes of LDS they are staged there once (every load in flight at
// the same time, one conversion per sample); else item (time, r) folds its
// P = ceil(T / M) taps straight from the history or the raw buffer (the raw
// stream is 2-8 B per sample and is re-read from L2; consecutive r read
// consecutive samples).  The NT folded rows go through an in-LDS Stockham DFT
// of radices {4, 2, 3, 5}, and the selected channels are written with time
// along the lanes: NT = 16 floats, 64 B, per row and burst.
// pfb_hist_kernel keeps the newest T - 1 converted samples for the next call in
// the other of two history buffers, so no workgroup reads what another writes.
//
// An output's arithmetic is a function of its own window only: every (time, r)
// item runs the same statements on the same values wherever the tile or call
// boundary falls (history entries are the stored results of the same
// conversion), taps are summed t ascending from 0 with product and sum rounded
// separately (no FMA contraction), and the DFT of one output never mixes with
// another's.  That makes split, selection, format and pointer offset bit-exact.
//
// rfa_pfb_create_rational runs the same raster at L / D times the input rate:
// pfb_rational_kernel below folds with one of L sub-filters per output and shares
// everything else; pfb_kernel is the code the integer entry launches, unchanged.
//
// rfa_pfb_set_tuning moves a slot off its raster centre: the TUNED instantiations
// of both kernels are the same tiles with a rotation by a table entry compiled
// into the store (pfb_store), so a tuned call is still two launches and a handle
// without a tuning launches the code it always did.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/rfa.h"

#pragma clang fp contract(off)

#include "stage_common.h"

namespace {

constexpr int kPfbThreads = 256;
constexpr int kPfbMaxStages = 12;
constexpr int kPfbTilePoints = 4096;     // NT * M at most: two LDS row sets of 8 B points, 64 KiB + padding
constexpr int kPfbMaxTimes = 16;         // NT at most: 64 B per row and store burst
constexpr int kPfbStageBytes = 64 * 1024;  // staged samples + taps at most; above it the fold reads global memory

struct PfbLaunch {
    const void *raw;
    long long S;                   // input samples this call
    const float *hist;             // [re T-1 | im T-1], oldest first, precedes raw[0]
    float *new_hist;
    const float *taps;
    int T, M, Mp, D;               // Mp: LDS row pitch in points, odd
    int NT;                        // output times per workgroup, a power of two
    int stage;                     // points of LDS in front of the DFT rows: staged run + taps, 0 = fold from global
    int run;                       // (NT-1) * D + T: samples a full workgroup depends on
    long long n0, in0, n_out;      // index of this call's first output / first input since reset
    const float2 *tw;              // stage s: tw[tw_off[s] + k * (R - 1) + (r - 1)] = exp(-j 2 pi k r / (p R))
    int nstages;
    int radix[kPfbMaxStages];
    int tw_off[kPfbMaxStages];
    const int *chan;               // slot -> channel
    int K;
    long long stride;              // floats between two slots' rows
    float *out_re, *out_im;
};

// ---------------------------------------------------------------- tuning (rfa_pfb_set_tuning)
//
// Slot j of a tuned handle writes y * exp(-j 2 pi m_j n / Q) with n the absolute output index:
// the table entry (n * m_j) mod Q.  The reduction is the one below on the host and on the
// device: x mod q from the high half of x * mu, mu = floor((2^64 - 1) / q).  With
// 2^64 / q - 1 <= mu <= 2^64 / q the estimate floor(x mu / 2^64) is floor(x / q) or one less for
// every x < 2^64, so one conditional subtraction ends in [0, q): no division, and no x for
// which the index leaves the table.
struct PfbTune {
    const float2 *w;               // W[i] = (cos, sin)(2 pi i / q), q entries
    const int *step;               // slot -> m_j, -q < m_j < q
    unsigned q;
    unsigned long long mu;         // floor((2^64 - 1) / q)
};

__host__ __device__ inline unsigned long long pfb_tune_mu(unsigned q) { return ~0ull / q; }

__host__ __device__ inline unsigned pfb_tune_mod(unsigned long long x, unsigned q, unsigned long long mu) {
#if defined(__HIP_DEVICE_COMPILE__)
    const unsigned long long est = __umul64hi(x, mu);
#else
    const unsigned long long est = (unsigned long long)(((unsigned __int128)x * mu) >> 64);
#endif
    unsigned long long r = x - est * q;
    if (r >= q) r -= q;
    return (unsigned)r;
}

// (n * m) mod q, mathematical mod, for -q < m < q <= RFA_PFB_TUNE_MAX_STEPS: n is reduced first,
// so the product stays below 2^40.
__host__ __device__ inline unsigned pfb_tune_index(unsigned q, unsigned long long mu, int m, unsigned long long n) {
    const unsigned r = pfb_tune_mod(n, q, mu);
    const unsigned mm = m < 0 ? (unsigned)(m + (int)q) : (unsigned)m;
    return pfb_tune_mod((unsigned long long)r * mm, q, mu);
}

// One complex input sample, converted by the code the front end converts with before it
// mixes (raw_to_iq of stage_common.h); g is call-relative, negative values index the history.
template <int FMT>
__device__ __forceinline__ float2 pfb_sample(const PfbLaunch &a, long long g) {
    if (g < 0) return float2{a.hist[a.T - 1 + g], a.hist[2 * (a.T - 1) + g]};
    float2 x;
    raw_to_iq<FMT>(raw_load<FMT>(a.raw, g), x.x, x.y);
    return x;
}

__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return float2{a.x + b.x, a.y + b.y}; }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return float2{a.x - b.x, a.y - b.y}; }
__device__ __forceinline__ float2 cmul(float2 a, float2 w) { return float2{a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x}; }
__device__ __forceinline__ float2 cscale(float s, float2 a) { return float2{s * a.x, s * a.y}; }
__device__ __forceinline__ float2 mul_mi(float2 m, float2 n) { return float2{m.x + n.y, m.y - n.x}; }   // m - j n
__device__ __forceinline__ float2 mul_pi(float2 m, float2 n) { return float2{m.x - n.y, m.y + n.x}; }   // m + j n

// One Stockham butterfly of radix R: inputs Q = M / R apart, twiddled by the
// stage's table (p: product of the radices already done), outputs p apart.
template <int R>
__device__ __forceinline__ void pfb_butterfly(const float2 *src, float2 *dst, const float2 *tw, int i, int p, int Q) {
    const int k = i % p;
    const int j = (i - k) * R + k;
    float2 u[R];
#pragma unroll
    for (int r = 0; r < R; r++) u[r] = src[i + r * Q];
    if (p > 1) {
#pragma unroll
        for (int r = 1; r < R; r++) u[r] = cmul(u[r], tw[k * (R - 1) + (r - 1)]);
    }
    float2 y[R];
    if constexpr (R == 2) {
        y[0] = cadd(u[0], u[1]);
        y[1] = csub(u[0], u[1]);
    } else if constexpr (R == 4) {
        const float2 a = cadd(u[0], u[2]), b = csub(u[0], u[2]), c = cadd(u[1], u[3]), d = csub(u[1], u[3]);
        y[0] = cadd(a, c);
        y[1] = mul_mi(b, d);
        y[2] = csub(a, c);
        y[3] = mul_pi(b, d);
    } else if constexpr (R == 3) {
        const float2 t = cadd(u[1], u[2]);
        const float2 m = csub(u[0], cscale(0.5f, t));
        const float2 s = cscale(0.86602540378443864676f, csub(u[1], u[2]));
        y[0] = cadd(u[0], t);
        y[1] = mul_mi(m, s);
        y[2] = mul_pi(m, s);
    } else {
        constexpr float c1 = 0.30901699437494742410f, c2 = -0.80901699437494742410f;
        constexpr float s1 = 0.95105651629515357212f, s2 = 0.58778525229247312917f;
        const float2 a1 = cadd(u[1], u[4]), a2 = cadd(u[2], u[3]), b1 = csub(u[1], u[4]), b2 = csub(u[2], u[3]);
        const float2 m1 = cadd(cadd(u[0], cscale(c1, a1)), cscale(c2, a2));
        const float2 m2 = cadd(cadd(u[0], cscale(c2, a1)), cscale(c1, a2));
        const float2 n1 = cadd(cscale(s1, b1), cscale(s2, b2));
        const float2 n2 = csub(cscale(s2, b1), cscale(s1, b2));
        y[0] = cadd(cadd(u[0], a1), a2);
        y[1] = mul_mi(m1, n1);
        y[2] = mul_mi(m2, n2);
        y[3] = mul_pi(m2, n2);
        y[4] = mul_pi(m1, n1);
    }
#pragma unroll
    for (int r = 0; r < R; r++) dst[j + r * p] = y[r];
}

template <int R>
__device__ __forceinline__ void pfb_stage(const PfbLaunch &a, const float2 *src, float2 *dst, const float2 *tw, int p,
                                          int nloc) {
    const int Q = a.M / R;
    for (int item = threadIdx.x; item < nloc * Q; item += kPfbThreads) {
        const int nl = item / Q, i = item - nl * Q;
        pfb_butterfly<R>(src + nl * a.Mp, dst + nl * a.Mp, tw, i, p, Q);
    }
}

// The selected channels of a tile's finished DFT rows, time along the lanes.  TUNED: slot j is
// rotated by W[(n * m_j) mod q] on its way out (include/rfa.h, rfa_pfb_set_tuning); a slot with
// m_j == 0 is stored as it is, without a multiply.
template <bool TUNED>
__device__ __forceinline__ void pfb_store(const PfbLaunch &a, const PfbTune &t, const float2 *src, long long m0,
                                          int nloc) {
    const int sh = 31 - __clz(a.NT);
    for (int item = threadIdx.x; item < a.K * a.NT; item += kPfbThreads) {
        const int slot = item >> sh, nl = item & (a.NT - 1);
        if (nl < nloc) {
            float2 v = src[nl * a.Mp + a.chan[slot]];
            const long long o = (long long)slot * a.stride + m0 + nl;
            if constexpr (TUNED) {
                const int m = t.step[slot];
                if (m != 0) {
                    const float2 w = t.w[pfb_tune_index(t.q, t.mu, m, (unsigned long long)(a.n0 + m0 + nl))];
                    v = float2{v.x * w.x + v.y * w.y, v.y * w.x - v.x * w.y};
                }
            }
            a.out_re[o] = v.x;
            a.out_im[o] = v.y;
        }
    }
}

// The kernel is instantiated per launch record.  Rec = PfbLaunch is the kernel of a handle without a
// tuning: no PfbTune reaches it and its code is what it was before tunings existed.
// Rec = PfbTunedLaunch carries the tuning behind the same record and compiles the rotation into the
// store.
struct PfbTunedLaunch {
    PfbLaunch a;
    PfbTune t;
};
__device__ __forceinline__ const PfbLaunch &pfb_record(const PfbLaunch &r) { return r; }
__device__ __forceinline__ const PfbLaunch &pfb_record(const PfbTunedLaunch &r) { return r.a; }
__device__ __forceinline__ PfbTune pfb_tuning(const PfbLaunch &) { return PfbTune{}; }
__device__ __forceinline__ PfbTune pfb_tuning(const PfbTunedLaunch &r) { return r.t; }

template <int FMT, class Rec = PfbLaunch>
__global__ __launch_bounds__(kPfbThreads) void pfb_kernel(Rec rec) {
    constexpr bool TUNED = !std::is_same_v<Rec, PfbLaunch>;
    const PfbLaunch &a = pfb_record(rec);
    const PfbTune t = pfb_tuning(rec);
    extern __shared__ __attribute__((aligned(16))) float2 pfb_lds[];
    // [staged run | taps] (a.stage points, absent where the fold reads global memory) | DFT rows x 2
    float2 *src = pfb_lds + a.stage, *dst = src + a.NT * a.Mp;
    const int tid = threadIdx.x;
    const long long m0 = (long long)blockIdx.x * a.NT;
    const int nloc = (int)min((long long)a.NT, a.n_out - m0);
    const float2 *xs = pfb_lds;                                  // xs[i]: sample i_first - (T-1) + i
    const float *hs = reinterpret_cast<const float *>(pfb_lds + a.run);
    if (a.stage) {
        const long long g_lo = (a.n0 + m0) * a.D + (a.D - 1) - (a.T - 1) - a.in0;
        const int span = (nloc - 1) * a.D + a.T;
        for (int i = tid; i < span; i += kPfbThreads) pfb_lds[i] = pfb_sample<FMT>(a, g_lo + i);
        float *hw = reinterpret_cast<float *>(pfb_lds + a.run);
        for (int i = tid; i < a.T; i += kPfbThreads) hw[i] = a.taps[i];
        __syncthreads();
    }
    // fold: item (nl, r) sums the taps t = t0, t0 + M, ... of output n0 + m0 + nl, t0 = (i_n - r) mod M
    for (int item = tid; item < nloc * a.M; item += kPfbThreads) {
        const int nl = item / a.M, r = item - nl * a.M;
        const long long i_abs = (a.n0 + m0 + nl) * a.D + (a.D - 1);
        int t0 = (int)(i_abs % a.M) - r;
        if (t0 < 0) t0 += a.M;
        long long g = i_abs - t0 - a.in0;
        float2 acc = {0.0f, 0.0f};
        if (a.stage) {
            const float2 *x = xs + nl * a.D + (a.T - 1);
#pragma unroll 4
            for (int t = t0; t < a.T; t += a.M) {
                const float2 v = lds_ld(x - t);
                const float h = hs[t];
                acc.x = acc.x + h * v.x;
                acc.y = acc.y + h * v.y;
            }
        } else {
#pragma unroll 4
            for (int t = t0; t < a.T; t += a.M, g -= a.M) {
                const float2 x = pfb_sample<FMT>(a, g);
                const float h = a.taps[t];
                acc.x = acc.x + h * x.x;
                acc.y = acc.y + h * x.y;
            }
        }
        src[nl * a.Mp + r] = acc;
    }
    __syncthreads();
    int p = 1;
    for (int s = 0; s < a.nstages; s++) {
        const int R = a.radix[s];
        const float2 *tw = a.tw + a.tw_off[s];
        if (R == 4) pfb_stage<4>(a, src, dst, tw, p, nloc);
        else if (R == 2) pfb_stage<2>(a, src, dst, tw, p, nloc);
        else if (R == 3) pfb_stage<3>(a, src, dst, tw, p, nloc);
        else pfb_stage<5>(a, src, dst, tw, p, nloc);
        __syncthreads();
        float2 *sw = src;
        src = dst;
        dst = sw;
        p *= R;
    }
    pfb_store<TUNED>(a, t, src, m0, nloc);
}

// new_hist[t] = sample S - (T-1) + t of the extended sequence [hist | raw].
template <int FMT>
__global__ __launch_bounds__(kPfbThreads) void pfb_hist_kernel(PfbLaunch a) {
    const int t = blockIdx.x * kPfbThreads + threadIdx.x;
    if (t >= a.T - 1) return;
    const float2 x = pfb_sample<FMT>(a, a.S - (a.T - 1) + t);
    a.new_hist[t] = x.x;
    a.new_hist[a.T - 1 + t] = x.y;
}

// ---------------------------------------------------------------- rational rate (rfa_pfb_create_rational)
//
// Output n has phase p_n = (n * D) mod L and newest sample m_n = floor(n * D / L):
//   y_k[n] = sum_{t < Tp} g[p_n + t * L] * x[m_n - t] * exp(-j 2 pi k (m_n - t) / M),  Tp = ceil(T / L)
// The phase of the NCO is still the integer sample index, so only the fold differs from
// pfb_kernel: item (time, r) sums gp[p_n][t] * x[m_n - t] over t = t0, t0 + M, ... < Tp with
// t0 = (m_n - r) mod M.  The taps sit on the device phase-major, gp[p][t] = g[p + t * L], zero
// padded to Tp per phase, so an item walks one row with stride M and consecutive r read
// neighbouring taps.  The launch's `a` is a PfbLaunch with T = Tp and taps = gp: pfb_sample,
// the Stockham stages and pfb_hist_kernel (history of Tp - 1 samples) are the integer path's.
//
// A tile of NT times spans at most ceil((NT-1) * D / L) + Tp samples and min(NT, L) different
// phases (gcd(L, D) = 1).  Three plans, chosen by pfb_plan_rational under the same
// kPfbStageBytes rule: run and the tile's tap rows staged; run staged, taps from global
// memory (the table is re-read from L2); run and taps from global memory.
struct PfbRatLaunch {
    PfbLaunch a;                   // T: taps per output Tp; taps: gp[L][Tp]; run: ceil((NT-1) D / L) + Tp
    int L;
    int stage_x;                   // 1: the run is staged at pfb_lds[0 .. run)
    int tap_rows;                  // tap rows staged behind the run: L (row = phase) where L <= NT, else NT
                                   // (row = time); 0: taps are read from global memory
};

// The stage loop and the store of pfb_kernel, which stays as it is.
template <bool TUNED>
__device__ __forceinline__ void pfb_dft_store(const PfbLaunch &a, const PfbTune &t, float2 *src, float2 *dst,
                                              long long m0, int nloc) {
    int p = 1;
    for (int s = 0; s < a.nstages; s++) {
        const int R = a.radix[s];
        const float2 *tw = a.tw + a.tw_off[s];
        if (R == 4) pfb_stage<4>(a, src, dst, tw, p, nloc);
        else if (R == 2) pfb_stage<2>(a, src, dst, tw, p, nloc);
        else if (R == 3) pfb_stage<3>(a, src, dst, tw, p, nloc);
        else pfb_stage<5>(a, src, dst, tw, p, nloc);
        __syncthreads();
        float2 *sw = src;
        src = dst;
        dst = sw;
        p *= R;
    }
    pfb_store<TUNED>(a, t, src, m0, nloc);
}

struct PfbRatTunedLaunch {
    PfbRatLaunch b;
    PfbTune t;
};
__device__ __forceinline__ const PfbRatLaunch &pfb_record(const PfbRatLaunch &r) { return r; }
__device__ __forceinline__ const PfbRatLaunch &pfb_record(const PfbRatTunedLaunch &r) { return r.b; }
__device__ __forceinline__ PfbTune pfb_tuning(const PfbRatLaunch &) { return PfbTune{}; }
__device__ __forceinline__ PfbTune pfb_tuning(const PfbRatTunedLaunch &r) { return r.t; }

template <int FMT, class Rec = PfbRatLaunch>
__global__ __launch_bounds__(kPfbThreads) void pfb_rational_kernel(Rec rec) {
    constexpr bool TUNED = !std::is_same_v<Rec, PfbRatLaunch>;
    const PfbRatLaunch &b = pfb_record(rec);
    const PfbTune t = pfb_tuning(rec);
    extern __shared__ __attribute__((aligned(16))) float2 pfb_lds[];
    __shared__ int t_dm[kPfbMaxTimes], t_ph[kPfbMaxTimes], t_mm[kPfbMaxTimes];   // m_n - m_first, p_n, m_n mod M
    const PfbLaunch &a = b.a;
    // [staged run | staged tap rows] (a.stage points) | DFT rows x 2
    float2 *src = pfb_lds + a.stage, *dst = src + a.NT * a.Mp;
    const int tid = threadIdx.x;
    const long long m0 = (long long)blockIdx.x * a.NT;
    const int nloc = (int)min((long long)a.NT, a.n_out - m0);
    const long long n_first = a.n0 + m0;
    const long long m_first = n_first * a.D / b.L;
    if (tid < nloc) {
        const long long nd = (n_first + tid) * a.D, m = nd / b.L;
        t_dm[tid] = (int)(m - m_first);
        t_ph[tid] = (int)(nd - m * b.L);
        t_mm[tid] = (int)(m % a.M);
    }
    const float2 *xs = pfb_lds;                                  // xs[i]: sample m_first - (Tp-1) + i
    const float *gs = reinterpret_cast<const float *>(pfb_lds + a.run);
    const bool by_phase = b.L <= a.NT;
    if (b.stage_x) {
        const long long m_last = (n_first + nloc - 1) * a.D / b.L;
        const long long g_lo = m_first - (a.T - 1) - a.in0;
        const int span = (int)(m_last - m_first) + a.T;
        for (int i = tid; i < span; i += kPfbThreads) pfb_lds[i] = pfb_sample<FMT>(a, g_lo + i);
        float *gw = reinterpret_cast<float *>(pfb_lds + a.run);
        for (int row = 0; row < b.tap_rows; row++) {
            const int ph = by_phase ? row : (int)(((n_first + row) * a.D) % b.L);
            for (int t = tid; t < a.T; t += kPfbThreads) gw[row * a.T + t] = a.taps[(long long)ph * a.T + t];
        }
    }
    __syncthreads();
    for (int item = tid; item < nloc * a.M; item += kPfbThreads) {
        const int nl = item / a.M, r = item - nl * a.M;
        int t0 = t_mm[nl] - r;
        if (t0 < 0) t0 += a.M;
        float2 acc = {0.0f, 0.0f};
        if (b.stage_x) {
            const float2 *x = xs + t_dm[nl] + (a.T - 1);
            const float *g = b.tap_rows ? gs + (by_phase ? t_ph[nl] : nl) * a.T : a.taps + (long long)t_ph[nl] * a.T;
#pragma unroll 4
            for (int t = t0; t < a.T; t += a.M) {
                const float2 v = lds_ld(x - t);
                const float h = g[t];
                acc.x = acc.x + h * v.x;
                acc.y = acc.y + h * v.y;
            }
        } else {
            const float *g = a.taps + (long long)t_ph[nl] * a.T;
            long long j = m_first + t_dm[nl] - t0 - a.in0;
#pragma unroll 4
            for (int t = t0; t < a.T; t += a.M, j -= a.M) {
                const float2 x = pfb_sample<FMT>(a, j);
                const float h = g[t];
                acc.x = acc.x + h * x.x;
                acc.y = acc.y + h * x.y;
            }
        }
        src[nl * a.Mp + r] = acc;
    }
    __syncthreads();
    pfb_dft_store<TUNED>(a, t, src, dst, m0, nloc);
}

int pfb_lds_bytes(const PfbLaunch &a) { return (a.stage + 2 * a.NT * a.Mp) * (int)sizeof(float2); }

// kernel: pfb_kernel<FMT, Rec> or pfb_rational_kernel<FMT, Rec>
template <class Rec>
hipError_t pfb_prepare(void (*kernel)(Rec)) {
    return hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                               kPfbStageBytes + 2 * (kPfbTilePoints + kPfbMaxTimes) * (int)sizeof(float2));
}

// The fold + DFT kernel on its record, then the history kernel on the record's PfbLaunch a.
template <int FMT, class Rec>
hipError_t pfb_launch(void (*kernel)(Rec), const Rec &rec, const PfbLaunch &a, hipStream_t st) {
    if (a.n_out > 0) {
        const long long blocks = (a.n_out + a.NT - 1) / a.NT;
        hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(kPfbThreads), pfb_lds_bytes(a), st, rec);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (a.T > 1) {
        hipLaunchKernelGGL(pfb_hist_kernel<FMT>, dim3((a.T - 1 + kPfbThreads - 1) / kPfbThreads), dim3(kPfbThreads), 0,
                           st, a);
        return hipGetLastError();
    }
    return hipSuccess;
}

// ---------------------------------------------------------------- host plan

// Radices of an M = 2^a 3^b 5^c point DFT: 4s, one 2 for an odd a, 3s, 5s; empty for any other M.
std::vector<int> pfb_radices(int32_t M) {
    std::vector<int> r;
    if (M < RFA_PFB_MIN_CHANNELS || M > RFA_PFB_MAX_CHANNELS) return r;
    int a = 0, b = 0, c = 0;
    while (M % 2 == 0) M /= 2, a++;
    while (M % 3 == 0) M /= 3, b++;
    while (M % 5 == 0) M /= 5, c++;
    if (M != 1) return r;
    r.insert(r.end(), a / 2, 4);
    r.insert(r.end(), a % 2, 2);
    r.insert(r.end(), b, 3);
    r.insert(r.end(), c, 5);
    return r;
}

// Stage tables in double, rounded once to float.
void pfb_twiddles(const std::vector<int> &radix, std::vector<float2> &tw, std::vector<int> &off) {
    tw.clear();
    off.clear();
    long long p = 1;
    for (int R : radix) {
        off.push_back((int)tw.size());
        const long long n = p * R;
        for (long long k = 0; k < p; k++)
            for (int r = 1; r < R; r++) {
                const double ang = -2.0 * M_PI * (double)((k * r) % n) / (double)n;
                tw.push_back(float2{(float)std::cos(ang), (float)std::sin(ang)});
            }
        p = n;
    }
}

int pfb_times_per_tile(int M) {
    int nt = kPfbMaxTimes;
    while (nt > 1 && nt * M > kPfbTilePoints) nt >>= 1;
    return nt;
}

// The tile plan of a handle: NT, and whether the run and the taps are staged in LDS.
void pfb_plan_tile(PfbLaunch &a) {
    a.Mp = a.M | 1;
    a.NT = pfb_times_per_tile(a.M);
    a.run = (a.NT - 1) * a.D + a.T;
    const int points = a.run + (a.T + 1) / 2;                    // taps: two floats per point
    a.stage = points * (int)sizeof(float2) <= kPfbStageBytes ? points : 0;
}

// The tile plan of a rational handle (b.a.T = Tp, b.a.M, b.a.D and b.L set): NT as above; the run
// is staged where its 8 B per sample fit kPfbStageBytes, and the tile's min(NT, L) tap rows of
// Tp floats behind it where both fit.
void pfb_plan_rational(PfbRatLaunch &b) {
    PfbLaunch &a = b.a;
    a.Mp = a.M | 1;
    a.NT = pfb_times_per_tile(a.M);
    a.run = (int)(((long long)(a.NT - 1) * a.D + b.L - 1) / b.L) + a.T;
    const long long rows = std::min(a.NT, b.L);
    const long long tap_points = (rows * a.T + 1) / 2;
    b.stage_x = (long long)a.run * (long long)sizeof(float2) <= kPfbStageBytes;
    b.tap_rows = b.stage_x && (a.run + tap_points) * (long long)sizeof(float2) <= kPfbStageBytes ? (int)rows : 0;
    a.stage = b.stage_x ? a.run + (b.tap_rows ? (int)tap_points : 0) : 0;
}

// The plan of a call's record (b.a.T = taps per output, b.a.M, b.a.D and b.L set): what
// rfa_pfb_process launches with and what rfa_pfb_tile_plan reports.
void pfb_plan(PfbRatLaunch &b, bool rational) {
    if (rational) pfb_plan_rational(b);
    else pfb_plan_tile(b.a);
}

long long pfb_gcd(long long a, long long b) {
    while (b) {
        const long long t = a % b;
        a = b;
        b = t;
    }
    return a;
}

// What rfa_pfb_create refuses as invalid in (M, D, T), and rfa_pfb_create_rational in (M, L, D, T).
bool pfb_integer_args_valid(int32_t M, int32_t D, int32_t T) {
    if (M < 1 || D < 1 || T < 1) return false;
    return D <= M && (long long)T <= (long long)RFA_PFB_MAX_PHASES * M;
}

bool pfb_rational_args_valid(int32_t M, int32_t L, int32_t D, int32_t T) {
    if (M < 1 || L < 1 || D < 1 || T < 1) return false;
    return L <= RFA_PFB_MAX_INTERPOLATION && L <= D && (long long)D <= (long long)L * M && pfb_gcd(L, D) == 1 &&
           (long long)T <= (long long)RFA_PFB_MAX_PHASES * M * L;
}

// Outputs due once c samples are consumed: ceil(c * L / D); c < 2^53 and L <= 64 keep the product in range.
long long pfb_rational_count(long long c, int L, int D) { return (c * L + D - 1) / D; }

// W[i] = (cos, sin)(2 pi i / q) of a tuning, in double and rounded to float once.  The angle is
// reduced to the first octant in integers (in eighths of a table step, so the octant's edges are
// exact), which makes the four axis points exact and the table symmetric.
float2 pfb_tune_entry(long long i, long long q) {
    long long e = 8 * i;                                         // angle = 2 pi e / (8 q), 0 <= e < 8 q
    bool neg_s = false, neg_c = false, swap = false;
    if (e > 4 * q) e = 8 * q - e, neg_s = true;                  // [0, pi]
    if (e > 2 * q) e = 4 * q - e, neg_c = true;                  // [0, pi / 2]
    if (e > q) e = 2 * q - e, swap = true;                       // [0, pi / 4]
    const double ang = 2.0 * M_PI * (double)e / (double)(8 * q);
    double c = std::cos(ang), s = std::sin(ang);
    if (swap) std::swap(c, s);
    return float2{(float)(neg_c ? -c : c), (float)(neg_s ? -s : s)};
}

bool pfb_tune_q_valid(int32_t q) { return q >= 1 && q <= RFA_PFB_TUNE_MAX_STEPS; }

}  // namespace

struct rfa_pfb : StageCore {
    int fmt = 0;
    int M = 0, D = 0, T = 0;
    int L = 1;                          // interpolation; above 1 only on a rational handle
    int Th = 0;                         // taps per output: T, or Tp = ceil(T / L) on a rational handle
    bool rational = false;              // created by rfa_pfb_create_rational (L = 1 included: m_n = n * D)
    std::vector<float> taps;
    std::vector<float> gp;              // rational: the device table gp[L][Tp], gp[p][t] = taps[p + t * L]
    std::vector<int> radix, tw_off;
    std::vector<int32_t> channels;      // slot -> channel
    long long in_done = 0;              // samples consumed since creation or reset
    float *d_taps = nullptr;
    float2 *d_tw = nullptr;
    int *d_chan = nullptr;              // M entries
    float *d_hist[2] = {nullptr, nullptr};
    int cur = 0;
    // tuning (rfa_pfb_set_tuning); tune_q == 0: none, and nothing below is read
    int32_t tune_q = 0;
    std::vector<int32_t> tune_steps;    // slot -> m_j as given
    float2 *d_tune_w = nullptr;         // tune_w_cap entries
    size_t tune_w_cap = 0;
    int *d_tune_step = nullptr;         // M entries
    bool tuned_prepared = false;        // the tuned kernels' LDS attribute is set
    // staging for the _host entry point
    void *d_in = nullptr;
    size_t d_in_cap = 0;
    float *d_out = nullptr;
    size_t d_out_cap = 0;
};

namespace {

long long pfb_outputs(const rfa_pfb *p, long long S) {
    if (p->rational) return pfb_rational_count(p->in_done + S, p->L, p->D) - pfb_rational_count(p->in_done, p->L, p->D);
    return (p->in_done + S) / p->D - p->in_done / p->D;
}

int pfb_upload(rfa_pfb *p) {
    std::vector<float2> tw;
    pfb_twiddles(p->radix, tw, p->tw_off);
    const size_t H = (size_t)std::max(1, p->Th - 1);
    const std::vector<float> &dtaps = p->rational ? p->gp : p->taps;
    if (hipMalloc(&p->d_taps, dtaps.size() * sizeof(float)) != hipSuccess ||
        hipMalloc(&p->d_tw, std::max<size_t>(1, tw.size()) * sizeof(float2)) != hipSuccess ||
        hipMalloc(&p->d_chan, (size_t)p->M * sizeof(int)) != hipSuccess ||
        hipMalloc(&p->d_hist[0], 2 * H * sizeof(float)) != hipSuccess ||
        hipMalloc(&p->d_hist[1], 2 * H * sizeof(float)) != hipSuccess)
        return stage_fail(p, RFA_ERR_NOMEM, "hipMalloc channelizer tables");
    STAGE_HIP(p, hipMemcpyAsync(p->d_taps, dtaps.data(), dtaps.size() * sizeof(float), hipMemcpyHostToDevice, p->stream));
    if (!tw.empty())
        STAGE_HIP(p, hipMemcpyAsync(p->d_tw, tw.data(), tw.size() * sizeof(float2), hipMemcpyHostToDevice, p->stream));
    STAGE_HIP(p, hipMemcpyAsync(p->d_chan, p->channels.data(), p->channels.size() * sizeof(int), hipMemcpyHostToDevice,
                           p->stream));
    STAGE_HIP(p, hipMemsetAsync(p->d_hist[0], 0, 2 * H * sizeof(float), p->stream));
    STAGE_HIP(p, hipMemsetAsync(p->d_hist[1], 0, 2 * H * sizeof(float), p->stream));
    STAGE_HIP(p, hipStreamSynchronize(p->stream));
    for (int fmt : {RFA_IN_S8, RFA_IN_U8, RFA_IN_S16LE, RFA_IN_F32_INTERLEAVED}) {
        STAGE_HIP(p, stage_dispatch_format(fmt, [](auto f) { return pfb_prepare(pfb_kernel<decltype(f)::value>); }));
        if (p->rational)
            STAGE_HIP(p, stage_dispatch_format(
                             fmt, [](auto f) { return pfb_prepare(pfb_rational_kernel<decltype(f)::value>); }));
    }
    return RFA_OK;
}

// Both create entries after their own argument checks: the handle for the raster M with the
// prototype `taps` at L times the input rate (rational: the L / D convention, L = 1 included),
// its stream, tables and history.
int pfb_create(int device, int input_format, int32_t M, int32_t L, int32_t D, bool rational, const float *taps,
               int32_t num_taps, rfa_pfb **out) {
    if (!rfa_pfb_supported(M)) return RFA_ERR_UNSUPPORTED;
    int rc = stage_check_device(device);
    if (rc != RFA_OK) return rc;
    rfa_pfb *p = new (std::nothrow) rfa_pfb();
    if (!p) return RFA_ERR_NOMEM;
    p->fmt = input_format;
    p->M = M;
    p->L = L;
    p->D = D;
    p->T = num_taps;
    p->Th = (num_taps + L - 1) / L;
    p->rational = rational;
    p->taps.assign(taps, taps + num_taps);
    if (rational) {
        p->gp.assign((size_t)L * p->Th, 0.0f);
        for (int s = 0; s < num_taps; s++) p->gp[(size_t)(s % L) * p->Th + s / L] = taps[s];
    }
    p->radix = pfb_radices(M);
    p->channels.resize(M);
    for (int k = 0; k < M; k++) p->channels[k] = k;
    rc = stage_open(p, device);
    if (rc == RFA_OK) rc = pfb_upload(p);
    if (rc != RFA_OK) {
        rfa_pfb_destroy(p);
        return rc;
    }
    *out = p;
    return RFA_OK;
}

}  // namespace

extern "C" {

int rfa_pfb_supported(int32_t n_channels) { return pfb_radices(n_channels).empty() ? 0 : 1; }

int rfa_pfb_create(int device, int input_format, int32_t n_channels, int32_t decimation, const float *taps,
                   int32_t num_taps, rfa_pfb **out) {
    if (!out) return RFA_ERR_INVALID;
    *out = nullptr;
    if (stage_sample_bytes(input_format) == 0 || !taps || !pfb_integer_args_valid(n_channels, decimation, num_taps))
        return RFA_ERR_INVALID;
    return pfb_create(device, input_format, n_channels, 1, decimation, false, taps, num_taps, out);
}

int rfa_pfb_create_rational(int device, int input_format, int32_t n_channels, int32_t interpolation, int32_t decimation,
                            const float *taps, int32_t num_taps, rfa_pfb **out) {
    if (!out) return RFA_ERR_INVALID;
    *out = nullptr;
    if (stage_sample_bytes(input_format) == 0 || !taps ||
        !pfb_rational_args_valid(n_channels, interpolation, decimation, num_taps))
        return RFA_ERR_INVALID;
    return pfb_create(device, input_format, n_channels, interpolation, decimation, true, taps, num_taps, out);
}

int rfa_pfb_get_ratio(const rfa_pfb *p, int32_t *interpolation, int32_t *decimation, int32_t *taps_per_output) {
    if (!p) return RFA_ERR_INVALID;
    if (interpolation) *interpolation = p->L;
    if (decimation) *decimation = p->D;
    if (taps_per_output) *taps_per_output = p->Th;
    return RFA_OK;
}

int rfa_pfb_rational_outputs(int32_t interpolation, int32_t decimation, uint64_t consumed, size_t n_samples, size_t *n) {
    constexpr uint64_t lim = (uint64_t)1 << 53;
    if (!n || interpolation < 1 || interpolation > RFA_PFB_MAX_INTERPOLATION || decimation < interpolation ||
        pfb_gcd(interpolation, decimation) != 1)
        return RFA_ERR_INVALID;
    if (consumed >= lim || (uint64_t)n_samples >= lim || consumed + (uint64_t)n_samples >= lim) return RFA_ERR_INVALID;
    *n = (size_t)(pfb_rational_count((long long)(consumed + n_samples), interpolation, decimation) -
                  pfb_rational_count((long long)consumed, interpolation, decimation));
    return RFA_OK;
}

int rfa_pfb_tile_plan(int32_t n_channels, int32_t interpolation, int32_t decimation, int32_t num_taps, int32_t *plan) {
    static_assert(RFA_PFB_PLAN_MAX_STAGES == kPfbMaxStages &&
                  RFA_PFB_PLAN_FIELDS == RFA_PFB_PLAN_RADIX0 + RFA_PFB_PLAN_MAX_STAGES);
    const bool rational = interpolation != 0;
    if (!plan) return RFA_ERR_INVALID;
    if (rational ? !pfb_rational_args_valid(n_channels, interpolation, decimation, num_taps)
                 : !pfb_integer_args_valid(n_channels, decimation, num_taps))
        return RFA_ERR_INVALID;
    const std::vector<int> radix = pfb_radices(n_channels);
    if (radix.empty()) return RFA_ERR_UNSUPPORTED;
    PfbRatLaunch b{};                                  // the record rfa_pfb_process fills, as pfb_create sizes it
    PfbLaunch &a = b.a;
    b.L = rational ? interpolation : 1;
    a.T = (num_taps + b.L - 1) / b.L;
    a.M = n_channels;
    a.D = decimation;
    pfb_plan(b, rational);
    plan[RFA_PFB_PLAN_TIMES] = a.NT;
    plan[RFA_PFB_PLAN_PITCH] = a.Mp;
    plan[RFA_PFB_PLAN_RUN] = a.run;
    plan[RFA_PFB_PLAN_STAGED_RUN] = rational ? b.stage_x : a.stage != 0;
    plan[RFA_PFB_PLAN_STAGED_TAPS] = rational ? b.tap_rows : a.stage != 0;
    plan[RFA_PFB_PLAN_ROWS_BY_TIME] = rational && b.tap_rows && b.L > a.NT;   // pfb_rational_kernel's !by_phase
    plan[RFA_PFB_PLAN_STAGE_POINTS] = a.stage;
    plan[RFA_PFB_PLAN_LDS_BYTES] = pfb_lds_bytes(a);
    plan[RFA_PFB_PLAN_STAGES] = (int32_t)radix.size();
    for (int s = 0; s < kPfbMaxStages; s++) plan[RFA_PFB_PLAN_RADIX0 + s] = s < (int)radix.size() ? radix[s] : 0;
    return RFA_OK;
}

int rfa_pfb_destroy(rfa_pfb *p) {
    if (!p) return RFA_ERR_INVALID;
    stage_close_stream(p);
    for (void *q : {(void *)p->d_taps, (void *)p->d_tw, (void *)p->d_chan, (void *)p->d_hist[0], (void *)p->d_hist[1],
                    p->d_in, (void *)p->d_out, (void *)p->d_tune_w, (void *)p->d_tune_step})
        if (q) hipFree(q);
    delete p;
    return RFA_OK;
}

const char *rfa_pfb_last_error(const rfa_pfb *p) { return stage_last_error(p); }

int rfa_pfb_get_plan(const rfa_pfb *p, int32_t *n_channels, int32_t *decimation, int32_t *num_taps, int32_t *radices,
                     int32_t cap, int32_t *count) {
    if (!p) return RFA_ERR_INVALID;
    if (n_channels) *n_channels = p->M;
    if (decimation) *decimation = p->D;
    if (num_taps) *num_taps = p->T;
    if (count) *count = (int32_t)p->radix.size();
    if (radices) {
        if (cap < (int32_t)p->radix.size()) return RFA_ERR_SIZE;
        for (size_t s = 0; s < p->radix.size(); s++) radices[s] = p->radix[s];
    }
    return RFA_OK;
}

int rfa_pfb_get_taps(const rfa_pfb *p, float *taps, size_t capacity, int32_t *num_taps) {
    if (!p) return RFA_ERR_INVALID;
    if (num_taps) *num_taps = p->T;
    if (taps) {
        if (capacity < p->taps.size()) return RFA_ERR_SIZE;
        std::memcpy(taps, p->taps.data(), p->taps.size() * sizeof(float));
    }
    return RFA_OK;
}

int rfa_pfb_set_channels(rfa_pfb *p, const int32_t *channels, int32_t count) {
    if (!p) return RFA_ERR_INVALID;
    if (count < 0 || count > p->M) return stage_fail(p, RFA_ERR_INVALID, "channel count outside 0 .. n_channels");
    std::vector<int32_t> ch;
    if (!channels || count == 0) {
        ch.resize(p->M);
        for (int k = 0; k < p->M; k++) ch[k] = k;
    } else {
        ch.assign(channels, channels + count);
        for (int32_t c : ch)
            if (c < 0 || c >= p->M) return stage_fail(p, RFA_ERR_INVALID, "channel outside 0 .. n_channels - 1");
    }
    STAGE_HIP(p, hipSetDevice(p->device));
    STAGE_HIP(p, hipStreamSynchronize(p->stream));     // an enqueued call still reads the old list
    STAGE_HIP(p, hipMemcpyAsync(p->d_chan, ch.data(), ch.size() * sizeof(int), hipMemcpyHostToDevice, p->stream));
    STAGE_HIP(p, hipStreamSynchronize(p->stream));
    p->channels = std::move(ch);
    p->tune_q = 0;                                     // the new slots are untuned
    p->tune_steps.clear();
    return RFA_OK;
}

int rfa_pfb_set_tuning(rfa_pfb *p, int32_t q, const int32_t *steps, int32_t count) {
    if (!p) return RFA_ERR_INVALID;
    if (q == 0 || !steps) {
        if (q != 0 && !pfb_tune_q_valid(q)) return stage_fail(p, RFA_ERR_INVALID, "tuning denominator outside 1 .. RFA_PFB_TUNE_MAX_STEPS");
        if (steps && count != (int32_t)p->channels.size())
            return stage_fail(p, RFA_ERR_INVALID, "tuning count differs from the selection");
        p->tune_q = 0;                                 // the next call launches the untuned kernels again
        p->tune_steps.clear();
        return RFA_OK;
    }
    if (!pfb_tune_q_valid(q)) return stage_fail(p, RFA_ERR_INVALID, "tuning denominator outside 1 .. RFA_PFB_TUNE_MAX_STEPS");
    if (count != (int32_t)p->channels.size())
        return stage_fail(p, RFA_ERR_INVALID, "tuning count differs from the selection");
    for (int32_t j = 0; j < count; j++)
        if (steps[j] <= -q || steps[j] >= q) return stage_fail(p, RFA_ERR_INVALID, "tuning step outside -q < m < q");
    STAGE_HIP(p, hipSetDevice(p->device));
    if (!p->tuned_prepared) {
        for (int fmt : {RFA_IN_S8, RFA_IN_U8, RFA_IN_S16LE, RFA_IN_F32_INTERLEAVED}) {
            STAGE_HIP(p, stage_dispatch_format(
                             fmt, [](auto f) { return pfb_prepare(pfb_kernel<decltype(f)::value, PfbTunedLaunch>); }));
            STAGE_HIP(p, stage_dispatch_format(
                             fmt, [](auto f) { return pfb_prepare(pfb_rational_kernel<decltype(f)::value, PfbRatTunedLaunch>); }));
        }
        p->tuned_prepared = true;
    }
    // a table or step list an enqueued call still reads is neither freed nor overwritten
    STAGE_HIP(p, hipStreamSynchronize(p->stream));
    if (!p->d_tune_step && hipMalloc(&p->d_tune_step, (size_t)p->M * sizeof(int)) != hipSuccess)
        return stage_fail(p, RFA_ERR_NOMEM, "hipMalloc tuning steps");
    const bool new_table = q != p->tune_q || !p->d_tune_w;
    if ((size_t)q > p->tune_w_cap) {
        float2 *w = nullptr;
        if (hipMalloc(&w, (size_t)q * sizeof(float2)) != hipSuccess)
            return stage_fail(p, RFA_ERR_NOMEM, "hipMalloc tuning table");
        if (p->d_tune_w) hipFree(p->d_tune_w);
        p->d_tune_w = w;
        p->tune_w_cap = (size_t)q;
        p->tune_q = 0;                                 // the old table is gone: no tuning until the new one is up
        p->tune_steps.clear();
    }
    if (new_table) {
        std::vector<float2> w((size_t)q);
        for (int32_t i = 0; i < q; i++) w[(size_t)i] = pfb_tune_entry(i, q);
        p->tune_q = 0;
        STAGE_HIP(p, hipMemcpyAsync(p->d_tune_w, w.data(), w.size() * sizeof(float2), hipMemcpyHostToDevice, p->stream));
        STAGE_HIP(p, hipStreamSynchronize(p->stream));
    }
    STAGE_HIP(p, hipMemcpyAsync(p->d_tune_step, steps, (size_t)count * sizeof(int), hipMemcpyHostToDevice, p->stream));
    STAGE_HIP(p, hipStreamSynchronize(p->stream));
    p->tune_q = q;
    p->tune_steps.assign(steps, steps + count);
    return RFA_OK;
}

int rfa_pfb_get_tuning(const rfa_pfb *p, int32_t *q, int32_t *steps, size_t capacity, int32_t *count) {
    if (!p) return RFA_ERR_INVALID;
    if (q) *q = p->tune_q;
    if (count) *count = (int32_t)p->tune_steps.size();
    if (steps) {
        if (capacity < p->tune_steps.size()) return RFA_ERR_SIZE;
        std::memcpy(steps, p->tune_steps.data(), p->tune_steps.size() * sizeof(int32_t));
    }
    return RFA_OK;
}

int rfa_pfb_tuning_index(int32_t q, int32_t step, uint64_t n, int32_t *i) {
    if (!i || !pfb_tune_q_valid(q) || step <= -q || step >= q || n >= (uint64_t)1 << 53) return RFA_ERR_INVALID;
    *i = (int32_t)pfb_tune_index((unsigned)q, pfb_tune_mu((unsigned)q), step, n);
    return RFA_OK;
}

int rfa_pfb_tuning_table(int32_t q, float *cos_t, float *sin_t, size_t capacity) {
    if (!pfb_tune_q_valid(q) || !cos_t || !sin_t) return RFA_ERR_INVALID;
    if (capacity < (size_t)q) return RFA_ERR_SIZE;
    for (int32_t j = 0; j < q; j++) {
        const float2 w = pfb_tune_entry(j, q);
        cos_t[j] = w.x;
        sin_t[j] = w.y;
    }
    return RFA_OK;
}

int rfa_pfb_get_channels(const rfa_pfb *p, int32_t *channels, size_t capacity, int32_t *count) {
    if (!p) return RFA_ERR_INVALID;
    if (count) *count = (int32_t)p->channels.size();
    if (channels) {
        if (capacity < p->channels.size()) return RFA_ERR_SIZE;
        std::memcpy(channels, p->channels.data(), p->channels.size() * sizeof(int32_t));
    }
    return RFA_OK;
}

int rfa_pfb_max_outputs(const rfa_pfb *p, size_t n_samples, size_t *n) {
    if (!p || !n || n_samples > (size_t)1 << 40) return RFA_ERR_INVALID;
    *n = (size_t)pfb_outputs(p, (long long)n_samples);
    return RFA_OK;
}

int rfa_pfb_process(rfa_pfb *p, const void *in, size_t n_samples, float *out_re, float *out_im, size_t channel_stride,
                    size_t *n_out) {
    if (!p || !n_out) return RFA_ERR_INVALID;
    *n_out = 0;
    if (n_samples == 0) return RFA_OK;
    const size_t sb = stage_sample_bytes(p->fmt);
    if (!in || (uintptr_t)in % sb != 0) return stage_fail(p, RFA_ERR_INVALID, "input pointer null or misaligned");
    if (n_samples > (size_t)1 << 40) return stage_fail(p, RFA_ERR_INVALID, "n_samples too large");
    const long long S = (long long)n_samples;
    if (p->rational && p->in_done + S >= (long long)1 << 53) return stage_fail(p, RFA_ERR_INVALID, "stream longer than 2^53 samples");
    const long long n = pfb_outputs(p, S);
    if ((size_t)n > channel_stride) return stage_fail(p, RFA_ERR_SIZE, "channel_stride smaller than the output count");
    if (n > 0 && (!out_re || !out_im)) return RFA_ERR_INVALID;
    PfbRatLaunch b{};
    PfbLaunch &a = b.a;
    a.raw = in;
    a.S = S;
    a.hist = p->d_hist[p->cur];
    a.new_hist = p->d_hist[p->cur ^ 1];
    a.taps = p->d_taps;
    a.T = p->Th;
    a.M = p->M;
    a.D = p->D;
    b.L = p->L;
    pfb_plan(b, p->rational);
    a.n0 = p->rational ? pfb_rational_count(p->in_done, p->L, p->D) : p->in_done / p->D;
    a.in0 = p->in_done;
    a.n_out = n;
    a.tw = p->d_tw;
    a.nstages = (int)p->radix.size();
    for (int s = 0; s < a.nstages; s++) a.radix[s] = p->radix[s], a.tw_off[s] = p->tw_off[s];
    a.chan = p->d_chan;
    a.K = (int)p->channels.size();
    a.stride = (long long)channel_stride;
    a.out_re = out_re;
    a.out_im = out_im;
    if ((n + a.NT - 1) / a.NT > (long long)INT32_MAX) return stage_fail(p, RFA_ERR_INVALID, "call too large for one grid");
    STAGE_HIP(p, hipSetDevice(p->device));
    const hipError_t e = stage_dispatch_format(p->fmt, [&](auto f) {
        constexpr int FMT = decltype(f)::value;
        if (p->tune_q) {                               // the tuned siblings, same grid and LDS: still two launches
            const PfbTune t{p->d_tune_w, p->d_tune_step, (unsigned)p->tune_q, pfb_tune_mu((unsigned)p->tune_q)};
            return p->rational ? pfb_launch<FMT>(pfb_rational_kernel<FMT, PfbRatTunedLaunch>, PfbRatTunedLaunch{b, t}, a,
                                                 p->stream)
                               : pfb_launch<FMT>(pfb_kernel<FMT, PfbTunedLaunch>, PfbTunedLaunch{a, t}, a, p->stream);
        }
        return p->rational ? pfb_launch<FMT>(pfb_rational_kernel<FMT>, b, a, p->stream)
                           : pfb_launch<FMT>(pfb_kernel<FMT>, a, a, p->stream);
    });
    if (e != hipSuccess) return stage_fail(p, RFA_ERR_HIP, std::string("channelizer launch: ") + hipGetErrorString(e));
    if (a.T > 1) p->cur ^= 1;
    p->in_done += S;
    *n_out = (size_t)n;
    return RFA_OK;
}

int rfa_pfb_process_host(rfa_pfb *p, const void *in, size_t n_samples, float *out_re, float *out_im,
                         size_t channel_stride, size_t *n_out) {
    if (!p || !n_out || (n_samples && !in)) return RFA_ERR_INVALID;
    *n_out = 0;
    if (n_samples == 0) return RFA_OK;
    if (n_samples > (size_t)1 << 40) return stage_fail(p, RFA_ERR_INVALID, "n_samples too large");
    const size_t K = p->channels.size();
    const size_t bytes = n_samples * stage_sample_bytes(p->fmt);
    const size_t most = (size_t)pfb_outputs(p, (long long)n_samples);
    if (most > channel_stride) return stage_fail(p, RFA_ERR_SIZE, "channel_stride smaller than the output count");
    if (most > 0 && (!out_re || !out_im)) return RFA_ERR_INVALID;
    STAGE_HIP(p, hipSetDevice(p->device));
    const size_t pitch = most + 1;
    int rc = stage_grow(p, p->d_in, p->d_in_cap, bytes, "input staging");
    if (rc == RFA_OK) rc = stage_grow(p, p->d_out, p->d_out_cap, 2 * K * pitch, "output staging");
    if (rc != RFA_OK) return rc;
    STAGE_HIP(p, hipMemcpyAsync(p->d_in, in, bytes, hipMemcpyHostToDevice, p->stream));
    size_t n = 0;
    rc = rfa_pfb_process(p, p->d_in, n_samples, p->d_out, p->d_out + K * pitch, pitch, &n);
    if (rc != RFA_OK) return rc;
    if (n) {
        STAGE_HIP(p, hipMemcpy2DAsync(out_re, channel_stride * sizeof(float), p->d_out, pitch * sizeof(float),
                                 n * sizeof(float), K, hipMemcpyDeviceToHost, p->stream));
        STAGE_HIP(p, hipMemcpy2DAsync(out_im, channel_stride * sizeof(float), p->d_out + K * pitch, pitch * sizeof(float),
                                 n * sizeof(float), K, hipMemcpyDeviceToHost, p->stream));
    }
    STAGE_HIP(p, hipStreamSynchronize(p->stream));
    *n_out = n;
    return RFA_OK;
}

int rfa_pfb_reset(rfa_pfb *p) {
    if (!p) return RFA_ERR_INVALID;
    STAGE_HIP(p, hipSetDevice(p->device));
    const size_t H = (size_t)std::max(1, p->Th - 1);
    STAGE_HIP(p, hipMemsetAsync(p->d_hist[p->cur], 0, 2 * H * sizeof(float), p->stream));
    STAGE_HIP(p, hipStreamSynchronize(p->stream));
    p->in_done = 0;
    return RFA_OK;
}

int rfa_pfb_set_stream(rfa_pfb *p, void *stream) { return stage_set_stream(p, stream); }

int rfa_pfb_get_stream(const rfa_pfb *p, void **stream) { return stage_get_stream(p, stream); }

int rfa_pfb_synchronize(rfa_pfb *p) { return stage_synchronize(p); }

}  // extern "C"
