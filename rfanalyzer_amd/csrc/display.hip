// Display preprocessing on the device: the reference's
// AnalyzerSurface.drawPreprocessing (app/.../ui/AnalyzerSurface.kt:599-743)
// computed from the waterfall ring where it already lives, so a frame of the UI
// needs width-sized rows back instead of N-float rows.
//
// Per ring row (newest first, rowNumber r -> bufferIndex (readIndex + r) % R) and
// pixel i inside (firstPixel, lastPixel - 1): the mean of the row's bins
// j in [(int)(i*spp), (i+1)*spp) (stopping at N), summed in bin order in fp32
// (AnalyzerSurface.kt:693-705); the colour map index ((avg - minDB) * scale)
// truncated and clamped (:721-722); black outside (:725).  Rows 0..L feed the
// time average, summed newest first per pixel (:710-714), whose spectrum-path y
// and autoscale min/max come from draw_finish_kernel; row 0 also gives the
// peak-hold y (:707).  Every float operation is the reference's single fp32
// operation in the reference's order (no FMA contraction), so the results are
// bit-identical to the JVM's.
#include <hip/hip_runtime.h>

#include <cmath>

#include "fft_kernels.h"
#include "wave.h"

namespace rfa {

#pragma clang fp contract(off)

// Kotlin Float.toInt(): truncation, NaN -> 0, saturating.
__device__ __forceinline__ int kt_toint(float x) {
    if (x != x) return 0;
    if (x >= 2147483648.0f) return 2147483647;
    if (x <= -2147483648.0f) return (-2147483647 - 1);
    return (int)x;
}

// java.lang.Math.min / max on floats: NaN wins, -0 < +0.
__device__ __forceinline__ float jmin(float a, float b) {
    if (a != a || b != b) return NAN;
    if (a == b) return signbit(a) ? a : b;
    return a < b ? a : b;
}
__device__ __forceinline__ float jmax(float a, float b) {
    if (a != a || b != b) return NAN;
    if (a == b) return signbit(a) ? b : a;
    return a > b ? a : b;
}

// `i in (firstPixel + 1)..<lastPixel-1` (AnalyzerSurface.kt:694) in Kotlin's Int arithmetic, which
// wraps: a viewport narrower than one bin has samplesPerPx == 0, firstPixel saturates to
// Int.MAX_VALUE or lastPixel to Int.MIN_VALUE (:668,671), and the bound lands at the other end of
// the range (lastPixel - 1 == Int.MAX_VALUE draws every pixel above firstPixel, from no bins).
__device__ __forceinline__ bool pixel_drawn(int i, int first_pixel, int last_pixel) {
    const int lo = (int)((unsigned)first_pixel + 1u), hi = (int)((unsigned)last_pixel - 1u);
    return i >= lo && i < hi;
}

// One block row per refreshed ring row (the host picks them as the reference's
// dirty-row loop does, AnalyzerSurface.kt:678-684); the other rows keep their colours.
__global__ void __launch_bounds__(256) draw_rows_kernel(DrawLaunch a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int2 sel = a.rows[blockIdx.y];
    const int row_number = sel.x;
    if (i >= a.width) return;
    const int buffer_index = sel.y;
    const float *row = a.ring + (size_t)buffer_index * a.n;
    const int lm = ring_logm(a.ring_logrs, 31 - __clz(a.n));  // ring storage order (ring_pos)
    unsigned *out = a.colors + (size_t)buffer_index * a.width + i;
    if (pixel_drawn(i, a.first_pixel, a.last_pixel)) {
        const bool peaks_here = row_number == 0 && a.peaks_y;
        float avg = 0.0f, peak_avg = 0.0f;
        int counter = 0;
        const float hi = (float)(i + 1) * a.samples_per_px;
        // (the reference reads fftRow[j + start] unchecked; a negative index -- which
        // would throw there -- is skipped here instead of read)
        int j = kt_toint((float)i * a.samples_per_px);
        if (j + a.start < 0) j = -a.start;
        for (; (float)j < hi && j + a.start < a.n; j++) {
            avg += row[ring_pos(j + a.start, a.ring_logrs, lm)];
            if (peaks_here) peak_avg += a.peaks[j + a.start];
            counter++;
        }
        avg = avg / (float)counter;
        if (peaks_here) {
            const float pk = peak_avg / (float)counter;
            a.peaks_y[i] = (float)a.fft_height - (pk - a.min_db) * a.db_width;
        }
        if (row_number <= a.avg_length) a.avg_rows[(size_t)row_number * a.width + i] = avg;
        int ci = kt_toint((avg - a.min_db) * a.scale);
        ci = ci < 0 ? 0 : (ci >= a.colormap_size ? a.colormap_size - 1 : ci);
        *out = a.colormap[ci];
    } else {
        *out = 0xff000000u;  // Color.rgb(0, 0, 0)
        if (row_number == 0 && a.peaks_y) a.peaks_y[i] = -1.0f;
    }
}

// Time average of rows 0..L per pixel (newest first), spectrum-path y, autoscale
// min/max starting from (VERTICAL_SCALE_UPPER_BOUNDARY, _LOWER_BOUNDARY) =
// (10, -100) (AppStateRepository.kt:92-93).  One workgroup; path y is NaN where
// the reference adds no path point.
__global__ void __launch_bounds__(1024) draw_finish_kernel(DrawLaunch a) {
    __shared__ float smin[16], smax[16];
    float mn = 10.0f, mx = -100.0f;
    for (int i = threadIdx.x; i < a.width; i += blockDim.x) {
        if (pixel_drawn(i, a.first_pixel, a.last_pixel)) {
            float acc = 0.0f;
            for (int r = 0; r <= a.avg_length; r++) acc += a.avg_rows[(size_t)r * a.width + i];
            const float ta = acc / (float)(a.avg_length + 1);
            a.path_y[i] = (float)a.fft_height - (ta - a.min_db) * a.db_width;
            mn = jmin(ta, mn);
            mx = jmax(ta, mx);
        } else {
            a.path_y[i] = NAN;
        }
    }
    // min / max are order independent (NaN propagates either way): per wave by
    // cross-lane moves (wave.h), then the waves' results
    mn = wave_reduce(mn, [](float x, float y) { return jmin(x, y); });
    mx = wave_reduce(mx, [](float x, float y) { return jmax(x, y); });
    const int nw = (blockDim.x + 63) / 64;
    if ((threadIdx.x & 63) == 0) {
        smin[threadIdx.x >> 6] = mn;
        smax[threadIdx.x >> 6] = mx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < nw; k++) {
            mn = jmin(mn, smin[k]);
            mx = jmax(mx, smax[k]);
        }
        a.autoscale[0] = mn;
        a.autoscale[1] = mx;
    }
}

// Newest-row window statistics for the scanners and squelch (SURVEY.md §8(f)
// row 2; MainViewModel.kt:861-929 detectIEMChannelsInFFT, :1391-1457
// getAverageSignalLevel / detectSignal, :1462-1540 detectSignalsInFFT): for every
// window [lo, hi] (inclusive bins of the fft-shifted row) the peak
// (FloatArray.maxOrNull: NaN wins) and FloatArray.average() -- a double sum
// divided by the count, then toFloat().  One workgroup per window; the double
// partial sums meet by wavefront shuffles and then across the four waves (a different
// summation order than the JVM's sequential one, equal after the final rounding to
// float up to one ulp).
__global__ void __launch_bounds__(256) row_window_kernel(const float *row, int logrs, int n, const int *lo,
                                                         const int *hi, int count, float *peak, float *avg) {
    const int w = blockIdx.x;
    if (w >= count) return;
    const int lm = ring_logm(logrs, 31 - __clz(n));  // ring storage order (ring_pos)
    const int a = lo[w], b = hi[w];
    float mx = -INFINITY;
    bool nan = false;
    double s = 0.0;
    for (int j = a + (int)threadIdx.x; j <= b; j += 256) {
        const float x = row[ring_pos(j, logrs, lm)];
        nan |= x != x;
        mx = x > mx ? x : mx;
        s += (double)x;
    }
    // per wave by cross-lane moves (wave.h), then the four waves in order
    s = wave_reduce(s, [](double x, double y) { return x + y; });
    mx = wave_reduce(mx, [](float x, float y) { return fmaxf(x, y); });
    const int anynan = wave_reduce((int)nan, [](int x, int y) { return x | y; });
    __shared__ double ss[4];
    __shared__ float sm[4];
    __shared__ int sn[4];
    if ((threadIdx.x & 63) == 0) {
        ss[threadIdx.x >> 6] = s;
        sm[threadIdx.x >> 6] = mx;
        sn[threadIdx.x >> 6] = anynan;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double sum = ((ss[0] + ss[1]) + ss[2]) + ss[3];
        const float m = fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3]));
        peak[w] = (sn[0] | sn[1] | sn[2] | sn[3]) ? NAN : m;
        avg[w] = (float)(sum / (double)(b - a + 1));
    }
}

hipError_t launch_row_windows(const float *row, int ring_logrs, int n, const int *lo, const int *hi, int count,
                              float *peak, float *avg, hipStream_t s) {
    if (count <= 0) return hipSuccess;
    hipLaunchKernelGGL(row_window_kernel, dim3(count), dim3(256), 0, s, row, ring_logrs, n, lo, hi, count, peak, avg);
    return hipGetLastError();
}

// The same two reductions for a window LIST and EVERY row of a batch (rfa_set_windows,
// rfa_ring_window_stats).  A (window, frame) grid of the kernel above re-reads
// the row once per window and starts a workgroup for a handful of loads; here a workgroup takes
// one block of a.block_bins natural bins of one row, copies it to LDS once -- 16-B loads that walk
// the block's STORAGE positions (WinSeg), each element dropped at its natural bin -- and then
// reduces every window piece that lies in the block from LDS: a piece of up to kWinNarrow bins by
// one lane in bin order, one of up to kWinWave bins by one wave (lane l takes bins lo + l,
// lo + l + 64, ..., the 64 partials meet by the wave.h shuffles), a wider one by the workgroup
// (thread t takes lo + t, lo + t + 256, ...; waves as before, then the four waves in order).  The host plan cuts windows at multiples of
// win_piece_bins(), so which lanes add which bins depends on (lo, hi) alone: a window's result
// does not depend on the rest of the list, on the frame's place in the batch or on the row
// source.  Windows of several pieces leave (double sum, NaN-wins max) per piece and
// window_fold_kernel adds them in bin order.  No prefix sums: rows hold -inf, +inf and NaN.
//
// WinSeg: the block's storage positions.  ring_pos permutes bits, so the positions of an aligned
// block are ring_pos(base) | q with q running over a fixed bit set; counting j = 0, 4, 8, ...
// and dealing j's bits into that set, lowest first, walks them in ascending storage order.  The
// set is at most three runs of adjacent bits in every ring order (two for the store tiles:
// bits 0-7 and 11 up), so q is three shift-and-mask terms.
struct WinSeg {
    int src[3], mask[3], dst[3];
};

__device__ __forceinline__ int win_pad(int o) { return o + (o >> 5); }  // LDS pitch 33: column-order scatters

__device__ __forceinline__ void win_emit(const WinLaunch &a, int f, const int4 p, float mx, bool nan, double s) {
    if (p.z >= 0) {
        const size_t o = (size_t)f * a.n_windows + p.z;
        a.peak[o] = nan ? NAN : mx;
        a.avg[o] = (float)(s / (double)(p.y - p.x + 1));
    } else {
        const size_t o = (size_t)f * a.n_slots + ~p.z;
        a.psum[o] = s;
        a.pmax[o] = nan ? NAN : mx;
    }
}

__global__ void __launch_bounds__(256) batch_window_kernel(WinLaunch a, WinSeg g) {
    extern __shared__ __attribute__((aligned(16))) float win_lds[];
    __shared__ double gs[4];
    __shared__ float gm[4];
    __shared__ int gn[4];
    const int4 job = a.jobs[blockIdx.x];
    const int end = a.jobs[blockIdx.x + 1].y;  // (the list ends with a sentinel job)
    const int code = a.ring_rows > 0 ? a.ring_logrs : 0;
    const int lm = ring_logm(code, 31 - __clz(a.n));
    const int base = job.x * a.block_bins, pbase = ring_pos(base, code, lm);
    // natural offsets of the four elements of a 16-B group
    const int d1 = ring_bin(1, code, lm), d2 = ring_bin(2, code, lm), d3 = ring_bin(3, code, lm);
    const int lane = threadIdx.x & 63;
    for (int f = blockIdx.y; f < a.n_frames; f += gridDim.y) {
        const float *row;
        if (a.ring_rows > 0) {
            int rr = (int)(((long long)a.ring_base + (long long)a.ring_dir * f) % a.ring_rows);
            row = a.rows + (size_t)(rr < 0 ? rr + a.ring_rows : rr) * a.n;
        } else {
            row = a.rows + (size_t)((long long)f * a.row_stride);
        }
        for (int j = 4 * (int)threadIdx.x; j < a.block_bins; j += 4 * 256) {
            const int q = (((j >> g.src[0]) & g.mask[0]) << g.dst[0]) | (((j >> g.src[1]) & g.mask[1]) << g.dst[1]) |
                          (((j >> g.src[2]) & g.mask[2]) << g.dst[2]);
            const float4 x = *reinterpret_cast<const float4 *>(row + (pbase | q));
            const int b0 = ring_bin(q, code, lm);
            win_lds[win_pad(b0)] = x.x;
            win_lds[win_pad(b0 | d1)] = x.y;
            win_lds[win_pad(b0 | d2)] = x.z;
            win_lds[win_pad(b0 | d3)] = x.w;
        }
        __syncthreads();
        for (int i = job.y + (int)threadIdx.x; i < job.z; i += 256) {  // narrow pieces: a lane each
            const int4 p = a.pieces[i];
            float mx = -INFINITY;
            bool nan = false;
            double s = 0.0;
            for (int o = p.x - base; o <= p.y - base; o++) {
                const float x = win_lds[win_pad(o)];
                nan |= x != x;
                mx = x > mx ? x : mx;
                s += (double)x;
            }
            win_emit(a, f, p, mx, nan, s);
        }
        for (int i = job.z + (int)(threadIdx.x >> 6); i < job.w; i += 4) {  // medium pieces: a wave each
            const int4 p = a.pieces[i];
            float mx = -INFINITY;
            bool nan = false;
            double s = 0.0;
            for (int o = p.x - base + lane; o <= p.y - base; o += 64) {
                const float x = win_lds[win_pad(o)];
                nan |= x != x;
                mx = x > mx ? x : mx;
                s += (double)x;
            }
            s = wave_reduce(s, [](double x, double y) { return x + y; });
            mx = wave_reduce(mx, [](float x, float y) { return fmaxf(x, y); });
            const int anynan = wave_reduce((int)nan, [](int x, int y) { return x | y; });
            if (lane == 0) win_emit(a, f, p, mx, anynan != 0, s);
        }
        for (int i = job.w; i < end; i++) {  // wide pieces: the workgroup, as row_window_kernel
            const int4 p = a.pieces[i];
            float mx = -INFINITY;
            bool nan = false;
            double s = 0.0;
            for (int o = p.x - base + (int)threadIdx.x; o <= p.y - base; o += 256) {
                const float x = win_lds[win_pad(o)];
                nan |= x != x;
                mx = x > mx ? x : mx;
                s += (double)x;
            }
            s = wave_reduce(s, [](double x, double y) { return x + y; });
            mx = wave_reduce(mx, [](float x, float y) { return fmaxf(x, y); });
            const int anynan = wave_reduce((int)nan, [](int x, int y) { return x | y; });
            if (lane == 0) {
                gs[threadIdx.x >> 6] = s;
                gm[threadIdx.x >> 6] = mx;
                gn[threadIdx.x >> 6] = anynan;
            }
            __syncthreads();
            if (threadIdx.x == 0)
                win_emit(a, f, p, fmaxf(fmaxf(gm[0], gm[1]), fmaxf(gm[2], gm[3])), (gn[0] | gn[1] | gn[2] | gn[3]) != 0,
                         ((gs[0] + gs[1]) + gs[2]) + gs[3]);
            __syncthreads();
        }
        __syncthreads();  // the next row overwrites the block
    }
}

// Windows that cross a piece boundary: their pieces' sums added in bin order, NaN-wins max.
__global__ void __launch_bounds__(256) window_fold_kernel(WinLaunch a) {
    const long long total = (long long)a.n_frames * a.n_folds;
    for (long long t = blockIdx.x * 256ll + threadIdx.x; t < total; t += (long long)gridDim.x * 256) {
        const long long f = t / a.n_folds;
        const int4 e = a.folds[(int)(t % a.n_folds)];
        const double *ps = a.psum + (size_t)f * a.n_slots + e.y;
        const float *pm = a.pmax + (size_t)f * a.n_slots + e.y;
        float mx = -INFINITY;
        bool nan = false;
        double s = 0.0;
        for (int i = 0; i < e.z; i++) {
            const float x = pm[i];
            nan |= x != x;
            mx = x > mx ? x : mx;
            s += ps[i];
        }
        const size_t o = (size_t)f * a.n_windows + e.x;
        a.peak[o] = nan ? NAN : mx;
        a.avg[o] = (float)(s / (double)e.w);
    }
}

hipError_t launch_batch_windows(const WinLaunch &a) {
    if (a.n_frames <= 0 || a.n_windows <= 0 || a.n_jobs <= 0) return hipSuccess;
    const int code = a.ring_rows > 0 ? a.ring_logrs : 0;
    int logn = 0, logb = 0;
    while ((1 << logn) < a.n) logn++;
    while ((1 << logb) < a.block_bins) logb++;
    if ((1 << logn) != a.n || (1 << logb) != a.block_bins || a.block_bins > a.n || a.block_bins < 4)
        return hipErrorInvalidValue;
    // the storage bits of a block's natural bits, as runs of adjacent bits (WinSeg)
    const int lm = ring_logm(code, logn);
    unsigned set = 0;
    for (int k = 0; k < logb; k++) set |= (unsigned)ring_pos(1 << k, code, lm);
    if ((set & 3u) != 3u) return hipErrorInvalidValue;  // 16-B groups
    WinSeg g{};
    int runs = 0, taken = 0;
    for (int b = 0; b < 32;) {
        if (!(set >> b & 1u)) { b++; continue; }
        int w = 0;
        while (b + w < 32 && (set >> (b + w) & 1u)) w++;
        if (runs == 3) return hipErrorInvalidValue;
        g.src[runs] = taken;
        g.mask[runs] = (1 << w) - 1;
        g.dst[runs] = b;
        runs++;
        taken += w;
        b += w;
    }
    const size_t lds = (size_t)(a.block_bins + (a.block_bins >> 5) + 1) * sizeof(float);
    if (lds > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&batch_window_kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    const int gy = a.n_frames < 32768 ? a.n_frames : 32768;
    hipLaunchKernelGGL(batch_window_kernel, dim3(a.n_jobs, gy), dim3(256), lds, a.stream, a, g);
    if (a.n_folds > 0) {
        const long long total = (long long)a.n_frames * a.n_folds;
        const int gx = (int)((total + 255) / 256 < 65536 ? (total + 255) / 256 : 65536);
        hipLaunchKernelGGL(window_fold_kernel, dim3(gx), dim3(256), 0, a.stream, a);
    }
    return hipGetLastError();
}

hipError_t launch_draw(const DrawLaunch &a) {
    if (a.width <= 0 || a.ring_rows <= 0 || a.n_rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(draw_rows_kernel, dim3((a.width + 255) / 256, a.n_rows), dim3(256), 0, a.stream, a);
    hipLaunchKernelGGL(draw_finish_kernel, dim3(1), dim3(1024), 0, a.stream, a);
    return hipGetLastError();
}

}  // namespace rfa
