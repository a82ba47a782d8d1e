// The form the batch window kernel replaces, timed alone: a (window, frame) grid of the
// one-workgroup-per-window reduction rfa_row_window_stats uses (csrc/display.hip
// row_window_kernel), over `frames` natural-order rows of n floats in HBM and a +-2-bin grid
// of `windows` windows.  tools/window_stats_bench.py runs it and records the figure beside the
// product kernel's.  Prints one JSON line.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHK(x)                                                                          \
    do {                                                                                \
        hipError_t e_ = (x);                                                            \
        if (e_ != hipSuccess) {                                                         \
            std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));                \
            return 1;                                                                   \
        }                                                                               \
    } while (0)

__global__ void fill_rows(float *p, size_t count) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x)
        p[i] = -80.0f + (float)((i * 2654435761u) >> 24 & 63) * 0.25f;
}

__global__ void __launch_bounds__(256) window_grid_kernel(const float *rows, int n, const int *lo, const int *hi,
                                                          int count, float *peak, float *avg) {
    const int w = blockIdx.x, f = blockIdx.y;
    const float *row = rows + (size_t)f * n;
    const int a = lo[w], b = hi[w];
    float mx = -INFINITY;
    bool nan = false;
    double s = 0.0;
    for (int j = a + (int)threadIdx.x; j <= b; j += 256) {
        const float x = row[j];
        nan |= x != x;
        mx = x > mx ? x : mx;
        s += (double)x;
    }
    __shared__ double ss[256];
    __shared__ float sm[256];
    __shared__ int sn[256];
    ss[threadIdx.x] = s;
    sm[threadIdx.x] = mx;
    sn[threadIdx.x] = nan;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) {
            ss[threadIdx.x] += ss[threadIdx.x + k];
            sm[threadIdx.x] = fmaxf(sm[threadIdx.x], sm[threadIdx.x + k]);
            sn[threadIdx.x] |= sn[threadIdx.x + k];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        peak[(size_t)f * count + w] = sn[0] ? NAN : sm[0];
        avg[(size_t)f * count + w] = (float)(ss[0] / (double)(b - a + 1));
    }
}

int main(int argc, char **argv) {
    const int n = argc > 1 ? std::atoi(argv[1]) : 65536, frames = argc > 2 ? std::atoi(argv[2]) : 500;
    const int windows = argc > 3 ? std::atoi(argv[3]) : 1600, reps = argc > 4 ? std::atoi(argv[4]) : 9;
    if (n < 8 || frames < 1 || frames > 65535 || windows < 1 || windows > n / 5 || reps < 1) {
        std::fprintf(stderr, "usage: window_grid_bench [n frames windows reps]\n");
        return 2;
    }
    std::vector<int> lo(windows), hi(windows);
    const int step = n / windows;
    for (int i = 0; i < windows; i++) {
        const int b = std::min(n - 3, 2 + i * step);
        lo[i] = b - 2;
        hi[i] = b + 2;
    }
    // two row sets, alternated, so a repeat does not find its rows in the Infinity Cache
    float *rows[2], *peak, *avg;
    int *dlo, *dhi;
    const size_t count = (size_t)frames * n;
    for (float *&r : rows) {
        CHK(hipMalloc(&r, count * sizeof(float)));
        fill_rows<<<4096, 256>>>(r, count);
    }
    CHK(hipMalloc(&peak, (size_t)frames * windows * sizeof(float)));
    CHK(hipMalloc(&avg, (size_t)frames * windows * sizeof(float)));
    CHK(hipMalloc(&dlo, windows * sizeof(int)));
    CHK(hipMalloc(&dhi, windows * sizeof(int)));
    CHK(hipMemcpy(dlo, lo.data(), windows * sizeof(int), hipMemcpyHostToDevice));
    CHK(hipMemcpy(dhi, hi.data(), windows * sizeof(int), hipMemcpyHostToDevice));
    hipEvent_t e0, e1;
    CHK(hipEventCreate(&e0));
    CHK(hipEventCreate(&e1));
    std::vector<float> us;
    for (int r = 0; r < reps + 2; r++) {
        CHK(hipEventRecord(e0, nullptr));
        window_grid_kernel<<<dim3(windows, frames), 256>>>(rows[r & 1], n, dlo, dhi, windows, peak, avg);
        CHK(hipEventRecord(e1, nullptr));
        CHK(hipEventSynchronize(e1));
        float ms = 0.f;
        CHK(hipEventElapsedTime(&ms, e0, e1));
        if (r >= 2) us.push_back(ms * 1e3f);
    }
    CHK(hipGetLastError());
    std::sort(us.begin(), us.end());
    std::printf("{\"n\": %d, \"frames\": %d, \"windows\": %d, \"workgroups\": %lld, \"grid_us_min_median_max\": [%.1f, %.1f, %.1f]}\n",
                n, frames, windows, (long long)windows * frames, us.front(), us[us.size() / 2], us.back());
    return 0;
}
