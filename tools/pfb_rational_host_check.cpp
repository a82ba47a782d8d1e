// Host-side check of the rational-rate channelizer's C-ABI entries that need no
// device: the count rule (rfa_pfb_rational_outputs), the argument checks of
// rfa_pfb_create_rational that return before any HIP call, each limit one step
// inside and one step outside, and the null-handle paths of the new entries.
// Built together with rfanalyzer_amd/csrc/channelizer.hip with the host compiled
// under AddressSanitizer and UBSan (tools/Makefile) and run as an ordinary
// program; exits 0 when every check holds.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../include/rfa.h"

static int failures = 0;

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            failures++;                                                    \
        }                                                                  \
    } while (0)

static unsigned __int128 ceil_ratio(uint64_t c, int l, int d) {
    return ((unsigned __int128)c * (unsigned)l + (unsigned)(d - 1)) / (unsigned)d;
}

static void check_count_rule() {
    size_t n = 99;
    const int ratios[][2] = {{1, 1}, {1, 7}, {3, 7}, {4, 9}, {3, 64}, {12, 125}, {3, 625}, {48, 125}, {64, 65}, {63, 64},
                             {64, 4095}};
    const uint64_t big = ((uint64_t)1 << 52) - 5;
    for (const auto &r : ratios) {
        uint64_t c = 0;
        uint64_t step = 1;
        for (int i = 0; i < 200; i++) {                       // a stream cut into growing calls
            CHECK(rfa_pfb_rational_outputs(r[0], r[1], c, (size_t)step, &n) == RFA_OK);
            CHECK((unsigned __int128)n == ceil_ratio(c + step, r[0], r[1]) - ceil_ratio(c, r[0], r[1]));
            c += step;
            step = (step * 3 + (uint64_t)i) % 1000;
        }
        CHECK(rfa_pfb_rational_outputs(r[0], r[1], 0, 0, &n) == RFA_OK && n == 0);
        CHECK(rfa_pfb_rational_outputs(r[0], r[1], 0, 1, &n) == RFA_OK && n == 1);   // output 0 is due with sample 0
        for (uint64_t k = 0; k < 12; k++) {                   // consumed near 2^52
            CHECK(rfa_pfb_rational_outputs(r[0], r[1], big + k, 1000 + (size_t)k, &n) == RFA_OK);
            CHECK((unsigned __int128)n == ceil_ratio(big + k + 1000 + k, r[0], r[1]) - ceil_ratio(big + k, r[0], r[1]));
        }
    }
    // consumed + n_samples < 2^53: the last valid total and the first invalid one
    const uint64_t lim = (uint64_t)1 << 53;
    CHECK(rfa_pfb_rational_outputs(64, 65, lim - 2, 1, &n) == RFA_OK);
    n = 77;
    CHECK(rfa_pfb_rational_outputs(64, 65, lim - 1, 1, &n) == RFA_ERR_INVALID && n == 77);
    CHECK(rfa_pfb_rational_outputs(64, 65, lim, 0, &n) == RFA_ERR_INVALID);
    CHECK(rfa_pfb_rational_outputs(64, 65, 0, (size_t)lim, &n) == RFA_ERR_INVALID);
    CHECK(rfa_pfb_rational_outputs(3, 7, UINT64_MAX, (size_t)2, &n) == RFA_ERR_INVALID);   // no wrap-around
    // the ratio's own limits
    CHECK(rfa_pfb_rational_outputs(3, 7, 0, 10, nullptr) == RFA_ERR_INVALID);
    CHECK(rfa_pfb_rational_outputs(0, 7, 0, 10, &n) == RFA_ERR_INVALID);
    CHECK(rfa_pfb_rational_outputs(-3, 7, 0, 10, &n) == RFA_ERR_INVALID);
    CHECK(rfa_pfb_rational_outputs(7, 3, 0, 10, &n) == RFA_ERR_INVALID);       // L > D
    CHECK(rfa_pfb_rational_outputs(2, 2, 0, 10, &n) == RFA_ERR_INVALID);       // gcd 2
    CHECK(rfa_pfb_rational_outputs(4, 6, 0, 10, &n) == RFA_ERR_INVALID);
    CHECK(rfa_pfb_rational_outputs(3, 0, 0, 10, &n) == RFA_ERR_INVALID);
    CHECK(rfa_pfb_rational_outputs(RFA_PFB_MAX_INTERPOLATION, 65, 0, 10, &n) == RFA_OK);
    CHECK(rfa_pfb_rational_outputs(RFA_PFB_MAX_INTERPOLATION + 1, 66, 0, 10, &n) == RFA_ERR_INVALID);
}

static int create(int fmt, int32_t m, int32_t l, int32_t d, const float *taps, int32_t t, bool *null_out) {
    rfa_pfb *p = reinterpret_cast<rfa_pfb *>(0x1);
    const int st = rfa_pfb_create_rational(0, fmt, m, l, d, taps, t, &p);
    *null_out = p == nullptr;
    if (st == RFA_OK && p) rfa_pfb_destroy(p);
    return st;
}

static bool valid(int st, bool nul) { return (st == RFA_OK && !nul) || (st == RFA_ERR_NODEVICE && nul); }

static void check_create_errors() {
    std::vector<float> taps((size_t)RFA_PFB_MAX_PHASES * 16 * RFA_PFB_MAX_INTERPOLATION + 1, 0.25f);
    const float *h = taps.data();
    bool nul = false;
    CHECK(rfa_pfb_create_rational(0, RFA_IN_S8, 16, 3, 7, h, 61, nullptr) == RFA_ERR_INVALID);
    CHECK(create(-1, 16, 3, 7, h, 61, &nul) == RFA_ERR_INVALID && nul);
    CHECK(create(RFA_IN_F32_PLANAR, 16, 3, 7, h, 61, &nul) == RFA_ERR_INVALID && nul);
    CHECK(create(RFA_IN_S8, 0, 3, 7, h, 61, &nul) == RFA_ERR_INVALID && nul);
    CHECK(create(RFA_IN_S8, -16, 3, 7, h, 61, &nul) == RFA_ERR_INVALID && nul);
    CHECK(create(RFA_IN_S8, 16, 3, 7, nullptr, 61, &nul) == RFA_ERR_INVALID && nul);
    // 1 <= L: 0 outside, 1 inside
    CHECK(create(RFA_IN_S8, 16, 0, 7, h, 61, &nul) == RFA_ERR_INVALID && nul);
    CHECK(create(RFA_IN_S8, 16, -1, 7, h, 61, &nul) == RFA_ERR_INVALID && nul);
    { const int st = create(RFA_IN_S8, 16, 1, 7, h, 61, &nul); CHECK(valid(st, nul)); }
    // L <= RFA_PFB_MAX_INTERPOLATION
    { const int st = create(RFA_IN_S8, 16, RFA_PFB_MAX_INTERPOLATION, 65, h, 61, &nul); CHECK(valid(st, nul)); }
    CHECK(create(RFA_IN_S8, 16, RFA_PFB_MAX_INTERPOLATION + 1, 66, h, 61, &nul) == RFA_ERR_INVALID && nul);
    // L <= D: 7 / 8 inside (and 1 / 1), 8 / 7 outside
    { const int st = create(RFA_IN_S8, 16, 7, 8, h, 61, &nul); CHECK(valid(st, nul)); }
    { const int st = create(RFA_IN_S8, 16, 1, 1, h, 61, &nul); CHECK(valid(st, nul)); }
    CHECK(create(RFA_IN_S8, 16, 8, 7, h, 61, &nul) == RFA_ERR_INVALID && nul);
    CHECK(create(RFA_IN_S8, 16, 3, 0, h, 61, &nul) == RFA_ERR_INVALID && nul);
    // D <= L * M: 3 * 16 = 48 is shared with 3, so 47 inside and 49 outside; 1 * 16 inside, 17 outside
    { const int st = create(RFA_IN_S8, 16, 3, 47, h, 61, &nul); CHECK(valid(st, nul)); }
    CHECK(create(RFA_IN_S8, 16, 3, 49, h, 61, &nul) == RFA_ERR_INVALID && nul);
    { const int st = create(RFA_IN_S8, 16, 1, 16, h, 61, &nul); CHECK(valid(st, nul)); }
    CHECK(create(RFA_IN_S8, 16, 1, 17, h, 61, &nul) == RFA_ERR_INVALID && nul);
    // gcd(L, D) = 1
    CHECK(create(RFA_IN_S8, 16, 3, 9, h, 61, &nul) == RFA_ERR_INVALID && nul);
    CHECK(create(RFA_IN_S8, 16, 4, 6, h, 61, &nul) == RFA_ERR_INVALID && nul);
    CHECK(create(RFA_IN_S8, 16, 2, 2, h, 61, &nul) == RFA_ERR_INVALID && nul);
    // 1 <= num_taps <= RFA_PFB_MAX_PHASES * M * L
    CHECK(create(RFA_IN_S8, 16, 3, 7, h, 0, &nul) == RFA_ERR_INVALID && nul);
    CHECK(create(RFA_IN_S8, 16, 3, 7, h, -2, &nul) == RFA_ERR_INVALID && nul);
    { const int st = create(RFA_IN_S8, 16, 3, 7, h, 1, &nul); CHECK(valid(st, nul)); }
    { const int st = create(RFA_IN_S8, 16, 3, 7, h, RFA_PFB_MAX_PHASES * 16 * 3, &nul); CHECK(valid(st, nul)); }
    CHECK(create(RFA_IN_S8, 16, 3, 7, h, RFA_PFB_MAX_PHASES * 16 * 3 + 1, &nul) == RFA_ERR_INVALID && nul);
    { const int st = create(RFA_IN_S8, 16, 64, 65, h, RFA_PFB_MAX_PHASES * 16 * 64, &nul); CHECK(valid(st, nul)); }
    CHECK(create(RFA_IN_S8, 16, 64, 65, h, RFA_PFB_MAX_PHASES * 16 * 64 + 1, &nul) == RFA_ERR_INVALID && nul);
    // a length the DFT does not take: unsupported, after the invalid arguments
    for (int32_t m : {7, 14, 22, 4097, 8192}) {
        CHECK(create(RFA_IN_U8, m, 3, 7, h, 8, &nul) == RFA_ERR_UNSUPPORTED && nul);
        CHECK(create(RFA_IN_U8, m, 3, 9, h, 8, &nul) == RFA_ERR_INVALID && nul);     // invalid comes first
    }
    // the app's ratios, every format: the device is looked for only now
    for (int fmt : {RFA_IN_S8, RFA_IN_U8, RFA_IN_S16LE, RFA_IN_F32_INTERLEAVED}) {
        { const int st = create(fmt, 256, 3, 64, h, 8000, &nul); CHECK(valid(st, nul)); }
        { const int st = create(fmt, 80, 12, 125, h, 10000, &nul); CHECK(valid(st, nul)); }
        { const int st = create(fmt, 800, 3, 625, h, 16000, &nul); CHECK(valid(st, nul)); }
        CHECK(create(fmt, 800, 6, 1250, h, 16000, &nul) == RFA_ERR_INVALID && nul);   // 20 Msps to 96 kHz unreduced
    }
}

static void check_null_handle() {
    int32_t w[3] = {9, 9, 9};
    CHECK(rfa_pfb_get_ratio(nullptr, &w[0], &w[1], &w[2]) == RFA_ERR_INVALID);
    CHECK(rfa_pfb_get_ratio(nullptr, nullptr, nullptr, nullptr) == RFA_ERR_INVALID);
    CHECK(w[0] == 9 && w[1] == 9 && w[2] == 9);
}

int main() {
    check_count_rule();
    check_create_errors();
    check_null_handle();
    if (failures) {
        std::fprintf(stderr, "pfb_rational_host_check: %d check(s) failed\n", failures);
        return 1;
    }
    std::printf("pfb_rational_host_check ok\n");
    return 0;
}
